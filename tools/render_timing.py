"""Cost of rendering the dense map (pi3_slam_amd/render.py, csrc/render.hip) for the chess-room run.

  1. the 13-chunk synthetic chess room (tools/synth_sequence.py, 1 000 frames at 308 x 406, 2 cm voxels) goes through
     the creator and stage 2 (no bundle adjustment) twice, alternated and repeated: without and with
     --render-every 50 --render-overview -> wall seconds of stage 2 and what the renders add (plus one run of the
     default stage 2, bundle adjustments on, for scale);
  2. the kernels alone on that run's map and its 20 selected cameras: splat and resolve, HIP events, median of
     `--reps` after 3 warm-up runs, per camera batch size (1, 4, the default, all);
  3. with the development library (PI3_LIB_PATH=.../libpi3slam_hip_dev.so, a run of its own: the counter costs time)
     the atomics issued against the footprint pixels tested (the rest were skipped by the load before the atomic).

Prints one JSON line.  Usage: python tools/render_timing.py [--chunks DIR] [--reps 20] [--rounds 3]"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")
VOXEL = 0.02


def make_chunks(out_dir: str, dev: str) -> float:
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_NONE))
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=dev, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=True, num_loader_workers=0, dense_voxel_size=VOXEL)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)

    def items():
        for c, (a, b) in enumerate(seq.chunks):
            yield {"frames": seq.frames(c, cr.device), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
                   "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}

    t0 = time.perf_counter()
    _, manifest, _ = cr.write_chunks(cr.process_chunks(items()))
    cr.write_run_metadata(manifest)
    return time.perf_counter() - t0


def stage_two(chunks: str, out: str, dev: str, render: bool, bundle_adjust: bool = False):
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    kw = dict(render_every=50, render_overview=True) if render else {}
    rec = OfflineReconstructor(chunks, out, device=dev, bundle_adjust=bundle_adjust, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        rec.run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, rec


def footprint_pixels(points: np.ndarray, cams: np.ndarray, H: int, W: int, sv: float, near: float) -> int:
    """Pixels the splat kernel tests (the sum of the footprints), by the kernel's own formulas on the host."""
    x, y, z = (points[:, i].astype(np.float64) for i in range(3))
    total = 0
    for c in cams:
        with np.errstate(all="ignore"):
            xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3]
            yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7]
            zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11]
            ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (zc > near)
            u, v, r = c[12] * (xc / zc) + c[14], c[13] * (yc / zc) + c[15], sv * c[12] / zc
            r = np.minimum(np.maximum(r, 0.5), 16.0)
            w = np.minimum(np.floor(u + r), W - 1) - np.maximum(np.ceil(u - r), 0) + 1
            h = np.minimum(np.floor(v + r), H - 1) - np.maximum(np.ceil(v - r), 0) + 1
            total += int(np.sum(np.where(ok & (w > 0) & (h > 0), w * h, 0)))
    return total


def kernel_times(rec, dev: str, reps: int):
    from pi3_slam_amd import export, lib, ops
    from pi3_slam_amd.dense_map import fuse_chunks
    from pi3_slam_amd.render import MapRenderer, default_batch, pack_cameras
    dense = fuse_chunks(rec.reconstructions, dev)
    pts, cols, w, voxel = dense.points, dense.colors, dense.weights, dense.voxel_size
    views = [v for v in export.render_views(rec.reconstructions)[::50] if v["K"] is not None]
    H, W = views[0]["H"], views[0]["W"]
    cams = pack_cameras(np.stack([v["pose"] for v in views]), np.stack([v["K"] for v in views]))
    M = len(cams)
    r = MapRenderer(pts, cols, w, voxel, dev)
    out = r.render(cams, H, W)
    res = {"voxels": int(len(pts)), "views": M, "H": H, "W": W, "non_empty_pixels": r.last_stats["pixels"],
           "clamped": r.last_stats["clamped"], "default_batch": default_batch(M, H, W), "library": lib.build_flavor()}
    del out
    if lib.build_flavor() != "product":
        tested = footprint_pixels(np.asarray(pts), cams, H, W, voxel, 0.05)
        res.update(footprint_pixels=tested, atomics_issued=r.last_stats["atomics"],
                   atomics_skipped_pct=100.0 * (1.0 - r.last_stats["atomics"] / max(tested, 1)))
        return res
    cams_dev = torch.as_tensor(cams).to(dev)
    depth = torch.empty(M, H, W, dtype=torch.float32, device=dev)
    color = torch.empty(M, H, W, 3, dtype=torch.uint8, device=dev)
    index = torch.empty(M, H, W, dtype=torch.int32, device=dev)
    zbuf = torch.empty(M * H * W, dtype=torch.int64, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    res["per_view_ms"] = {}
    for batch in sorted({1, 4, 16, default_batch(M, H, W), M}):
        ts, tr = [], []
        for i in range(3 + reps):
            splat = resolve = 0.0
            marks = []
            for a in range(0, M, batch):
                b = min(M, a + batch)
                e = [ev() for _ in range(3)]
                e[0].record()
                ops.render_splat(r.points, r.weights, cams_dev[a:b], zbuf, r.stats, H, W, voxel)
                e[1].record()
                ops.render_resolve(zbuf, r.colors, r.stats, b - a, H, W, out=(depth[a:b], color[a:b], index[a:b]))
                e[2].record()
                marks.append(e)
            torch.cuda.synchronize()
            for e in marks:
                splat += e[0].elapsed_time(e[1])
                resolve += e[1].elapsed_time(e[2])
            if i >= 3:
                ts.append(splat / M)
                tr.append(resolve / M)
        res["per_view_ms"][str(batch)] = {"splat": float(np.median(ts)), "resolve": float(np.median(tr))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default=None, help="a directory of chess-room chunks made by an earlier call (else a "
                                                   "temporary one is filled first)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "voxel_size": VOXEL}
    chunks = a.chunks or tempfile.mkdtemp(prefix="render_timing_")
    if not os.path.exists(os.path.join(chunks, "chunk_metadata.json")):
        out["create_s"] = make_chunks(chunks, dev)
    work = tempfile.mkdtemp(prefix="render_timing_out_")
    plain, rendered, rec = [], [], None
    stage_two(chunks, os.path.join(work, "warm"), dev, True)
    for i in range(a.rounds):
        plain.append(stage_two(chunks, os.path.join(work, f"plain{i}"), dev, False)[0])
        t, rec = stage_two(chunks, os.path.join(work, f"render{i}"), dev, True)
        rendered.append(t)
    out["stage2_s"] = {"plain": plain, "with_renders": rendered, "median_plain": float(np.median(plain)),
                       "median_with_renders": float(np.median(rendered)),
                       "renders_add_s": float(np.median(rendered) - np.median(plain))}
    # the default stage 2 (both bundle adjustments on) for scale: one warm-up, then one timed run
    stage_two(chunks, os.path.join(work, "ba_warm"), dev, False, bundle_adjust=True)
    out["stage2_s"]["plain_bundle_adjust"] = stage_two(chunks, os.path.join(work, "ba"), dev, False, bundle_adjust=True)[0]
    out["write_renders_s"] = rec.render_seconds        # the last rendered run: total and its PNG-encoding share
    out["kernels"] = kernel_times(rec, dev, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
