"""The numbers of DESIGN.md 7d: what the cloud search (csrc/cloud_nn.hip) costs and what map scoring says about the
dense map's cleaning and carving flags on the synthetic room.  Needs the GPU.

    python tools/map_eval_timing.py --timing      # build / query time at 1 M x 1 M and 4 M x 4 M reference_cloud points
    python tools/map_eval_timing.py --example     # F-score of the plain, cleaned, carved and carved + cleaned map
    python tools/map_eval_timing.py --icp         # the ICP reduction (csrc/cloud_icp.hip) beside the search, 1 M x 1 M
    python tools/map_eval_timing.py --mesh        # the triangle search (csrc/mesh_nn.hip) and the sampler, 1 M queries

--timing: cloud A = reference_cloud(frame_step=2, pixel_stride=2), cloud B = reference_cloud(frame_step=1,
pixel_stride=4) of the 1 000-frame chess-room sequence, n random points of each (in frame order, and shuffled), index
A, query B, max_dist = 4 voxels of 2 cm; hip events around the ops calls, median and minimum of 5 after one warm-up.
--example: 180 frames at 308 x 406 in chunks of 100 / 20 through the real creator (2 cm voxels, confidence 0.7,
--dense-min-views 2, depth keyframes every 2nd frame at stride 2) and OfflineReconstructor without bundle adjustment;
dense_points.ply against reference_cloud() after the trajectory pair's alignment, both resampled at 2 cm.
--icp: the clouds and the search of --timing at n = m = 1 M (and 4 M) in frame order, then ops.cloud_pair_equations on
the search's idx / d2 in each normals_of mode (random normals; mode 2 with a rotation), timed the same way.
--mesh: the planted room of tests/cloud_icp_ref.py (4 x 3 x 2.5 m with a cabinet).  Mesh 1: surface nets (MapMesher) of
4 M of its points with their normals fused at 1.1 cm voxels, about 1 M triangles; mesh 2: the same room as 22 wall-sized
triangles (tests/test_mesh_eval.py: room_mesh).  Queries: 1 M further points of the room with 5 mm Gaussian noise, in
sampling order.  max_dist as above; count + fill (with the host's read between them), the search, and the sampler at
one sample per (1 cm)^2 timed with hip events, median and minimum of 5 after one warm-up."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth_sequence as ss  # noqa: E402

GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")
VOXEL = 0.02
MAX_DIST = 4 * VOXEL
THRESHOLDS = (0.02, 0.05)
VARIANTS = {"plain": {},
            "cleaned (--dense-min-support 4 --dense-min-component 50)": dict(dense_min_support=4, dense_min_component=50),
            "carved (--dense-carve-min-conflicts 3)": dict(dense_carve_min_conflicts=3),
            "carved + cleaned": dict(dense_carve_min_conflicts=3, dense_min_support=4, dense_min_component=50)}


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def pick(cloud, n, gen, shuffle):
    idx = torch.randperm(len(cloud), device=cloud.device, generator=gen)[:n]
    if not shuffle:
        idx = idx.sort().values
    return cloud[idx].contiguous()


def timing(dev):
    from pi3_slam_amd import ops
    seq = ss.SyntheticSequence(GT)
    a = seq.reference_cloud(frame_step=2, pixel_stride=2, device=dev)
    b = seq.reference_cloud(frame_step=1, pixel_stride=4, device=dev)
    print(f"cloud A: {len(a)} points; cloud B: {len(b)} points", flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    inv = ops.cloud_inv_cell(MAX_DIST)
    for n in (1_000_000, 4_000_000):
        for shuffle in (False, True):
            p, q = pick(a, n, gen, shuffle), pick(b, n, gen, shuffle)
            table = torch.empty(ops.voxel_capacity(n) * 8, dtype=torch.int64, device=dev)
            cells = torch.empty((n, 4), dtype=torch.int32, device=dev)
            d2 = torch.empty(n, dtype=torch.float64, device=dev)
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            cb, cq = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            tb = timed(lambda: ops.cloud_index_build(p, inv, table, cells, cb))
            tq = timed(lambda: ops.cloud_nearest(table, cells, inv, q, MAX_DIST, d2, idx, cq))
            bs = dict(zip(ops.CLOUD_INDEX_COUNTERS, cb.tolist()))
            qs = dict(zip(ops.CLOUD_NEAREST_COUNTERS, cq.tolist()))
            print(json.dumps(dict(n=n, m=n, order="shuffled" if shuffle else "frame order", max_dist=MAX_DIST,
                                  build_ms_median=tb[0], build_ms_min=tb[1], query_ms_median=tq[0], query_ms_min=tq[1],
                                  build=bs, query=qs, evaluations_per_query=qs["evaluations"] / n,
                                  points_per_cell=(n - bs["dropped"]) / max(bs["cells"], 1))), flush=True)
            del table, cells, d2, idx, p, q


def icp_timing(dev):
    from pi3_slam_amd import ops
    seq = ss.SyntheticSequence(GT)
    a = seq.reference_cloud(frame_step=2, pixel_stride=2, device=dev)
    b = seq.reference_cloud(frame_step=1, pixel_stride=4, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    inv = ops.cloud_inv_cell(MAX_DIST)
    rot = [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]
    for n in (1_000_000, 4_000_000):
        p, q = pick(a, n, gen, False), pick(b, n, gen, False)
        table = torch.empty(ops.voxel_capacity(n) * 8, dtype=torch.int64, device=dev)
        cells = torch.empty((n, 4), dtype=torch.int32, device=dev)
        d2 = torch.empty(n, dtype=torch.float64, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        cb, cq = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        ops.cloud_index_build(p, inv, table, cells, cb)
        tq = timed(lambda: ops.cloud_nearest(table, cells, inv, q, MAX_DIST, d2, idx, cq))
        normals = torch.randn((n, 3), device=dev, generator=gen)
        partials = torch.empty((ops.cloud_icp_partial_rows(n), ops.CLOUD_ICP_DOUBLES), dtype=torch.float64, device=dev)
        out = torch.zeros(ops.CLOUD_ICP_DOUBLES, dtype=torch.float64, device=dev)
        ce = torch.zeros(4, dtype=torch.int64, device=dev)
        centre = p.double().mean(0).tolist()
        for mode in (0, 1, 2):
            te = timed(lambda: ops.cloud_pair_equations(q, p, idx, d2, MAX_DIST, centre, normals if mode else None, mode,
                                                        rot if mode == 2 else None, partials, out, ce))
            print(json.dumps(dict(n=n, m=n, normals_of=mode, query_ms_median=tq[0], equations_ms_median=te[0],
                                  equations_ms_min=te[1], counters=dict(zip(ops.CLOUD_ICP_COUNTERS, ce.tolist())),
                                  rows=int(partials.shape[0]))), flush=True)
        del table, cells, d2, idx, p, q, normals, partials


def mesh_timing(dev):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cloud_icp_ref as icpref
    from test_mesh_eval import room_mesh
    from pi3_slam_amd import map_eval, ops
    from pi3_slam_amd.dense_map import MapMesher, NormalAccumulator, VoxelFuser
    rng = np.random.default_rng(3)
    pts, nrm = icpref.sample_room(4_000_000, rng)
    P, N = torch.from_numpy(pts.astype(np.float32)).to(dev), torch.from_numpy(nrm.astype(np.float32)).to(dev)
    fz = VoxelFuser(0.011, dev)
    fz.reserve(len(P))
    fz.fuse_points(P, None, None)
    acc = NormalAccumulator(fz)
    acc.clear()
    acc.add_points(P, N, torch.ones(len(P), dtype=torch.int32, device=dev),
                   torch.eye(3, dtype=torch.float64, device=dev).reshape(9).contiguous())
    mesher = MapMesher()
    nets = mesher.apply(fz, acc)
    print(f"surface nets: {mesher.summary()}", flush=True)
    del fz, acc, P, N
    q = icpref.sample_room(1_000_000, rng)[0] + 0.005 * rng.standard_normal((1_000_000, 3))
    q = torch.from_numpy(q.astype(np.float32)).to(dev)
    wall_v, wall_f = room_mesh()
    for name, v, f in (("surface nets", nets["vertices"], nets["faces"]), ("22 triangles", wall_v, wall_f)):
        v, f = torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev)
        holder = {}

        def build():
            holder["index"] = map_eval.MeshIndex(v, f, MAX_DIST, dev)
        tb = timed(build)
        index = holder["index"]
        m = len(q)
        d2 = torch.empty(m, dtype=torch.float64, device=dev)
        face = torch.empty(m, dtype=torch.int32, device=dev)
        closest = torch.empty((m, 3), dtype=torch.float32, device=dev)
        cq = torch.zeros(4, dtype=torch.int64, device=dev)
        tq = timed(lambda: ops.mesh_nearest(index.table, index.rows, index.packed, index.inv_cell, q, MAX_DIST, d2, face,
                                            closest, cq))
        ts = timed(lambda: map_eval.sample_surface(v, f, 0.01, 0, dev))
        samples = int(map_eval.sample_surface(v, f, 0.01, 0, dev)[0].shape[0])
        bs, qs = index.build_stats, dict(zip(ops.MESH_NEAREST_COUNTERS, cq.tolist()))
        kept = max(bs["faces"] - bs["dropped"], 1)
        print(json.dumps(dict(mesh=name, faces=bs["faces"], queries=m, max_dist=MAX_DIST, build_ms_median=tb[0],
                              build_ms_min=tb[1], query_ms_median=tq[0], query_ms_min=tq[1], sample_ms_median=ts[0],
                              sample_ms_min=ts[1], samples=samples, build=bs, query=qs, rows_per_triangle=bs["rows"] / kept,
                              evaluations_per_query=qs["evaluations"] / m,
                              mean_distance_mm=float(d2[torch.isfinite(d2)].sqrt().mean()) * 1e3)), flush=True)
        del index, holder


def items(seq, dev):
    for c, (a, b) in enumerate(seq.chunks):
        yield {"frames": seq.frames(c, dev), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
               "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}


def create(seq, out_dir, dev):
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=dev, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=True, num_loader_workers=0, dense_voxel_size=VOXEL,
                               dense_conf_threshold=0.7, dense_min_views=2, dense_depth_every=2, dense_depth_stride=2)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    _, manifest, _ = cr.write_chunks(cr.process_chunks(items(seq, cr.device)))
    cr.write_run_metadata(manifest)


def example(dev):
    from pi3_slam_amd import map_eval
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    tmp = tempfile.mkdtemp()
    for noise in ("NOISE_BF16", "NOISE_NONE"):
        seq = ss.SyntheticSequence(GT, noise=dict(getattr(ss, noise)), n_frames=180)
        ref = seq.reference_cloud(device=dev)
        cdir = os.path.join(tmp, noise)
        create(seq, cdir, dev)
        for i, (name, kw) in enumerate(VARIANTS.items()):
            rdir = os.path.join(cdir, f"rec_{i}")
            OfflineReconstructor(chunk_dir=cdir, output_dir=rdir, bundle_adjust=False, device=dev, **kw).run()
            est, _ = map_eval.read_ply_points(os.path.join(rdir, "dense_points.ply"))
            T = map_eval.trajectory_alignment(os.path.join(rdir, "trajectory_tum.txt"), GT)
            res = map_eval.compare_clouds(est, ref, THRESHOLDS, transform=T, voxel_size=VOXEL, device=dev)
            print(f"==== {noise} / {name}\n{map_eval.format_table(res)}", flush=True)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--example", action="store_true")
    ap.add_argument("--icp", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not (a.timing or a.example or a.icp or a.mesh):
        ap.error("give --timing, --example, --icp and / or --mesh")
    if a.timing:
        timing(a.device)
    if a.icp:
        icp_timing(a.device)
    if a.mesh:
        mesh_timing(a.device)
    if a.example:
        example(a.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
