"""Multi-view depth consistency filter on the GPU (csrc/dense_filter.hip, dense_map.ConsistencyFilter) against the numpy
oracle, byte for byte: the kernel on damaged analytic scenes, its argument checks, the creator's filtered dense_cloud
on the chess-room sequence with planted floaters, the no-intrinsics fallback and the online facade."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")

import dense_consistency_ref as cref   # noqa: E402
import dense_map_ref as mref           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.6                               # sigmoid threshold of the kernel tests; the logits are drawn around its logit

SHAPES = [(1, 8, 8), (2, 16, 24), (5, 24, 40), (12, 64, 80), (16, 77, 101)]
PARAMS = [(1, 1, 1), (2, 3, 2), (3, 4, 1)]          # (min_views, radius, stride)


@functools.lru_cache(maxsize=None)
def damaged_scene(N, H, W):
    """The analytic plane scene with 0.2 % multiplicative depth noise, one rectangle pulled to 0.5x and one pushed to
    1.6x depth, NaN / inf / negative-z holes, logits around the threshold and 90 % random masks (never modified)."""
    s = cref.plane_scene(N, H, W, seed=N * 10007 + H * 101 + W, noise_rel=0.002)
    rng = np.random.default_rng(H * 1009 + W)
    rows, cols = slice(H // 3, 2 * H // 3), slice(W // 3, 2 * W // 3)
    cref.scale_block(s, N // 2, rows, cols, 0.5)
    cref.scale_block(s, (N // 2 + 1) % N, slice(H // 8, H // 3), slice(W // 8, W // 2), 1.6)
    n = N * H * W
    pts, lp = s["points"].reshape(-1, 3), s["local_points"].reshape(-1, 3)
    idx = rng.choice(n, max(6, n // 100), replace=False)
    pts[idx[0::6], 0] = np.nan
    pts[idx[1::6], 1] = np.inf
    pts[idx[2::6], 2] = -np.inf
    lp[idx[3::6], 2] = -lp[idx[3::6], 2]
    lp[idx[4::6], 2] = np.nan
    lp[idx[5::6], 2] = np.inf
    s["conf"] = (mref.conf_logit(THR) + 1.5 * rng.standard_normal((N, H, W, 1))).astype(np.float32)
    s["masks"] = (rng.random((N, H, W)) < 0.9).astype(np.uint8)
    for v in s.values():
        v.setflags(write=False)
    return s


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)       # a copy: the scenes are read-only


def _run_kernel(s, conf, masks, mv, radius, stride, rel_tol=0.03):
    from pi3_slam_amd import ops
    mask, counts, stats = ops.dense_consistency(_dev(s["points"]), _dev(s["local_points"]), _dev(conf), _dev(masks),
                                                _dev(s["poses"]), _dev(s["fxfycxcy"]), float(mref.conf_logit(THR)),
                                                radius, stride, mv, rel_tol, want_counts=True)
    return mask.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "mv%d_r%d_s%d" % p)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernel_matches_oracle_byte_for_byte(shape, params):
    s = damaged_scene(*shape)
    mv, radius, stride = params
    for conf, masks in ((s["conf"], s["masks"]), (None, None)):
        exp = cref.consistency(s["points"], s["local_points"], conf, masks, s["poses"], s["fxfycxcy"],
                               mref.conf_logit(THR), radius, stride, mv, 0.03)
        got = _run_kernel(s, conf, masks, mv, radius, stride)
        again = _run_kernel(s, conf, masks, mv, radius, stride)
        print(f"{shape} {params} conf/masks {'on' if conf is not None else 'off'}: candidates {exp['stats'][0]}, kept "
              f"{exp['stats'][1]}, pixels with a conflict {int((exp['counts'][..., 1] > 0).sum())}; kernel stats {got[2]}")
        assert got[0].dtype == np.uint8 and got[0].shape == shape and got[1].shape == shape + (2,)
        assert got[2].tolist() == exp["stats"].tolist()
        assert got[0].tobytes() == exp["mask"].tobytes()
        assert got[1].tobytes() == exp["counts"].tobytes()
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
    if shape[0] >= 5:          # the scene exercises every branch: agreement, conflicts, holes
        assert 0 < exp["stats"][1] < exp["stats"][0] and (exp["counts"][..., 1] > 0).any()


def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    N, H, W = 3, 8, 8
    s = damaged_scene(2, 16, 24)
    pts, lp = _dev(s["points"][:, :8, :8].copy()), _dev(s["local_points"][:, :8, :8].copy())
    pts, lp = torch.cat([pts, pts[:1]]), torch.cat([lp, lp[:1]])
    poses, K = _dev(np.tile(s["poses"][:1], (3, 1, 1))), _dev(np.tile(s["fxfycxcy"][:1], (3, 1)))
    zplane = torch.full((N, H, W), 5.0, device=DEV)
    out = torch.full((N, H, W), 7, dtype=torch.uint8, device=DEV)
    stats = torch.full((2,), 11, dtype=torch.int64, device=DEV)

    def call(radius=3, stride=2, mv=2, tol=0.03, **null):
        p = dict(points=pts.data_ptr(), local=lp.data_ptr(), poses=poses.data_ptr(), K=K.data_ptr(),
                 zplane=zplane.data_ptr(), out=out.data_ptr(), stats=stats.data_ptr())
        p.update({k: None for k in null})
        return lib.pi3_dense_consistency(p["points"], p["local"], None, None, p["poses"], p["K"], N, H, W, 0.0, radius,
                                         stride, mv, tol, p["zplane"], p["out"], None, p["stats"], L.stream_ptr())

    bad = [dict(radius=0), dict(radius=17), dict(stride=0), dict(stride=-1), dict(mv=0), dict(mv=7), dict(radius=1, mv=3),
           dict(tol=0.0), dict(tol=-1.0), dict(tol=float("inf")), dict(tol=float("nan")), dict(points=1), dict(local=1),
           dict(poses=1), dict(K=1), dict(zplane=1), dict(out=1), dict(stats=1)]
    for kw in bad:
        lib.pi3_set_knob(b"no_such_knob", 0)          # leaves another message behind: the next one must replace it
        before = lib.pi3_last_error()
        assert call(**kw) == -1, kw                   # PI3_ERR_ARG
        msg = lib.pi3_last_error()
        assert msg and msg != before and b"pi3_dense_consistency" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((zplane == 5.0).all()) and stats.tolist() == [11, 11]
    assert call() == 0                                # and the same buffers with good values run
    torch.cuda.synchronize()
    assert stats.tolist()[0] > 0 and not bool((out == 7).any())


# ------------------------------------------------------------------------------------------------ creator end to end
VOXEL, CONF_THR, REL_TOL = 0.02, 0.7, 0.03
FLOATER_FRAMES, FLOATER_ROWS, FLOATER_COLS = (30, 61), slice(120, 160), slice(180, 220)
CHUNKS = (0, 2)             # the full chunk with the floaters and the ragged 20-frame tail


class FloaterEngine:
    """SceneEngine whose chunk 0 carries two confident floaters: in two frames a 40 x 40 block of local_points is pulled
    to half its depth, its world points follow through the frame's pose, its logits are set high."""

    def __init__(self, seq):
        import synth_sequence as ss
        self.inner = ss.SceneEngine(seq)

    def flops(self, *a):
        return self.inner.flops(*a)

    def __call__(self, imgs, **kw):
        out = self.inner(imgs, **kw)
        if int(round(float(imgs[0, 0, 0, 0, 0]) * 1024.0)) == 0:           # chunk 0 starts at frame 0
            for f in FLOATER_FRAMES:
                lp = out["local_points"][0, f, FLOATER_ROWS, FLOATER_COLS] * 0.5
                pose = out["camera_poses"][0, f]
                out["local_points"][0, f, FLOATER_ROWS, FLOATER_COLS] = lp
                out["points"][0, f, FLOATER_ROWS, FLOATER_COLS] = (lp[..., None, :] * pose[:3, :3]).sum(-1) + pose[:3, 3]
                out["conf"][0, f, FLOATER_ROWS, FLOATER_COLS] = 8.0
        return out


def _creator(seq, out_dir, **kw):
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    kw.setdefault("keypoint_type", "grid")
    kw.setdefault("estimate_camera_params", True)
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, max_num_keypoints=seq.max_kp, num_loader_workers=0, **kw)
    cr = OfflineChunkCreator(cfg, model=FloaterEngine(seq))
    cr.target_size = (seq.H, seq.W)
    return cr


def _items(seq, dev, chunks):
    for c in chunks:
        a, b = seq.chunks[c]
        yield {"frames": seq.frames(c, dev), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
               "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}


def _run_creator(seq, out_dir, chunks, **kw):
    cr = _creator(seq, out_dir, **kw)
    return [ch for _, ch in cr.process_chunks(_items(seq, cr.device, chunks))]


def surface_distance(P, seq, c):
    """Voxels of chunk c (its own gauge) -> (world points, distance to the nearest wall or sphere), f64."""
    G = seq.gauge_matrix(c)
    Xw = np.asarray(P, np.float64) @ G[:3, :3].T + G[:3, 3]
    d = np.min(np.concatenate([np.abs(Xw - seq.lo), np.abs(Xw - seq.hi)], 1), 1)
    for ctr, r in seq.spheres:
        d = np.minimum(d, np.abs(np.linalg.norm(Xw - ctr, axis=1) - r))
    return Xw, d


def nearest_view_depth(Xw, seq, c):
    """z-depth of every world point in the nearest camera of chunk c that has it inside its image (ground-truth poses,
    true intrinsics); a point no camera frames gets its distance to the nearest camera centre."""
    a, b = seq.chunks[c]
    best = np.full(len(Xw), np.inf)
    centre = np.full(len(Xw), np.inf)
    for T in seq.poses_gt[a:b]:
        d = (Xw - T[:3, 3]) @ T[:3, :3]
        with np.errstate(all="ignore"):
            u, v = seq.fx * d[:, 0] / d[:, 2] + seq.cx, seq.fy * d[:, 1] / d[:, 2] + seq.cy
            see = (d[:, 2] > 0) & (u >= -0.5) & (u <= seq.W - 0.5) & (v >= -0.5) & (v <= seq.H - 0.5)
        best = np.where(see, np.minimum(best, d[:, 2]), best)
        centre = np.minimum(centre, np.linalg.norm(d, axis=1))
    return np.where(np.isfinite(best), best, centre)


def check_filtered_cloud(seq, c, off_exp, on_exp):
    """The geometric claims about one chunk's clouds (oracle dicts with keys / points); -> retention."""
    s = seq.chunk_draws(c)["gauge_s"]                            # chunk units -> metres
    _, d_off = surface_distance(off_exp["points"], seq, c)
    Xw, d_on = surface_distance(on_exp["points"], seq, c)
    reach = s * VOXEL * np.sqrt(3.0) / 2
    far = d_on > reach                                           # only these need their depth
    slack = np.zeros(len(d_on))
    slack[far] = REL_TOL * nearest_view_depth(Xw[far], seq, c)
    on_surface = d_off <= 1e-3
    kept = np.isin(off_exp["keys"][on_surface], on_exp["keys"])
    retention = float(kept.mean())
    print(f"chunk {c}: off {len(d_off)} voxels ({int((d_off > 0.10).sum())} more than 10 cm from every surface, max "
          f"{d_off.max():.3f} m), on {len(d_on)} voxels (max {d_on.max():.3f} m, {int(far.sum())} beyond the voxel's reach, "
          f"worst excess over the bound {np.max(d_on - reach - slack):.4f} m); retention of the {int(on_surface.sum())} "
          f"on-surface voxels {retention:.4f}")
    return dict(d_off=d_off, d_on=d_on, bound=reach + slack, retention=retention)


# Retention: the share of the unfiltered cloud's on-surface voxels (centroid within 1 mm of a wall or sphere) that the
# filtered cloud still holds.  Computed first with the oracles alone, without the device (the same scene and floaters
# through FloaterEngine on the CPU, masks from oracle/post_ref.compute_masks, the scene's true intrinsics):
# chunk 0: 0.9887 of 6 015 voxels, chunk 2: 0.9555 of 1 416.  The floors are 0.05 below.  On the device the result
# equals the oracle's on the device's own maps (its noise draw differs from the CPU generator's: 0.9891 of 6 034 and
# 0.9560 of 1 386 on an MI355X); the floor only guards against a scene change that silently empties the map.
RETENTION_ORACLE = {0: 0.9887, 2: 0.9555}
RETENTION_FLOOR = {c: v - 0.05 for c, v in RETENTION_ORACLE.items()}


def test_creator_filters_floaters_and_matches_oracle(tmp_path):
    """Runs 10 s on an MI355X box: three creator runs over a 100-frame and a 20-frame chunk of the 180-frame scene, and on
    the host the consistency oracle and two fuse_pixels oracles per chunk at full chunk size (12.5 M pixels)."""
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), n_frames=180)
    dense = dict(dense_voxel_size=VOXEL, dense_conf_threshold=CONF_THR)
    flt = dict(min_views=2, radius=3, stride=2, rel_tol=REL_TOL)
    off = _run_creator(seq, str(tmp_path / "off"), CHUNKS, **dense)
    on = _run_creator(seq, str(tmp_path / "on"), CHUNKS, dense_min_views=2, **dense)
    maps = _run_creator(seq, str(tmp_path / "maps"), CHUNKS, keypoint_type="none")
    for c, a, b, m in zip(CHUNKS, off, on, maps):
        # every non-dense entry is untouched
        assert set(a) == set(b)
        for k in a:
            if k in ("_metrics", "dense_cloud"):
                continue
            x, y = a[k], b[k]
            if isinstance(x, dict):
                assert set(x) == set(y) and all(torch.equal(x[i], y[i]) for i in x), k
            elif torch.is_tensor(x):
                assert torch.equal(x, y), k
            else:
                assert x == y, k
        assert "consistency" not in a["dense_cloud"] and "dense_consistent" not in a["_metrics"]
        assert b["dense_cloud"]["consistency"] == flt
        pts, lp, conf, masks = (m[k].numpy() for k in ("points", "local_points", "conf", "masks"))
        imgs = seq.frames(c, "cpu")[0].numpy()
        cam = b["camera_params"]
        K = np.stack([cam[k][0].numpy() for k in ("fx", "fy", "cx", "cy")], 1).astype(np.float32)
        oracle = cref.consistency(pts, lp, conf, masks, b["camera_poses"].numpy(), K, mref.conf_logit(CONF_THR),
                                  flt["radius"], flt["stride"], flt["min_views"], flt["rel_tol"])
        off_exp = mref.fuse_pixels(pts, conf, masks, imgs, CONF_THR, VOXEL)
        on_exp = mref.fuse_pixels(pts, conf, masks.astype(bool) & oracle["mask"].astype(bool), imgs, CONF_THR, VOXEL)
        for run, exp in ((a, off_exp), (b, on_exp)):
            dc = run["dense_cloud"]
            assert dc["points"].numpy().tobytes() == exp["points"].tobytes()
            assert dc["colors"].numpy().tobytes() == exp["colors"].tobytes()
            assert dc["weights"].numpy().tobytes() == exp["weights"].tobytes()
        assert b["_metrics"]["dense_candidates"] == int(oracle["stats"][0])
        assert b["_metrics"]["dense_consistent"] == int(oracle["stats"][1]) > 0
        assert b["_metrics"]["dense_voxels"] == len(on_exp["keys"]) > 1000
        g = check_filtered_cloud(seq, c, off_exp, on_exp)
        if c == 0:        # not vacuous: the unfiltered cloud holds the floaters, and the filter removes their pixels
            assert int((g["d_off"] > 0.10).sum()) >= 50
            for f in FLOATER_FRAMES:
                blk = (f, FLOATER_ROWS, FLOATER_COLS)
                assert masks[blk].sum() > 1000 and not oracle["mask"][blk].any()
        assert np.all(g["d_on"] <= g["bound"])
        assert g["retention"] >= RETENTION_FLOOR[c]


def test_without_intrinsics_the_cloud_is_fused_unfiltered(tmp_path, capsys):
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), n_frames=180)
    dense = dict(dense_voxel_size=VOXEL, dense_conf_threshold=CONF_THR, estimate_camera_params=False)
    plain = _run_creator(seq, str(tmp_path / "plain"), (2,), **dense)[0]
    capsys.readouterr()
    got = _run_creator(seq, str(tmp_path / "flt"), (2,), dense_min_views=2, **dense)[0]
    assert "consistency filter" in capsys.readouterr().out
    assert "consistency" not in got["dense_cloud"] and "dense_consistent" not in got["_metrics"]
    assert "camera_params" not in got
    assert set(got["dense_cloud"]) == set(plain["dense_cloud"])
    for k in ("points", "colors", "weights"):
        assert torch.equal(got["dense_cloud"][k], plain["dense_cloud"][k]) and len(got["dense_cloud"][k]) > 1000


# ------------------------------------------------------------------------------------------------ online facade
def _oracle_world(chunks, voxel):
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import chunk_transform
    sets = []
    for d in chunks:
        cl = d.get("dense_cloud")
        if cl is None or int(cl["points"].shape[0]) == 0:
            continue
        pts = cl["points"].to(DEV, torch.float32).contiguous().clone()
        ops.sim3_apply(chunk_transform(d).reshape(16).to(DEV).contiguous(), pts, None)
        sets.append((pts.cpu().numpy(), cl["colors"].numpy(), cl["weights"].numpy()))
    return mref.fuse_point_sets(sets, voxel)


def test_online_filtered_dense_map_under_hip_graph(tmp_path):
    from PIL import Image

    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.export import write_ply
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (232, 296, 3)).astype(np.float32)
    k = 9
    sm = np.cumsum(np.cumsum(base, 0), 1)
    sm = (sm[k:, k:] - sm[:-k, k:] - sm[k:, :-k] + sm[:-k, :-k]) / (k * k)
    paths = []
    for i in range(20):
        p = str(frames / f"frame_{i:05d}.png")
        Image.fromarray(np.clip(sm[i % 20: i % 20 + 192, (2 * i) % 20: (2 * i) % 20 + 256], 0, 255).astype(np.uint8)).save(p)
        paths.append(p)
    engine = Pi3Engine(Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5), DEV)
    with torch.no_grad():     # non-empty masks (the edit bench.py makes to plain recipe weights)
        w_, b_ = engine.w["point_head.proj.weight"], engine.w["point_head.proj.bias"]
        w_[392:588] = 0.05 * w_[392:393].clone()
        b_[392:588] = b_[392].clone()
        engine.w["conf_head.proj.bias"][:196] -= 2.2
    slam = Pi3SLAMOnline(model=engine, chunk_length=8, overlap=3, device=DEV, keypoint_type="grid", max_num_keypoints=100,
                         estimate_camera_params=True, hip_graph=True, output_dir=str(tmp_path / "online"),
                         bundle_adjust=False, conf_threshold=0.05, dense_voxel_size=0.05, dense_min_views=1)
    slam.process_chunks(paths)
    chunks = slam.chunk_reconstructions
    assert len(chunks) >= 3
    for c in chunks:
        assert c["dense_cloud"]["consistency"] == {"min_views": 1, "radius": 3, "stride": 2, "rel_tol": 0.03}
        m = c["_metrics"]
        assert 0 <= m["dense_consistent"] <= m["dense_candidates"]
    out = str(tmp_path / "online" / "dense_points.ply")
    n = slam.save_dense_map(out)
    exp = _oracle_world(chunks, 0.05)
    print(f"online filtered dense map: {n} voxels; per chunk candidates "
          f"{[c['_metrics']['dense_candidates'] for c in chunks]}, consistent "
          f"{[c['_metrics']['dense_consistent'] for c in chunks]}, voxels {[c['_metrics']['dense_voxels'] for c in chunks]}")
    assert n == len(exp["keys"])
    write_ply(exp["points"], np.asarray(exp["colors"], np.uint8), str(tmp_path / "oracle.ply"))
    assert open(out, "rb").read() == open(str(tmp_path / "oracle.ply"), "rb").read()
