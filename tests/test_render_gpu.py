"""Map renderer on the GPU (csrc/render.hip, pi3_slam_amd/render.py) against the numpy oracle, bit for bit: seeded clouds
at three shapes, the designed plane scene with its derived bounds, the 13-chunk chess room end to end (files, oracle
equality, no floater in front of a true surface) and the online facade's save_renders."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")

import render_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pose_looking(eye, target, roll=0.0):
    """cam->world pose with +z towards the target (x right, y down)."""
    z = np.asarray(target, float) - np.asarray(eye, float)
    z /= np.linalg.norm(z)
    up = np.array([0.0, -1.0, 0.0]) if abs(z[1]) < 0.95 else np.array([0.0, 0.0, 1.0])
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = math.cos(roll), math.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def _seeded_scene(V, M, H, W, seed):
    """A room of 6 x 4 x 6 m sampled on its walls and on two spheres with millimetre noise, NaN / inf / far rows,
    weights 0..5 (min_weight 3 is used), cameras inside the room, outside it, one at 30 cm from a wall (radius clamps)
    and, from M >= 2 on, one orthographic camera."""
    rng = np.random.default_rng(seed)
    half = np.array([3.0, 2.0, 3.0])
    n_s = V // 5
    face = rng.integers(0, 6, V - n_s)
    p = rng.uniform(-1, 1, (V - n_s, 3)) * half
    ax = face // 2
    p[np.arange(len(p)), ax] = np.where(face % 2 == 0, -1.0, 1.0) * half[ax]
    d = rng.standard_normal((n_s, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ctr = np.where(rng.random((n_s, 1)) < 0.5, np.array([[1.0, 0.5, 0.8]]), np.array([[-1.2, -0.3, -1.0]]))
    pts = np.concatenate([p, ctr + 0.5 * d], 0) + 1e-3 * rng.standard_normal((V, 3))
    pts = pts[rng.permutation(V)].astype(np.float32)
    bad = rng.integers(0, V, max(3, V // 400))
    pts[bad[0::3], 0] = np.nan
    pts[bad[1::3], 1] = np.inf
    pts[bad[2::3], 2] = 3.0e5
    colors = rng.integers(0, 256, (V, 3), dtype=np.uint8)
    weights = rng.integers(0, 6, V).astype(np.int32)
    f = 0.9 * W
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    poses, ortho = [], []
    for m in range(M):
        kind = m % 4
        if M >= 2 and m == M - 1:
            poses.append(_pose_looking([0.2, -1.5, 0.1], [0.2, 2.0, 0.1]))                    # from above, looking down
            ortho.append(True)
            continue
        if kind == 0:
            poses.append(_pose_looking(rng.uniform(-1.5, 1.5, 3) * [1, 0.5, 1], rng.uniform(-3, 3, 3), rng.uniform(-0.3, 0.3)))
        elif kind == 1:
            poses.append(_pose_looking(rng.uniform(7, 9) * np.array([math.cos(m), 0.2, math.sin(m)]), [0, 0, 0]))
        elif kind == 2:
            poses.append(_pose_looking([2.7, rng.uniform(-1, 1), rng.uniform(-2, 2)], [3.0, 0.0, 0.0]))   # 30 cm off a wall
        else:
            poses.append(_pose_looking(rng.uniform(-2.5, 2.5, 3) * [1, 0.6, 1], [1.0, 0.5, 0.8]))
        ortho.append(False)
    from pi3_slam_amd.render import pack_cameras
    cams = pack_cameras(np.stack(poses), K, ortho=ortho)
    cams[np.asarray(ortho), 12:14] = W / 8.0           # orthographic: pixels per metre
    return pts, colors, weights, cams


def _same(out, exp, stats=None):
    for k in ("depth", "color", "index"):
        a, b = np.ascontiguousarray(out[k].numpy() if torch.is_tensor(out[k]) else out[k]), np.ascontiguousarray(exp[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, int((a != b).sum()))
    if stats is not None:
        assert stats["pixels"] == exp["pixels"] and stats["culled"] == exp["culled"] and stats["clamped"] == exp["clamped"], \
            (stats, exp["pixels"], exp["culled"], exp["clamped"])


@pytest.mark.parametrize("shape", [(5000, 1, 16, 24), (200000, 8, 64, 80), (1000000, 20, 308, 406)])
def test_render_matches_oracle_bit_for_bit(shape):
    from pi3_slam_amd.render import MapRenderer
    V, M, H, W = shape
    pts, colors, weights, cams = _seeded_scene(V, M, H, W, seed=sum(shape))
    kw = dict(min_weight=3, splat_scale=1.0, near=0.05, far=12.0)
    r = MapRenderer(pts, colors, weights, 0.02, DEV)
    out = r.render(cams, H, W, **kw)
    st = dict(r.last_stats)
    exp = ref.render(pts, colors, weights, cams, H, W, 0.02, **kw)
    print(f"render {shape}: {exp['pixels']} of {M * H * W} pixels, {exp['culled']} culled, {exp['clamped']} clamped")
    assert 0 < exp["pixels"]
    if M >= 8:
        assert exp["clamped"] > 0 and exp["culled"] > 0 and exp["pixels"] < M * H * W
    _same(out, exp, st)
    assert st["atomics"] == 0                                 # the product build carries no timing counter
    again = r.render(cams, H, W, **kw)                        # the same call twice: the same bytes
    for k in out:
        assert out[k].numpy().tobytes() == again[k].numpy().tobytes(), k
    for batch in (1, M):                                      # the batch size does not show in the result
        other = r.render(cams, H, W, batch=batch, **kw)
        for k in out:
            assert out[k].numpy().tobytes() == other[k].numpy().tobytes(), (k, batch)
        assert r.last_stats == st
    dev = r.render(cams, H, W, to_host=False, **kw)
    assert all(t.is_cuda for t in dev.values()) and torch.equal(dev["depth"].cpu(), out["depth"])
    # weights None: every finite voxel counts
    r2 = MapRenderer(pts, colors, None, 0.02, DEV)
    o2 = r2.render(cams[:1], H, W, **kw)
    _same(o2, ref.render(pts, colors, None, cams[:1], H, W, 0.02, **kw), r2.last_stats)


def test_render_of_an_empty_map_and_wrapper_checks():
    from pi3_slam_amd import ops
    from pi3_slam_amd.lib import Pi3HipError
    from pi3_slam_amd.render import MapRenderer, pack_cameras
    cams = pack_cameras(np.eye(4), np.array([[20.0, 0, 11.5], [0, 20.0, 7.5], [0, 0, 1]]))
    r = MapRenderer(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), None, 0.02, DEV)
    out = r.render(cams, 16, 24)
    assert (out["depth"] == 0).all() and (out["index"] == -1).all() and (out["color"] == 0).all()
    assert r.last_stats["pixels"] == 0
    pts = torch.zeros(4, 3, device=DEV)
    z = torch.empty(16 * 24, dtype=torch.int64, device=DEV)
    st = torch.zeros(4, dtype=torch.int64, device=DEV)
    cd = torch.as_tensor(cams).to(DEV)
    with pytest.raises(AssertionError):
        ops.render_splat(pts, None, cd, z[:10], st, 16, 24, 0.02)             # z-buffer too small
    with pytest.raises(AssertionError):
        ops.render_splat(pts.double(), None, cd, z, st, 16, 24, 0.02)         # dtype
    with pytest.raises(Pi3HipError):
        ops.render_splat(pts, None, cd, z, st, 16, 24, 0.0)                   # voxel size
    with pytest.raises(Pi3HipError):
        ops.render_splat(pts.cpu(), None, cd, z, st, 16, 24, 0.02)            # host tensor


def test_designed_plane_scene_on_the_device():
    from pi3_slam_amd.render import MapRenderer
    from test_render import PLANE, check_plane_scene, plane_scene
    points, colors, weights, cam = plane_scene()
    r = MapRenderer(points, colors, weights, PLANE["v"], DEV)
    out = r.render(cam, PLANE["H"], PLANE["W"], splat_scale=1.0)
    out = {k: t.numpy() for k, t in out.items()}
    check_plane_scene(out, points, cam)
    _same(out, ref.render(points, colors, weights, cam, PLANE["H"], PLANE["W"], PLANE["v"]), r.last_stats)


# ------------------------------------------------------------------------------------------------ chess room, end to end
def _creator(seq, out_dir, **kw):
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=True, num_loader_workers=0, **kw)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    return cr


def _items(seq, dev, chunks):
    for c in chunks:
        a, b = seq.chunks[c]
        yield {"frames": seq.frames(c, dev), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
               "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}


def _read_ply(path):
    data = open(path, "rb").read()
    head = data.index(b"end_header\n") + len(b"end_header\n")
    rec = np.frombuffer(data[head:], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    return np.ascontiguousarray(rec["xyz"]), np.ascontiguousarray(rec["rgb"])


def _u16(depth):
    return np.minimum(np.rint(np.asarray(depth, np.float64) * 1000.0), 65535.0).astype(np.uint16)


def _gt_depth(seq, frame):
    """Ray-cast z-depth (metres) of a frame at its ground-truth pose, sampled at the pixel centres."""
    v, u = torch.meshgrid(torch.arange(seq.H, dtype=torch.float64), torch.arange(seq.W, dtype=torch.float64), indexing="ij")
    d_cam = torch.stack([(u.reshape(-1) - seq.cx) / seq.fx, (v.reshape(-1) - seq.cy) / seq.fy,
                         torch.ones(seq.H * seq.W, dtype=torch.float64)], -1)
    Pw = torch.as_tensor(seq.poses_gt[frame])
    d_w = (d_cam @ Pw[:3, :3].T)[None]
    t, _ = seq._cast(Pw[None, None, :3, 3], d_w)             # the ray's camera z is 1: t is the z-depth
    return t.reshape(seq.H, seq.W).numpy()


def _check_files_against_oracle(out_dir, seq, v):
    """(a) the files of <out_dir>/renders, (b) every PNG == the oracle's render of dense_points.ply through the cameras
    of cameras.json -> (cameras.json, the oracle's render, the voxel count, the set of file names)."""
    from PIL import Image

    from pi3_slam_amd.render import pack_cameras
    # (a)
    rd = out_dir / "renders"
    rec = json.load(open(rd / "cameras.json"))
    frames = [vw["frame"] for vw in rec["views"]]
    assert frames == [seq.frame_name(i) for i in range(0, 1000, 50)]
    assert rec["depth_scale"] == 1000.0 and rec["voxel_size"] == v
    expected = {"cameras.json", "overview.png"}
    for vw in rec["views"]:
        stem = os.path.splitext(vw["frame"])[0]
        assert vw["depth"] == f"depth_{stem}.png" and vw["color"] == f"color_{stem}.png"
        assert (vw["H"], vw["W"]) == (seq.H, seq.W)
        expected |= {vw["depth"], vw["color"]}
    assert set(os.listdir(rd)) == expected
    ov = np.asarray(Image.open(rd / "overview.png"))
    assert ov.shape == (seq.H, seq.W, 3)
    red = (ov[..., 0] == 255) & (ov[..., 1] == 0) & (ov[..., 2] == 0)
    print(f"overview: {100 * np.mean(ov.any(-1)):.1f} % of the pixels drawn, {int(red.sum())} trajectory pixels")
    assert red.sum() >= 100                                   # the trajectory is in the picture

    # (b)
    pts, cols = _read_ply(str(out_dir / "dense_points.ply"))
    poses = np.array([vw["pose"] for vw in rec["views"]])
    Ks = np.array([[[vw["fx"], 0, vw["cx"]], [0, vw["fy"], vw["cy"]], [0, 0, 1]] for vw in rec["views"]])
    assert np.allclose(Ks[:, 0, 2], seq.W // 2 - 0.5) and np.allclose(Ks[:, 1, 2], seq.H // 2 - 0.5)
    exp = ref.render(pts, cols, None, pack_cameras(poses, Ks), seq.H, seq.W, v, splat_scale=1.0, min_weight=1, near=0.05)
    for j, vw in enumerate(rec["views"]):
        d16 = np.asarray(Image.open(rd / vw["depth"]))
        assert d16.dtype == np.uint16 and d16.tobytes() == _u16(exp["depth"][j]).tobytes(), vw["frame"]
        assert np.asarray(Image.open(rd / vw["color"])).tobytes() == exp["color"][j].tobytes(), vw["frame"]

    return rec, exp, len(pts), expected


def test_chess_room_end_to_end_renders(tmp_path):
    """(a) files, (b) PNG == oracle, (c) no floater in front of a true surface, (d) the other side and the empty share
    are printed, not gated.

    (c): every centroid lies within sqrt(3)/2 v of a real surface point, that point projects inside the window, and the
    first hit along a ray is never behind a real surface point on it; 1 mm is the alignment slack of the map test.
    Measured on an MI355X (printed below): 2 291 303 pixels with a whole window, none in front of the bound,
    none deeper than max(z_gt) + the same slack, 0.296 % of all pixels empty (about the pixels that look at sphere 0)."""
    from PIL import Image
    from scipy.ndimage import maximum_filter, minimum_filter

    import synth_sequence as ss
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    from pi3_slam_amd.render import pack_cameras
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_NONE))
    v = 0.02
    cr = _creator(seq, str(tmp_path), dense_voxel_size=v)
    saved, manifest, _ = cr.write_chunks(cr.process_chunks(_items(seq, cr.device, range(len(seq.chunks)))))
    cr.write_run_metadata(manifest)
    assert len(saved) == 13
    out_dir = tmp_path / "r1"
    OfflineReconstructor(str(tmp_path), str(out_dir), device=DEV, bundle_adjust=False, render_every=50,
                         render_overview=True).run()
    # without the flags: the same files as before, and no renders
    plain = tmp_path / "r0"
    OfflineReconstructor(str(tmp_path), str(plain), device=DEV, bundle_adjust=False).run()
    assert not (plain / "renders").exists()
    for name in ("dense_points.ply", "trajectory_tum.txt", "final_points.ply", "final_camera_poses.ply"):
        assert open(plain / name, "rb").read() == open(out_dir / name, "rb").read(), name
    assert sorted(os.listdir(plain)) == sorted(set(os.listdir(out_dir)) - {"renders"})

    rec, exp, n_voxels, expected = _check_files_against_oracle(out_dir, seq, v)
    rd = out_dir / "renders"

    # (c), (d): metres through chunk 0's gauge
    s0 = float(np.cbrt(np.linalg.det(seq.gauge_matrix(0)[:3, :3])))
    tol = math.sqrt(3.0) / 2.0 * v + 1e-3
    n_checked = n_front = n_behind = n_hit = n_all = 0
    worst = 0.0
    for j, vw in enumerate(rec["views"]):
        depth = exp["depth"][j].astype(np.float64)            # == the PNG before its rounding
        hit = depth > 0
        z_gt = _gt_depth(seq, int(vw["frame"].split("-")[1].split(".")[0]))
        dz = np.where(hit, depth, 1.0)
        r = np.minimum(np.maximum(v * vw["fx"] / dz, 0.5), 16.0)
        k = (np.ceil(r) + np.ceil(math.sqrt(3.0) / 2.0 * v * vw["fx"] / dz) + 1).astype(np.int64)
        yy, xx = np.meshgrid(np.arange(seq.H), np.arange(seq.W), indexing="ij")
        whole = hit & (xx - k >= 0) & (xx + k <= seq.W - 1) & (yy - k >= 0) & (yy + k <= seq.H - 1)
        lo, hi = np.full(depth.shape, np.nan), np.full(depth.shape, np.nan)
        for kk in np.unique(k[whole]):
            sel = whole & (k == kk)
            lo[sel] = minimum_filter(z_gt, size=2 * int(kk) + 1, mode="nearest")[sel]
            hi[sel] = maximum_filter(z_gt, size=2 * int(kk) + 1, mode="nearest")[sel]
        dm = s0 * depth
        front = whole & (dm < lo - tol)
        behind = whole & (dm > hi + tol)
        worst = max(worst, float(np.max((lo - dm)[whole])) if whole.any() else 0.0)
        n_checked += int(whole.sum())
        n_front += int(front.sum())
        n_behind += int(behind.sum())
        n_hit += int(hit.sum())
        n_all += depth.size
    print(f"chess room renders: {n_voxels} voxels, {n_all} pixels in {len(rec['views'])} views, {n_all - n_hit} "
          f"({100 * (1 - n_hit / n_all):.3f} %) empty; {n_checked} pixels with a whole window: {n_front} in front of "
          f"min(z_gt) - {1e3 * tol:.1f} mm (the nearest to the bound: {1e3 * worst:.3f} mm in front of min z_gt), "
          f"{n_behind} ({100 * n_behind / max(n_checked, 1):.4f} %) deeper than max(z_gt) + {1e3 * tol:.1f} mm")
    assert n_checked > 0.5 * n_hit
    assert n_front == 0, (n_front, worst)

    # two ranks (gloo on this one card): rank 0 collects the chunks with their intrinsics and writes the same renders
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, PI3_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(key, None)
    dist_out = tmp_path / "dist"
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(os.path.dirname(__file__), "render_dist_worker.py"), str(tmp_path), str(dist_out)],
                         env=env, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rec_d, _, n_d, expected_d = _check_files_against_oracle(dist_out, seq, v)
    assert expected_d == expected and abs(n_d - n_voxels) <= 0.001 * n_voxels
    assert np.allclose(np.array([vw["pose"] for vw in rec_d["views"]]), np.array([vw["pose"] for vw in rec["views"]]),
                       atol=1e-5)


def test_online_save_renders_writes_the_same_files(tmp_path):
    from PIL import Image

    from pi3_slam_amd.dense_map import fuse_chunks
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.render import pack_cameras
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
                         bundle_adjust=False, conf_threshold=0.05, dense_voxel_size=0.05)
    slam.process_chunks(paths)
    rd = tmp_path / "online" / "renders"
    n = slam.save_renders(str(rd), every=5, overview=True)
    rec = json.load(open(rd / "cameras.json"))
    assert n == len(rec["views"]) == 4 and [vw["frame"] for vw in rec["views"]] == [f"frame_{i:05d}.png" for i in (0, 5, 10, 15)]
    expected = {"cameras.json", "overview.png"} | {vw["depth"] for vw in rec["views"]} | {vw["color"] for vw in rec["views"]}
    assert set(os.listdir(rd)) == expected and rec["overview"]["ortho"] is True
    fused = fuse_chunks(slam.chunk_reconstructions, DEV, voxel_size=0.05)
    pts, cols, w = fused.points, fused.colors, fused.weights
    poses = np.array([vw["pose"] for vw in rec["views"]])
    Ks = np.array([[[vw["fx"], 0, vw["cx"]], [0, vw["fy"], vw["cy"]], [0, 0, 1]] for vw in rec["views"]])
    H, W = rec["views"][0]["H"], rec["views"][0]["W"]
    exp = ref.render(pts, cols, w, pack_cameras(poses, Ks), H, W, 0.05)
    filled = 0
    for j, vw in enumerate(rec["views"]):
        d16 = np.asarray(Image.open(rd / vw["depth"]))
        assert d16.shape == (H, W) and d16.tobytes() == _u16(exp["depth"][j]).tobytes(), vw["frame"]
        assert np.asarray(Image.open(rd / vw["color"])).tobytes() == exp["color"][j].tobytes()
        filled += int((d16 > 0).sum())
    print(f"online renders: {len(pts)} voxels, {filled} non-empty pixels in {n} views of {H} x {W}")
    assert np.asarray(Image.open(rd / "overview.png")).shape == (H, W, 3)
    slam2 = Pi3SLAMOnline(model=engine, chunk_length=8, overlap=3, device=DEV, keypoint_type="grid", max_num_keypoints=100,
                          estimate_camera_params=True, hip_graph=False, output_dir=str(tmp_path / "o2"), bundle_adjust=False)
    with pytest.raises(RuntimeError):
        slam2.save_renders(str(tmp_path / "o2" / "renders"))
