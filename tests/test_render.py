"""Map renderer, the parts that need no GPU: the numpy oracle (tests/render_ref.py) on a designed scene with derived
bounds and on hand-made cases, the host helpers of pi3_slam_amd/render.py, the C ABI's argument checks, the CLI flags
(off by default) and stage 2 on chunk files without dense clouds."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

import dense_map_ref as dref
import render_ref as ref

sys.path.insert(0, os.path.join(ROOT, "tools"))
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")


def _cam(fx=60.0, fy=60.0, cx=31.5, cy=23.5, ortho=0.0, t=(0.0, 0.0, 0.0)):
    c = np.zeros(20)
    c[0] = c[5] = c[10] = 1.0
    c[3], c[7], c[11] = t
    c[12:17] = fx, fy, cx, cy, ortho
    return c


# ------------------------------------------------------------------------------------------------ the designed scene
PLANE = dict(v=0.02, H=48, W=64, f=60.0, z_plane=(75 + 0.5) * 0.02, z_patch=(40 + 0.5) * 0.02,
             plane_box=(-0.6, 1.0, -0.8, 0.8), patch_box=(-0.2, 0.2, -0.15, 0.15),
             plane_rgb=(10, 200, 30), patch_rgb=(250, 40, 90))


def plane_scene():
    """A plane z = 1.51 m facing the camera and a nearer patch at 0.81 m, both sampled on a lattice of v / 3 and fused
    into voxels of v = 2 cm by the dense-map oracle -> (points, colors, weights, cams (1,20))."""
    s = PLANE
    step = s["v"] / 3.0
    sets = []
    for z, box, rgb in ((s["z_plane"], s["plane_box"], s["plane_rgb"]), (s["z_patch"], s["patch_box"], s["patch_rgb"])):
        xs = np.arange(box[0], box[1] + 0.5 * step, step)
        ys = np.arange(box[2], box[3] + 0.5 * step, step)
        X, Y = np.meshgrid(xs, ys)
        p = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1).astype(np.float32)
        sets.append((p, np.tile(np.array([rgb], np.uint8), (len(p), 1)), None))
    m = dref.fuse_point_sets(sets, s["v"])
    return m["points"], m["colors"], m["weights"], _cam(s["f"], s["f"], (s["W"] - 1) / 2.0, (s["H"] - 1) / 2.0)[None]


def check_plane_scene(out, points, cam):
    """The derived bounds (no measured number).  All samples of a voxel lie on their plane, so its centroid does: every
    drawn depth is the plane's z up to the fixed-point centroid (<= v / 2 is generous).  The layer of occupied voxels is
    complete inside the sampled area (lattice v / 3 < v), neighbouring centroids are at most 2 v apart, so squares of
    half-width v f / z pixels leave no gap: a pixel whose ray meets the plane inside the area, more than the footprint
    + 1 px from its border, is covered."""
    s = PLANE
    H, W, f, v = s["H"], s["W"], s["f"], s["v"]
    depth, color, index = out["depth"][0], out["color"][0], out["index"][0]
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dx, dy = (px - (W - 1) / 2.0) / f, (py - (H - 1) / 2.0) / f          # the ray's x / z, y / z

    def inside(box, z, margin_px):
        m = margin_px * z / f
        X, Y = dx * z, dy * z
        return (X > box[0] + m) & (X < box[1] - m) & (Y > box[2] + m) & (Y < box[3] - m)

    def outside(box, z, margin_px):
        m = margin_px * z / f
        X, Y = dx * z, dy * z
        return (X < box[0] - m) | (X > box[1] + m) | (Y < box[2] - m) | (Y > box[3] + m)

    foot_plane = math.ceil(v * f / s["z_plane"]) + 1
    foot_patch = math.ceil(v * f / s["z_patch"]) + 1
    on_patch = inside(s["patch_box"], s["z_patch"], foot_patch)
    on_plane = inside(s["plane_box"], s["z_plane"], foot_plane) & outside(s["patch_box"], s["z_patch"], foot_patch)
    assert on_patch.sum() > 100 and on_plane.sum() > 800, (on_patch.sum(), on_plane.sum())
    for sel, z, rgb in ((on_patch, s["z_patch"], s["patch_rgb"]), (on_plane, s["z_plane"], s["plane_rgb"])):
        assert (index[sel] >= 0).all(), "an interior pixel is empty"
        assert np.abs(depth[sel].astype(np.float64) - z).max() <= v / 2
        assert (color[sel] == np.array(rgb, np.uint8)).all()
    # index: a voxel whose projection is within its radius of the pixel
    pr = ref.project(points, None, cam[0], H, W, v, 1.0, 1, 0.05, float("inf"))
    hit = index >= 0
    i = index[hit]
    assert (np.abs(pr["u"][i] - px[hit]) <= pr["r"][i]).all() and (np.abs(pr["v"][i] - py[hit]) <= pr["r"][i]).all()
    assert np.array_equal(depth[hit], pr["zc"][i].astype(np.float32))


def test_designed_plane_scene_meets_its_derived_bounds():
    points, colors, weights, cam = plane_scene()
    out = ref.render(points, colors, weights, cam, PLANE["H"], PLANE["W"], PLANE["v"], splat_scale=1.0)
    check_plane_scene(out, points, cam)
    assert out["pixels"] == int((out["index"] >= 0).sum())


# ------------------------------------------------------------------------------------------------ hand-made cases
def test_oracle_filters_min_weight_depth_range_and_non_finite_rows():
    p = np.array([[0, 0, 2.0], [0.5, 0, 2.0], [0, 0, -2.0], [np.nan, 0, 2.0], [0, np.inf, 2.0], [0, 0, 0.04],
                  [-0.5, 0, 9.0], [0, 0.5, 3.0]], np.float32)
    w = np.array([5, 2, 5, 5, 5, 5, 5, 3], np.int32)
    cam = _cam()
    out = ref.render(p, None, w, cam[None], 48, 64, 0.02, min_weight=3, near=0.05, far=8.0)
    drawn = set(np.unique(out["index"][out["index"] >= 0]).tolist())
    assert drawn == {0, 7}          # 1: weight 2 < 3; 2: behind; 3, 4: not finite; 5: zc <= near; 6: zc > far
    assert out["culled"] == 0 and out["clamped"] == 0
    drawn_all = set(np.unique(ref.render(p, None, None, cam[None], 48, 64, 0.02, near=0.05, far=9.0)["index"]).tolist())
    assert drawn_all == {-1, 0, 1, 6, 7}                     # far is inclusive, near exclusive, no weights: all count
    assert 5 in set(np.unique(ref.render(p, None, None, cam[None], 48, 64, 0.02, near=0.0)["index"]).tolist())
    # a voxel in front of the camera but outside the image is culled and counted
    side = np.array([[10.0, 0, 1.0]], np.float32)
    o = ref.render(side, None, None, cam[None], 48, 64, 0.02)
    assert o["culled"] == 1 and o["pixels"] == 0 and (o["depth"] == 0).all() and (o["index"] == -1).all()


def test_oracle_radius_clamps_and_their_counter():
    cam = _cam()
    # r = v f / z: 0.02 * 60 / 0.06 = 20 -> clamped to 16 (counted); / 10 = 0.12 -> raised to 0.5 (not counted)
    p = np.array([[0, 0, 0.06], [0.0, 0.0, 10.0]], np.float32)
    pr = ref.project(p, None, cam, 48, 64, 0.02, 1.0, 1, 0.05, float("inf"))
    assert pr["r"].tolist() == [16.0, 0.5] and pr["clamped"] == 1
    assert (pr["x0"][0], pr["x1"][0], pr["y0"][0], pr["y1"][0]) == (16, 47, 8, 39)      # 31.5 -+ 16, 23.5 -+ 16
    # half-width 0.5 around (31.5, 23.5): ceil(31) .. floor(32)
    assert (pr["x0"][1], pr["x1"][1], pr["y0"][1], pr["y1"][1]) == (31, 32, 23, 24)
    far_only = ref.render(p[1:], None, None, cam[None], 48, 64, 0.02)
    assert far_only["pixels"] == 4 and far_only["clamped"] == 0
    # a projection exactly on a pixel centre with r = 0.5 covers that pixel only
    q = ref.project(np.array([[0.5 / 60.0 * 10.0, 0.5 / 60.0 * 10.0, 10.0]], np.float32), None, cam, 48, 64, 0.02, 1.0, 1,
                    0.05, float("inf"))
    assert abs(q["u"][0] - 32.0) < 1e-5


def test_oracle_orthographic_depth_is_independent_of_lateral_position():
    cam = _cam(fx=20.0, fy=20.0, ortho=1.0)
    p = np.array([[-1.0, -0.5, 3.0], [0.0, 0.0, 3.0], [1.2, 0.7, 3.0], [0.3, 0.2, 5.0]], np.float32)
    pr = ref.project(p, None, cam, 48, 64, 0.05, 1.0, 1, 0.05, float("inf"))
    assert pr["draw"].all()
    assert np.allclose(pr["u"], 20.0 * p[:, 0] + 31.5) and np.allclose(pr["v"], 20.0 * p[:, 1] + 23.5)
    assert (pr["r"] == 1.0).all()                               # s v fx, whatever the depth
    out = ref.render(p, None, None, cam[None], 48, 64, 0.05)
    d = out["depth"][0]
    assert set(np.unique(d).tolist()) == {0.0, 3.0, 5.0}
    for i in range(3):
        assert (d[out["index"][0] == i] == np.float32(3.0)).all() and (out["index"][0] == i).sum() >= 4


def test_oracle_ties_go_to_the_lower_row_and_nearer_wins():
    cam = _cam()
    p = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 1.5], [0.0, 0.0, 2.0]], np.float32)
    out = ref.render(p[[0, 1, 3]], None, None, cam[None], 48, 64, 0.02)
    assert set(np.unique(out["index"]).tolist()) == {-1, 0}     # three voxels at one depth on the same pixels: row 0
    out = ref.render(p, None, None, cam[None], 48, 64, 0.02)
    near = out["index"][0] == 2
    assert near.sum() >= 4 and (out["depth"][0][near] == np.float32(1.5)).all()
    assert not (out["index"][0] == 1).any() and not (out["index"][0] == 3).any()
    # the result does not depend on the order of the rows beyond the tie rule
    rng = np.random.default_rng(1)
    q = np.c_[rng.uniform(-1, 1, (3000, 2)), rng.uniform(1, 4, 3000)].astype(np.float32)
    a = ref.render(q, None, None, cam[None], 48, 64, 0.02)
    perm = rng.permutation(3000)
    b = ref.render(q[perm], None, None, cam[None], 48, 64, 0.02)
    assert np.array_equal(a["depth"], b["depth"])
    hit = b["index"] >= 0
    assert np.array_equal(q[perm][b["index"][hit]][:, 2], q[a["index"][hit]][:, 2])


def test_oracle_slabs_do_not_change_the_image():
    rng = np.random.default_rng(2)
    q = np.c_[rng.uniform(-1, 1, (2000, 2)), rng.uniform(0.5, 4, 2000)].astype(np.float32)
    a, _, _ = ref.splat_one(q, None, _cam(), 48, 64, 0.02)
    b, _, _ = ref.splat_one(q, None, _cam(), 48, 64, 0.02, max_elems=97)
    assert np.array_equal(a, b)
    # ... and equal a plain per-voxel loop over the footprints
    pr = ref.project(q, None, _cam(), 48, 64, 0.02, 1.0, 1, 0.05, float("inf"))
    z = np.full((48, 64), ref.EMPTY, np.uint64)
    for i in np.flatnonzero(pr["draw"]):
        val = (np.uint64(np.float32(pr["zc"][i]).view(np.uint32)) << np.uint64(32)) | np.uint64(i)
        blk = z[pr["y0"][i]:pr["y1"][i] + 1, pr["x0"][i]:pr["x1"][i] + 1]
        np.minimum(blk, val, out=blk)
    assert np.array_equal(a, z)


# ------------------------------------------------------------------------------------------------ host helpers
def _pose(rotvec, c):
    from scipy.spatial.transform import Rotation
    P = np.eye(4)
    P[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix()
    P[:3, 3] = c
    return P


def test_pack_cameras_inverts_the_pose_and_removes_a_scale():
    from pi3_slam_amd.render import pack_cameras
    P = np.stack([_pose([0.3, -0.2, 0.5], [1.0, 2.0, -0.5]), _pose([0.0, 1.0, 0.1], [-3.0, 0.2, 0.7])])
    K = np.array([[370.0, 0, 202.5], [0, 371.0, 153.5], [0, 0, 1]])
    cams = pack_cameras(P, K)
    assert cams.shape == (2, 20) and cams.dtype == np.float64
    for m in range(2):
        w2c = np.eye(4)
        w2c[:3] = cams[m, :12].reshape(3, 4)
        assert np.allclose(w2c @ P[m], np.eye(4), atol=1e-12)
        assert cams[m, 12:17].tolist() == [370.0, 371.0, 202.5, 153.5, 0.0] and (cams[m, 17:] == 0).all()
    # a similarity of scale 1.3 applied to the pose: the same camera as the rigid pose with the centre moved
    S = np.eye(4)
    S[:3, :3] = 1.3 * _pose([0.1, 0.2, -0.4], [0, 0, 0])[:3, :3]
    S[:3, 3] = [0.5, -1.0, 2.0]
    rigid = P.copy()
    rigid[:, :3, :3] = (S[:3, :3] / 1.3) @ P[:, :3, :3]
    rigid[:, :3, 3] = P[:, :3, 3] @ S[:3, :3].T + S[:3, 3]
    assert np.allclose(pack_cameras(S @ P, K), pack_cameras(rigid, K), atol=1e-12)
    # per-view intrinsics, a single pose, the orthographic flag
    Ks = np.stack([K, 2 * K])
    assert pack_cameras(P, Ks)[1, 12] == 740.0
    assert pack_cameras(P[0], K, ortho=True)[0, 16] == 1.0 and pack_cameras(P, K, ortho=[False, True])[:, 16].tolist() == [0, 1]
    with pytest.raises(ValueError):
        pack_cameras(np.diag([1.0, 1.0, -1.0, 1.0]), K)


def test_overview_camera_contains_every_camera_centre_and_looks_down():
    from pi3_slam_amd.render import overview_camera, pack_cameras
    import synth_sequence as ss
    P = ss.load_tum_poses(GT)[::7]
    rng = np.random.default_rng(0)
    lo, hi = P[:, :3, 3].min(0) - 1.2, P[:, :3, 3].max(0) + 1.2
    pts = rng.uniform(lo, hi, (20000, 3))
    pts[::100] = np.nan                                   # the map may carry non-finite rows
    H, W = 308, 406
    pose, K = overview_camera(P, pts, H, W, near=0.05)
    assert np.allclose(pose[:3, :3].T @ pose[:3, :3], np.eye(3), atol=1e-12) and np.linalg.det(pose[:3, :3]) > 0
    assert K[0, 0] == K[1, 1] > 0                          # isotropic
    down = P[:, :3, 1].mean(0)
    assert pose[:3, 2] @ down / np.linalg.norm(down) > 0.999
    cam = pack_cameras(pose, K, ortho=True)
    pr = ref.project(P[:, :3, 3].astype(np.float32), None, cam[0], H, W, 0.02, 1.0, 1, 0.05, float("inf"))
    assert pr["draw"].all() and pr["culled"] == 0           # every centre: beyond the near plane and inside the image
    assert (pr["u"] >= 0).all() and (pr["u"] <= W - 1).all() and (pr["v"] >= 0).all() and (pr["v"] <= H - 1).all()
    assert pr["zc"].min() == pytest.approx(0.1, abs=1e-5)  # near + margin above the highest camera
    # the 1st-99th percentile box of the map is inside the frame too
    q = ref.project(pts[np.isfinite(pts).all(1)].astype(np.float32), None, cam[0], H, W, 0.02, 1.0, 1, -1.0, float("inf"))
    u, v = q["u"], q["v"]
    assert np.mean((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)) >= 0.95


def test_depth_png_round_trip_millimetres_saturation_and_empty(tmp_path):
    from PIL import Image

    from pi3_slam_amd.render import depth_to_u16, write_color_png, write_depth_png
    d = np.array([[0.0, 1.2344, 1.2346, 65.534], [65.5354, 70.0, 0.0004, 2.0005]], np.float32)
    path = str(tmp_path / "d.png")
    write_depth_png(d, path)
    im = Image.open(path)
    assert im.mode in ("I;16", "I;16L", "I;16B", "I")
    got = np.asarray(im).astype(np.int64)
    assert got.tolist() == [[0, 1234, 1235, 65534], [65535, 65535, 0, int(np.rint(np.float64(np.float32(2.0005)) * 1000))]]
    assert np.array_equal(got, depth_to_u16(d).astype(np.int64))
    assert np.abs(got / 1000.0 - np.where(d > 65.535, 65.535, d)).max() <= 0.5e-3 + 1e-9       # millimetre rounding
    assert depth_to_u16(np.array([[np.nan, np.inf, -1.0]])).tolist() == [[0, 0, 0]]
    write_depth_png(d, str(tmp_path / "cm.png"), scale=100.0)
    assert np.asarray(Image.open(str(tmp_path / "cm.png")))[0, 1] == 123
    c = np.arange(2 * 4 * 3, dtype=np.uint8).reshape(2, 4, 3)
    write_color_png(c, str(tmp_path / "c.png"))
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "c.png"))), c)


def test_default_batch_keeps_the_z_buffers_within_the_stated_bytes():
    from pi3_slam_amd.render import ZBUF_BATCH_BYTES, default_batch
    n = default_batch(1000, 308, 406)
    assert 1 < n < 1000 and n * 308 * 406 * 8 <= ZBUF_BATCH_BYTES < (n + 1) * 308 * 406 * 8
    assert default_batch(3, 308, 406) == 3 and default_batch(5, 4000, 4000) == 1


# ------------------------------------------------------------------------------------------------ ABI, CLI, stage 2
def test_header_declares_and_library_exports_render_entries(built_lib):
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dll = ctypes.CDLL(built_lib)
    from pi3_slam_amd import lib
    for name in ("pi3_render_splat", "pi3_render_resolve"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(dll, name), name
        assert name in lib.SIGNATURES, name
    assert lib.load(require_gpu=False).pi3_abi_version() == 7


def test_render_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    from pi3_slam_amd import lib
    dll = lib.load(require_gpu=False)
    p = ctypes.c_void_p(16)
    inf = float("inf")
    good = dict(points=p, weights=None, V=10, cams=p, M=1, H=4, W=4, v=0.02, s=1.0, mw=1, near=0.05, far=inf, zbuf=p,
                stats=p)

    def splat(**kw):
        a = dict(good, **kw)
        return dll.pi3_render_splat(a["points"], a["weights"], a["V"], a["cams"], a["M"], a["H"], a["W"], a["v"], a["s"],
                                    a["mw"], a["near"], a["far"], a["zbuf"], a["stats"], None)

    for bad in (dict(points=None), dict(cams=None), dict(zbuf=None), dict(stats=None), dict(V=-1), dict(V=1 << 31),
                dict(M=0), dict(H=0), dict(W=-3), dict(v=0.0), dict(v=inf), dict(v=float("nan")), dict(s=0.0),
                dict(s=inf), dict(near=-0.1), dict(near=float("nan")), dict(far=float("nan")), dict(M=70000)):
        assert splat(**bad) == -1, bad
    assert b"pi3_render_splat" in dll.pi3_last_error()
    assert dll.pi3_render_resolve(None, p, 10, 1, 4, 4, p, p, p, p, None) == -1
    assert dll.pi3_render_resolve(p, None, 10, 1, 4, 4, p, p, p, p, None) == -1
    assert dll.pi3_render_resolve(p, p, 1 << 31, 1, 4, 4, p, p, p, p, None) == -1
    assert dll.pi3_render_resolve(p, p, 10, 1, 0, 4, p, p, p, p, None) == -1
    assert dll.pi3_render_resolve(p, p, 10, 1, 4, 4, None, p, p, p, None) == -1
    assert dll.pi3_render_resolve(p, p, 10, 1, 4, 4, p, p, p, None, None) == -1
    assert b"pi3_render_resolve" in dll.pi3_last_error()


def test_cli_render_flags_parse_and_default_to_off():
    from pi3_slam_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert a.render_every is None and a.render_overview is False
    assert a.render_min_weight == 1 and a.render_splat_scale == 1.0
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o", "--render-every", "50", "--render-overview",
                      "--render-min-weight", "3", "--render-splat-scale", "0.75"])
    assert a.render_every == 50 and a.render_overview is True
    assert a.render_min_weight == 3 and a.render_splat_scale == 0.75
    assert p.parse_args(["online", "--output_path", "o"]).render_every is None
    assert p.parse_args(["online", "--output_path", "o", "--render_every", "10"]).render_every == 10


def test_reconstructor_render_options_default_to_off_and_are_checked(tmp_path):
    import inspect

    from pi3_slam_amd.reconstructor import OfflineReconstructor
    sig = inspect.signature(OfflineReconstructor.__init__).parameters
    assert sig["render_every"].default is None and sig["render_overview"].default is False
    with pytest.raises(ValueError):
        OfflineReconstructor(str(tmp_path), str(tmp_path / "o"), device="cpu", render_every=0)


def test_stage_two_without_dense_clouds_writes_no_renders(tmp_path, capsys):
    import synth_sequence as ss
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_NONE), n_frames=80)
    ss.write_chunks_sparse(seq, str(tmp_path))
    assert len(seq.chunks) == 1                              # one chunk: nothing to align, no kernel is needed
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), device="cpu", bundle_adjust=False, render_every=10,
                               render_overview=True)
    rec.run()
    assert os.path.exists(tmp_path / "out" / "trajectory_tum.txt")
    assert not os.path.exists(tmp_path / "out" / "renders") and not os.path.exists(tmp_path / "out" / "dense_points.ply")
    assert "no renders" in capsys.readouterr().out
    from pi3_slam_amd import export
    views = export.render_views(rec.reconstructions)
    assert len(views) == 80 and views[0]["H"] == seq.H and views[0]["W"] == seq.W
    assert views[3]["K"][0, 2] == seq.W // 2 - 0.5 == seq.cx and views[3]["K"][1, 2] == seq.H // 2 - 0.5 == seq.cy


def test_product_does_not_import_the_render_oracle():
    for sub in ("pi3_slam_amd", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith(".py"):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+(tests\.)?render_ref\b", src, flags=re.M), f
