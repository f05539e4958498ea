"""Carving the fused dense map with depth keyframes, without a GPU: what the numpy oracle (tests/dense_carve_ref.py)
does on the analytic plane scene, MapCarver's validation and view list, the options' defaults and flags, and the new
entry points' declarations and argument checks."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_carve_ref as ref
import dense_consistency_ref as cref
import dense_map_ref as mref

REL_TOL = 0.03
# (N, H, W, voxel, S, K)
CONFIGS = [(12, 64, 80, 0.05, 1, 1), (12, 64, 80, 0.05, 2, 1), (12, 64, 80, 0.05, 2, 2), (16, 77, 101, 0.04, 2, 2),
           (16, 77, 101, 0.04, 4, 3), (5, 24, 40, 0.1, 2, 1)]
PLANE_N = np.array([0.15, -0.1, -1.0]) / np.linalg.norm([0.15, -0.1, -1.0])      # plane_scene's plane n . x = d
PLANE_D = -3.0


@functools.lru_cache(maxsize=None)
def floater_scene(N, H, W, voxel):
    """plane_scene with 0.2 % depth noise and the middle rectangle pulled to half depth in two frames (one for N = 5),
    every pixel fused -> (scene, map rows, distance of every voxel to the plane); never modified."""
    s = cref.plane_scene(N, H, W, seed=0, noise_rel=0.002)
    rows, cols = slice(H // 3, 2 * H // 3), slice(W // 3, 2 * W // 3)
    for f in ([2] if N == 5 else [N // 2 - 1, N // 2 + 1]):
        cref.scale_block(s, f, rows, cols, 0.5)
    m = mref.fuse_pixels(s["points"], None, None, None, 0.5, voxel)
    dist = np.abs(m["points"].astype(np.float64) @ PLANE_N - PLANE_D)
    for v in list(s.values()) + [m["points"], m["keys"], dist]:
        v.setflags(write=False)
    return s, m, dist


def scene_views(s, S, K, scale=1.0):
    """The keyframes of the scene: (views (M,20), planes fp16 (M,H',W') = the local z of the frames 0, K, ..)."""
    planes = np.ascontiguousarray(s["local_points"][::K, ::S, ::S, 2]).astype(np.float16)
    return ref.pack_views(s["poses"][::K], s["fxfycxcy"][::K], scale), planes


@pytest.mark.parametrize("min_conflicts", [1, 2, 3])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%dx%d_v%g_S%d_K%d" % c)
def test_oracle_carves_the_floaters_and_nothing_of_the_plane(cfg, min_conflicts):
    """With seed 0: 206 floater voxels at 12 x 64 x 80, 336 at 16 x 77 x 101, 29 at 5 x 24 x 40; no voxel lies between
    6 cm and 0.5 m from the plane.  These are this oracle's own counts on plane_scene(seed=0) (an earlier
    prototype, whose seed is not recorded, counted 206, 330 and 41); what is asserted here are the conditions, and where a later test names 336 it
    is this count."""
    N, H, W, voxel, S, K = cfg
    s, m, dist = floater_scene(N, H, W, voxel)
    views, planes = scene_views(s, S, K)
    r = ref.carve(m["points"], views, planes, S, REL_TOL, voxel, min_conflicts)
    on_plane, floater = dist < 0.06, dist > 0.5
    print(f"{cfg} min_conflicts {min_conflicts}: {len(dist)} voxels, {int(floater.sum())} floaters, "
          f"{r['stats']['carved']} carved, {r['stats']['unvoted']} without a vote")
    assert int(floater.sum()) > 0
    assert int(r["conflict"][on_plane].sum()) == 0              # not a single conflict vote near the plane
    assert not r["carved"][on_plane].any()
    assert r["carved"][floater].all()
    assert not r["carved"][~floater].any()
    assert r["stats"] == {"voxels": len(dist), "carved": int(floater.sum()),
                          "unvoted": int(((r["agree"] + r["conflict"]) == 0).sum())}


def test_more_conflicts_than_views_or_empty_planes_carve_nothing():
    N, H, W, voxel, S, K = CONFIGS[2]
    s, m, dist = floater_scene(N, H, W, voxel)
    views, planes = scene_views(s, S, K)
    r = ref.carve(m["points"], views, planes, S, REL_TOL, voxel, len(views) + 1)
    assert r["conflict"].max() <= len(views) and not r["carved"].any() and r["conflict"].any()
    z = ref.carve(m["points"], views, np.zeros_like(planes), S, REL_TOL, voxel, 1)
    assert not z["agree"].any() and not z["conflict"].any() and not z["carved"].any()
    assert z["stats"] == {"voxels": len(dist), "carved": 0, "unvoted": len(dist)}


def test_pixel_stride_is_honoured():
    """A stride-2 plane read as if it were stride 1 looks at the wrong pixels: the votes change."""
    N, H, W, voxel, _, K = CONFIGS[1]
    s, m, dist = floater_scene(N, H, W, voxel)
    views, planes = scene_views(s, 2, K)
    right = ref.carve(m["points"], views, planes, 2, REL_TOL, voxel, 2)
    wrong = ref.carve(m["points"], views, planes, 1, REL_TOL, voxel, 2)
    assert right["carved"][dist > 0.5].all()
    assert not np.array_equal(right["agree"], wrong["agree"])


def _gauged_chunk(s, S, K, gauge, with_planes=True):
    """The scene as a chunk would carry it after stage 2: expressed in a frame scaled by `gauge` (and rotated, moved),
    brought back by the inverse similarity.  camera_poses are the final poses (similarity . chunk pose, fp32)."""
    N = len(s["poses"])
    a = 0.3
    Rg = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    tg = np.array([0.5, -0.25, 1.0])
    F = np.eye(4)                       # world -> chunk frame
    F[:3, :3], F[:3, 3] = gauge * Rg, tg
    G = np.linalg.inv(F)                # the chunk's transform: chunk frame -> world, scale 1 / gauge
    P = s["poses"].astype(np.float64)
    Pc = P.copy()                       # rigid poses in the chunk frame
    Pc[:, :3, :3] = Rg @ P[:, :3, :3]
    Pc[:, :3, 3] = (gauge * (Rg @ P[:, :3, 3].T)).T + tg
    final = (G[None] @ Pc).astype(np.float32)
    chunk = {"camera_poses": torch.from_numpy(final), "_sim3_global": None if gauge == 1.0 else torch.from_numpy(G)}
    if with_planes:
        z = np.ascontiguousarray(s["local_points"][::K, ::S, ::S, 2]).astype(np.float64) * gauge
        chunk["dense_depth"] = {"depth": torch.from_numpy(z.astype(np.float16)),
                                "frames": torch.arange(0, N, K, dtype=torch.int32), "pixel_stride": S,
                                "height": s["points"].shape[1], "width": s["points"].shape[2],
                                "fxfycxcy": torch.from_numpy(s["fxfycxcy"][::K].copy())}
    return chunk


def test_depth_scale_and_view_list_of_a_gauged_chunk():
    """The same scene in a gauge scaled by 1.7 and rotated, with the inverse similarity as its chunk transform, carves
    the same voxels; MapCarver.chunk_views builds the rows (rigid world->camera, the planes' intrinsics, the scale)."""
    from pi3_slam_amd.dense_map import MapCarver
    N, H, W, voxel, S, K = CONFIGS[3]
    s, m, dist = floater_scene(N, H, W, voxel)
    out = []
    for gauge in (1.0, 1.7):
        chunk = _gauged_chunk(s, S, K, gauge)
        views, planes, stride = MapCarver.chunk_views([chunk, {"camera_poses": chunk["camera_poses"]}])
        assert views.shape == (len(range(0, N, K)), 20) and views.dtype == np.float64 and stride == S
        assert planes.dtype == torch.float16 and tuple(planes.shape) == (len(views), -(-H // S), -(-W // S))
        assert np.allclose(views[:, ref.SCALE_AT], 1.0 / gauge, rtol=1e-12, atol=0)
        exp = ref.pack_views(s["poses"][::K], s["fxfycxcy"][::K], 1.0 / gauge)
        assert np.abs(views - exp).max() < 1e-5                 # the final poses went through fp32
        R = views[:, :12].reshape(-1, 3, 4)[:, :, :3]
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6       # the scale is divided out
        r = ref.carve(m["points"], views, planes.numpy(), stride, REL_TOL, voxel, 2)
        assert r["carved"][dist > 0.5].all() and not r["carved"][dist <= 0.5].any()
        out.append(set(m["keys"][r["carved"]].tolist()))
    assert out[0] == out[1] and len(out[0]) == 336
    # read without its scale, the gauged chunk's planes are 1.7 x too deep: every view looks through the whole map
    views[:, ref.SCALE_AT] = 1.0
    bad = ref.carve(m["points"], views, planes.numpy(), stride, REL_TOL, voxel, 2)
    assert bad["carved"].sum() > 10 * len(out[0])


def test_view_list_two_chunks_refusals_and_no_planes():
    from pi3_slam_amd.dense_map import MapCarver
    N, H, W, voxel, S, K = CONFIGS[2]
    s, _, _ = floater_scene(N, H, W, voxel)
    a, b = _gauged_chunk(s, S, K, 1.0), _gauged_chunk(s, S, K, 1.7)
    views, planes, stride = MapCarver.chunk_views([a, b])
    M = len(range(0, N, K))
    assert views.shape == (2 * M, 20) and tuple(planes.shape) == (2 * M, H // S, W // S)      # not de-duplicated
    assert np.allclose(views[:M, ref.SCALE_AT], 1.0) and np.allclose(views[M:, ref.SCALE_AT], 1 / 1.7)
    with pytest.raises(ValueError, match="differing size or stride"):
        MapCarver.chunk_views([a, _gauged_chunk(s, 1, K, 1.0)])
    other = _gauged_chunk(s, S, K, 1.0)
    other["dense_depth"]["pixel_stride"] = 4                    # the same H' x W', another stride
    with pytest.raises(ValueError, match="differing size or stride"):
        MapCarver.chunk_views([a, other])
    views, planes, _ = MapCarver.chunk_views([_gauged_chunk(s, S, K, 1.0, with_planes=False)])
    assert views.shape == (0, 20) and planes is None


def test_depth_plane_oracle_rounding_and_holes():
    """fp16 nearest-even; what rounds to 0 or inf, and every non-candidate, is 0; odd sizes round H / S up."""
    lp = np.zeros((3, 3, 5, 3), np.float32)
    lp[..., 2] = 1.0
    pts = np.ones_like(lp)
    lp[0, 0, 0, 2] = 2049.0          # halfway between 2048 and 2050: to even
    lp[0, 0, 2, 2] = 2051.0          # halfway between 2050 and 2052: to even
    lp[0, 0, 4, 2] = 70000.0         # rounds to inf
    lp[0, 2, 0, 2] = 65519.0         # the largest value that still rounds to 65504
    lp[0, 2, 2, 2] = 2.0 ** -26      # rounds to 0
    lp[0, 2, 4, 2] = 2.0 ** -24      # the smallest subnormal
    lp[2, 0, 0, 2] = -1.0
    lp[2, 0, 2, 2] = np.nan
    pts[2, 0, 4, 1] = np.inf
    conf = np.zeros((3, 3, 5), np.float32)
    conf[2, 2, 0] = -1.0
    masks = np.ones((3, 3, 5), np.uint8)
    masks[2, 2, 2] = 0
    d, n = ref.depth_planes(pts, lp, conf, masks, -0.5, 2, 2)
    assert d.dtype == np.float16 and d.shape == (2, 2, 3)
    assert d[0].astype(np.float64).tolist() == [[2048.0, 2052.0, 0.0], [65504.0, 0.0, 2.0 ** -24]]
    assert d[1].astype(np.float64).tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    assert n == 5
    d1, n1 = ref.depth_planes(pts, lp, None, None, 0.0, 1, 4)
    assert d1.shape == (3, 1, 2) and d1.astype(np.float64).reshape(3, 2).tolist() == [[2048.0, 0.0], [1.0, 1.0], [0.0, 0.0]]
    assert n1 == 3


def test_map_carver_validates_and_reports():
    from pi3_slam_amd.dense_map import MapCarver
    c = MapCarver(3)
    assert c.settings() == {"min_conflicts": 3, "rel_tol": 0.03} and MapCarver.MARGIN_VOXELS == 1.0
    assert MapCarver(2.0, 0.05).settings() == {"min_conflicts": 2, "rel_tol": 0.05}
    for bad in (0, -1, 1.5, True, "3", None, 1 << 31):
        with pytest.raises((ValueError, TypeError)):
            MapCarver(bad)
    for tol in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="rel_tol"):
            MapCarver(2, tol)
    assert MapCarver.from_options() is None and MapCarver.from_options(None, 0.1) is None
    assert MapCarver.from_options(4, 0.02).settings() == {"min_conflicts": 4, "rel_tol": 0.02}
    c.last_stats = {"views": 7, "voxels": 100, "carved": 5, "unvoted": 2}
    line = c.summary()
    assert "7 views" in line and "5 of 100" in line and "2 voxels no view voted on" in line


def test_everything_is_off_by_default(tmp_path, capsys):
    from pi3_slam_amd.chunk_creator import OfflineCreatorConfig
    from pi3_slam_amd.cli import build_parser
    from pi3_slam_amd.dense_map import ChunkCloudBuilder, MapCleaner, fuse_chunks
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    from pi3_slam_amd import export
    cfg = OfflineCreatorConfig("recipe", str(tmp_path))
    assert cfg.dense_depth_every is None and cfg.dense_depth_stride == 2
    p = build_parser()
    a = p.parse_args(["create", "--images", "x", "--output", "o"])
    assert a.dense_depth_every is None and a.dense_depth_stride == 2
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert a.dense_carve_min_conflicts is None and a.dense_carve_tolerance == 0.03
    a = p.parse_args(["online", "--output_path", "o"])
    assert a.dense_depth_every is None and a.dense_depth_stride == 2
    assert a.dense_carve_min_conflicts is None and a.dense_carve_tolerance == 0.03
    sig = inspect.signature(Pi3SLAMOnline.__init__).parameters
    assert sig["dense_depth_every"].default is None and sig["dense_depth_stride"].default == 2
    assert sig["dense_carve_min_conflicts"].default is None and sig["dense_carve_tolerance"].default == 0.03
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"))
    assert rec.dense_carver is None and rec.dense_cleaner is None
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), dense_carve_min_conflicts=3)
    assert rec.dense_carver.settings() == {"min_conflicts": 3, "rel_tol": 0.03} and rec.dense_cleaner is None
    # trailing keywords, None by default
    for fn, name in ((export.write_outputs, "dense_carver"), (export.write_renders, "dense_carver")):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == name and params[-1].default is None, fn.__name__
    params = inspect.signature(fuse_chunks).parameters
    for name in ("cleaner", "carver", "mesher"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None, name
    assert list(inspect.signature(MapCleaner.apply).parameters)[-1] == "exclude"
    # the creator's options need the dense map
    capsys.readouterr()
    cfg.dense_depth_every = 2
    assert ChunkCloudBuilder.from_config(cfg, "cpu") is None
    said = capsys.readouterr().out
    assert said.count("dense_depth_every has no effect without dense_voxel_size") == 1
    from pi3_slam_amd.dist import COLLECT_KEYS
    assert "dense_depth" in COLLECT_KEYS


def test_builder_refuses_bad_depth_options_before_it_touches_a_device():
    from pi3_slam_amd.dense_map import ChunkCloudBuilder
    for every in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="dense_depth_every"):
            ChunkCloudBuilder(0.02, 0.5, "cpu", depth_every=every)
    for stride in (0, 3, 8, True, 2.5):
        with pytest.raises(ValueError, match="dense_depth_stride"):
            ChunkCloudBuilder(0.02, 0.5, "cpu", depth_every=2, depth_stride=stride)


def test_flags_parse():
    from pi3_slam_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["create", "--images", "x", "--output", "o", "--dense-voxel-size", "0.02", "--dense-depth-every", "2",
                      "--dense-depth-stride", "4"])
    assert a.dense_depth_every == 2 and a.dense_depth_stride == 4
    with pytest.raises(SystemExit):
        p.parse_args(["create", "--images", "x", "--output", "o", "--dense-depth-stride", "3"])
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o", "--dense-carve-min-conflicts", "3",
                      "--dense-carve-tolerance", "0.05", "--no-bundle-adjust"])
    assert a.dense_carve_min_conflicts == 3 and a.dense_carve_tolerance == 0.05 and a.no_bundle_adjust
    a = p.parse_args(["online", "--output_path", "o", "--dense_voxel_size", "0.05", "--dense_depth_every", "3",
                      "--dense_depth_stride", "1", "--dense_carve_min_conflicts", "2", "--dense_carve_tolerance", "0.04"])
    assert (a.dense_depth_every, a.dense_depth_stride, a.dense_carve_min_conflicts, a.dense_carve_tolerance) == (3, 1, 2, 0.04)
    text = p._subparsers._group_actions[0].choices["reconstruct"].format_help()
    assert "starting point" in re.sub(r"\s+", " ", text.split("--dense-carve-min-conflicts")[2])


def test_online_takes_the_dense_flags_of_create_and_reconstruct_respelled():
    """One table, two spellings: every --dense-* flag of create or reconstruct except --dense-conf-threshold (online
    has --conf_threshold for it) is a flag of online with underscores and the same type, default and choices; and no
    help text names a dense flag in the other commands' spelling."""
    from pi3_slam_amd.cli import build_parser
    sub = build_parser()._subparsers._group_actions[0].choices

    def dense(cmd):
        return {a.option_strings[0]: a for a in sub[cmd]._actions if a.option_strings[0].startswith("--dense")}
    online = dense("online")
    hyphened = {**dense("create"), **dense("reconstruct")}
    assert len(hyphened) == len(dense("create")) + len(dense("reconstruct")) == 16
    assert "--dense-conf-threshold" in hyphened and "--dense_conf_threshold" not in online
    del hyphened["--dense-conf-threshold"]
    assert {"--" + f[2:].replace("-", "_") for f in hyphened} == set(online)
    for flag, a in hyphened.items():
        b = online["--" + flag[2:].replace("-", "_")]
        assert (type(a), a.dest, a.type, a.default, a.choices, a.nargs) == \
            (type(b), b.dest, b.type, b.default, b.choices, b.nargs), flag
        assert a.help and b.help
    for cmd, wrong in (("online", r"--dense-"), ("create", r"--dense_"), ("reconstruct", r"--dense_")):
        for a in sub[cmd]._actions:
            assert not re.search(wrong, a.help or ""), (cmd, a.option_strings, a.help)


def test_new_symbols_are_declared_bound_and_refuse_bad_arguments(built_lib):
    from conftest import ROOT
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dll = lib.load(require_gpu=False)
    assert dll.pi3_abi_version() == 7
    names = ("pi3_dense_depth_planes", "pi3_voxel_carve", "pi3_voxel_support_excluding")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and name in lib.SIGNATURES and hasattr(dll, name), name
    buf = (C.c_ulonglong * 64)()                 # a host address: every call below must be refused before any launch
    p = C.addressof(buf)
    inf, nan = float("inf"), float("nan")
    bad = {
        "pi3_dense_depth_planes": [
            (None,) * 4 + (0, 0, 0, 0.0, 0, 0, None, None, None),
            (None, p, None, None, 1, 4, 4, 0.0, 1, 1, p, p, None), (p, None, None, None, 1, 4, 4, 0.0, 1, 1, p, p, None),
            (p, p, None, None, 1, 4, 4, 0.0, 1, 1, None, p, None), (p, p, None, None, 1, 4, 4, 0.0, 1, 1, p, None, None),
            (p, p, None, None, -1, 4, 4, 0.0, 1, 1, p, p, None), (p, p, None, None, 1, 0, 4, 0.0, 1, 1, p, p, None),
            (p, p, None, None, 1, 4, 0, 0.0, 1, 1, p, p, None), (p, p, None, None, 1, 4, 4, 0.0, 0, 1, p, p, None),
            (p, p, None, None, 1, 4, 4, 0.0, 1, 0, p, p, None), (p, p, None, None, 1, 4, 4, 0.0, 1, 3, p, p, None),
            (p, p, None, None, 1, 4, 4, 0.0, 1, 8, p, p, None),
            (p, p, None, None, 1 << 11, 1 << 10, 1 << 10, 0.0, 1, 1, p, p, None)],        # N H W >= 2^31
        "pi3_voxel_carve": [
            (None, 0, 0.0, None, 0, None, 0, 0, 0, 0.0, 0.0, 0, None, None, None, None, None),
            (None, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 48, 0.1, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.0, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, inf, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, None, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, None, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, -1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 0, 4, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 0, 2, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 3, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 0, 0.03, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.0, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, nan, 0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, -0.1, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, inf, 1, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, 0.1, 0, p, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, None, None, None, p, None),
            (p, 64, 0.1, p, 1, p, 4, 4, 2, 0.03, 0.1, 1, p, None, None, None, None)],
        "pi3_voxel_support_excluding": [
            (None, 0, 0, 0, 0, None, None, None, None, None),
            (None, 64, 1, 1, 0, p, None, p, p, None), (p, 48, 1, 1, 0, p, None, p, p, None),
            (p, 64, 1, 3, 0, p, None, p, p, None), (p, 64, 1, 1, 27, p, None, p, p, None),
            (p, 64, 1, 1, -1, p, None, p, p, None), (p, 64, 1, 1, 0, None, None, p, p, None),
            (p, 64, 1, 1, 0, p, None, None, p, None), (p, 64, 1, 1, 0, p, None, p, None, None)],
    }
    for name, cases in bad.items():
        fn = getattr(dll, name)
        for args in cases:
            assert len(args) == len(lib.SIGNATURES[name])
            assert fn(*args) < 0, (name, args)
            assert name.encode() in dll.pi3_last_error()
