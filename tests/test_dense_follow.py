"""The dense map following bundle-adjusted poses, without a GPU: the numpy oracle (tests/dense_follow_ref.py) on
hand-worked cases, MapFollower's moves, the options' defaults and flags, and the new entry point's declaration and
argument checks."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_carve_ref as cref
import dense_follow_ref as ref

HP, WP = 12, 16
K = np.array([10.0, 10.0, 8.0, 6.0])            # a point on the axis at depth z lands on pixel (8, 6)


def rigid(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    D = np.zeros((3, 4))
    D[:, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    D[:, 3] = t
    return D


def camera(pose=None, scale=1.0):
    return cref.pack_views(np.eye(4)[None] if pose is None else np.asarray(pose)[None], K[None], scale)[0]


def plane(depth):
    return np.full((HP, WP), depth, np.float16)


def run(points, views, moves, planes, normals=None, stride=1, rel_tol=0.03, margin=0.01):
    return ref.follow(np.asarray(points, np.float32), normals, np.stack(views), np.stack(moves).reshape(-1, 12),
                      np.stack(planes), stride, rel_tol, margin)


def test_one_point_one_view_is_moved_by_that_view():
    D = rigid(0.5, [1.0, -2.0, 0.25])
    X = np.array([[0.25, -0.5, 2.0]], np.float32)           # zc = 2: w = 1/4, exact
    n = np.array([[0.0, 0.6, -0.8]], np.float32)
    r = run(X, [camera()], [D], [plane(2.0)], normals=n)
    exp = D[:, :3] @ X[0].astype(np.float64) + D[:, 3]
    assert r["points"].dtype == np.float32 and r["points"].tobytes() == exp.astype(np.float32)[None].tobytes()
    Rn = D[:, :3] @ n[0].astype(np.float64)
    assert np.abs(r["normals"][0] - Rn / np.linalg.norm(Rn)).max() < 1e-7
    assert r["level"].tolist() == [1] and r["support"].tolist() == [1] and r["counters"].tolist() == [0, 1, 0, 0]


def test_a_point_follows_the_view_that_agrees_with_it_only():
    Da, Db = rigid(0.1, [0.0, 0.0, 1.0]), rigid(-0.7, [5.0, 5.0, 5.0])
    X = np.array([[0.0, 0.0, 2.0]], np.float32)
    r = run(X, [camera(), camera()], [Da, Db], [plane(2.0), plane(5.0)])
    assert r["points"].tobytes() == np.array([[0.0, 0.0, 3.0]], np.float32).tobytes()
    assert r["level"].tolist() == [1] and r["support"].tolist() == [1]
    # both agree: the mean (equal depths, equal weights)
    both = run(X, [camera(), camera()], [Da, Db], [plane(2.0), plane(2.0)])
    mean = 0.5 * ((Da[:, :3] @ [0, 0, 2.0] + Da[:, 3]) + (Db[:, :3] @ [0, 0, 2.0] + Db[:, 3]))
    assert np.abs(both["points"][0] - mean).max() < 1e-6 and both["support"].tolist() == [2]
    # the tolerance is rel_tol zo + margin, inclusive
    edge = run(X, [camera()], [Da], [plane(1.875)], rel_tol=0.0625, margin=0.0078125)
    assert edge["level"].tolist() == [1]                     # |2 - 1.875| = 0.125 = 0.0625 * 1.875 + 0.0078125
    out = run(X, [camera()], [Da], [plane(1.875)], rel_tol=0.0625, margin=0.0078124)
    assert out["level"].tolist() == [2]


def test_depth_zero_or_not_finite_in_the_plane_is_level_two():
    Da, Db = rigid(0.1, [0.0, 0.0, 1.0]), rigid(0.0, [1.0, 0.0, 0.0])
    X = np.array([[0.0, 0.0, 2.0]], np.float32)
    for hole in (0.0, np.inf, np.nan):
        r = run(X, [camera()], [Da], [plane(hole)])
        assert r["level"].tolist() == [2] and r["support"].tolist() == [0] and r["counters"].tolist() == [0, 0, 1, 0]
        assert r["points"].tobytes() == np.array([[0.0, 0.0, 3.0]], np.float32).tobytes()
    # a second camera twice as far has a quarter of the weight: (4 Ya + Yb) / 5
    far = np.eye(4)
    far[2, 3] = -2.0
    r = run(X, [camera(), camera(far)], [Da, Db], [plane(0.0), plane(0.0)])
    exp = (4.0 * np.array([0.0, 0.0, 3.0]) + np.array([1.0, 0.0, 2.0])) / 5.0
    assert np.abs(r["points"][0] - exp).max() < 1e-6 and r["level"].tolist() == [2]


def test_a_point_no_camera_sees_follows_the_mean_move():
    moves = [rigid(0.1, [0.0, 0.0, 1.0]), rigid(0.0, [1.0, 0.0, 0.0]), rigid(0.0, [0.0, 4.0, 0.0])]
    X = np.array([[0.0, 0.0, -2.0], [100.0, 0.0, 2.0]], np.float32)          # behind / beside every camera
    r = run(X, [camera()] * 3, moves, [plane(2.0)] * 3)
    for i in range(2):
        exp = np.mean([D[:, :3] @ X[i].astype(np.float64) + D[:, 3] for D in moves], 0)
        assert np.abs(r["points"][i] - exp).max() < 1e-5
    assert r["level"].tolist() == [3, 3] and r["support"].tolist() == [0, 0] and r["counters"].tolist() == [0, 0, 0, 2]


def test_a_point_that_is_not_finite_is_left_alone():
    X = np.array([[np.nan, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, np.inf, 1.0]], np.float32)
    n = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], np.float32)
    r = run(X, [camera()], [rigid(0.3, [1.0, 1.0, 1.0])], [plane(2.0)], normals=n)
    assert r["points"][[0, 2]].tobytes() == X[[0, 2]].tobytes() and r["normals"][[0, 2]].tobytes() == n[[0, 2]].tobytes()
    assert r["level"].tolist() == [0, 1, 0] and r["counters"].tolist() == [2, 1, 0, 0]
    assert r["normals"][1].tolist() == [0.0, 0.0, 0.0]       # a zero normal stays zero


def test_pixels_round_half_to_even_and_the_last_row_and_column_count():
    D = rigid(0.0, [0.0, 0.0, 0.0])
    p = np.zeros((HP, WP), np.float16)
    p[8, 10] = p[8, 0] = 2.0
    # x / z = 0.25: u = 10.5 -> 10;  y / z = 0.25: v = 8.5 -> 8;  x / z = -0.75: u = 0.5 -> 0 (all exact in binary)
    X = np.array([[0.5, 0.5, 2.0], [-1.5, 0.5, 2.0]], np.float32)
    r = run(X, [camera()], [D], [p])
    assert r["level"].tolist() == [1, 1]                     # half away from zero would read (9, 11) and (9, 1): holes
    q = np.zeros((HP, WP), np.float16)
    q[HP - 1, WP - 1] = 2.0
    last = np.array([[(WP - 1 - 8) / 10 * 2.0, (HP - 1 - 6) / 10 * 2.0, 2.0],      # the last pixel
                     [1.5, 0.0, 2.0],                                               # u = 15.5 -> 16: outside
                     [0.0, 1.25, 2.0]], np.float32)                                 # v = 12.25 -> 12: outside
    r = run(last, [camera()], [D], [q])
    assert r["level"].tolist() == [1, 3, 3]


def _chunk(created, final, G=None, frames=(0, 2)):
    n = len(frames)
    return {"camera_poses": torch.from_numpy(np.asarray(final, np.float32)),
            "_poses_created": torch.from_numpy(np.asarray(created, np.float32)), "_sim3_global": G,
            "dense_cloud": {"points": torch.zeros(0, 3), "voxel_size": 0.05},
            "dense_depth": {"depth": torch.full((n, HP, WP), 2.0, dtype=torch.float16),
                            "frames": torch.tensor(frames, dtype=torch.int32), "pixel_stride": 1, "height": HP, "width": WP,
                            "fxfycxcy": torch.from_numpy(np.tile(K.astype(np.float32), (n, 1)))}}


def _poses(n, seed):
    rng = np.random.default_rng(seed)
    P = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        P[i, :3, :3] = q * np.sign(np.linalg.det(q))
        P[i, :3, 3] = rng.normal(size=3)
    return P


def test_chunk_moves_are_final_times_scale_times_created_inverse():
    from pi3_slam_amd.dense_map import MapFollower
    created, s = _poses(3, 0), 1.7
    G = np.eye(4)
    G[:3, :3] = s * _poses(1, 5)[0, :3, :3]
    G[:3, 3] = [0.5, -1.0, 2.0]
    final = _poses(3, 1)
    final[:, :3, :3] *= s                                    # a pose that went through the similarity carries its scale
    chunk = _chunk(created, final, torch.from_numpy(G))
    views, moves, planes, stride = MapFollower.chunk_moves(chunk)
    assert views.shape == (2, 20) and moves.shape == (2, 12) and moves.dtype == np.float64 and stride == 1
    assert planes.dtype == torch.float16 and tuple(planes.shape) == (2, HP, WP)
    assert np.all(views[:, ref.SCALE_AT] == 1.0)
    assert np.abs(views - cref.pack_views(created[[0, 2]], np.tile(K, (2, 1)), 1.0)).max() < 1e-6
    for m, f in enumerate((0, 2)):
        Pf = final[f].copy()
        Pf[:3, :3] /= s
        D = Pf @ np.diag([s, s, s, 1.0]) @ np.linalg.inv(created[f])
        assert np.abs(moves[m].reshape(3, 4) - D[:3]).max() < 1e-5          # the poses went through fp32
    # the oracle restates it byte for byte
    o = ref.chunk_moves({k: (v if not torch.is_tensor(v) else v.numpy()) for k, v in chunk.items()} |
                        {"dense_depth": {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in chunk["dense_depth"].items()}})
    assert o[0].tobytes() == views.tobytes() and o[1].tobytes() == moves.tobytes()
    assert o[2].tobytes() == planes.numpy().tobytes() and o[3] == stride
    # without an adjustment final = G . created: every move is the chunk's similarity
    same = _chunk(created, G[None] @ created, torch.from_numpy(G))
    for D in MapFollower.chunk_moves(same)[1].reshape(-1, 3, 4):
        assert np.abs(D - G[:3]).max() < 1e-5
    # nothing to follow
    for drop in ("dense_depth", "_poses_created"):
        assert MapFollower.chunk_moves({k: v for k, v in chunk.items() if k != drop}) is None
    assert MapFollower.chunk_moves(_chunk(created, final, None, frames=())) is None


def test_map_follower_validates_and_reports():
    from pi3_slam_amd.dense_map import MapFollower
    f = MapFollower()
    assert f.rel_tol == 0.03 and MapFollower.MARGIN_VOXELS == 1.0 and f.settings() == {"rel_tol": 0.03}
    assert set(f.last_stats) == {"chunks_followed", "chunks_fallen_back", "points", "dropped", "level1", "level2", "level3"}
    assert not any(f.last_stats.values())
    for tol in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="rel_tol"):
            MapFollower(tol)
    assert MapFollower.from_options() is None and MapFollower.from_options(False, 0.1) is None
    assert MapFollower.from_options(True, 0.02).rel_tol == 0.02
    f.last_stats.update(chunks_followed=2, chunks_fallen_back=1, points=100, level1=70, level2=20, level3=9, dropped=1)
    line = f.summary()
    assert "2 clouds" in line and "of 100 points 70" in line and "\n" not in line
    # a chunk that cannot be followed is counted and handed back
    assert f.apply({"dense_cloud": {"voxel_size": 0.1}}, torch.zeros(1, 3), None) is None
    assert f.last_stats["chunks_fallen_back"] == 2


def test_everything_is_off_by_default(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.cli import build_parser
    from pi3_slam_amd.dense_map import MapFollower, fuse_chunks
    from pi3_slam_amd.dist import COLLECT_KEYS
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    p = build_parser()
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert a.map_follow_poses is False and a.map_follow_tolerance == 0.03
    a = p.parse_args(["online", "--output_path", "o"])
    assert a.map_follow_poses is False and a.map_follow_tolerance == 0.03
    for cls in (Pi3SLAMOnline, OfflineReconstructor):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["map_follow_poses"].default is False and sig["map_follow_tolerance"].default == 0.03
        assert list(sig)[-2:] == ["map_follow_poses", "map_follow_tolerance"]
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"))
    assert rec.dense_follower is None and Pi3SLAMOnline.dense_follower is None
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), map_follow_poses=True, map_follow_tolerance=0.05)
    assert isinstance(rec.dense_follower, MapFollower) and rec.dense_follower.rel_tol == 0.05
    assert OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), map_follow_tolerance=0.05).dense_follower is None
    for fn in (export.write_outputs, export.write_renders):         # a keyword beside dense_carver, which stays the last
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params[-2:]] == ["dense_follower", "dense_carver"], fn.__name__
        assert params[-2].default is None
    params = list(inspect.signature(fuse_chunks).parameters.values())
    assert params[-1].name == "follower" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY
    assert params[-1].default is None
    assert "_poses_created" in COLLECT_KEYS


def test_load_chunk_keeps_the_created_poses_only_when_on(tmp_path):
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    os.makedirs(tmp_path / "chunks")
    poses = torch.from_numpy(_poses(4, 2).astype(np.float32))
    torch.save({"camera_poses": poses}, str(tmp_path / "chunks" / "chunk_000000.pt"))
    files = [str(tmp_path / "chunks" / "chunk_000000.pt")]
    off = OfflineReconstructor(str(tmp_path), str(tmp_path / "a"), bundle_adjust=False, device="cpu")
    assert "_poses_created" not in off._load_chunk(files, 0)[0]
    on = OfflineReconstructor(str(tmp_path), str(tmp_path / "b"), bundle_adjust=False, device="cpu", map_follow_poses=True)
    data = on._load_chunk(files, 0)[0]
    assert torch.equal(data["_poses_created"], poses) and data["_poses_created"] is not data["camera_poses"]
    assert data["_poses_created"].data_ptr() != data["camera_poses"].data_ptr()


def test_flags_parse_in_both_spellings():
    from pi3_slam_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o", "--map-follow-poses", "--map-follow-tolerance", "0.05"])
    assert a.map_follow_poses is True and a.map_follow_tolerance == 0.05
    a = p.parse_args(["online", "--output_path", "o", "--map_follow_poses", "--map_follow_tolerance", "0.04"])
    assert a.map_follow_poses is True and a.map_follow_tolerance == 0.04
    for wrong in (["reconstruct", "--chunks", "c", "--output", "o", "--map_follow_poses"],
                  ["online", "--output_path", "o", "--map-follow-poses"],
                  ["create", "--images", "x", "--output", "o", "--map-follow-poses"]):
        with pytest.raises(SystemExit):
            p.parse_args(wrong)
    sub = p._subparsers._group_actions[0].choices
    for cmd, flag, needs, wrong in (("reconstruct", "--map-follow-poses", "--dense-depth-every", "--dense_"),
                                    ("online", "--map_follow_poses", "--dense_depth_every", "--dense-")):
        act = {a.option_strings[0]: a for a in sub[cmd]._actions}
        text = re.sub(r"\s+", " ", act[flag].help)
        assert needs in text and "keep their similarity" in text and wrong not in text
        assert not any(o.startswith("--dense") for o in (flag, flag.replace("poses", "tolerance")))
        assert act[flag.replace("poses", "tolerance")].type is float


def test_new_symbol_is_declared_bound_and_refuses_bad_arguments(built_lib):
    from conftest import ROOT
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dll = lib.load(require_gpu=False)
    assert dll.pi3_abi_version() == 7
    name = "pi3_cloud_follow_views"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text) and name in lib.SIGNATURES and hasattr(dll, name)
    buf = (C.c_ulonglong * 64)()                 # a host address: every call below must be refused before any launch
    p = C.addressof(buf)
    inf, nan = float("inf"), float("nan")
    good = dict(points=p, normals=None, P=4, views=p, moves=p, M=1, planes=p, Hp=4, Wp=4, stride=2, tol=0.03, margin=0.1,
                out=p, out_n=None, level=None, support=None, counters=p)
    bad = [dict(M=0), dict(M=-1), dict(stride=0), dict(stride=3), dict(stride=8), dict(Hp=0), dict(Wp=-1), dict(tol=0.0),
           dict(tol=-1.0), dict(tol=inf), dict(tol=nan), dict(margin=-1e-9), dict(margin=inf), dict(margin=nan),
           dict(points=None), dict(views=None), dict(moves=None), dict(planes=None), dict(out=None), dict(counters=None),
           dict(normals=p), dict(out_n=p), dict(P=-1)]
    for kw in bad:
        a = dict(good, **kw)
        args = (a["points"], a["normals"], a["P"], a["views"], a["moves"], a["M"], a["planes"], a["Hp"], a["Wp"],
                a["stride"], a["tol"], a["margin"], a["out"], a["out_n"], a["level"], a["support"], a["counters"], None)
        assert len(args) == len(lib.SIGNATURES[name])
        dll.pi3_set_knob(b"no_such_knob", 0)
        before = dll.pi3_last_error()
        assert dll.pi3_cloud_follow_views(*args) == -1, kw
        msg = dll.pi3_last_error()
        assert msg and msg != before and name.encode() in msg, (kw, msg)
    assert not any(buf)
