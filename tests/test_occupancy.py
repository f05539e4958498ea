"""The occupancy grid and the clearance field without a GPU: the numpy oracle against scipy's exact distance transform
and against the geometry of a convex room, the grid's bounds, the stage's validation, the flags, the signatures, the
.npz file, the entry points' argument checks, and the flag-off paths."""
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

import occupancy_ref as ref


# ------------------------------------------------------------------------------------------------ 1. the transform
def _scipy_d2(state, R, unknown=False):
    from scipy import ndimage
    site = state == 2
    if unknown:
        site |= state == 0
    if not site.any():
        return np.full(state.shape, ref.FAR, np.uint16)
    d2 = np.rint(ndimage.distance_transform_edt(~site) ** 2).astype(np.int64)
    return np.where(d2 > R * R, ref.FAR, d2).astype(np.uint16)


def _random_state(shape, density, seed):
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 2, shape).astype(np.uint8)           # unknown / free
    state[rng.random(shape) < density] = 2
    return state


@pytest.mark.parametrize("R", [1, 3, 6, 255])
def test_edt_ref_equals_scipy(R):
    shapes = [(9, 11, 13), (1, 1, 40), (17, 1, 5), (4, 30, 2)] if R < 255 else [(5, 6, 40), (3, 300, 2)]
    for n, shape in enumerate(shapes):
        for density in (0.002, 0.02, 0.3):
            state = _random_state(shape, density, 100 * R + n)
            for unknown in (False, True):
                assert ref.edt_ref(state, R, unknown).tobytes() == _scipy_d2(state, R, unknown).tobytes(), \
                    (shape, density, unknown)
        corner = np.zeros(shape, np.uint8)
        corner[0, 0, 0] = 2
        got = ref.edt_ref(corner, R)
        assert got.tobytes() == _scipy_d2(corner, R).tobytes() and got[0, 0, 0] == 0
        assert (ref.edt_ref(np.ones(shape, np.uint8), R) == ref.FAR).all()                   # no sites
        assert (ref.edt_ref(np.full(shape, 2, np.uint8), R) == 0).all()                      # all sites
        assert (ref.edt_ref(np.zeros(shape, np.uint8), R, True) == 0).all()


def test_clearance_is_cell_times_root_and_inf_beyond():
    d2 = np.array([[[0, 1, 2, 25, 65025, ref.FAR]]], np.uint16)
    c = ref.clearance(d2, 0.05)
    assert c.dtype == np.float32 and c[0, 0, -1] == np.inf
    assert c[0, 0, :5].tolist() == [np.float32(0.05 * math.sqrt(v)) for v in (0, 1, 2, 25, 65025)]


# ------------------------------------------------------------------------------------------------ 2. the box room
@pytest.fixture(scope="module")
def room():
    r = ref.box_room()
    m = ref.mark(r["points"], r["cell"], r["origin"], r["dims"])
    o = ref.observe(m["state"], r["cell"], r["origin"], r["views"], r["planes"], 1, r["rel_tol"], r["margin"],
                    r["min_free_views"])
    return r, m, o


def test_box_room_invariants_hold_on_the_oracle(room):
    r, m, o = room
    assert r["dims"] == (50, 40, 35) and o["stats"]["cells"] == 70000
    assert m["stats"] == {"marked": 12 * 48 * 64, "dropped": 0, "outside": 0}
    st = o["stats"]
    assert st["occupied"] + st["free"] + st["unknown"] == st["cells"] and st["occupied"] == int((m["state"] == 2).sum())
    assert min(st["occupied"], st["free"], st["unknown"]) > 5000
    clear = ref.clearance(ref.edt_ref(o["state"], 20), r["cell"])
    inv = ref.room_invariants(r, o["state"], o["free"], o["hit"], o["seen"], clear)
    print(st, inv)
    assert inv["free_outside"] == 0
    assert inv["deep_seen"] > 5000 and inv["deep_seen_not_free"] == 0
    assert inv["cameras"] == 12 and inv["cameras_not_free"] == 0
    cams = ref.centre_cells(r["views"], r["cell"]) - np.asarray(r["origin"])
    assert o["voted_free"][cams[:, 2], cams[:, 1], cams[:, 0]].all() and st["camera_cells_freed"] == 0     # by the votes alone
    assert inv["occupied_deep"] == 0
    assert inv["clearance_short"] == 0
    assert 0.3 < inv["d_min"] < 0.45


def test_camera_cells_become_free_in_the_oracle():
    """A lone view looking at a wall: nobody looks through the cell it stands in, and it is free all the same."""
    r = ref.box_room(dict(n_views=1))
    m = ref.mark(r["points"], r["cell"], r["origin"], r["dims"])
    o = ref.observe(m["state"], r["cell"], r["origin"], r["views"], r["planes"], 1, r["rel_tol"], r["margin"], 1)
    cam = (ref.centre_cells(r["views"], r["cell"]) - np.asarray(r["origin"]))[0]
    at = (cam[2], cam[1], cam[0])
    assert not o["voted_free"][at] and o["state"][at] == 1 and o["stats"]["camera_cells_freed"] == 1
    assert o["stats"]["free"] == int(o["voted_free"].sum()) + 1 == int((o["state"] == 1).sum())
    assert o["stats"]["occupied"] + o["stats"]["free"] + o["stats"]["unknown"] == o["stats"]["cells"]


def test_thresholds_of_the_vote(room):
    """free == min_free_views - 1 stays unknown; a tie free == hit stays unknown."""
    r, m, o = room
    free, hit, state = o["free"], o["hit"], o["state"]
    open_ = state != 2
    assert ((free == 1) & open_).any() and not (state[(free == 1) & open_] == 1).any()
    tie = open_ & (free == hit) & (free >= 2)
    assert not (state[tie] == 1).any()
    assert (state[open_ & (free >= 2) & (free > hit)] == 1).all()
    three = ref.observe(m["state"], r["cell"], r["origin"], r["views"], r["planes"], 1, r["rel_tol"], r["margin"], 3)
    assert three["stats"]["free"] < o["stats"]["free"] and (three["free"] == free).all()


# ------------------------------------------------------------------------------------------------ 3. bounds
def _views_at(centres):
    poses = np.tile(np.eye(4), (len(centres), 1, 1))
    poses[:, :3, 3] = centres
    return ref.carve_ref.pack_views(poses, np.tile([40.0, 40.0, 31.5, 23.5], (len(centres), 1)))


def test_bounds_cover_points_and_cameras_with_padding():
    from pi3_slam_amd.dense_map import MapOccupancy
    pts = np.array([[0.05, 0.05, 0.05], [1.95, 0.95, 0.55], [np.nan, 0, 0], [-0.01, 0.5, 0.2]], np.float32)
    views = _views_at([[3.01, 0.5, -0.75], [0.5, 0.5, 0.5]])
    assert np.array_equal(MapOccupancy.view_cells(views, 0.1), [[30, 5, -8], [5, 5, 5]])
    assert np.array_equal(MapOccupancy.view_cells(views, 0.1), ref.centre_cells(views, 0.1))
    ok, k = ref.point_cells(pts, 0.1)
    assert np.array_equal(MapOccupancy.point_cells(pts, 0.1), k[ok]) and len(k[ok]) == 3
    origin, dims = MapOccupancy(0.1).bounds(pts, views)
    lo, hi = np.array([-1, 0, -8]), np.array([30, 9, 5])
    assert origin.dtype == np.int64 and np.array_equal(origin, lo - 1) and dims == tuple((hi - lo + 3).tolist())
    origin, dims = MapOccupancy(0.1, clearance=0.45).bounds(pts, views)            # R = 5: pad 6
    assert np.array_equal(origin, lo - 6) and dims == tuple((hi - lo + 13).tolist())
    # cameras only; nothing at all
    origin, dims = MapOccupancy(0.1).bounds(np.zeros((0, 3), np.float32), views)
    assert np.array_equal(origin, [4, 4, -9]) and dims == (28, 3, 16)
    with pytest.raises(ValueError, match="no map point"):
        MapOccupancy(0.1).bounds(np.zeros((0, 3), np.float32), np.zeros((0, 20)))


def test_max_cells_error_names_a_cell_size_that_fits():
    from pi3_slam_amd.dense_map import MapOccupancy
    rng = np.random.default_rng(3)
    pts = rng.uniform([-2, -1.5, 0], [2, 1.5, 2.5], (5000, 3)).astype(np.float32)
    views = _views_at([[0.0, 0.0, 1.2]])
    for clearance in (None, 0.5):
        stage = MapOccupancy(0.02, clearance=clearance, max_cells=200000)
        with pytest.raises(ValueError) as e:
            stage.bounds(pts, views)
        msg = str(e.value)
        assert "max_cells = 200000" in msg and "smallest cell size that fits is " in msg
        suggested = float(msg.rsplit(" ", 1)[1])
        assert 0.02 < suggested < 0.2 and suggested == stage.smallest_cell(pts, views)
        _, dims = MapOccupancy(suggested, clearance=clearance, max_cells=200000).bounds(pts, views)
        assert dims[0] * dims[1] * dims[2] <= 200000
        with pytest.raises(ValueError):                          # and not by a wide margin
            MapOccupancy(0.9 * suggested, clearance=clearance, max_cells=200000).bounds(pts, views)


# ------------------------------------------------------------------------------------------------ 4. the stage
def test_map_occupancy_validation_and_options():
    from pi3_slam_amd.dense_map import MapOccupancy
    assert MapOccupancy.from_options() is None and MapOccupancy.from_options(None, 3, 0.1, 1.0, True, 10) is None
    s = MapOccupancy.from_options(0.05, 3, 0.04, 1.0, True, 1000)
    assert (s.cell, s.min_free_views, s.rel_tol, s.clearance, s.unknown_is_obstacle, s.max_cells) == \
        (0.05, 3, 0.04, 1.0, True, 1000)
    assert s.radius == 20 and s.pad == 21 and MapOccupancy(0.05).radius is None and MapOccupancy(0.05).pad == 1
    assert MapOccupancy(0.05, clearance=0.99).radius == 20 and MapOccupancy(0.05, clearance=1.01).radius == 21
    assert MapOccupancy.MARGIN_CELLS == 1.0 and s.settings()["margin"] == 0.05 and s.settings()["radius"] == 20
    assert json.loads(json.dumps(s.settings())) == s.settings()
    d = MapOccupancy(0.1)
    assert (d.min_free_views, d.rel_tol, d.clearance, d.unknown_is_obstacle, d.max_cells) == (2, 0.03, None, False, 1 << 27)
    assert MapOccupancy(0.1, clearance=25.5).radius == 255
    bad = [dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")),
           dict(cell=0.1, min_free_views=0), dict(cell=0.1, min_free_views=1.5), dict(cell=0.1, min_free_views=True),
           dict(cell=0.1, rel_tol=0.0), dict(cell=0.1, rel_tol=float("inf")), dict(cell=0.1, clearance=0.0),
           dict(cell=0.1, clearance=float("nan")), dict(cell=0.1, clearance=25.7), dict(cell=0.1, max_cells=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            MapOccupancy(**kw)
    with pytest.raises(ValueError, match="at most 255"):
        MapOccupancy(0.01, clearance=3.0)


def test_no_depth_keyframes_is_a_notice_not_an_error(capsys):
    from pi3_slam_amd.dense_map import MapCarver, MapOccupancy
    assert callable(MapCarver.chunk_views)
    stage = MapOccupancy(0.1, clearance=0.5)
    assert stage.apply(np.zeros((4, 3), np.float32), [{"camera_poses": torch.eye(4)[None]}], "cpu") is None
    assert capsys.readouterr().out.count("No depth keyframes") == 1
    assert stage.last_stats == {"views": 0}


# ------------------------------------------------------------------------------------------------ 5. flags, signatures
NAMES = ("occupancy_cell", "occupancy_min_free_views", "occupancy_tolerance", "occupancy_clearance",
         "occupancy_unknown_obstacle", "occupancy_max_cells")
DEFAULTS = (None, 2, 0.03, None, False, 1 << 27)


def test_parser_defaults_and_values():
    from pi3_slam_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert tuple(getattr(a, n) for n in NAMES) == DEFAULTS
    a = p.parse_args(["reconstruct", "--chunks", "c", "--output", "o", "--occupancy-cell", "0.05",
                      "--occupancy-min-free-views", "3", "--occupancy-tolerance", "0.05", "--occupancy-clearance", "1.5",
                      "--occupancy-unknown-obstacle", "--occupancy-max-cells", "1000"])
    assert tuple(getattr(a, n) for n in NAMES) == (0.05, 3, 0.05, 1.5, True, 1000)
    a = p.parse_args(["online", "--output_path", "o"])
    assert tuple(getattr(a, n) for n in NAMES) == DEFAULTS
    a = p.parse_args(["online", "--output_path", "o", "--occupancy_cell", "0.1", "--occupancy_min_free_views", "4",
                      "--occupancy_tolerance", "0.02", "--occupancy_clearance", "2", "--occupancy_unknown_obstacle",
                      "--occupancy_max_cells", "5"])
    assert tuple(getattr(a, n) for n in NAMES) == (0.1, 4, 0.02, 2.0, True, 5)
    assert set(NAMES) <= set(cli.option_names(cli.DENSE_MAP_FLAGS))
    helps = dict(cli.DENSE_MAP_FLAGS)
    text = helps["--occupancy-cell"]["help"]
    assert "--map-follow-poses" in text and "--no-bundle-adjust" in text
    assert "--map_follow_poses" in dict(cli.ONLINE_DENSE_FLAGS)["--occupancy_cell"]["help"]
    for f in ("--occupancy-min-free-views", "--occupancy-tolerance"):
        assert "starting point" in helps[f]["help"] and "not a measured optimum" in helps[f]["help"]


def test_signatures_keep_their_pinned_tails(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.dense_map import DenseMap, MapOccupancy, fuse_chunks
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    for cls in (Pi3SLAMOnline, OfflineReconstructor):
        sig = inspect.signature(cls.__init__).parameters
        names = list(sig)
        assert names[-2:] == ["map_follow_poses", "map_follow_tolerance"]
        assert tuple(names[-8:-2]) == NAMES and tuple(sig[n].default for n in NAMES) == DEFAULTS
    params = list(inspect.signature(export.write_outputs).parameters.values())
    assert [p.name for p in params[-3:]] == ["dense_occupancy", "dense_follower", "dense_carver"]
    assert params[-3].default is None
    params = list(inspect.signature(fuse_chunks).parameters.values())
    assert [p.name for p in params[-2:]] == ["occupancy", "follower"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None for p in params[-2:])
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"))
    assert rec.dense_occupancy is None
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), occupancy_cell=0.05, occupancy_clearance=1.0,
                               occupancy_unknown_obstacle=True)
    assert isinstance(rec.dense_occupancy, MapOccupancy) and rec.dense_occupancy.radius == 20
    assert rec.dense_occupancy.unknown_is_obstacle is True
    assert OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), occupancy_clearance=1.0).dense_occupancy is None
    with pytest.raises(ValueError, match="at most 255"):
        OfflineReconstructor(str(tmp_path), str(tmp_path / "out"), occupancy_cell=0.01, occupancy_clearance=3.0)
    assert Pi3SLAMOnline.dense_occupancy is None and callable(Pi3SLAMOnline.save_occupancy)
    fields = DenseMap.__dataclass_fields__
    assert fields["occupancy"].default is None and fields["occupancy_error"].default is None


# ------------------------------------------------------------------------------------------------ 6. the file
def _grid(clearance=True):
    from pi3_slam_amd.dense_map import MapOccupancy, OccupancyGrid
    rng = np.random.default_rng(5)
    state = rng.integers(0, 2, (4, 5, 6)).astype(np.uint8)
    state[0, 0, 0] = state[2, 3, 4] = 2                         # two obstacles: most cells lie beyond 3 cells of both
    clear = ref.clearance(ref.edt_ref(state, 3), 0.25) if clearance else None
    return OccupancyGrid(state, np.array([-3, 2, 7], np.int64), 0.25, clear, {"cells": 120, "free": 40},
                         MapOccupancy(0.25, clearance=0.75 if clearance else None).settings())


@pytest.mark.parametrize("clearance", [True, False])
def test_occupancy_npz_round_trip(tmp_path, clearance):
    from pi3_slam_amd import export
    g = _grid(clearance)
    path = str(tmp_path / "occupancy.npz")
    assert export.write_occupancy(g, path) == int((g.state == 1).sum())
    assert os.listdir(tmp_path) == ["occupancy.npz"]
    with np.load(path) as z:
        assert set(z.files) == {"state", "index_origin", "origin", "cell", "settings", "counts"} | \
            ({"clearance"} if clearance else set())
        assert z["state"].dtype == np.uint8 and z["state"].tobytes() == g.state.tobytes() and z["state"].shape == (4, 5, 6)
        assert z["index_origin"].dtype == np.int64 and z["index_origin"].tolist() == [-3, 2, 7]
        assert z["origin"].dtype == np.float64 and z["origin"].tolist() == [-0.75, 0.5, 1.75] == g.origin.tolist()
        assert float(z["cell"]) == 0.25
        if clearance:
            assert z["clearance"].dtype == np.float32 and z["clearance"].tobytes() == g.clearance.tobytes()
            assert np.isinf(z["clearance"]).any()
        assert json.loads(str(z["settings"])) == g.settings and json.loads(str(z["counts"])) == g.counts


# ------------------------------------------------------------------------------------------------ 7. entry points
def test_entry_points_refuse_bad_arguments():
    from pi3_slam_amd import lib as L
    lib = L.load(require_gpu=False)
    P = 0x1000                      # a non-null address: no call below gets as far as using it
    nan, inf = float("nan"), float("inf")

    def mark(points=P, n=10, inv=10.0, o=(0, 0, 0), d=(4, 4, 4), state=P, counters=P):
        return lib.pi3_occupancy_mark(points, n, inv, *o, *d, state, counters, None)

    def observe(state=P, d=(4, 4, 4), o=(0, 0, 0), cell=0.1, views=P, M=2, planes=P, Hp=8, Wp=8, S=1, tol=0.03,
                margin=0.1, mfv=2, counters=P):
        return lib.pi3_occupancy_observe(state, *d, *o, cell, views, M, planes, Hp, Wp, S, tol, margin, mfv, None, None,
                                         counters, None)

    def edt(state=P, d=(4, 4, 4), R=3, d2=P, work=2 * P):
        return lib.pi3_grid_edt(state, *d, R, 0, d2, work, None)

    cases = [(mark, b"pi3_occupancy_mark", [dict(points=None), dict(n=-1), dict(inv=0.0), dict(inv=nan), dict(inv=inf),
                                            dict(d=(0, 4, 4)), dict(d=(4, -1, 4)), dict(d=(4, 4, 1 << 21)),
                                            dict(d=((1 << 21) - 1,) * 3), dict(o=(1 << 21, 0, 0)),
                                            dict(o=(0, 0, -(1 << 21))), dict(state=None), dict(counters=None)]),
             (observe, b"pi3_occupancy_observe", [dict(state=None), dict(d=(4, 0, 4)), dict(o=(0, 1 << 21, 0)),
                                                  dict(cell=0.0), dict(cell=nan), dict(views=None), dict(planes=None),
                                                  dict(M=-1), dict(Hp=0), dict(Wp=-2), dict(S=0), dict(S=3), dict(S=8),
                                                  dict(tol=0.0), dict(tol=inf), dict(margin=-0.1), dict(margin=nan),
                                                  dict(mfv=0), dict(counters=None)]),
             (edt, b"pi3_grid_edt", [dict(state=None), dict(d=(0, 1, 1)), dict(d=(4, 4, -4)), dict(R=0), dict(R=256),
                                     dict(R=-1), dict(d2=None), dict(work=None), dict(work=P)])]
    for call, name, bad in cases:
        for kw in bad:
            lib.pi3_set_knob(b"no_such_knob", 0)
            before = lib.pi3_last_error()
            assert call(**kw) == -1, (name, kw)
            msg = lib.pi3_last_error()
            assert msg and msg != before and name in msg, (kw, msg)
    assert lib.pi3_abi_version() == 7
    assert {"pi3_occupancy_mark", "pi3_occupancy_observe", "pi3_grid_edt"} <= set(L.SIGNATURES)


# ------------------------------------------------------------------------------------------------ 8. flag off / on
def test_write_outputs_writes_the_grid_only_when_asked(tmp_path, monkeypatch, capsys):
    from pi3_slam_amd import export
    from pi3_slam_amd.dense_map import DenseMap
    seen = []

    def fake_fuse(chunks, device="cuda", **kw):
        seen.append(kw)
        dense = DenseMap(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), np.ones(2, np.int32), 0.02)
        stage = kw.get("occupancy")
        if stage == "grid":
            dense.occupancy = _grid()
        elif stage == "broken":
            dense.occupancy_error = RuntimeError("the grid broke")
        return dense

    monkeypatch.setattr(export, "fuse_chunks", fake_fuse)
    off = tmp_path / "off"
    off.mkdir()
    export.write_outputs([], str(off), "cpu")
    assert seen[-1]["occupancy"] is None and "occupancy.npz" not in os.listdir(off) and "dense_points.ply" in os.listdir(off)
    plain = open(off / "dense_points.ply", "rb").read()
    on = tmp_path / "on"
    on.mkdir()
    export.write_outputs([], str(on), "cpu", dense_occupancy="grid")
    assert seen[-1]["occupancy"] == "grid" and {"occupancy.npz", "dense_points.ply"} <= set(os.listdir(on))
    assert open(on / "dense_points.ply", "rb").read() == plain
    with np.load(on / "occupancy.npz") as z:
        assert z["state"].tobytes() == _grid().state.tobytes()
    capsys.readouterr()
    broken = tmp_path / "broken"
    broken.mkdir()
    export.write_outputs([], str(broken), "cpu", dense_occupancy="broken")
    assert "Failed to save the occupancy grid: the grid broke" in capsys.readouterr().out
    assert "occupancy.npz" not in os.listdir(broken) and open(broken / "dense_points.ply", "rb").read() == plain
