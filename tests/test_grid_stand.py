"""Routes for a body that stands without a GPU: the oracle (tests/grid_stand_ref.py) against closed forms, its mirror
symmetry, the candidate rule's promise for thin bands, the band's conversion from metres, GridRouter's, ViewPlanner's and
FrontierFinder's argument checks, the parsers, and the argument errors of the three entry points on the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_route_ref as rref           # noqa: E402
import grid_stand_ref as ref            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _along(shape_n, up_axis, up_sign, other=(2, 2)):
    """A state of `shape_n` cells along up and `other` cells on the two other axes, all free, and a function that
    addresses it by (level from the -up side): state_view[level] is a 2-D slab."""
    n = [0, 0, 0]
    n[up_axis], n[(up_axis + 1) % 3], n[(up_axis + 2) % 3] = shape_n, other[0], other[1]
    state = np.ones((n[2], n[1], n[0]), np.uint8)
    return state, (lambda a: ref._scan_first(a, up_axis, up_sign))


@pytest.mark.parametrize("up_axis,up_sign", ref.UPS)
def test_closed_forms(up_axis, up_sign):
    # a single occupied slab under free space: the distance to the slab, 255 from 255 cells up
    state, lv = _along(300, up_axis, up_sign)
    lv(state)[10] = 2
    h = lv(ref.height(state, up_axis, up_sign))
    level = np.arange(300)[:, None, None] + np.zeros(h.shape, np.int64)
    above = level > 10
    exp = np.where(level - 10 <= 254, level - 10, 255)
    assert h.dtype == np.uint8 and (h[above] == exp[above]).all()
    assert (h[11] == 1).all() and (h[264] == 254).all() and (h[265] == 255).all() and (h[299] == 255).all()
    assert (h[:11] == 0).all()                      # under the slab: the border comes first (the slab's own cell too)
    # an unknown cell in a column: 0 above it up to the next occupied cell; with through_unknown it does not count
    state, lv = _along(40, up_axis, up_sign)
    lv(state)[0] = 2
    lv(state)[5, 1, 1] = 0
    lv(state)[20, 1, 1] = 2
    h = lv(ref.height(state, up_axis, up_sign))
    assert h[1:6, 1, 1].tolist() == [1, 2, 3, 4, 5] and (h[6:21, 1, 1] == 0).all()
    assert h[21:, 1, 1].tolist() == list(range(1, 20)) and h[1:, 0, 0].tolist() == list(range(1, 40))
    h = lv(ref.height(state, up_axis, up_sign, True))
    assert h[1:21, 1, 1].tolist() == list(range(1, 21)) and h[21:, 1, 1].tolist() == list(range(1, 20))
    # all free: 0 within 254 of the border, 255 beyond; all occupied: 1 everywhere but the bottom layer
    state, lv = _along(300, up_axis, up_sign, (1, 2))
    h = lv(ref.height(state, up_axis, up_sign))
    assert (h[:254] == 0).all() and (h[254:] == 255).all()
    h = lv(ref.height(np.full_like(state, 2), up_axis, up_sign))
    assert (h[0] == 0).all() and (h[1:] == 1).all()
    h = lv(ref.height(np.zeros_like(state), up_axis, up_sign))         # all unknown: no support, then through it
    assert (h == 0).all()
    assert (ref.height(np.zeros_like(state), up_axis, up_sign, True) == ref.height(np.ones_like(state), up_axis, up_sign)).all()


@pytest.mark.parametrize("through_unknown", [False, True])
def test_mirroring_the_grid_and_flipping_the_sign_mirrors_the_height(through_unknown):
    state = ref.random_state((9, 8, 7), 0.2, 3)
    for up_axis in range(3):
        ax = 2 - up_axis
        a = ref.height(state, up_axis, 1, through_unknown)
        b = ref.height(np.flip(state, ax), up_axis, -1, through_unknown)
        assert a.tobytes() == np.ascontiguousarray(np.flip(b, ax)).tobytes()
        assert set(np.unique(a)) <= set(range(0, 10)) and (a > 0).any() and (a == 0).any()


def test_height_by_brute_force():
    """The vectorised oracle against the definition, cell by cell."""
    state = ref.random_state((5, 6, 4), 0.25, 11)
    nz, ny, nx = state.shape
    for up_axis, up_sign in ref.UPS:
        for tu in (False, True):
            h = ref.height(state, up_axis, up_sign, tu)
            for z in range(nz):
                for y in range(ny):
                    for x in range(nx):
                        c, exp = [x, y, z], 255
                        for j in range(1, 255):
                            c[up_axis] -= up_sign
                            inside = 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz
                            s = int(state[c[2], c[1], c[0]]) if inside else -1
                            if not inside or (s == 2 if tu else s != 1):
                                exp = j if s == 2 else 0
                                break
                        assert h[z, y, x] == exp, (up_axis, up_sign, tu, x, y, z)


def test_walk_and_init():
    state = np.array([[[2, 1, 1, 1, 0, 1, 2, 1]]], np.uint8)
    h = ref.height(state, 0, 1)
    assert h.tolist() == [[[0, 1, 2, 3, 4, 0, 0, 1]]]
    assert ref.walk_stand(state, h, 1, 2).tolist() == [[[0, 1, 1, 0, 0, 0, 0, 1]]]
    assert ref.walk_stand(state, h, 2, 254).tolist() == [[[0, 0, 1, 1, 0, 0, 0, 0]]]
    ht = ref.height(state, 0, 1, True)
    assert ht.tolist() == [[[0, 1, 2, 3, 4, 5, 6, 1]]]
    assert ref.walk_stand(state, ht, 4, 5, through_unknown=True).tolist() == [[[0, 0, 0, 0, 1, 1, 0, 0]]]
    got = ref.init_stand(state, None, 0, False, h, 1, 2, [1, 1, 3, 0, -1, 8, 7])
    assert got["counters"] == [3, 3, 2, 2, 2] and got["dist"].tolist() == [[[rref.FAR, 0] + [rref.FAR] * 5 + [0]]]
    # the widest band over a grid whose every open cell has a floor is the plain rule
    state = np.ones((4, 3, 5), np.uint8)
    state[0] = 2
    h = ref.height(state, 2, 1)
    assert ref.walk_stand(state, h, 1, 254).tobytes() == rref.walk_mask(state).tobytes()


def test_a_band_thinner_than_the_stride_keeps_a_cell_in_every_standing_column():
    """Floors at random levels under free space: with the world lattice along up most columns offer no candidate inside
    a band of one or two cells; the floor-following lattice offers exactly the lowest band cell of every column that
    stands, on the lattice of the two other axes."""
    rng = np.random.default_rng(5)
    for up_axis, up_sign in ref.UPS:
        n = [0, 0, 0]
        n[up_axis], n[(up_axis + 1) % 3], n[(up_axis + 2) % 3] = 24, 17, 16
        state = np.ones((n[2], n[1], n[0]), np.uint8)
        lv = ref._scan_first(state, up_axis, up_sign)
        floors = rng.integers(0, 9, lv.shape[1:])
        for t in range(9):
            lv[t][floors >= t] = 2
        h = ref.height(state, up_axis, up_sign)
        origin = (-3, 2, 5)
        for stride, (h_lo, h_hi) in ((4, (6, 6)), (4, (5, 6)), (3, (7, 8)), (1, (2, 4))):
            walk = ref.walk_stand(state, h, h_lo, h_hi)
            dist = np.where(walk != 0, 12, rref.FAR).astype(np.uint32)           # every standing cell counts as reached
            cand = ref.candidates_stand(dist, h, origin, stride, 1000, up_axis, h_lo)
            got = np.zeros(state.size, bool)
            got[cand] = True
            got = ref._scan_first(got.reshape(state.shape), up_axis, up_sign)
            hs = ref._scan_first(h, up_axis, up_sign)
            idx = np.meshgrid(*(np.arange(m) for m in state.shape), indexing="ij")     # z, y, x
            on = np.ones(state.shape, bool)
            for axis in range(3):
                if axis != up_axis:
                    on &= (idx[2 - axis] + origin[axis]) % stride == 0
            on = ref._scan_first(on, up_axis, up_sign)
            per_column, lattice_columns = got.sum(0), on[0]
            assert lattice_columns.sum() >= 4
            # every column stands here (free space above every floor): one candidate per column per stride of band
            assert (per_column[lattice_columns] == -(-(h_hi - h_lo + 1) // stride)).all() and not per_column[~lattice_columns].any()
            assert (hs[got].astype(int) - h_lo).min() == 0 and ((hs[got].astype(int) - h_lo) % stride == 0).all()
            if stride > h_hi - h_lo + 1:                # the world lattice loses columns of the same band
                world = np.ones(state.shape, bool)
                for axis in range(3):
                    world &= (idx[2 - axis] + origin[axis]) % stride == 0
                lost = (ref._scan_first(world & (walk != 0), up_axis, up_sign).sum(0) == 0) & lattice_columns
                assert lost.any()
    # a cell that is not reached, or beyond max_cost, is no candidate
    state = np.ones((1, 1, 12), np.uint8)
    state[0, 0, 0] = 2
    h = ref.height(state, 0, 1)
    dist = (12 * np.arange(12, dtype=np.uint32)).reshape(1, 1, 12)
    dist[0, 0, 5] = dist[0, 0, 1] = dist[0, 0, 2] = rref.FAR        # under the band nothing stands, so nothing is reached
    assert ref.candidates_stand(dist, h, (0, 0, 0), 2, 12 * 8, 0, 3).tolist() == [3, 7]


def test_band_conversion_and_its_errors():
    from pi3_slam_amd import ops
    from pi3_slam_amd.grid_route import GridRouter
    assert (ops.STAND_MAX_HEIGHT, ops.STAND_NONE, ops.STAND_FAR) == (254, 0, 255) == (ref.MAX_HEIGHT, ref.NONE, ref.FAR_HEIGHT)
    assert ops.ROUTE_INIT_STAND_COUNTERS == ops.ROUTE_INIT_COUNTERS + ("off_band",)
    assert GridRouter().stand_cells(0.05) is None
    for (lo, hi), cell, exp in (((1.4, 1.6), 0.05, (28, 32)), ((0.6, 0.8), 0.1, (6, 8)), ((0.61, 0.89), 0.1, (7, 8)),
                                ((0.05, 12.72), 0.05, (1, 254)), ((0.25, 0.25), 0.125, (2, 2))):
        assert GridRouter(stand=(lo, hi)).stand_cells(cell) == exp == ref.band_cells(lo, hi, cell), (lo, hi, cell)
    for (lo, hi), cell, ints in (((0.61, 0.69), 0.1, "7 .. 6"), ((0.01, 0.09), 0.1, "1 .. 0"), ((1.0, 25.5), 0.1, "10 .. 255"),
                                 ((30.0, 31.0), 0.1, "300 .. 310")):
        with pytest.raises(ValueError) as e:
            GridRouter(stand=(lo, hi)).stand_cells(cell)
        text = str(e.value)
        assert f"lo = {lo:g}" in text and f"hi = {hi:g}" in text and f"cells of {cell:g}" in text and ints in text
    with pytest.raises(ValueError, match="positive finite"):
        GridRouter(stand=(1.0, 2.0)).stand_cells(0.0)


def test_router_planner_and_finder_arguments():
    from pi3_slam_amd.frontier import FrontierFinder
    from pi3_slam_amd.grid_route import GridRouter, RouteField
    from pi3_slam_amd.view_planner import ViewPlanner
    plain = GridRouter()
    assert plain.stand is None and plain.up == (0, -1, 0)
    assert plain.settings() == {"radius": 0.0, "through_unknown": False, "approach_unknown": False, "costs": [12, 17, 21]}
    r = GridRouter(0.2, stand=[1, 2], up=[0.0, 0, 1])
    assert r.stand == (1.0, 2.0) and r.up == (0, 0, 1)
    assert r.settings() == dict(GridRouter(0.2).settings(), stand=[1.0, 2.0], up=[0, 0, 1])
    for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0), (1.0,), "ab", 3.0, (1, 2, 3)):
        with pytest.raises(ValueError, match="stand must be"):
            GridRouter(stand=bad)
    for bad in ((0, 0, 0), (1, 1, 0), (0, -2, 0), (0, 0.5, 0), "up", (0, 1)):
        with pytest.raises(ValueError, match="up must be one of the six signed axes"):
            GridRouter(stand=(1.0, 2.0), up=bad)
        with pytest.raises(ValueError, match="up must be one of the six signed axes"):
            ViewPlanner(stand=(1.0, 2.0), up=bad)
        with pytest.raises(ValueError, match="up must be one of the six signed axes"):
            FrontierFinder(stand=(1.0, 2.0), up=bad)
    GridRouter(up=(7, 7, 7))                        # not read without stand: nothing runs differently
    p = ViewPlanner(0.2, stand=(1.4, 1.6), up=(0, 0, -1))
    assert p.router.stand == (1.4, 1.6) == p.stand and p.router.up == (0, 0, -1) == p.up and p.router.approach_unknown
    assert p.settings()["stand"] == [1.4, 1.6] and p.settings()["up"] == [0, 0, -1]
    assert p.settings()["router"]["stand"] == [1.4, 1.6] and p.settings()["router"]["up"] == [0, 0, -1]
    q = ViewPlanner(0.2)
    assert q.stand is None and q.router.stand is None and "stand" not in q.settings() and "up" not in q.settings()
    assert "stand" not in q.settings()["router"] and "up" not in q.settings()["router"]
    f = ViewPlanner(0.2, frustum=(90, 67.5), up=(0, 0, 1), stand=(0.5, 1.0))        # one up for the frames and the floor
    assert f.router.up == (0, 0, 1) and f.settings()["frustum"]["up"] == [0, 0, 1]
    with pytest.raises(ValueError, match="stand must be"):
        ViewPlanner(stand=(2.0, 1.0))
    ff = FrontierFinder(0.1, 3, stand=(0.5, 1.0))
    assert ff.router.stand == (0.5, 1.0) and ff.settings()["router"]["stand"] == [0.5, 1.0]
    assert "stand" not in FrontierFinder().settings()["router"]
    # what is wrong with a refused cell
    state = np.array([[[2, 1, 1, 1, 0, 1]]], np.uint8)
    h = ref.height(state, 0, 1)
    h[0, 0, 2] = 255
    fld = RouteField(None, None, np.zeros_like(state), np.zeros(3, np.int64), 0.1, state, None, {},
                     {"stand_cells": [28, 32]}, height=h)
    assert GridRouter._describe(fld, 3) == "cell (3, 0, 0) is free, 3 cells above its floor (band 28 .. 32)"
    assert GridRouter._describe(fld, 5) == "cell (5, 0, 0) is free, and has no verified floor below it"
    assert GridRouter._describe(fld, 2) == "cell (2, 0, 0) is free, and has no floor within 254 cells below it"
    bare = RouteField(None, None, np.zeros_like(state), np.zeros(3, np.int64), 0.1, state)
    assert bare.height is None and GridRouter._describe(bare, 3) == "cell (3, 0, 0) is free"
    # an impossible band is refused before anything reaches the device
    from pi3_slam_amd.dense_map import OccupancyGrid
    with pytest.raises(ValueError, match="7 .. 6 cells"):
        GridRouter(stand=(0.61, 0.69)).field(OccupancyGrid(state, np.zeros(3, np.int64), 0.1), [[0.15, 0.05, 0.05]], "cpu")


def test_parsers():
    from pi3_slam_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--start", "1", "2", "3"])
    assert a.stand is None and a.up == [0, -1, 0]
    a = p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--start", "1", "2", "3", "--stand", "1.4", "1.6",
                      "--up", "0", "0", "1"])
    assert a.stand == [1.4, 1.6] and a.up == [0, 0, 1]
    a = p.parse_args(["frontiers", "--occupancy", "o.npz", "--output", "out", "--stand", "0.5", "1", "--up", "-1", "0", "0"])
    assert a.stand == [0.5, 1.0] and a.up == [-1, 0, 0]
    a = p.parse_args(["views", "--occupancy", "o.npz", "--output", "out", "--start", "1", "2", "3", "--stand", "0.5", "1"])
    assert a.stand == [0.5, 1.0] and a.up == [0, -1, 0] and a.frustum is None
    assert p.parse_args(["views", "--occupancy", "o.npz", "--output", "out"]).stand is None
    for cmd in ("route", "frontiers", "views"):
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "--occupancy", "o.npz", "--output", "out", "--stand", "1"])
    with pytest.raises(SystemExit, match="route: stand must be"):
        cli.main(["route", "--occupancy", "missing.npz", "--output", "out", "--start", "0", "0", "0", "--stand", "2", "1"])
    with pytest.raises(SystemExit, match="views: up must be one of the six signed axes"):
        cli.main(["views", "--occupancy", "missing.npz", "--output", "out", "--start", "0", "0", "0", "--stand", "1", "2",
                  "--up", "1", "1", "0"])
    with pytest.raises(SystemExit, match="frontiers: stand must be"):
        cli.main(["frontiers", "--occupancy", "missing.npz", "--output", "out", "--stand", "0", "1"])


def test_signatures_header_and_makefile_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()

    def names(fn):
        return [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % fn, text).group(1).split(",")]
    assert names("pi3_grid_stand_height") == ["state", "nx", "ny", "nz", "up_axis", "up_sign", "through_unknown", "height",
                                              "stream"]
    init, stand = names("pi3_grid_route_init"), names("pi3_grid_route_init_stand")
    assert stand == init[:4] + ["height", "h_lo", "h_hi"] + init[4:]
    cand, cstand = names("pi3_grid_view_candidates"), names("pi3_grid_view_candidates_stand")
    assert cstand == cand[:1] + ["height"] + cand[1:9] + ["up_axis", "h_lo"] + cand[9:]
    for fn in ("pi3_grid_stand_height", "pi3_grid_route_init_stand", "pi3_grid_view_candidates_stand"):
        assert len(lib.SIGNATURES[fn]) == len(names(fn))
    sig, was = lib.SIGNATURES["pi3_grid_route_init_stand"], lib.SIGNATURES["pi3_grid_route_init"]
    assert sig == was[:4] + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + was[4:]
    sig, was = lib.SIGNATURES["pi3_grid_view_candidates_stand"], lib.SIGNATURES["pi3_grid_view_candidates"]
    assert sig == was[:1] + [ctypes.c_void_p] + was[1:9] + [ctypes.c_int, ctypes.c_int] + was[9:]
    assert " grid_stand.hip" in open(os.path.join(ROOT, "pi3_slam_amd", "csrc", "Makefile")).read()


def test_the_library_has_the_symbols_and_refuses_bad_arguments_without_a_gpu(built_lib):
    from pi3_slam_amd import lib as L
    lib = L.load(require_gpu=False)
    p = 4096                                        # never dereferenced: a refused call returns before any launch
    H, I, C = lib.pi3_grid_stand_height, lib.pi3_grid_route_init_stand, lib.pi3_grid_view_candidates_stand
    big = (1 << 21)

    def height(**k):
        return H(k.get("state", p), *k.get("dims", (5, 4, 3)), k.get("axis", 1), k.get("sign", -1), 0, k.get("out", p), None)

    def init(**k):
        return I(k.get("state", p), k.get("d2", None), k.get("min_d2", 0), 0, k.get("height", p), *k.get("band", (3, 5)),
                 *k.get("dims", (5, 4, 3)), k.get("sources", p), k.get("Ns", 1), k.get("walk", p), k.get("dist", p),
                 k.get("counters", p), None)

    def cand(**k):
        return C(k.get("dist", p), k.get("height", p), *k.get("dims", (5, 4, 3)), 0, 0, 0, k.get("stride", 4),
                 k.get("max_cost", 100), k.get("axis", 1), k.get("h_lo", 3), k.get("cells", p), k.get("cap", 8),
                 k.get("count", p), None)

    bad_dims = [dict(dims=(0, 4, 3)), dict(dims=(5, -1, 3)), dict(dims=(5, 4, big)), dict(dims=(1 << 10, 1 << 10, 129))]
    for case in bad_dims + [dict(state=None), dict(out=None), dict(axis=-1), dict(axis=3), dict(sign=0), dict(sign=2),
                            dict(sign=-2)]:
        assert height(**case) == -1, case
        err = lib.pi3_last_error()
        nx, ny, nz = case.get("dims", (5, 4, 3))
        assert err.startswith(b"pi3_grid_stand_height:") and (b"dims=(%d, %d, %d)" % (nx, ny, nz)) in err, (case, err)
        assert (b"up_axis=%d (0 .. 2) up_sign=%d (1 or -1)" % (case.get("axis", 1), case.get("sign", -1))) in err, (case, err)
    for case in bad_dims + [dict(state=None), dict(height=None), dict(walk=None), dict(dist=None), dict(counters=None),
                            dict(band=(0, 5)), dict(band=(5, 4)), dict(band=(3, 255)), dict(band=(-2, -1)),
                            dict(min_d2=-1), dict(min_d2=4), dict(min_d2=65026, d2=p), dict(Ns=-1), dict(Ns=1 << 39),
                            dict(sources=None)]:
        assert init(**case) == -1, case
        err = lib.pi3_last_error()
        nx, ny, nz = case.get("dims", (5, 4, 3))
        assert err.startswith(b"pi3_grid_route_init_stand:") and (b"dims=(%d, %d, %d)" % (nx, ny, nz)) in err, (case, err)
        assert (b"band=(%d, %d) (1 <= h_lo <= h_hi <= 254)" % case.get("band", (3, 5))) in err, (case, err)
        assert (b"min_d2=%d " % case.get("min_d2", 0)) in err and (b"Ns=%d " % case.get("Ns", 1)) in err, (case, err)
    for case in bad_dims + [dict(dist=None), dict(height=None), dict(count=None), dict(cells=None), dict(stride=0),
                            dict(max_cost=-1), dict(cap=-1), dict(axis=-1), dict(axis=3), dict(h_lo=0), dict(h_lo=255)]:
        assert cand(**case) == -1, case
        err = lib.pi3_last_error()
        nx, ny, nz = case.get("dims", (5, 4, 3))
        assert err.startswith(b"pi3_grid_view_candidates_stand:") and (b"dims=(%d, %d, %d)" % (nx, ny, nz)) in err, (case, err)
        assert (b"up_axis=%d (0 .. 2) h_lo=%d (1 .. 254)" % (case.get("axis", 1), case.get("h_lo", 3))) in err, (case, err)
        assert (b"stride=%d (>= 1)" % case.get("stride", 4)) in err, (case, err)
