"""Views that cover on the GPU (csrc/grid_view.hip: pi3_grid_view_gain_unseen, pi3_grid_view_mark), byte for byte against
the oracle (tests/grid_cover_ref.py): the unseen gain under zero, seeded and full masks, single marks, batches of marks,
the mask's last word, the argument checks, the box room through ViewPlanner.cover, and `cli views --cover` on a
two-chunk sequence.  Every output is filled with a poison value before each call, and every mask has two guard words
behind it."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_cover_ref as cref               # noqa: E402
import grid_route_ref as rref               # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_gpu as view_gpu       # noqa: E402  (its states, candidates and comparison)
from test_grid_view_gpu import reconstructed  # noqa: E402,F401  (the two-chunk sequence's reconstruction, a fixture)

pytestmark = pytest.mark.gpu
DEV = view_gpu.DEV
POISON32, POISON64, POISON16 = view_gpu.POISON32, view_gpu.POISON64, -7
GUARD = np.uint32(0xA5A5A5A5)
HD = vref.headings26()
F90, F180 = vref.cos2(90), vref.cos2(180)
_dev = view_gpu._dev


class Mask:
    """A seen mask on the device with two guard words behind it."""

    def __init__(self, cells, words=None):
        n = cref.seen_words(cells)
        host = np.concatenate([np.zeros(n, np.uint32) if words is None else np.asarray(words, np.uint32), [GUARD, GUARD]])
        assert len(host) == n + 2
        self.buf = _dev(host.view(np.int32))
        self.words = self.buf[:n]

    def host(self):
        """The mask's words, after checking the guard."""
        got = self.buf.cpu().numpy().view(np.uint32)
        assert got[-2:].tolist() == [GUARD, GUARD], "the guard words behind the mask changed"
        return got[:-2].copy()


def _gain_unseen_device(state, mask, cand, R, headings, num, den):
    from pi3_slam_amd import ops
    V, H = len(cand), len(headings)
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    before = mask.host()
    ops.grid_view_gain_unseen(state, mask.words, _dev(np.asarray(cand, np.int64)), R, headings, num, den, gain, visible,
                              best, counters)
    assert mask.host().tobytes() == before.tobytes()            # read only
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _mark_device(state, mask, cells, heading_of, R, headings, num, den, owner=None, tag=0):
    from pi3_slam_amd import ops
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_mark(state, mask.words, _dev(np.asarray(cells, np.int64)), heading_of, R, headings, num, den, counters,
                       owner, tag)
    return counters.tolist()


# ------------------------------------------------------------------------------------------------ 1. the unseen gain
@pytest.mark.parametrize("dims", [(1, 1, 1), (300, 1, 1), (9, 8, 7), (17, 9, 20)], ids=lambda d: "%dx%dx%d" % d)
def test_a_zero_mask_gives_the_plain_kernels_bytes(dims):
    cand = view_gpu._candidates(dims, sum(dims))
    for name, state in view_gpu._states(dims).items():
        if name in ("0.1/0.8/0.1", "free"):
            continue
        st = _dev(state)
        mask = Mask(state.size)
        for R in (1, 2, 7):
            for num, den in (F90, F180):
                plain = view_gpu._gain_device(st, cand, R, HD, num, den)
                view_gpu._same(_gain_unseen_device(st, mask, cand, R, HD, num, den), plain, (dims, name, R, num))
                assert plain["counters"][0] == len(cand) - (state.size > 600)
        assert name != "unknown" or state.size == 1 or plain["counters"][3] > 0


@pytest.mark.parametrize("dims", [(9, 8, 7), (17, 9, 20)], ids=lambda d: "%dx%dx%d" % d)
def test_seeded_masks_match_the_oracle(dims):
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.1, nx + ny + nz)
    st = _dev(state)
    cand = view_gpu._candidates(dims, sum(dims))
    rng = np.random.default_rng(7)
    for R in (2, 7):
        casts = cref.cast(state, cand, R)
        plain = cref.gain_unseen(state, np.zeros(cref.seen_words(state.size), np.uint32), cand, R, HD, *F90, casts=casts)
        for density in (0.1, 0.5, 0.9, 1.0):
            words = cref.pack(rng.random(state.size) < density)
            exp = cref.gain_unseen(state, words, cand, R, HD, *F90, casts=casts)
            view_gpu._same(_gain_unseen_device(st, Mask(state.size, words), cand, R, HD, *F90), exp, (dims, R, density))
            assert exp["counters"][1] < plain["counters"][1] and (density < 1.0) == (exp["counters"][1] > 0)


def test_a_mask_at_the_largest_range():
    dims = (65, 67, 66)
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.02, 9)
    centre = (33 * ny + 33) * nx + 32
    cand = np.concatenate([[centre], np.random.default_rng(5).integers(0, state.size, 7)]).astype(np.int64)
    words = cref.pack(np.random.default_rng(6).random(state.size) < 0.5)
    exp = cref.gain_unseen(state, words, cand, 32, HD, *F90)
    assert exp["counters"][2] > 1000 and exp["counters"][3] > 1000
    view_gpu._same(_gain_unseen_device(_dev(state), Mask(state.size, words), cand, 32, HD, *F90), exp, "R = 32")


# ------------------------------------------------------------------------------------------------ 2. the mark
@pytest.mark.parametrize("dims", [(9, 8, 7), (17, 9, 20)], ids=lambda d: "%dx%dx%d" % d)
def test_single_marks_match_the_oracle(dims):
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.1, nx + ny + nz)
    st = _dev(state)
    rng = np.random.default_rng(11)
    for R in (2, 7):
        words = cref.pack(rng.random(state.size) < 0.2)
        mask = Mask(state.size, words)
        owner_np = np.full(state.shape, POISON16, np.int16)
        owner = _dev(owner_np)
        turned = 0
        for tag, (v, h) in enumerate(zip(rng.integers(0, state.size, 6).tolist(), [-1, 0, 13, 25, 7, -1])):
            tag = 32767 if tag == 5 else tag
            before = _gain_unseen_device(st, mask, [v], R, HD, *F90)
            exp = cref.mark(state, words, [v], [h], R, HD, *F90, owner_np, tag)["counters"]
            got = _mark_device(st, mask, [v], [h], R, HD, *F90, owner, tag)
            assert got == exp, (dims, R, v, h, got, exp)
            assert h < 0 or got[4] == int(before["gain"][0][h])
            assert mask.host().tobytes() == words.tobytes() and owner.cpu().numpy().tobytes() == owner_np.tobytes()
            again = _mark_device(st, mask, [v], [h], R, HD, *F90, owner, (tag + 1) % 32768)
            assert again == exp[:4] + [0] and mask.host().tobytes() == words.tobytes()
            assert owner.cpu().numpy().tobytes() == owner_np.tobytes()
            turned += got[4]
        assert turned > 10


def test_batches_of_marks_give_the_union():
    dims = (17, 9, 20)
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.1, nx + ny + nz)
    st = _dev(state)
    rng = np.random.default_rng(12)
    # 64 rows with mixed headings, two of them outside the grid, into a mask that is not empty
    cells = np.concatenate([rng.integers(0, state.size, 62), [-1, state.size]]).astype(np.int64)
    hof = [int(h) for h in rng.integers(-1, 26, 64)]
    hof[:3] = [-1, 0, 25]
    words = cref.pack(rng.random(state.size) < 0.3)
    mask = Mask(state.size, words)
    was = cref.popcount(words)
    exp = cref.mark(state, words, cells, hof, 7, HD, *F90)["counters"]
    got = _mark_device(st, mask, cells, hof, 7, HD, *F90)
    assert got == exp and got[0] == 62 and got[4] == cref.popcount(words) - was > 100
    assert mask.host().tobytes() == words.tobytes()
    # every candidate in any heading: the seeable cells; one heading for all 3060 rows is one launch
    every = np.arange(state.size, dtype=np.int64)
    total, seen = cref.seeable(state, every, 2, HD, *F90)
    mask = Mask(state.size)
    got = _mark_device(st, mask, every, [-1] * len(every), 2, HD, *F90)
    assert got[0] == state.size and got[4] == total == cref.popcount(mask.host()) and mask.host().tobytes() == seen.tobytes()
    # and with a heading per row: three launches of at most 1024 rows, the headings change across them
    hof = [(i % 27) - 1 for i in range(len(every))]
    words = np.zeros(cref.seen_words(state.size), np.uint32)
    exp = cref.mark(state, words, every, hof, 2, HD, *F90)["counters"]
    mask = Mask(state.size)
    assert _mark_device(st, mask, every, hof, 2, HD, *F90) == exp and mask.host().tobytes() == words.tobytes()
    # no row: the counters are zeroed, nothing else happens
    assert _mark_device(st, mask, [], [], 2, HD, *F90) == [0, 0, 0, 0, 0] and mask.host().tobytes() == words.tobytes()


@pytest.mark.parametrize("dims", [(33, 1, 1), (10, 6, 5)], ids=lambda d: "%dx%dx%d" % d)
def test_a_mark_at_the_masks_end(dims):
    nx, ny, nz = dims
    state = np.zeros((nz, ny, nx), np.uint8)
    cells = state.size
    assert cells in (33, 300) and cells & 31
    mask = Mask(cells)
    words = np.zeros(cref.seen_words(cells), np.uint32)
    exp = cref.mark(state, words, [cells - 2], [-1], 2, HD, *F180)["counters"]
    assert _mark_device(_dev(state), mask, [cells - 2], [-1], 2, HD, *F180) == exp and exp[4] >= 3
    got = mask.host()
    assert got.tobytes() == words.tobytes() and (int(got[-1]) >> ((cells - 1) & 31)) & 1     # the last cell's bit
    assert int(got[-1]) >> (cells & 31) == 0                                                 # and none above it


# ------------------------------------------------------------------------------------------------ 3. the arguments
def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    shape = (3, 4, 5)
    state = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    mask = Mask(60)
    cand = torch.zeros(2, dtype=torch.int64, device=DEV)
    gain = torch.full((2, 2), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    owner = torch.full(shape, POISON16, dtype=torch.int16, device=DEV)
    sp = L.stream_ptr()
    s, m, ca, g, v, b, c, o = (t.data_ptr() for t in (state, mask.words, cand, gain, visible, best, counters, owner))
    ints = lambda *a: (ctypes.c_int * len(a))(*a)               # noqa: E731
    hd = ints(1, 0, 0, 0, 0, -1)
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    G, M = lib.pi3_grid_view_gain_unseen, lib.pi3_grid_view_mark
    two, one = ints(0, -1), ints(1)
    calls = [lambda: G(s, 5, 4, 3, None, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),               # a null mask
             lambda: G(None, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, None, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, None, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, None, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, None, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, v, None, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, v, b, None, sp),
             lambda: G(s, 5, 4, 3, m, ca, -1, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 0, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 33, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 0, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, ints(*([1, 0, 0] * 33)), 33, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, ints(1, 0, 0, 0, 0, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, ints(1, 0, 0, 0, 1025, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 0, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, -2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 1 << 31, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, -1, 2, g, v, b, c, sp),
             lambda: G(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 3, 2, g, v, b, c, sp),
             lambda: G(s, 5, -4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: G(s, *big, m, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: M(s, 5, 4, 3, None, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),             # a null mask
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, o, 0, c, sp),                   # an owner and two rows
             lambda: M(s, 5, 4, 3, m, ca, one, 1, 4, hd, 2, 1, 2, o, -1, c, sp),                  # the tag
             lambda: M(s, 5, 4, 3, m, ca, one, 1, 4, hd, 2, 1, 2, o, 32768, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 32768, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, ints(0, 2), 2, 4, hd, 2, 1, 2, None, 0, c, sp),         # a heading that is none
             lambda: M(s, 5, 4, 3, m, ca, ints(-2, 0), 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(None, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, None, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, None, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, None, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, None, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, -1, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 0, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 33, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 0, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, ints(*([1, 0, 0] * 33)), 33, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, ints(1, 0, 0, 0, 0, 0), 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, ints(1, 0, 0, 0, 1025, 0), 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 0, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, -2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 1 << 31, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, -1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 3, 2, None, 0, c, sp),
             lambda: M(s, 5, -4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, *big, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp)]
    names = [b"gain_unseen"] * 22 + [b"mark"] * 26
    assert len(calls) == len(names)
    for i, (call, name) in enumerate(zip(calls, names)):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert err.startswith(b"pi3_grid_view_" + name + b":") and b"2^27" in err, (i, err)
    torch.cuda.synchronize()
    assert counters.tolist() == [POISON64] * 5 and not mask.host().any() and bool((owner == POISON16).all())
    assert bool((gain == POISON32).all()) and bool((visible == POISON32).all()) and bool((best == POISON32).all())


# ------------------------------------------------------------------------------------------------ 4. the box room
BOX_RANGE_CELLS = 8


@pytest.fixture(scope="module")
def box_room():
    from pi3_slam_amd.dense_map import OccupancyGrid
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    dist = rref.distances(rref.walk_mask(state, d2a, min_d2), lin)
    cand = vref.candidates(dist, origin, 4)
    cost = dist.reshape(-1)[cand].astype(np.int64)
    full = cref.cover(state, cand, cost, BOX_RANGE_CELLS, HD, *F90)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    return grid, centres, dist, full


def _same_cover(found, full, n, dist):
    """The first n rounds of the oracle's cover."""
    assert found.mode == "cover" and len(found.views) == n == found.counts["rounds"] == found.counts["views"]
    assert [(v.cell, v.heading, v.gain) for v in found.views] == full["picks"][:n]
    assert [v.new for v in found.views] == full["new"][:n] and [v.covered for v in found.views] == full["covered"][:n]
    assert [v.rank for v in found.views] == list(range(n)) and [v.visible for v in found.views] == full["visible"][:n]
    assert all(v.cost == int(dist.reshape(-1)[v.cell]) and v.axis.tolist() == HD[v.heading].tolist() for v in found.views)
    by = np.where(full["seen_by"] < n, full["seen_by"], -1).astype(np.int16)
    assert found.seen_by.dtype == np.int16 and found.seen_by.tobytes() == by.tobytes()
    c = found.counts
    assert c["seeable"] == full["seeable"] == 13828 and c["covered"] == full["covered"][n - 1] == int((by >= 0).sum())
    assert c["unknown"] == 46000 and c["candidates"] == 230 and 0 < c["recomputed_rows"] < c["rounds"] * c["candidates"]
    assert c["mark_rays"] > c["covered"]


def test_box_room_through_the_cover(box_room):
    from pi3_slam_amd.view_planner import ViewPlanner
    grid, centres, dist, full = box_room
    cell = float(grid.cell)
    args = (route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4)
    ten = ViewPlanner(*args, 10).cover(grid, centres, DEV)
    print(f"box room, ten views: {ten.counts}")
    _same_cover(ten, full, 10, dist)
    assert ten.counts["covered"] == 3016 and ten.settings["mode"] == "cover" and ten.settings["until"] is None
    assert ten.settings["separation_m"] is None and ten.settings["range_cells"] == 8
    # the first pass is find's: the same maps, the same counters
    plain = ViewPlanner(*args, 10).find(grid, centres, DEV)
    assert plain.mode == "gain" and plain.seen_by is None and "seeable" not in plain.counts
    assert ten.gain.tobytes() == plain.gain.tobytes() and ten.heading.tobytes() == plain.heading.tobytes()
    for k in ("candidates", "rays", "rays_blocked", "rays_visible", "reachable", "best_gain", "low_gain"):
        assert ten.counts[k] == plain.counts[k], k
    first = ten.views[0]
    route = ten.route_to(0)
    assert route.cells.tolist()[-1] == first.cell == 18671 and route.cost == first.cost == int(dist.reshape(-1)[first.cell])
    assert route.waypoints[-1].tolist() == first.position.tolist()
    half = ViewPlanner(*args, 1000).cover(grid, centres, DEV, until=0.5)
    _same_cover(half, full, 29, dist)
    assert half.settings["until"] == 0.5 and half.counts["covered"] >= 6914 > half.views[-2].covered
    every = ViewPlanner(*args, 1000).cover(grid, centres, DEV)
    _same_cover(every, full, 267, dist)
    assert every.counts["covered"] == every.counts["seeable"] and len({v.cell for v in every.views}) == 145
    low = ViewPlanner(*args, 1000, min_gain=50).cover(grid, centres, DEV)
    _same_cover(low, full, 79, dist)
    assert low.counts["covered"] == 11511


# ------------------------------------------------------------------------------------------------ 5. end to end
def _files(d):
    """A views directory's bytes; of the archive every member's (its zip header carries the time of writing)."""
    out = {n: open(d / n, "rb").read() for n in ("views.json", "views.ply")}
    with np.load(d / "views.npz") as z:
        out.update({"npz/" + k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files})
    return out


def test_cli_views_cover_on_a_reconstruction(reconstructed, capsys):   # noqa: F811
    from pi3_slam_amd import cli
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    base = ["views", "--occupancy", occ, "--from-trajectory", tum, "--radius", str(view_gpu.ROUTE_RADIUS), "--range",
            "0.8", "--stride", "2", "--count", "5", "--device", DEV]
    cli.main(base + ["--output", str(tmp / "plain_a")])
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp / "cover"), "--cover", "--route-to", "0"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("views: ")]
    cli.main(base + ["--output", str(tmp / "plain_b")])
    a, b = _files(tmp / "plain_a"), _files(tmp / "plain_b")
    assert a == b and "npz/seen_by" not in a and b'"new"' not in a["views.json"] and b'"mode"' not in a["views.json"]
    assert sorted(os.listdir(tmp / "cover")) == ["route.json", "route.npz", "route.ply", "views.json", "views.npz", "views.ply"]
    rec = json.load(open(tmp / "cover" / "views.json"))
    views, counts = rec["views"], rec["counts"]
    assert 1 <= len(views) <= 5 and rec["settings"]["mode"] == "cover" and rec["settings"]["until"] is None
    assert [v["covered"] for v in views] == np.cumsum([v["new"] for v in views]).tolist()
    assert all(v["new"] == v["gain"] >= 1 for v in views)
    assert [v["gain"] for v in views] == sorted((v["gain"] for v in views), reverse=True)
    with np.load(tmp / "cover" / "views.npz") as z:
        by = z["seen_by"]
        assert by.dtype == np.int16 and z["gain"].tobytes() == a["npz/gain"][2] and z["heading"].tobytes() == a["npz/heading"][2]
    assert views[-1]["covered"] == int((by >= 0).sum()) == counts["covered"] <= counts["seeable"] <= counts["unknown"]
    assert np.bincount(by[by >= 0], minlength=len(views)).tolist() == [v["new"] for v in views]
    assert views[0]["gain"] == json.loads(a["views.json"])["views"][0]["gain"]       # the first pick is find's best
    assert len(line) == 1 and f"covered {counts['covered']} of {counts['seeable']} seeable unknown cells (" in line[0]
    print(line[0])
    way = json.load(open(tmp / "cover" / "route.json"))
    assert way["cost"] == views[0]["cost"] and way["waypoints"][-1] == views[0]["position"]
    with pytest.raises(SystemExit, match="views: --separation has no meaning with --cover"):
        cli.main(base + ["--output", str(tmp / "w"), "--cover", "--separation", "0.4"])
    with pytest.raises(SystemExit, match="views: the fraction to cover must lie in"):
        cli.main(base + ["--output", str(tmp / "w"), "--cover", "--cover-until", "0"])
