"""Views that see farther on the GPU (csrc/grid_view.hip: pi3_grid_view_gain_far, pi3_grid_view_gain_unseen_far,
pi3_grid_view_mark_far), byte for byte against the oracles as they stand (tests/grid_view_ref.py,
tests/grid_cover_ref.py have no range limit), against the near entry points up to 32 cells, against the lattice alone on
an open ball of 64 cells, and against themselves under the 48 signed axis permutations.  Every output is filled with a
poison value before each call, and every mask has two guard words behind it."""
import ctypes
import itertools
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
import test_grid_cover_gpu as cover_gpu     # noqa: E402  (its guarded mask)
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_gpu as view_gpu       # noqa: E402  (its states, candidates and comparison)

pytestmark = pytest.mark.gpu
DEV = view_gpu.DEV
POISON32, POISON64, POISON16 = view_gpu.POISON32, view_gpu.POISON64, cover_gpu.POISON16
HD = vref.headings26()
F90 = vref.cos2(90)
Mask = cover_gpu.Mask
_dev = view_gpu._dev
_same = view_gpu._same


def _gain(state, cand, R, headings, num, den, far=False, mask=None):
    """ops.grid_view_gain, or with a mask ops.grid_view_gain_unseen, into poisoned outputs."""
    from pi3_slam_amd import ops
    V, H = len(cand), len(headings)
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    cells = _dev(np.asarray(cand, np.int64))
    if mask is None:
        ops.grid_view_gain(state, cells, R, headings, num, den, gain, visible, best, counters, far=far)
    else:
        before = mask.host()
        ops.grid_view_gain_unseen(state, mask.words, cells, R, headings, num, den, gain, visible, best, counters, far=far)
        assert mask.host().tobytes() == before.tobytes()        # read only
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _mark(state, mask, cells, heading_of, R, headings, num, den, owner=None, tag=0, far=False):
    from pi3_slam_amd import ops
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_mark(state, mask.words, _dev(np.asarray(cells, np.int64)), heading_of, R, headings, num, den, counters,
                       owner, tag, far=far)
    return counters.tolist()


def _lin(shape, z, y, x):
    return (z * shape[1] + y) * shape[2] + x


# ------------------------------------------------------------------------------------------------ 1. the oracle's cases
def _line():
    state = np.zeros((1, 1, 140), np.uint8)
    state[0, 0, 100] = 2
    return state


SMALL = (20, 9, 70)
SMALL_CAND = [0, 69, 6615, 12599]
TABLE = {
    "line-64": (_line, 64, [0, 70, 139], [64, 93, 38], None, [3, 254, 59, 195]),
    "small-33": (lambda: vref.three_state(SMALL, 0.5, 0.02, 5), 33, SMALL_CAND, [1588, 1704, 3409, 651], [25, 20, 13, 0],
                 [4, 14293, 6941, 7352]),
    "small-64": (lambda: vref.three_state(SMALL, 0.5, 0.02, 5), 64, SMALL_CAND, [2337, 2691, 3568, 651], [22, 20, 13, 0],
                 [4, 23508, 14261, 9247]),
    "open-33": (lambda: np.zeros((69, 67, 70), np.uint8), 33, [_lin((69, 67, 70), 34, 33, 34)], [150554], [0],
                [1, 150554, 0, 150554]),
    "large-64": (lambda: vref.three_state((129, 40, 131), 0.4, 0.002, 7), 64, [_lin((129, 40, 131), 64, 20, 65), 0],
                 [177352, 41182], [5, 25], [2, 244860, 26326, 218534]),
}


@pytest.mark.parametrize("case", list(TABLE))
def test_gain_matches_the_oracle_beyond_32_cells(case):
    make, R, cand, visible, best, counters = TABLE[case]
    state = make()
    exp = vref.gain(state, cand, R, HD, *F90)
    got = _gain(_dev(state), cand, R, HD, *F90)
    print(case, got["visible"].tolist(), got["best"].tolist(), got["counters"])
    _same(got, exp, case)
    assert got["visible"].tolist() == visible and got["counters"] == counters
    assert best is None or got["best"].tolist() == best


def test_the_open_ball_of_64_cells_from_the_lattice_alone():
    shape = (129, 129, 129)
    state = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    got = _gain(state, [_lin(shape, 64, 64, 64)], 64, HD, *F90)
    ball = vref.ball_offsets(64)
    assert len(ball) == 1097916
    assert got["visible"].tolist() == [1097916] and got["counters"] == [1, 1097916, 0, 1097916]
    cone = np.array([int(vref.in_cone(ball, a, *F90).sum()) for a in HD], np.uint32)
    assert got["gain"][0].tobytes() == cone.tobytes() and got["best"].tolist() == [int(np.argmax(cone))]


# ------------------------------------------------------------------------------------------------ 2. far equals near
@pytest.mark.parametrize("dims", [(9, 8, 7), (17, 9, 20)], ids=lambda d: "%dx%dx%d" % d)
def test_far_gives_the_near_bytes_up_to_32_cells(dims):
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.1, nx + ny + nz)
    st = _dev(state)
    cand = view_gpu._candidates(dims, sum(dims))                # every cell; or corners, 64 seeded cells and one outside
    rng = np.random.default_rng(21)
    words = cref.pack(rng.random(state.size) < 0.4)
    hof = [int(h) for h in rng.integers(-1, 26, len(cand))]
    for R in (1, 2, 7, 32):
        near = _gain(st, cand, R, HD, *F90)
        _same(_gain(st, cand, R, HD, *F90, far=True), near, (dims, R, "gain"))
        assert near["counters"][0] == len(cand) - (state.size > 600) and near["counters"][3] > 0
        near = _gain(st, cand, R, HD, *F90, mask=Mask(state.size, words))
        _same(_gain(st, cand, R, HD, *F90, far=True, mask=Mask(state.size, words)), near, (dims, R, "unseen"))
        for rows in (hof, [-1] * len(cand)):
            a, b = Mask(state.size, words), Mask(state.size, words)
            assert _mark(st, b, cand, rows, R, HD, *F90, far=True) == _mark(st, a, cand, rows, R, HD, *F90)
            assert a.host().tobytes() == b.host().tobytes() != words.tobytes()
        owners = [torch.full(state.shape, POISON16, dtype=torch.int16, device=DEV) for _ in range(2)]
        a, b = Mask(state.size, words), Mask(state.size, words)
        got = [_mark(st, m, cand[5:6], [3], R, HD, *F90, o, 9, far=f) for m, o, f in ((a, owners[0], False), (b, owners[1], True))]
        assert got[0] == got[1] and a.host().tobytes() == b.host().tobytes() and torch.equal(owners[0], owners[1])


def test_far_gives_the_near_bytes_at_32_cells_on_the_mixed_grid():
    dims = (65, 67, 66)                                         # test_grid_view_gpu.test_gain_at_the_largest_range's
    nx, ny, nz = dims
    mixed = vref.three_state((nz, ny, nx), 0.5, 0.02, 9)
    centre = (33 * ny + 33) * nx + 32
    cand = np.concatenate([[centre], np.random.default_rng(5).integers(0, mixed.size, 7)]).astype(np.int64)
    st = _dev(mixed)
    near = _gain(st, cand, 32, HD, *F90)
    assert near["counters"][2] > 1000 and near["counters"][3] > 1000
    _same(_gain(st, cand, 32, HD, *F90, far=True), near, "gain")
    words = cref.pack(np.random.default_rng(6).random(mixed.size) < 0.5)
    _same(_gain(st, cand, 32, HD, *F90, far=True, mask=Mask(mixed.size, words)),
          _gain(st, cand, 32, HD, *F90, mask=Mask(mixed.size, words)), "unseen")
    a, b = Mask(mixed.size, words), Mask(mixed.size, words)
    hof = [0, 25, -1, 13, 7, 7, -1, 2]
    assert _mark(st, b, cand, hof, 32, HD, *F90, far=True) == _mark(st, a, cand, hof, 32, HD, *F90)
    assert a.host().tobytes() == b.host().tobytes() != words.tobytes()


# ------------------------------------------------------------------------------------------------ 3. symmetry
def _signed_permutations():
    return [(perm, flips) for perm in itertools.permutations(range(3)) for flips in itertools.product((False, True), repeat=3)]


def _moved(a, perm, flips):
    """An array (n, n, n) under a signed permutation of its axes."""
    a = np.transpose(a, perm)
    for ax, f in enumerate(flips):
        if f:
            a = np.flip(a, ax)
    return np.ascontiguousarray(a)


def test_the_48_signed_axis_permutations_see_the_same():
    n, c, R = 67, 33, 33
    state = vref.three_state((n, n, n), 0.5, 0.02, 17)
    centre = [_lin(state.shape, c, c, c)]
    z, y, x = np.meshgrid(*[np.arange(n) - c] * 3, indexing="ij")           # every cell's offset from the centre
    index_of = {tuple(a): h for h, a in enumerate(HD.tolist())}
    first = _gain(_dev(state), centre, R, HD, *F90)
    _same(first, vref.gain(state, centre, R, HD, *F90), "the first orientation")
    assert first["counters"][2] > 1000 and first["counters"][3] > 1000 and len(set(first["gain"][0].tolist())) > 13
    moves = _signed_permutations()
    assert len(moves) == 48
    for perm, flips in moves:
        got = _gain(_dev(_moved(state, perm, flips)), centre, R, HD, *F90)
        assert got["visible"].tolist() == first["visible"].tolist() and got["counters"] == first["counters"], (perm, flips)
        # where the moved grid has the offset a, the first one had `was`: the heading a now sees what `was` saw
        mx, my, mz = (_moved(k, perm, flips) for k in (x, y, z))
        was = [index_of[(int(mx[c + a[2], c + a[1], c + a[0]]), int(my[c + a[2], c + a[1], c + a[0]]),
                         int(mz[c + a[2], c + a[1], c + a[0]]))] for a in HD.tolist()]
        assert sorted(was) == list(range(26))
        assert got["gain"][0].tolist() == first["gain"][0][was].tolist(), (perm, flips)


# ------------------------------------------------------------------------------------------------ 4. flat grids
@pytest.mark.parametrize("shape", [(1, 70, 70), (70, 1, 70)], ids=lambda s: "%dx%dx%d" % s)
def test_flat_grids_where_every_target_has_a_zero_component(shape):
    state = vref.three_state(shape, 0.5, 0.02, sum(shape))
    nz, ny, nx = shape
    last = [n - 1 for n in shape]
    half = [n // 2 for n in shape]
    cand = [_lin(shape, zz, yy, xx) for zz in sorted({0, last[0]}) for yy in sorted({0, last[1]}) for xx in (0, last[2])]
    cand += [_lin(shape, half[0], half[1], 0), _lin(shape, half[0], half[1], last[2]),
             _lin(shape, 0, 0, half[2]), _lin(shape, last[0], last[1], half[2])]
    assert len(cand) == 8 and len(set(cand)) == 8
    exp = vref.gain(state, cand, 33, HD, *F90)
    assert exp["counters"][2] > 100 and exp["counters"][3] > 1000
    _same(_gain(_dev(state), cand, 33, HD, *F90), exp, shape)


# ------------------------------------------------------------------------------------------------ 5. unseen and mark
@pytest.mark.parametrize("R", [33, 64])
def test_unseen_and_mark_beyond_32_cells(R):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    st = _dev(state)
    cand = SMALL_CAND
    casts = cref.cast(state, cand, R)
    rng = np.random.default_rng(R)
    # the unseen gain: a zero mask gives the plain bytes, a seeded one the oracle's
    plain = _gain(st, cand, R, HD, *F90)
    _same(_gain(st, cand, R, HD, *F90, mask=Mask(state.size)), plain, "zero mask")
    words = cref.pack(rng.random(state.size) < 0.5)
    exp = cref.gain_unseen(state, words, cand, R, HD, *F90, casts=casts)
    assert 0 < exp["counters"][1] < plain["counters"][1]
    _same(_gain(st, cand, R, HD, *F90, mask=Mask(state.size, words)), exp, "seeded mask")
    # marks: any heading, and a heading per row
    for hof in ([-1] * 4, [25, -1, 13, 0]):
        words = cref.pack(rng.random(state.size) < 0.2)
        mask = Mask(state.size, words)
        exp = cref.mark(state, words, cand, hof, R, HD, *F90, casts=casts)["counters"]
        assert _mark(st, mask, cand, hof, R, HD, *F90) == exp and exp[4] > 100
        assert mask.host().tobytes() == words.tobytes()
    # one row with an owner
    words = cref.pack(rng.random(state.size) < 0.2)
    mask = Mask(state.size, words)
    owner_np = np.full(state.shape, POISON16, np.int16)
    owner = _dev(owner_np)
    exp = cref.mark(state, words, cand[2:3], [13], R, HD, *F90, owner_np, 77)["counters"]
    assert _mark(st, mask, cand[2:3], [13], R, HD, *F90, owner, 77) == exp and exp[4] > 100
    assert mask.host().tobytes() == words.tobytes() and owner.cpu().numpy().tobytes() == owner_np.tobytes()
    # two rows that see the same cells: each new bit is counted by exactly one of them
    mask = Mask(state.size)
    got = _mark(st, mask, [cand[2], cand[2]], [-1, -1], R, HD, *F90)
    assert got[0] == 2 and got[3] == 2 * got[4] and got[4] == cref.popcount(mask.host()) > 100
    mask = Mask(state.size)
    got = _mark(st, mask, [cand[2], cand[2] + 1], [13, 13], R, HD, *F90)      # neighbours looking the same way
    assert got[0] == 2 and got[3] > got[4] == cref.popcount(mask.host()) > 100


# ------------------------------------------------------------------------------------------------ 6. the arguments
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
    wide = ints(1024, 1024, 1024, 1, 0, 0)                      # |a|^2 = 3 * 2^20: at range 64 den may be at most 715827882
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    P, U, M = lib.pi3_grid_view_gain_far, lib.pi3_grid_view_gain_unseen_far, lib.pi3_grid_view_mark_far
    two, one = ints(0, -1), ints(1)
    calls = [lambda: P(s, 5, 4, 3, ca, 2, 0, hd, 2, 1, 2, g, v, b, c, sp),                      # the range
             lambda: P(s, 5, 4, 3, ca, 2, 65, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 64, wide, 2, 1, 715827883, g, v, b, c, sp),           # the cone's 64 bits
             lambda: P(s, 5, 4, 3, ca, 2, 48, wide, 2, 1, (1 << 31) - 1, g, v, b, c, sp),       # 48^2 * 3 * 2^20 * 2^31 > 2^63
             lambda: P(None, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),                   # the namesake's cases
             lambda: P(s, 5, 4, 3, None, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, None, 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, None, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, None, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, None, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, None, sp),
             lambda: P(s, 5, 4, 3, ca, -1, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 0, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, ints(*([1, 0, 0] * 33)), 33, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, ints(1, 0, 0, 0, 0, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, ints(1, 0, 0, 0, 1025, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 0, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 1 << 31, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, -1, 2, g, v, b, c, sp),
             lambda: P(s, 5, 4, 3, ca, 2, 4, hd, 2, 3, 2, g, v, b, c, sp),
             lambda: P(s, 5, -4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: P(s, *big, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: U(s, 5, 4, 3, None, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),                # a null mask
             lambda: U(s, 5, 4, 3, m, ca, 2, 0, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: U(s, 5, 4, 3, m, ca, 2, 65, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: U(s, 5, 4, 3, m, ca, 2, 64, wide, 2, 1, 715827883, g, v, b, c, sp),
             lambda: U(s, 5, 4, 3, m, None, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: U(s, 5, 4, 3, m, ca, 2, 4, hd, 2, 1, 2, g, v, None, c, sp),
             lambda: U(s, *big, m, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: M(s, 5, 4, 3, None, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),           # a null mask
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 0, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 65, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 64, wide, 2, 1, 715827883, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, o, 0, c, sp),                 # an owner and two rows
             lambda: M(s, 5, 4, 3, m, ca, one, 1, 4, hd, 2, 1, 2, o, -1, c, sp),                # the tag
             lambda: M(s, 5, 4, 3, m, ca, one, 1, 4, hd, 2, 1, 2, o, 32768, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, ints(0, 2), 2, 4, hd, 2, 1, 2, None, 0, c, sp),       # a heading that is none
             lambda: M(s, 5, 4, 3, m, ca, ints(-2, 0), 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(None, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, None, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, None, 2, 4, hd, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, None, 2, 1, 2, None, 0, c, sp),
             lambda: M(s, 5, 4, 3, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, None, sp),
             lambda: M(s, *big, m, ca, two, 2, 4, hd, 2, 1, 2, None, 0, c, sp)]
    names = [b"gain_far"] * 22 + [b"gain_unseen_far"] * 7 + [b"mark_far"] * 15
    assert len(calls) == len(names)
    for i, (call, name) in enumerate(zip(calls, names)):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert err.startswith(b"pi3_grid_view_" + name + b":") and b"2^27" in err and b"range=" in err, (i, err)
        assert b"(1 .. 64)" in err and b"range^2 * max |axis|^2 * den < 2^63" in err, (i, err)
    torch.cuda.synchronize()
    assert counters.tolist() == [POISON64] * 5 and not mask.host().any() and bool((owner == POISON16).all())
    assert bool((gain == POISON32).all()) and bool((visible == POISON32).all()) and bool((best == POISON32).all())


def test_the_cone_just_inside_its_64_bits():
    """range^2 max|a|^2 den = 64^2 * 3 * 2^20 * 715827882 = 2^63 - 2^33: the largest den the far form takes there."""
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    axes = np.array([(1024, 1024, 1024), (-1024, 1024, -1024), (1024, 0, 0), (3, -2, 1)], np.int64)
    den = 715827882
    assert 64 * 64 * 3 * 1024 * 1024 * den < 1 << 63 <= 64 * 64 * 3 * 1024 * 1024 * (den + 1)
    for num in (den // 2, den, 0):
        exp = vref.gain(state, SMALL_CAND, 64, axes, num, den)
        _same(_gain(_dev(state), SMALL_CAND, 64, axes, num, den), exp, num)
    assert exp["counters"][3] > 1000


# ------------------------------------------------------------------------------------------------ 7. planner and cli
BOX_RANGE_CELLS, BOX_STRIDE = 33, 8


def test_box_room_through_the_far_planner(tmp_path, capsys):
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner
    room, state, cams, d2u, walk_u, (Rb, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    dist = rref.distances(rref.walk_mask(state, oref.edt_ref(state, Rb, False), min_d2), lin)
    range_m = (BOX_RANGE_CELLS - 0.1) * cell                    # ceil: 33 cells, whatever the division rounds to
    planner = ViewPlanner(route_cases.BOX_RADIUS, range_m, 90, BOX_STRIDE, 10, far=True)
    R, sep, max_cost = planner.cells_of(cell)
    assert (R, max_cost) == (BOX_RANGE_CELLS, vref.FAR - 1)
    cand = vref.candidates(dist, origin, BOX_STRIDE)
    assert 10 <= len(cand) <= 40
    # find
    exp = vref.view_set(state, dist, origin, R, BOX_STRIDE, 90, 10, sep)
    found = planner.find(grid, centres, DEV)
    c = found.counts
    print(f"box room at 33 cells: {c}")
    assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == exp["gain"]["counters"]
    assert c["candidates"] == len(cand) and c["views"] == len(exp["views"]) >= 1 and c["low_gain"] == exp["low_gain"]
    assert found.gain.tobytes() == exp["gain_map"].tobytes() and found.heading.tobytes() == exp["heading_map"].tobytes()
    assert [(v.cell, v.heading, v.gain, v.visible, v.cost) for v in found.views] == [
        (e["cell"], e["heading"], e["gain"], e["visible"], e["cost"]) for e in exp["views"]]
    assert found.settings["far"] is True and found.settings["range_cells"] == 33
    # cover
    cost = dist.reshape(-1)[cand].astype(np.int64)
    full = cref.cover(state, cand, cost, R, HD, *F90, count=3)
    three = ViewPlanner(route_cases.BOX_RADIUS, range_m, 90, BOX_STRIDE, 3, far=True).cover(grid, centres, DEV)
    assert [(v.cell, v.heading, v.gain) for v in three.views] == full["picks"] and len(full["picks"]) == 3
    assert [v.new for v in three.views] == full["new"] and [v.covered for v in three.views] == full["covered"]
    assert [v.visible for v in three.views] == full["visible"] and three.counts["seeable"] == full["seeable"]
    assert three.seen_by.tobytes() == full["seen_by"].tobytes() and three.settings["far"] is True
    # the tour replays its marks (view_tour.py compares each with the view's own count)
    tour = three.tour()
    assert len(tour.stops) == 3
    # the command line
    occ = str(tmp_path / "occupancy.npz")
    export.write_occupancy(grid, occ)
    base = ["views", "--occupancy", occ, "--start"] + [repr(float(v)) for v in centres[0]] + [
        "--radius", str(route_cases.BOX_RADIUS), "--range", repr(range_m), "--stride", str(BOX_STRIDE), "--device", DEV]
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp_path / "v"), "--far"])
    rec = json.load(open(tmp_path / "v" / "views.json"))
    assert rec["settings"]["far"] is True and rec["settings"]["range_cells"] == 33 and len(rec["views"]) >= 1
    with pytest.raises(SystemExit, match="views: a range of .* is 33 cells: at most 32 "):
        cli.main(base + ["--output", str(tmp_path / "w")])
    assert not os.path.exists(tmp_path / "w")
