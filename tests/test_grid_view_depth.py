"""Unknown space that ends a ray, on the CPU (csrc/grid_view.hip's _depth entry points): the oracle
(tests/grid_view_depth_ref.py) against plain Python over grid_view_ref.between and against hand-made rows, the identity
with the transparent rule, the planner's switch and record, the flag, and the built library's argument checks, which need
no GPU because a refused call launches nothing."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_view_depth_ref as dref          # noqa: E402
import grid_view_ref as vref                # noqa: E402

SHAPE = (17, 19, 21)                        # (nz, ny, nx)
POSE = (9, 9, 12)                           # (x, y, z)
DEPTHS = (0, 1, 2, 3, 5, 8, 13, 255)
SEEN_AT = (48, 174, 340, 513, 751, 824, 827, 827)


def _grid():
    return vref.three_state(SHAPE, 0.5, 0.02, 5)


def _targets(state, v, R):
    """The offsets of v's targets: inside the grid, in the ball, unknown."""
    ball = vref.ball_offsets(R)
    u = np.asarray(v) + ball
    ok = ((u >= 0) & (u < np.array(state.shape[::-1]))).all(1)
    ok[ok] = state[u[ok][:, 2], u[ok][:, 1], u[ok][:, 0]] == 0
    return ball[ok]


# ------------------------------------------------------------------------------------------------ the oracle
def test_the_grid_separates_the_depths():
    state = _grid()
    assert state[POSE[2], POSE[1], POSE[0]] != 2
    offs = _targets(state, POSE, 8)
    assert len(offs) == 912
    seen = [int(dref.rays_depth(state, POSE, offs, d).sum()) for d in DEPTHS]
    assert tuple(seen) == SEEN_AT
    assert int(vref.rays(state, POSE, offs).sum()) == 827


def test_rays_depth_against_plain_python():
    state = _grid()
    rng = np.random.default_rng(1)
    poses = [POSE] + [tuple(int(rng.integers(0, n)) for n in SHAPE[::-1]) for _ in range(3)]
    rays = 0
    for v in poses:
        offs = _targets(state, v, 8)
        tied = np.abs(offs)
        # every kind of offset is there: three tied axes, two tied axes, one and two zero components
        assert ((tied[:, 0] == tied[:, 1]) & (tied[:, 1] == tied[:, 2])).any()
        assert ((tied[:, 0] == tied[:, 1]) & (tied[:, 1] != tied[:, 2]) & (tied[:, 0] > 0)).any()
        assert ((offs == 0).sum(1) == 1).any() and ((offs == 0).sum(1) == 2).any()
        for d in (0, 1, 2, 5, 255):
            got = dref.rays_depth(state, v, offs, d)
            exp = np.array([dref.ray_brute(state, v, o, d) for o in offs.tolist()])
            assert (got == exp).all(), (v, d)
            rays += len(offs)
    assert rays > 10000


def test_the_row_table():
    row = np.array([1, 1, 0, 0, 2, 0], np.uint8).reshape(1, 1, 6)
    table = {0: (True, False, False), 1: (True, True, False), 2: (True, True, False)}
    for d, exp in table.items():
        got = tuple(bool(dref.rays_depth(row, [0, 0, 0], [[x, 0, 0]], d)[0]) for x in (2, 3, 5))
        assert got == exp, d
    # the target's own state never counts, the pose's neither: an unknown pose next to its unknown target
    pair = np.zeros((1, 1, 2), np.uint8)
    assert dref.rays_depth(pair, [0, 0, 0], [[1, 0, 0]], 0).tolist() == [True]


def test_the_corridor():
    g = np.ones((1, 1, 12), np.uint8)
    g[0, 0, 4:] = 0
    offs = [[x, 0, 0] for x in range(4, 12)]
    assert [int(dref.rays_depth(g, [0, 0, 0], offs, d).sum()) for d in (0, 1, 2, 3, 7)] == [1, 2, 3, 4, 8]


def test_visibility_is_monotone_in_the_depth():
    state = _grid()
    offs = _targets(state, POSE, 8)
    before = np.zeros(len(offs), bool)
    for d in range(0, 15):
        now = dref.rays_depth(state, POSE, offs, d)
        assert not (before & ~now).any(), d
        before = now
    assert (before == vref.rays(state, POSE, offs)).all()      # 12 cells between at the most at R = 8


def test_a_ray_has_at_most_l1_minus_1_cells_between():
    for R, most in ((8, 12), (32, 54), (64, 109)):
        best = 0
        for x in range(R + 1):
            for y in range(x + 1):
                z2 = R * R - x * x - y * y
                if z2 >= 0:
                    best = max(best, x + y + int(np.floor(np.sqrt(z2) + 1e-9)))
        assert best - 1 == most
    assert dref.TRANSPARENT == 110 > 109
    ball = vref.ball_offsets(8)
    longest = ball[np.abs(ball).sum(1) == 13][0]
    assert len(vref.between(longest)) <= 12
    assert max(len(vref.between(o)) for o in ball[::7].tolist()) <= 12


def test_depth_110_and_255_are_the_transparent_rule():
    state = _grid()
    for v in (POSE, (0, 0, 0), (20, 18, 16)):
        offs = _targets(state, v, 8)
        plain = vref.rays(state, v, offs)
        for d in (110, 255):
            assert (dref.rays_depth(state, v, offs, d) == plain).all()
    big = vref.three_state((20, 9, 70), 0.5, 0.002, 5)          # R = 64 from a corner: rays up to 69 cells long
    offs = _targets(big, (0, 0, 0), 64)
    plain = vref.rays(big, (0, 0, 0), offs)
    assert plain.sum() > 1000 and (~plain).sum() > 500        # both answers occur: the fixture can tell them apart
    for d in (110, 255):
        assert (dref.rays_depth(big, (0, 0, 0), offs, d) == plain).all()
    assert (dref.rays_depth(big, (0, 0, 0), offs, 20) != plain).any()


def test_cast_depth_serves_the_cover_oracle():
    import grid_cover_ref as cref
    state = _grid()
    cand = [(POSE[2] * SHAPE[1] + POSE[1]) * SHAPE[2] + POSE[0], 0, -1, state.size]
    hd, (num, den) = vref.headings26(), vref.cos2(90)
    plain = vref.gain(state, cand, 8, hd, num, den)
    same = dref.gain(state, cand, 8, 255, hd, num, den)
    for k in ("gain", "visible", "best"):
        assert same[k].tobytes() == plain[k].tobytes()
    assert same["counters"] == plain["counters"]
    k0, k255 = dref.cast_depth(state, cand, 8, 0), cref.cast(state, cand, 8)
    assert (k0["u"] == k255["u"]).all() and k0["arrived"].sum() < k255["arrived"].sum()
    shallow = dref.gain(state, cand, 8, 0, hd, num, den, casts=k0)
    assert shallow["visible"].tolist()[0] == 48 and shallow["counters"][1] == plain["counters"][1]
    assert shallow["counters"][2] + shallow["counters"][3] == shallow["counters"][1]


# ------------------------------------------------------------------------------------------------ the host side
def test_planner_validation_and_settings():
    from pi3_slam_amd import ops
    from pi3_slam_amd.view_planner import ViewPlanner
    assert ops.VIEW_MAX_DEPTH == 255
    plain = ViewPlanner(0, 1.0).settings()
    assert "unknown_depth" not in plain and plain["unknown_is_transparent"] is True
    assert ViewPlanner(0, 1.0, unknown_depth=None).settings() == plain
    for k in (0, 2, 255, np.int64(7)):
        st = ViewPlanner(0, 1.0, unknown_depth=k).settings()
        assert st["unknown_depth"] == int(k) and type(st["unknown_depth"]) is int
        assert st["unknown_is_transparent"] is False
        assert {a: b for a, b in st.items() if a not in ("unknown_depth", "unknown_is_transparent")} == {
            a: b for a, b in plain.items() if a != "unknown_is_transparent"}
        assert list(st)[:len(plain)] == list(plain)             # the record's other keys keep their order
    both = ViewPlanner(0, 3.3, far=True, unknown_depth=3).settings()
    assert both["far"] is True and both["unknown_depth"] == 3
    for bad in (-1, 256, True, False, 1.0, 2.5, "2"):
        with pytest.raises(ValueError, match="unknown_depth must be an integer in 0 .. 255 or None"):
            ViewPlanner(0, 1.0, unknown_depth=bad)


def test_flag_parses_and_the_help_says_what_it_is():
    from pi3_slam_amd import cli
    base = ["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"]
    assert cli.build_parser().parse_args(base).unknown_depth is None
    a = cli.build_parser().parse_args(base + ["--unknown-depth", "2", "--far", "--cover", "--tour", "--taut"])
    assert a.unknown_depth == 2 and a.far and a.cover and a.tour and a.taut
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert "--unknown-depth K" in text and "no measured optimum" in text and "transparent" in text
    assert "[--unknown-depth K]" in cli.__doc__
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--unknown-depth", "1.5"])
    for other in ("route", "frontiers"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([other, "--unknown-depth", "1"])


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    for name, base, extra in (("pi3_grid_view_gain_depth", "pi3_grid_view_gain_unseen", 2),
                              ("pi3_grid_view_mark_depth", "pi3_grid_view_mark", 2)):
        args = [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % name, text).group(1).split(",")]
        old = [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % base, text).group(1).split(",")]
        assert len(args) == len(lib.SIGNATURES[name]) == len(old) + extra
        at = args.index("range")
        assert args[at:at + 3] == ["range", "depth", "far"] and args[:at + 1] + args[at + 3:] == old
        sig, was = lib.SIGNATURES[name], lib.SIGNATURES[base]
        assert sig[:at + 1] + sig[at + 3:] == was and sig[at + 1:at + 3] == [ctypes.c_int, ctypes.c_int]


def test_the_library_has_the_symbols_and_refuses_bad_arguments_without_a_gpu():
    from pi3_slam_amd import lib as L
    lib = L.load(require_gpu=False)
    assert lib.pi3_abi_version() == 7
    G, M = lib.pi3_grid_view_gain_depth, lib.pi3_grid_view_mark_depth
    # never dereferenced: a refused call returns before anything is launched or read on the host side but the headings
    p = 4096
    ints = lambda *a: (ctypes.c_int * len(a))(*a)               # noqa: E731
    hd, two = ints(1, 0, 0, 0, 0, -1), ints(0, -1)
    gain = lambda **k: G(k.get("state", p), 5, 4, 3, k.get("seen", None), p, 2, k.get("range", 4), k.get("depth", 1),  # noqa: E731
                         k.get("far", 0), hd, 2, 1, 2, p, p, p, k.get("counters", p), None)
    mark = lambda **k: M(k.get("state", p), 5, 4, 3, k.get("seen", p), p, two, 2, k.get("range", 4), k.get("depth", 1),  # noqa: E731
                         k.get("far", 0), hd, 2, 1, 2, None, 0, k.get("counters", p), None)
    cases = [dict(state=None), dict(counters=None), dict(depth=-1), dict(depth=256), dict(range=33, far=0),
             dict(range=65, far=1), dict(range=0)]
    for call, name in ((gain, b"pi3_grid_view_gain_depth:"), (mark, b"pi3_grid_view_mark_depth:")):
        for case in cases:
            assert call(**case) == -1, case
            err = lib.pi3_last_error()
            d = case.get("depth", 1)
            assert err.startswith(name) and (b" depth=%d (0 .. 255)" % d) in err, (case, err)
            most = 64 if case.get("far") else 32
            assert (b"range=%d (1 .. %d)" % (case.get("range", 4), most)) in err and b"null pointer" in err, (case, err)
    assert mark(seen=None) == -1 and b"depth=1 (0 .. 255)" in lib.pi3_last_error()
    # the far form's word on the cone stays with the far form
    assert gain(range=65, far=1) == -1 and b"< 2^63" in lib.pi3_last_error()
    assert gain(range=33, far=0) == -1 and b"< 2^63" not in lib.pi3_last_error()
