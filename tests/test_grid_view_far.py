"""Views that see farther, on the CPU (csrc/grid_view.hip): the planner's switch, the constants, the
bindings, the `--far` flag, and the octant rule the kernels rest on, held against things the oracle
(tests/grid_view_ref.py) did not compute."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_view_ref as vref                # noqa: E402

FAR_NAMES = ("pi3_grid_view_gain_far", "pi3_grid_view_gain_unseen_far", "pi3_grid_view_mark_far")


def owner(offs):
    """The octant that casts at each offset (N,3): bit a is set when axis a is negative, and axis a is positive when
    o_a >= 0 (grid_view_ray.h's RayBox::owns)."""
    o = np.asarray(offs, np.int64).reshape(-1, 3)
    return (o[:, 0] < 0) * 1 + (o[:, 1] < 0) * 2 + (o[:, 2] < 0) * 4


def in_closed_octant(q, cells, R):
    """Do the offsets `cells` lie in octant q's staged box: 0 .. R on a positive axis, -R .. 0 on a negative one?"""
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    ok = np.ones(len(c), bool)
    for a in range(3):
        ok &= (c[:, a] <= 0) & (c[:, a] >= -R) if (q >> a) & 1 else (c[:, a] >= 0) & (c[:, a] <= R)
    return ok


# ------------------------------------------------------------------------------------------------ the host side
def test_planner_far_switch():
    from pi3_slam_amd import ops
    from pi3_slam_amd.view_planner import ViewPlanner
    assert ops.VIEW_FAR_MAX_RANGE == 64 and ops.VIEW_MAX_RANGE == 32
    assert ViewPlanner(0, 3.3, far=True).cells_of(0.1)[0] == 33
    assert ViewPlanner(0, 6.4, far=True).cells_of(0.1)[0] == 64
    assert ViewPlanner(0, 1.0, far=True).cells_of(0.1) == ViewPlanner(0, 1.0).cells_of(0.1)
    with pytest.raises(ValueError, match="65 cells: at most 64 .*larger occupancy cell"):
        ViewPlanner(0, 6.5, far=True).cells_of(0.1)
    with pytest.raises(ValueError, match="33 cells: at most 32 .*larger occupancy cell"):
        ViewPlanner(0, 3.3).cells_of(0.1)
    with pytest.raises(ValueError, match="33 cells: at most 32 .*larger occupancy cell"):
        ViewPlanner(0, 3.3, far=False).cells_of(0.1)
    with pytest.raises(ValueError, match="far must be True or False"):
        ViewPlanner(0, 1.0, far=1)
    assert "far" not in ViewPlanner(0, 1.0).settings() and "far" not in ViewPlanner(0.2, 1.6, far=False).settings()
    st = ViewPlanner(0, 3.3, far=True).settings()
    assert st["far"] is True and {k: v for k, v in st.items() if k != "far"} == ViewPlanner(0, 3.3).settings()


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    for name in FAR_NAMES:
        near = name[:-len("_far")]
        assert lib.SIGNATURES[name] == lib.SIGNATURES[near]
        args = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert len(args.split(",")) == len(lib.SIGNATURES[name]) == (16 if name == FAR_NAMES[0] else 17)
        assert [a.split()[-1] for a in args.split(",")] == [
            a.split()[-1] for a in re.search(r"int %s\(([^;]*)\);" % near, text).group(1).split(",")]


def test_far_flag_parses_and_the_help_keeps_its_phrases():
    from pi3_slam_amd import cli
    base = ["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"]
    assert cli.build_parser().parse_args(base).far is False
    a = cli.build_parser().parse_args(base + ["--far", "--range", "3.3"])
    assert a.far is True and a.range == 3.3
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert text.count("a starting point, not a measured optimum") == 3
    assert "--far" in text and "64 occupancy cells" in text
    assert "[--range 1.0 [--far]]" in cli.__doc__
    for other in ("route", "frontiers", "online"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([other, "--far"])


# ------------------------------------------------------------------------------------------------ the octant rule
def test_a_ray_stays_in_the_closed_octant_of_its_target():
    offs = vref.ball_offsets(5)
    assert len(offs) == 514                                     # |o|^2 <= 25, o != 0
    q = owner(offs)
    longest = 0
    for o, oq in zip(offs.tolist(), q.tolist()):
        between = vref.between(o)
        longest = max(longest, len(between))
        if between:
            assert in_closed_octant(oq, between, 5).all(), (o, oq)
        for c in between:                                       # the sharper fact: between 0 and o_a on every axis
            assert all(min(0, oa) <= ca <= max(0, oa) for ca, oa in zip(c, o)), (o, c)
    assert longest >= 4                                         # (5, 0, 0) alone has four cells between


@pytest.mark.parametrize("R", [1, 2, 33])
def test_the_eight_owners_partition_the_ball(R):
    ball = vref.ball_offsets(R)
    q = owner(ball)
    claimed = np.zeros(len(ball), np.int64)
    for k in range(8):
        # what the kernel of octant k casts at: box cells b in 0 .. R per axis with offset b - p, p = R on a negative axis
        # and 0 on a positive one, never a cell of the plane b_a = R of a negative axis, inside the ball, not the pose
        neg = np.array([(k >> a) & 1 for a in range(3)], bool)
        cast = np.ones(len(ball), bool)
        for a in range(3):
            b = ball[:, a] + (R if neg[a] else 0)
            cast &= (b >= 0) & (b <= R) & ~(neg[a] & (b == R))
        assert (cast == (q == k)).all(), k
        assert in_closed_octant(k, ball[cast], R).all()
        claimed += cast
    assert (claimed == 1).all()                                 # every offset once: axes and planes included
    # the axes and planes go to the octants that are positive there
    assert owner([(R, 0, 0), (0, 0, -R), (0, -1, 0), (-1, 0, 1)]).tolist() == [0, 4, 2, 1]
    sizes = np.bincount(q, minlength=8)
    assert sizes.sum() == len(ball) and sizes[0] == sizes.max() and sizes[7] == sizes.min()
    assert (sizes[7] > 0) == (R > 1)                            # (-1, -1, -1) lies outside the ball of R = 1


def test_ball_sizes():
    def ball_size(R):                                           # the lattice points with 0 < |o|^2 <= R^2, by rows
        r = np.arange(-R, R + 1, dtype=np.int64)
        rest = R * R - (r[:, None] ** 2 + r[None, :] ** 2)       # what x^2 may still be, per (y, z)
        rest = rest[rest >= 0]
        return int((2 * np.floor(np.sqrt(rest.astype(np.float64)) + 1e-9).astype(np.int64) + 1).sum()) - 1
    assert ball_size(32) == 137064 == len(vref.ball_offsets(32))
    assert [ball_size(R) for R in (33, 40, 64)] == [150554, 267760, 1097916]
    assert len(vref.ball_offsets(33)) == 150554


def test_bounds_at_the_largest_range():
    """The figures grid_view_ray.h writes next to its code."""
    R = 64
    W = R + 1
    assert W ** 3 == 274625 and 8 * ((W ** 3 + 255) // 256) == 8 * ((65 ** 3 + 255) // 256) == 8584   # = the near form's at 32
    # a key is (2k - 1) P with P <= R^2; after the last of an axis's R crossings it stands at (2R + 1) R^2
    assert (2 * R + 1) * R * R < 2 * 64 * 8192 == 1 << 20 < 1 << 30                                    # below kNever
    assert R < 128                                                                                      # 7-bit queue fields
    # the cone's 64 bits: the planner's headings (|a|^2 <= 3, den = 2^20) are far inside, +-1024 with a large den is not
    assert R * R * 3 * (1 << 20) < 1 << 63
    assert R * R * 3 * 1024 * 1024 * 715827882 < 1 << 63 <= R * R * 3 * 1024 * 1024 * 715827883
