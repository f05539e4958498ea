"""The oracle of the views of the occupancy grid (tests/grid_view_ref.py) against things it did not compute: the
open-interval rule in exact fractions, lattice-point counts, single blockers, walls, cones, the 48 symmetries of the cube,
and the box room; and the host side of view_planner.py (selection, lattice, arguments, files, parser).  No GPU."""
import itertools
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_route_ref as rref               # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

HD = vref.headings26()
FOV90 = vref.cos2(90)


def _centre(R, pad=0):
    """An all-unknown cube with the candidate at least R cells from every border -> (state, the candidate's index)."""
    n = 2 * (R + pad) + 1
    c = R + pad
    return np.zeros((n, n, n), np.uint8), (c * n + c) * n + c


# ------------------------------------------------------------------------------------------------ between
def _between_by_intervals(o):
    """The cells m != 0, o whose open interior the open segment from 0 to o meets, by exact fractions per axis."""
    out = set()
    spans = [range(min(0, c), max(0, c) + 1) for c in o]
    for m in itertools.product(*spans):
        if m == (0, 0, 0) or m == tuple(o):
            continue
        lo, hi = Fraction(0), Fraction(1)
        for a in range(3):
            if o[a] == 0:
                if m[a] != 0:
                    lo, hi = Fraction(1), Fraction(0)
                continue
            t0, t1 = sorted((Fraction(2 * m[a] - 1, 2 * o[a]), Fraction(2 * m[a] + 1, 2 * o[a])))
            lo, hi = max(lo, t0), min(hi, t1)
        if lo < hi:
            out.add(m)
    return out


def test_the_dda_is_the_open_interval_rule():
    offs = [o for o in itertools.product(range(-5, 6), repeat=3) if 0 < sum(c * c for c in o) <= 25]
    assert len(offs) == 514
    for o in offs:
        got = vref.between(o)
        assert len(set(got)) == len(got) and set(got) == _between_by_intervals(o), o
    # the tie rule: the diagonal passes through corners and steps both axes at once
    assert vref.between((2, 2, 0)) == [(1, 1, 0)] and vref.between((2, 0, 0)) == [(1, 0, 0)]
    assert vref.between((3, 3, 3)) == [(1, 1, 1), (2, 2, 2)] and vref.between((1, 1, 1)) == []
    assert vref.between((2, 1, 0)) == [(1, 0, 0), (1, 1, 0)]


def test_the_vectorised_rays_are_the_scalar_dda():
    state = vref.three_state((11, 11, 11), 0.5, 0.2, 7)
    v = (5, 5, 5)
    offs = vref.ball_offsets(5)
    got = vref.rays(state, v, offs)
    for o, g in zip(offs.tolist(), got.tolist()):
        clear = all(state[5 + m[2], 5 + m[1], 5 + m[0]] != 2 for m in vref.between(o))
        assert g == clear, o
    assert 0 < got.sum() < len(got)


# ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("R, cells", [(1, 6), (2, 32), (3, 122), (7, 1418), (16, 17076)])
def test_an_open_ball_is_seen_whole(R, cells):
    r = np.arange(-R, R + 1)
    assert int((np.add.outer(np.add.outer(r * r, r * r), r * r) <= R * R).sum()) - 1 == cells      # lattice points
    state, c = _centre(R)
    g = vref.gain(state, [c], R, HD, *FOV90)
    assert g["visible"].tolist() == [cells] and g["counters"] == [1, cells, 0, cells]


@pytest.mark.parametrize("blocker, hidden", [((1, 0, 0), 198), ((1, 1, 0), 75), ((1, 1, 1), 51), ((2, 1, 0), 24)])
def test_one_occupied_cell_hides_its_shadow(blocker, hidden):
    R = 7
    state, c = _centre(R)
    state[R + blocker[2], R + blocker[1], R + blocker[0]] = 2
    g = vref.gain(state, [c], R, HD, *FOV90)
    assert 1418 - 1 - int(g["visible"][0]) == hidden            # the blocker itself is no target
    assert g["counters"] == [1, 1417, hidden, 1417 - hidden]
    # from the rule itself: the offsets whose between-set holds the blocker
    ball = vref.ball_offsets(R).tolist()
    assert sum(1 for o in ball if tuple(blocker) in vref.between(o)) == hidden


def test_the_tie_rule_of_the_diagonal_blocker():
    state, _ = _centre(7)
    state[7, 8, 8] = 2                                          # offset (1, 1, 0)
    seen = vref.rays(state, (7, 7, 7), np.array([(2, 2, 0), (2, 0, 0), (2, 1, 0), (3, 1, 0), (1, 3, 0)]))
    assert seen.tolist() == [False, True, False, True, True]    # (3,1,0) and (1,3,0) only touch the blocker's edge


def test_a_wall_and_the_grids_corner():
    R = 5
    for k in (1, 2, 4):
        state, c = _centre(R)
        state[:, :, R + k] = 2
        g = vref.gain(state, [c], R, HD, *FOV90)
        ball = vref.ball_offsets(R)
        assert int(g["visible"][0]) == int((ball[:, 0] < k).sum())
    state = np.zeros((9, 8, 7), np.uint8)
    g = vref.gain(state, [0, state.size - 1, -1, state.size], R, HD, *FOV90)
    ball = vref.ball_offsets(R)
    first = int(((ball >= 0).all(1) & (ball < np.array([7, 8, 9])).all(1)).sum())
    last = int(((ball <= 0).all(1) & (ball > -np.array([7, 8, 9])).all(1)).sum())
    assert g["visible"].tolist() == [first, last, 0, 0] and g["best"].tolist()[2:] == [-1, -1]
    assert g["counters"] == [2, first + last, 0, first + last] and not g["gain"][2:].any()


# ------------------------------------------------------------------------------------------------ cones
def test_cones():
    R = 7
    state, c = _centre(R)
    axes = [(1, 0, 0), (1, 1, 0), (1, 1, 1)]
    g = vref.gain(state, [c], R, axes, *FOV90)
    assert g["gain"].tolist() == [[211, 214, 205]] and g["best"].tolist() == [1]
    assert FOV90 == (1 << 19, 1 << 20) and vref.cos2(180) == (0, 1 << 20) and vref.cos2(60) == (786432, 1 << 20)
    assert vref.in_cone([(1, 1, 0), (1, -1, 0), (1, 1, 1), (0, 1, 0)], (1, 0, 0), *FOV90).tolist() == [True, True, False,
                                                                                                      False]
    ball = vref.ball_offsets(R)
    half = vref.in_cone(ball, (1, 0, 0), *vref.cos2(180))
    assert (half == (ball[:, 0] > 0)).all() and half.sum() == (1418 - 148) // 2       # 148 offsets have o_x = 0
    # all unknown: opposite headings tie, and best is the smaller one
    g = vref.gain(state, [c], R, [(0, 0, 1), (0, 0, -1), (-1, 0, 0)], *FOV90)
    assert g["gain"][0, 0] == g["gain"][0, 1] == g["gain"][0, 2] == 211 and g["best"].tolist() == [0]
    g = vref.gain(np.ones((3, 3, 3), np.uint8), [13], 1, HD, *FOV90)                  # nothing to see: heading 0
    assert g["best"].tolist() == [0] and not g["gain"].any() and g["counters"] == [1, 0, 0, 0]


def test_headings_are_the_26_neighbours_in_z_y_x_order():
    from pi3_slam_amd.view_planner import view_headings
    assert HD.shape == (26, 3) and HD[0].tolist() == [-1, -1, -1] and HD[1].tolist() == [0, -1, -1]
    assert HD[12].tolist() == [-1, 0, 0] and HD[13].tolist() == [1, 0, 0] and HD[25].tolist() == [1, 1, 1]
    assert view_headings().tolist() == HD.tolist()


# ------------------------------------------------------------------------------------------------ symmetry
def test_the_48_symmetries_of_the_cube():
    n, R = 9, 4
    state = vref.three_state((n, n, n), 0.5, 0.15, 11)
    cand = np.array([(4 * n + 4) * n + 4, (2 * n + 6) * n + 3, 0, n ** 3 - 1], np.int64)
    base = vref.gain(state, cand, R, HD, *FOV90)
    assert base["counters"][2] > 0 and base["counters"][3] > 0
    xyz = np.stack([cand % n, (cand // n) % n, cand // (n * n)], 1)
    seen = 0
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            # new axis a is old axis perm[a], mirrored when signs[a] < 0; state is indexed [z][y][x]
            t = np.transpose(state, [2 - perm[2 - d] for d in range(3)])
            t = t[tuple(slice(None, None, signs[2 - d]) for d in range(3))]
            moved = np.stack([xyz[:, perm[a]] if signs[a] > 0 else n - 1 - xyz[:, perm[a]] for a in range(3)], 1)
            lin = (moved[:, 2] * n + moved[:, 1]) * n + moved[:, 0]
            hd = np.stack([signs[a] * HD[:, perm[a]] for a in range(3)], 1)
            g = vref.gain(np.ascontiguousarray(t), lin, R, hd, *FOV90)
            assert g["visible"].tolist() == base["visible"].tolist(), (perm, signs)
            assert g["gain"].tobytes() == base["gain"].tobytes() and g["counters"] == base["counters"], (perm, signs)
            seen += 1
    assert seen == 48


# ------------------------------------------------------------------------------------------------ selection, lattice
def test_select_views():
    from pi3_slam_amd.view_planner import select_views
    shape = (4, 20, 20)
    lin = lambda x, y, z: (z * 20 + y) * 20 + x                 # noqa: E731
    cells = np.array([lin(0, 0, 0), lin(10, 0, 0), lin(10, 10, 0), lin(11, 10, 0), lin(0, 10, 0), lin(5, 5, 3),
                      lin(19, 19, 3)], np.int64)
    gain = np.array([50, 50, 50, 49, 50, 2, 0])
    cost = np.array([30, 20, 20, 5, 30, 1, 1])
    rows, low = select_views(cells, gain, cost, shape, 10, 3, 1)
    # the gain tie: cost 20 before 30, and at one cost the smaller cell; (11,10,0) lies one cell from (10,10,0)
    assert rows.tolist() == [1, 2, 0, 4, 5] and low == 1
    assert select_views(cells, gain, cost, shape, 10, 1, 1)[0].tolist() == [1, 2, 0, 4, 3, 5]      # distance 1 is not < 1
    rows, low = select_views(cells, gain, cost, shape, 10, 0, 0)
    assert rows.tolist() == [1, 2, 0, 4, 3, 5, 6] and low == 0
    assert select_views(cells, gain, cost, shape, 2, 3, 1)[0].tolist() == [1, 2]
    rows, low = select_views(cells, gain, cost, shape, 10, 3, 50)
    assert rows.tolist() == [1, 2, 0, 4] and low == 3
    rows, low = select_views(cells[:0], gain[:0], cost[:0], shape, 10, 3, 1)
    assert rows.tolist() == [] and low == 0
    # the oracle's own selection agrees
    assert vref.select(cells, gain, cost, shape, 10, 3, 1) == ([1, 2, 0, 4, 5], 1)
    assert vref.select(cells, gain, cost, shape, 2, 3, 1) == ([1, 2], 1)


def test_the_lattice_uses_the_absolute_index():
    dist = np.zeros((5, 6, 7), np.uint32)
    got = vref.candidates(dist, (-5, 3, -1), 4)
    xyz = np.stack([got % 7, (got // 7) % 6, got // 42], 1)
    assert sorted(set(xyz[:, 0])) == [1, 5] and sorted(set(xyz[:, 1])) == [1, 5] and sorted(set(xyz[:, 2])) == [1]
    assert len(got) == 4 and (np.diff(got) > 0).all()
    # padding the grid by two cells on the low side moves the origin, not the lattice
    padded = vref.candidates(np.zeros((7, 8, 9), np.uint32), (-7, 1, -3), 4)
    pxyz = np.stack([padded % 9, (padded // 9) % 8, padded // 72], 1)
    assert {tuple(p) for p in (pxyz - 2).tolist()} >= {tuple(p) for p in xyz.tolist()}
    dist[1, 1, 1], dist[1, 1, 5], dist[1, 5, 1] = vref.FAR, 25, 24
    assert vref.candidates(dist, (-5, 3, -1), 4, 24).tolist() == [(1 * 6 + 5) * 7 + 1, (1 * 6 + 5) * 7 + 5]
    assert len(vref.candidates(dist, (-5, 3, -1), 1)) == dist.size - 1


# ------------------------------------------------------------------------------------------------ the box room
@pytest.fixture(scope="module")
def box_room():
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    dist = rref.distances(rref.walk_mask(state, d2a, min_d2), lin)
    return room, state, dist


@pytest.mark.parametrize("R, vmin, vmed, vmax, gain, cell, axis",
                         [(8, 14, 416, 1042, 316, (21, 13, 9), (1, 1, -1)),
                          (16, 2416, 4162, 5751, 2202, (25, 21, 13), (0, 0, -1))])
def test_box_room_on_the_oracle(box_room, R, vmin, vmed, vmax, gain, cell, axis):
    room, state, dist = box_room
    nz, ny, nx = state.shape
    assert int((dist != rref.FAR).sum()) == 15896
    s = vref.view_set(state, dist, room["origin"], R, 4, 90, 10, 4)
    vis = s["gain"]["visible"]
    assert len(s["cells"]) == 230 and s["gain"]["counters"][0] == 230
    assert (int(vis.min()), float(np.median(vis)), int(vis.max())) == (vmin, vmed, vmax)
    best = s["views"][0]
    c = best["cell"]
    assert best["gain"] == gain == int(s["best_gain"].max())
    assert (c % nx, (c // nx) % ny, c // (nx * ny)) == cell and tuple(best["axis"]) == axis
    assert s["gain_map"].reshape(-1)[c] == gain and HD[s["heading_map"].reshape(-1)[c]].tolist() == list(axis)
    assert (s["gain_map"] >= 0).sum() == 230 and ((s["heading_map"] >= 0) == (s["gain_map"] >= 0)).all()
    kept = [v["cell"] for v in s["views"]]
    xyz = np.array([(k % nx, (k // nx) % ny, k // (nx * ny)) for k in kept])
    for i in range(len(kept)):
        for j in range(i):
            assert ((xyz[i] - xyz[j]) ** 2).sum() >= 16
    assert [v["gain"] for v in s["views"]] == sorted((v["gain"] for v in s["views"]), reverse=True)


# ------------------------------------------------------------------------------------------------ the host side
def test_planner_arguments():
    from pi3_slam_amd import ops
    from pi3_slam_amd.view_planner import ViewPlanner
    p = ViewPlanner(0.2, 1.6)
    assert (p.separation_m, p.fov_deg, p.stride, p.count, p.min_gain) == (0.8, 90.0, 4, 10, 1)
    assert (p.cos2_num, p.cos2_den) == (1 << 19, ops.VIEW_COS2_DEN) and ops.VIEW_COS2_DEN == 1 << 20
    assert ops.VIEW_MAX_RANGE == 32 and ops.VIEW_MAX_HEADINGS == 32
    assert ops.VIEW_COUNTERS == ("candidates", "rays", "rays_blocked", "rays_visible")
    assert p.cells_of(0.1) == (16, 8, ops.ROUTE_FAR - 1) and p.cells_of(0.05)[0] == 32
    assert ViewPlanner(0, 1.0, max_distance_m=2.0).cells_of(0.1)[2] == 240
    assert ViewPlanner(0, 1.0, fov_deg=180).cos2_num == 0
    st = p.settings()
    assert st["cos2_num"] == 1 << 19 and st["cos2_den"] == 1 << 20 and st["router"]["approach_unknown"] is True
    with pytest.raises(ValueError, match="33 cells: at most 32 .*larger occupancy cell"):
        ViewPlanner(0, 3.3).cells_of(0.1)
    for bad in (dict(range_m=0.0), dict(range_m=float("nan")), dict(fov_deg=0.0), dict(fov_deg=181.0), dict(stride=0),
                dict(stride=1.5), dict(count=0), dict(min_gain=-1), dict(separation_m=-1.0), dict(max_distance_m=-1.0),
                dict(radius=-0.1)):
        with pytest.raises(ValueError):
            ViewPlanner(**dict(dict(radius=0.0, range_m=1.0), **bad))
    with pytest.raises(ValueError, match="views need a source"):
        p.find(None, None)


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    assert len(lib.SIGNATURES["pi3_grid_view_candidates"]) == 13 and len(lib.SIGNATURES["pi3_grid_view_gain"]) == 16
    for name in ("pi3_grid_view_candidates", "pi3_grid_view_gain"):
        assert f"int {name}(" in text


def _hand_made_set():
    from pi3_slam_amd.view_planner import View, ViewSet
    shape = (3, 4, 5)
    gain = np.full(shape, -1, np.int32)
    heading = np.full(shape, -1, np.int8)
    gain[1, 2, 3], heading[1, 2, 3] = 40, 13
    gain[0, 0, 0], heading[0, 0, 0] = 7, 25
    origin = np.array([-2, 1, 0], np.int64)
    views = [View(0, 33, 0.5 * (origin + [3, 2, 1] + 0.5), 13, HD[13].copy(), HD[13] / 1.0, 40, 90, 24, 1.0),
             View(1, 0, 0.5 * (origin + [0, 0, 0] + 0.5), 25, HD[25].copy(), HD[25] / np.sqrt(3.0), 7, 9, 0, 0.0)]
    return ViewSet(views, gain, heading, HD, origin, 0.5, {"candidates": 2, "views": 2}, {"range_m": 1.0})


def test_view_files(tmp_path):
    from pi3_slam_amd import export, map_eval
    vset = _hand_made_set()
    assert export.write_views(vset, str(tmp_path / "v")) == 2
    assert sorted(os.listdir(tmp_path / "v")) == ["views.json", "views.npz", "views.ply"]
    rec = json.load(open(tmp_path / "v" / "views.json"))
    assert rec["counts"] == {"candidates": 2, "views": 2} and rec["settings"] == {"range_m": 1.0}
    assert [v["rank"] for v in rec["views"]] == [0, 1] and rec["views"][0]["axis"] == [1, 0, 0]
    assert rec["views"][0]["position"] == [0.75, 1.75, 0.75] and rec["views"][0]["direction"] == [1.0, 0.0, 0.0]
    assert rec["views"][1]["gain"] == 7 and rec["views"][1]["visible"] == 9 and rec["views"][0]["distance_m"] == 1.0
    with np.load(tmp_path / "v" / "views.npz") as z:
        assert z["gain"].dtype == np.int32 and z["gain"].tobytes() == vset.gain.tobytes()
        assert z["heading"].dtype == np.int8 and z["heading"].tobytes() == vset.heading.tobytes()
        assert z["headings"].shape == (26, 3) and z["headings"].tolist() == HD.tolist()
        assert z["index_origin"].tolist() == [-2, 1, 0] and float(z["cell"]) == 0.5
    pts = map_eval.read_ply_points(str(tmp_path / "v" / "views.ply"))[0]
    assert np.asarray(pts).tolist() == [[0.75, 1.75, 0.75], [-0.75, 0.75, 0.25]]
    head = open(tmp_path / "v" / "views.ply", "rb").read(400)
    assert b"element vertex 2" in head and b"property float nx" in head


def test_views_parser():
    from pi3_slam_amd import cli
    a = cli.build_parser().parse_args(["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"])
    assert (a.radius, a.range, a.fov, a.stride, a.count, a.separation, a.max_distance, a.min_gain, a.route_to) == (
        0.0, 1.0, 90.0, 4, 10, None, None, 1, None)
    with pytest.raises(SystemExit, match="views: give --start X Y Z or --from-trajectory"):
        cli.main(["views", "--occupancy", "o.npz", "--output", "d"])
    with pytest.raises(SystemExit, match="views: give --start X Y Z or --from-trajectory"):
        cli.main(["views", "--occupancy", "o.npz", "--output", "d", "--start", "0", "0", "0", "--from-trajectory", "t"])
    with pytest.raises(SystemExit, match="views: the range must be"):
        cli.main(["views", "--occupancy", "o.npz", "--output", "d", "--start", "0", "0", "0", "--range", "0"])
    with pytest.raises(SystemExit, match="views: .*o.npz"):
        cli.main(["views", "--occupancy", "/nonexistent/o.npz", "--output", "d", "--start", "0", "0", "0"])
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert text.count("a starting point, not a measured optimum") == 3
