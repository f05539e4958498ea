"""Line of sight between cells and the taut way, without a GPU: the supercover of tests/grid_sight_ref.py against a
brute-force closed-cube test in exact fractions, its symmetry, the move rule it reduces to, the 32-bit key bound,
grid_route.pull_taut against the oracle's dynamic programme on the cases of DESIGN 7l's table, and the exporters."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_route_ref as rref               # noqa: E402
import grid_sight_ref as sref               # noqa: E402

HAND = [(0, 0, 0), (1, 0, 0), (0, -1, 0), (1, 1, 0), (-1, 1, 1), (3, 0, 0), (2, 1, 0), (3, 3, 3), (3, -6, 2), (5, 3, 1),
        (-7, 7, 4), (6, 4, -2)]


def seeded_offsets():
    return np.random.default_rng(11).integers(-7, 8, (300, 3)).tolist()


def xyz_of(cells, shape):
    nz, ny, nx = shape
    c = np.asarray(cells, np.int64)
    return np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], 1)


# ------------------------------------------------------------------------------------------------ 1. the supercover
@pytest.mark.parametrize("offsets", [HAND, seeded_offsets()], ids=["hand", "seeded"])
def test_supercover_is_the_closed_cube_test(offsets):
    assert len(offsets) in (12, 300)
    for o in offsets:
        a = (2, -3, 5)
        b = tuple(u + int(v) for u, v in zip(a, o))
        got = sref.supercover(a, b)
        assert len(set(got)) == len(got) and got[0] == a and got[-1] == b, o
        assert set(got) == sref.slab_cover(a, b), o
        assert set(sref.supercover(b, a)) == set(got), o          # symmetric in a and b


def test_ties_touch_every_cell_around_the_edge_or_corner():
    assert sref.supercover((0, 0, 0), (0, 0, 0)) == [(0, 0, 0)]
    assert set(sref.supercover((0, 0, 0), (1, 1, 0))) == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)}
    assert len(sref.supercover((0, 0, 0), (1, 1, 1))) == 8
    assert len(sref.supercover((0, 0, 0), (3, 3, 3))) == 1 + 3 * 7
    assert sref.supercover((0, 0, 0), (2, 1, 0)) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)]      # through (1, 0.5)
    assert sref.supercover((0, 0, 0), (-3, 0, 0)) == [(0, 0, 0), (-1, 0, 0), (-2, 0, 0), (-3, 0, 0)]


def test_unit_offsets_are_the_move_rule():
    state = rref.maze((7, 8, 9), 0.3, 1)
    walk = rref.walk_mask(state)
    nz, ny, nx = walk.shape
    ok = rref.allowed_moves(walk)
    cells = np.arange(walk.size, dtype=np.int64)
    xyz = xyz_of(cells, walk.shape)
    differences = 0
    for k, (dx, dy, dz, _) in enumerate(rref.MOVES):
        t = xyz + np.array([dx, dy, dz])
        inside = ((t >= 0) & (t < np.array([nx, ny, nz]))).all(1)
        assert not ok[k].reshape(-1)[~inside].any()
        to = (t[:, 2] * ny + t[:, 1]) * nx + t[:, 0]
        sees, touched, _ = sref.sight_pairs(walk, None, cells[inside], to[inside])
        assert (touched == 2 ** ((dx != 0) + (dy != 0) + (dz != 0))).all()
        differences += int((sees.astype(bool) != ok[k].reshape(-1)[inside]).sum())
    assert differences == 0


def test_the_vectorised_walk_is_the_supercover():
    state = rref.maze((9, 10, 11), 0.04, 5)
    walk = rref.walk_mask(state)
    d2 = np.random.default_rng(2).integers(0, 50, walk.shape).astype(np.uint16)
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, walk.size, 200), rng.integers(0, walk.size, 200)
    a[:3], b[:3] = (-1, 5, walk.size), (5, walk.size + 7, 3)       # ends outside the grid
    b[3] = a[3]
    sees, touched, low = sref.sight_pairs(walk, d2, a, b)
    assert sees[:3].tolist() == [0, 0, 0] and touched[:3].tolist() == [0, 0, 0] and low[:3].tolist() == [0xFFFF] * 3
    assert touched[3] == 1 and sees[3] == walk.reshape(-1)[a[3]] and low[3] == d2.reshape(-1)[a[3]]
    A, B = xyz_of(a, walk.shape), xyz_of(b, walk.shape)
    for i in range(3, 200):
        cover = sref.supercover(A[i], B[i])
        assert touched[i] == len(cover)
        assert bool(sees[i]) == all(walk[z, y, x] for x, y, z in cover) == sref.sees(walk, A[i], B[i])
        assert low[i] == min(d2[z, y, x] for x, y, z in cover)
    back = sref.sight_pairs(walk, d2, b, a)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(back, (sees, touched, low)))
    assert sref.sight_pairs(walk, None, a, b)[2].tolist() == [0xFFFF] * 200
    assert 20 < sees.sum() < 180                                    # both answers occur


def test_keys_fit_32_bits():
    assert sref.max_key((511, 511, 511)) == 266604541 < 1 << 28 < sref.NEVER
    assert 512 ** 3 == 1 << 27                                      # the bounding box of that offset is a full grid
    for o in ((1 << 27) - 1, 0, 0), (0, 0, 1), (8191, 16383, 0), (2, 8191, 4095):
        box = (abs(o[0]) + 1) * (abs(o[1]) + 1) * (abs(o[2]) + 1)
        assert box <= 1 << 27 and sref.max_key(o) < 1 << 28, o
        first, inc = sref.keys(o)
        assert max(inc) <= 1 << 28
        # an axis past its last crossing stays above every waiting key and below the mark of an axis that never moves
        assert all(sref.max_key(o) < f + abs(v) * i < sref.NEVER for f, i, v in zip(first, inc, o) if v)


# ------------------------------------------------------------------------------------------------ 2. the taut way
def _maze_case(seed):
    n = 17 * 9 * 20
    return rref.maze((17, 9, 20), 0.3, seed, free_cells=(0, n - 1)), 0, n - 1, 1.0


def _box_case(goal_xyz):
    box = np.ones((13, 11, 9), np.uint8)                            # 9 x 11 x 13 as (nx, ny, nz)
    return box, 0, (goal_xyz[2] * 11 + goal_xyz[1]) * 9 + goal_xyz[0], 1.0


def _door_case(a_xyz, b_xyz):
    r = rref.door_room()
    lin = (lambda c: (c[2] * 16 + c[1]) * 24 + c[0])
    return r["state"], (r["start"] if a_xyz is None else lin(a_xyz)), (r["goal"] if b_xyz is None else lin(b_xyz)), r["cell"]


CASES = {
    # name: (scene, trace cells, cost / 12, polyline, taut, the taut way's vertices or their number)
    "box_corner": (lambda: _box_case((8, 10, 12)), 13, 18.8333, 18.6848, 17.5499, [0, 12]),
    "box_3_10_5": (lambda: _box_case((3, 10, 5)), 11, 13.0833, 13.0246, 11.5758, [0, 10]),
    "door": (lambda: _door_case(None, None), 18, 4.2500, 4.2500, 4.2500, [0, 17]),
    "door_across": (lambda: _door_case((2, 1, 1), (21, 14, 1)), 20, 6.1042, 6.0962, 5.7554, [0, 19]),
    "serpentine": (lambda: rref.serpentine() + (1.0,), 305, 310.6667, 310.6274, 304.4683,
                   [0] + [v for k in range(32, 273, 34) for v in (k, k + 2)] + [304]),
    "maze_3": (lambda: _maze_case(3), 25, 31.5000, 31.3882, 29.0556, [0, 3, 8, 13, 14, 24]),
    "maze_4": (lambda: _maze_case(4), 26, 33.1667, 33.0915, 29.6561, [0, 1, 3, 6, 10, 14, 18, 20, 25]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (walk, trace cells source .. goal, their (x, y, z), cost, cell, the full-span visibility bits); computed once."""
    state, src, goal, cell = CASES[name][0]()
    walk = rref.walk_mask(state)
    dist = rref.distances(walk, [src])
    cells = np.asarray(rref.trace(walk, dist, goal)[::-1], np.int64)
    bits = sref.vis_bits(walk, cells, [0, len(cells)], len(cells) - 1)
    return walk, cells, xyz_of(cells, walk.shape), int(dist.reshape(-1)[goal]), cell, bits


def pulled(name, span):
    from pi3_slam_amd.grid_route import pull_taut
    walk, cells, xyz, cost, cell, bits = case(name)
    (idx, length), = pull_taut(sref.pack_words(bits[:, :span]), cells, [0, len(cells)], span, walk.shape)
    return idx, length


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_and_pull_taut_against_the_oracle(name):
    _, n_cells, cost12, poly, taut_len, vertices = CASES[name]
    walk, cells, xyz, cost, cell, bits = case(name)
    L = len(cells)
    assert L == n_cells and bits[:, 0].tolist() == [True] * (L - 1) + [False]       # neighbours see each other
    exp_idx, exp_len = sref.taut(bits, xyz, L - 1)
    idx, length = pulled(name, L - 1)
    assert idx.dtype == np.int64 and idx.tolist() == exp_idx and np.float64(length).tobytes() == np.float64(exp_len).tobytes()
    line = sref.polyline(xyz)
    straight = math.sqrt(float(((xyz[-1] - xyz[0]) ** 2).sum()))
    print(f"{name}: {L} cells, cost {cell * cost / 12:.4f}, polyline {cell * line:.4f}, taut {cell * length:.4f}, "
          f"vertices {idx.tolist()}")
    assert abs(cell * cost / 12 - cost12) < 5e-5 and abs(cell * line - poly) < 5e-5 and abs(cell * length - taut_len) < 5e-5
    assert idx.tolist() == vertices
    assert straight <= length <= line
    # every chosen segment sees, and no longer span than the trace changes anything
    for i, j in zip(idx[:-1], idx[1:]):
        assert sref.sees(walk, xyz[i], xyz[j])
    # span 1 is the trace itself
    one_idx, one_len = pulled(name, 1)
    assert one_idx.tolist() == list(range(L)) and one_len == sref.taut(bits, xyz, 1)[1]
    assert abs(one_len - line) < 1e-9 * line


def test_open_boxes_reach_the_straight_line():
    assert abs(pulled("box_corner", 12)[1] - math.sqrt(308)) <= 1e-12 * math.sqrt(308)
    assert abs(pulled("box_3_10_5", 10)[1] - math.sqrt(134)) <= 1e-12 * math.sqrt(134)


def test_a_short_span_can_cost_length():
    walk, cells, xyz, cost, cell, bits = case("serpentine")
    got = {}
    for span in (8, 32, 304):
        idx, length = pulled("serpentine", span)
        exp_idx, exp_len = sref.taut(bits, xyz, span)
        assert idx.tolist() == exp_idx and length == exp_len and int(np.diff(idx).max()) <= span
        got[span] = length
    assert abs(got[8] - 305.848) < 5e-4 and abs(got[32] - 304.4683) < 5e-5 and got[32] == got[304]


def test_equal_lengths_take_the_smallest_index_and_legs_stay_apart():
    from pi3_slam_amd.grid_route import pull_taut
    shape = (1, 16, 16)
    lin = (lambda x, y: y * 16 + x)
    # 0 -> 1 -> 3 and 0 -> 2 -> 3 are both 5 + 5; nobody sees 3 from 0
    cells = np.array([lin(0, 0), lin(3, 4), lin(4, 3), lin(7, 7)], np.int64)
    bits = np.zeros((4, 3), bool)
    bits[0, 0] = bits[0, 1] = bits[1, 1] = bits[2, 0] = True
    (idx, length), = pull_taut(sref.pack_words(bits), cells, [0, 4], 3, shape)
    assert idx.tolist() == [0, 1, 3] == sref.taut(bits, xyz_of(cells, shape), 3)[0] and length == 10.0
    # three traces in one call, one of a single cell and one empty: indices are the trace's own
    many = np.concatenate([cells, cells[:1], cells])
    both = np.zeros((9, 3), bool)
    both[0:4], both[5:9] = bits, bits
    both[5, 2] = True                                               # the second copy sees its end from its start
    out = pull_taut(sref.pack_words(both), many, [0, 4, 5, 5, 9], 3, shape)
    assert [o[0].tolist() for o in out] == [[0, 1, 3], [0], [], [0, 3]]
    assert [o[1] for o in out] == [10.0, 0.0, 0.0, math.sqrt(98.0)]
    # 65 bits per row: the second word is read
    wide = np.zeros((4, 65), bool)
    wide[:, :3] = bits
    assert pull_taut(sref.pack_words(wide), cells, [0, 4], 65, shape)[0][0].tolist() == [0, 1, 3]
    bits[2, 0] = bits[1, 1] = False
    with pytest.raises(ValueError, match="trace 0: cell 3 is seen by none of the 3 cells before it"):
        pull_taut(sref.pack_words(bits), cells, [0, 4], 3, shape)


def test_span_is_checked():
    from pi3_slam_amd.grid_route import check_span
    assert check_span(1) == 1 and check_span(4096) == 4096
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="the span of a taut way is 1 .. 4096 trace cells"):
            check_span(bad)


# ------------------------------------------------------------------------------------------------ 3. the files
def test_route_files_with_and_without_a_taut_way(tmp_path):
    from pi3_slam_amd import export, map_eval
    from pi3_slam_amd.grid_route import Route, RouteField, TautRoute
    cost = np.array([[[0, 12, 24, 36]]], np.uint32)
    f = RouteField(np.array([[[0.0, 0.5, 1.0, 1.5]]], np.float32), cost, np.ones((1, 1, 4), np.uint8),
                   np.array([1, 2, 3], np.int64), 0.5, np.ones((1, 1, 4), np.uint8), None, {"reachable": 4, "sweeps": 2},
                   {"radius": 0.0})
    way = 0.5 * (np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float64) + [1.5, 2.5, 3.5])
    route = Route(way, np.arange(4), 36, 1.5, 0.25, {"radius": 0.2})
    taut = TautRoute(way[[0, 3]], np.array([0, 3]), np.array([0, 3]), 1.5, float("inf"), 256, {"radius": 0.2})
    export.write_route(f, route, str(tmp_path / "off"))
    export.write_route(f, route, str(tmp_path / "on"), taut)
    assert sorted(os.listdir(tmp_path / "off")) == ["route.json", "route.npz", "route.ply"]
    assert sorted(os.listdir(tmp_path / "on")) == ["route.json", "route.npz", "route.ply", "route_taut.ply"]
    off = json.load(open(tmp_path / "off" / "route.json"))
    on = json.load(open(tmp_path / "on" / "route.json"))
    assert off == {"waypoints": way.tolist(), "cost": 36, "length_m": 1.5, "min_clearance_m": 0.25, "settings": {"radius": 0.2}}
    assert open(tmp_path / "off" / "route.json").read() == json.dumps(off, indent=1)      # the text itself, as before
    assert {k: on[k] for k in off} == off and list(on)[:len(off)] == list(off)
    assert {k: on[k] for k in on if k not in off} == {
        "taut_waypoints": way[[0, 3]].tolist(), "taut_indices": [0, 3], "taut_length_m": 1.5,
        "taut_min_clearance_m": "inf", "taut_span": 256}
    for name in ("route.npz", "route.ply"):
        assert open(tmp_path / "on" / name, "rb").read() == open(tmp_path / "off" / name, "rb").read()
    pts, cols = map_eval.read_ply_points(str(tmp_path / "on" / "route_taut.ply"))
    assert pts.tolist() == way.astype(np.float32).tolist()          # once per cell length, the last vertex included
    assert cols.tolist() == [list(export.TAUT_COLOR)] * 4
    uneven = export.sample_polyline(np.array([[0.0, 0, 0], [0.0, 1.25, 0], [0.0, 1.25, 0.25]]), 0.5)
    assert len(uneven) == 5 and np.diff(uneven[:4, 1]).max() <= 0.5 and uneven[3].tolist() == [0, 1.25, 0]
    assert export.sample_polyline(np.array([[0.0, 0, 0], [0.0, 1.5, 0], [0.0, 1.5, 0.25]]), 0.5).tolist() == [
        [0, 0, 0], [0, 0.5, 0], [0, 1.0, 0], [0, 1.5, 0], [0, 1.5, 0.25]]
    assert export.sample_polyline(way[:1], 0.5).tolist() == way[:1].tolist()


def test_tour_files_with_and_without_taut_legs(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.view_tour import Tour, TourStop
    D = np.array([[0, 24, 12], [24, 0, 12], [12, 12, 0]], np.int64)
    legs = [np.array([5, 6]), np.array([6, 7, 8])]
    ways = [np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]]),
            np.array([[0.75, 0.25, 0.25], [1.25, 0.25, 0.25], [1.75, 0.25, 0.25]])]

    def make(**taut):
        stops = [TourStop(1, 6, ways[0][-1], [1], 12, 12, 0.5, None, [7], [7]),
                 TourStop(0, 8, ways[1][-1], [0, 2], 12, 24, 1.0, float("inf"), [9, 2], [16, 18])]
        if taut:
            stops[0].taut_length_m, stops[1].taut_length_m = 0.5, 1.0
            stops[1].taut_min_clearance_m = float("inf")
        return Tour(stops, [1, 0], 5, ways[0][0], D, np.array([5, 8, 6]), legs, ways, 24, 1.5, 36, 24, 0, "exact", [], 18,
                    {"fields": 3, "stops": 2}, {"cell": 0.5, "radius": 0.0}, **taut)
    export.write_tour(make(), str(tmp_path / "off"))
    export.write_tour(make(taut_leg_cells=[legs[0], legs[1][[0, 2]]], taut_leg_waypoints=[ways[0], ways[1][[0, 2]]],
                           taut_leg_indices=[np.array([0, 1]), np.array([0, 2])], taut_length_m=1.5, taut_span=64),
                      str(tmp_path / "on"))
    off = json.load(open(tmp_path / "off" / "tour.json"))
    on = json.load(open(tmp_path / "on" / "tour.json"))
    assert "taut_length_m" not in off and all("taut_length_m" not in s for s in off["stops"])
    assert sorted(off["stops"][0]) == ["cell", "cumulative_cost", "leg_cost", "length_m", "min_clearance_m", "number",
                                       "position", "views"]
    assert [s["taut_length_m"] for s in on["stops"]] == [0.5, 1.0]
    assert [s["taut_min_clearance_m"] for s in on["stops"]] == [None, "inf"]
    for s in on["stops"]:
        del s["taut_length_m"], s["taut_min_clearance_m"]
    assert (on.pop("taut_length_m"), on.pop("taut_span"), on.pop("taut_vertices")) == (1.5, 64, 4)
    assert on == off
    with np.load(tmp_path / "off" / "tour.npz") as z:
        old = {k: z[k].copy() for k in z.files}
    assert sorted(old) == ["cells", "matrix", "offsets", "order", "waypoint_cells", "waypoints"]
    with np.load(tmp_path / "on" / "tour.npz") as z:
        assert sorted(set(z.files) - set(old)) == ["taut_offsets", "taut_waypoint_cells", "taut_waypoints"]
        assert all(z[k].tobytes() == old[k].tobytes() for k in old)
        assert z["taut_offsets"].tolist() == [0, 2, 4] and z["taut_waypoint_cells"].tolist() == [5, 6, 6, 8]
        assert z["taut_waypoints"].tolist() == np.concatenate([ways[0], ways[1][[0, 2]]]).tolist()
    assert open(tmp_path / "on" / "tour.ply", "rb").read() == open(tmp_path / "off" / "tour.ply", "rb").read()


def test_cli_knows_the_taut_flags():
    from pi3_slam_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["route", "--occupancy", "o", "--output", "d", "--start", "0", "0", "0"])
    assert a.taut is False and a.taut_span == 256
    for cmd in ("route", "frontiers", "views"):
        a = p.parse_args([cmd, "--occupancy", "o", "--output", "d", "--taut", "--taut-span", "64"])
        assert a.taut is True and a.taut_span == 64
    with pytest.raises(SystemExit, match="route: --taut needs --goal X Y Z"):
        cli.main(["route", "--occupancy", "o", "--output", "d", "--start", "0", "0", "0", "--taut"])
    with pytest.raises(SystemExit, match=r"route: --taut-span is 1 \.\. 4096 trace cells, got 0"):
        cli.main(["route", "--occupancy", "o", "--output", "d", "--start", "0", "0", "0", "--goal", "1", "1", "1", "--taut",
                  "--taut-span", "0"])
    with pytest.raises(SystemExit, match="frontiers: --taut needs --route-to RANK"):
        cli.main(["frontiers", "--occupancy", "o", "--output", "d", "--start", "0", "0", "0", "--taut"])
    with pytest.raises(SystemExit, match="views: --taut needs --route-to RANK or --tour"):
        cli.main(["views", "--occupancy", "o", "--output", "d", "--start", "0", "0", "0", "--taut"])
