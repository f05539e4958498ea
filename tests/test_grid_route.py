"""Routes through the occupancy grid without a GPU: the oracle (tests/grid_route_ref.py) against closed forms and
against its own emulation of the kernel's tile schedule, the door and box-room scenes on the oracle, occupancy.npz
round trip, GridRouter's argument checks and the `route` parser."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_route_ref as ref            # noqa: E402
import occupancy_ref as oref            # noqa: E402


def _lin(x, y, z, shape):
    nz, ny, nx = shape
    return (z * ny + y) * nx + x


def test_open_box_distance_is_the_closed_form():
    shape = (13, 11, 9)                 # x 9, y 11, z 13
    walk = np.ones(shape, np.uint8)
    for src in [(0, 0, 0), (4, 5, 6), (8, 10, 12), (8, 0, 6)]:
        d = ref.distances(walk, [_lin(*src, shape)])
        z, y, x = np.meshgrid(np.arange(13), np.arange(11), np.arange(9), indexing="ij")
        off = np.sort(np.stack([abs(x - src[0]), abs(y - src[1]), abs(z - src[2])], -1), -1)
        exp = 12 * (off[..., 2] - off[..., 1]) + 17 * (off[..., 1] - off[..., 0]) + 21 * off[..., 0]
        assert d.dtype == np.uint32 and (d == exp).all()
        assert ref.open_box_distance((0, 3, 7), (5, 1, 2)) == 12 * 0 + 17 * 3 + 21 * 2
    two = ref.distances(walk, [_lin(0, 0, 0, shape), _lin(8, 10, 12, shape)])
    one_a, one_b = ref.distances(walk, [_lin(0, 0, 0, shape)]), ref.distances(walk, [_lin(8, 10, 12, shape)])
    assert (two == np.minimum(one_a, one_b)).all()


def test_no_corner_is_cut():
    # 2-D: the cell behind two blocked edge neighbours is not reached diagonally
    state = np.ones((1, 3, 3), np.uint8)
    state[0, 0, 1] = state[0, 1, 0] = 2
    d = ref.distances(ref.walk_mask(state), [_lin(0, 0, 0, state.shape)])
    assert d[0, 0, 0] == 0 and (d.reshape(-1)[1:] == ref.FAR).all()
    # one blocked edge neighbour is enough to forbid a diagonal: round (1, 0) every step is an edge step
    state = np.ones((1, 3, 3), np.uint8)
    state[0, 0, 1] = 2
    d = ref.distances(ref.walk_mask(state), [0])
    assert d[0, 1, 0] == 12 and d[0, 1, 1] == 24 and d[0, 1, 2] == 36 and d[0, 0, 2] == 48 and d[0, 2, 1] == 12 + 17
    # 3-D: the space diagonal needs all six cells between
    walk = np.ones((2, 2, 2), np.uint8)
    assert ref.distances(walk, [0])[1, 1, 1] == 21
    walk[0, 1, 1] = 0
    assert ref.distances(walk, [0])[1, 1, 1] == 12 + 17
    ok = ref.allowed_moves(walk)
    k = ref.MOVES.index((1, 1, 1, 21))
    assert not ok[k].any()
    # the rule is symmetric
    walk = ref.walk_mask(ref.maze((4, 6, 7), 0.35, 9))
    ok = ref.allowed_moves(walk)
    for k, (dx, dy, dz, _) in enumerate(ref.MOVES):
        back = ref.MOVES.index((-dx, -dy, -dz, ref.MOVES[k][3]))
        fwd = np.argwhere(ok[k])
        assert ok[back][fwd[:, 0] + dz, fwd[:, 1] + dy, fwd[:, 2] + dx].all()


def test_walk_mask_and_init():
    state = np.array([[[0, 1, 2, 1, 1, 0]]], np.uint8)
    d2 = np.array([[[9, 4, 0, 1, ref.D2_FAR, 3]]], np.uint16)
    assert ref.walk_mask(state).tolist() == [[[0, 1, 0, 1, 1, 0]]]
    assert ref.walk_mask(state, through_unknown=True).tolist() == [[[1, 1, 0, 1, 1, 1]]]
    assert ref.walk_mask(state, d2, 4).tolist() == [[[0, 1, 0, 0, 1, 0]]]
    assert ref.walk_mask(state, d2, 4, True).tolist() == [[[1, 1, 0, 0, 1, 0]]]
    got = ref.init(state, d2, 4, False, [1, 1, 4, 0, 3, -1, 6, 99])
    assert got["counters"] == [2, 3, 2, 3] and got["dist"].tolist() == [[[ref.FAR, 0, ref.FAR, ref.FAR, 0, ref.FAR]]]
    none = ref.init(state, None, 0, False, [])
    assert none["counters"] == [3, 0, 0, 0] and (none["dist"] == ref.FAR).all()
    assert (ref.distances(none["walk"], []) == ref.FAR).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", [(5, 17, 19), (17, 9, 20), (3, 24, 24)], ids=lambda s: "%dx%dx%d" % s)
def test_the_tile_schedule_reaches_dijkstras_field(shape, seed):
    walk = ref.walk_mask(ref.maze(shape, 0.3, seed))
    src = int(np.flatnonzero(walk.reshape(-1))[0])
    d, launches, changing = ref.tile_sweeps(walk, [src])
    exp = ref.distances(walk, [src])
    reached = int((exp != ref.FAR).sum())
    print(f"{shape} seed {seed}: {launches} launches, {reached} cells reached")
    assert d.tobytes() == exp.tobytes() and launches == changing + 1
    assert 1000 < reached and launches <= 9


def test_tiles_relax_to_their_own_fixed_point():
    walk = np.ones((1, 1, 300), np.uint8)
    d, launches, changing = ref.tile_sweeps(walk, [0])
    assert d.tobytes() == ref.distances(walk, [0]).tobytes() and d[0, 0, -1] == 12 * 299
    assert changing == 38 and launches == 39                   # one per tile the line crosses
    state, src, corner = ref.serpentine()
    walk = ref.walk_mask(state)
    d, launches, changing = ref.tile_sweeps(walk, [src])
    assert d.tobytes() == ref.distances(walk, [src]).tobytes()
    assert d.reshape(-1)[corner] == 3728 and launches == 38
    path = ref.trace(walk, d, corner)
    assert path[0] == corner and path[-1] == src
    assert sum(ref.step_cost(a, b, walk.shape) for a, b in zip(path, path[1:])) == 3728


def _door(radius):
    r = ref.door_room()
    R, min_d2 = int(np.ceil(radius / r["cell"])), int(np.ceil((radius / r["cell"]) ** 2))
    d2 = oref.edt_ref(r["state"], R, True)
    walk = ref.walk_mask(r["state"], d2, min_d2)
    dist = ref.distances(walk, [r["start"]])
    return r, R, min_d2, walk, dist, ref.trace(walk, dist, r["goal"])


def test_the_door_lets_through_what_fits():
    nx, ny = 24, 16
    r, R, m, walk, dist, path = _door(0.25)
    assert (R, m) == (1, 1) and path and path[0] == r["goal"] and path[-1] == r["start"]
    r, R, m, walk, dist, path = _door(0.5)
    assert (R, m) == (2, 4) and path
    in_wall = [((p // nx) % ny) for p in path if p % nx == r["wall_x"]]
    assert in_wall and set(in_wall) == {7}
    r, R, m, walk, dist, path = _door(0.625)
    assert (R, m) == (3, 7) and path == [] and dist.reshape(-1)[r["goal"]] == ref.FAR
    assert walk.reshape(-1)[r["goal"]] == 1                     # the goal itself is fine: the door is too narrow


BOX_RADIUS = 0.2        # all 12 camera cells of the box room have nothing within 2 cells (their d2 is the far mark)


def box_room_case():
    """The box room's observed state, its 12 camera cells as sources -> (room, state, cams (12,3), d2, walk, dist)."""
    room = oref.box_room()
    m = oref.mark(room["points"], room["cell"], room["origin"], room["dims"])
    o = oref.observe(m["state"], room["cell"], room["origin"], room["views"], room["planes"], 1, room["rel_tol"],
                     room["margin"], room["min_free_views"])
    cams = oref.centre_cells(room["views"], room["cell"]) - np.asarray(room["origin"], np.int64)
    R, min_d2 = int(np.ceil(BOX_RADIUS / room["cell"])), int(np.ceil((BOX_RADIUS / room["cell"]) ** 2))
    d2 = oref.edt_ref(o["state"], R, True)
    walk = ref.walk_mask(o["state"], d2, min_d2)
    return room, o["state"], cams, d2, walk, (R, min_d2)


def check_box_room(room, state, cams, d2, walk, dist, path, first, last):
    """The conditions of the box room on a distance field and a route between the camera cells `first` and `last`."""
    inside, _ = oref.wall_distance(room)
    reach = dist != ref.FAR
    assert reach.sum() > 5000
    assert (state[reach] == 1).all() and inside[reach].all()
    assert path[0] == _lin(*cams[last], state.shape) and path[-1] == _lin(*cams[first], state.shape)
    clear = oref.clearance(d2, room["cell"]).reshape(-1)[path].min()
    assert clear >= BOX_RADIUS
    cost = sum(ref.step_cost(a, b, state.shape) for a, b in zip(path, path[1:]))
    assert cost == dist.reshape(-1)[path[0]] >= ref.open_box_distance(cams[first], cams[last]) > 0


def test_box_room_on_the_oracle():
    room, state, cams, d2, walk, (R, min_d2) = box_room_case()
    assert (R, min_d2) == (2, 4)
    at = (cams[:, 2], cams[:, 1], cams[:, 0])
    assert (d2[at] >= min_d2).all() and walk[at].all()          # the radius the GPU test uses fits all 12 cameras
    dist = ref.distances(walk, [_lin(*cams[0], state.shape)])
    check_box_room(room, state, cams, d2, walk, dist, ref.trace(walk, dist, _lin(*cams[6], state.shape)), 0, 6)
    every = ref.distances(walk, [_lin(*c, state.shape) for c in cams])
    assert ((every != ref.FAR) == (dist != ref.FAR)).all()      # one room: every camera reaches the same cells


def test_occupancy_file_round_trip(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.dense_map import OccupancyGrid
    rng = np.random.default_rng(4)
    state = rng.integers(0, 3, (3, 4, 5)).astype(np.uint8)
    clear = rng.uniform(0, 1, (3, 4, 5)).astype(np.float32)
    clear[0, 0, 0] = np.inf
    g = OccupancyGrid(state, np.array([-3, 2, 7], np.int64), 0.125, clear, {"cells": 60, "free": 17},
                      {"cell": 0.125, "clearance": 0.5, "unknown_is_obstacle": False})
    export.write_occupancy(g, str(tmp_path / "occupancy.npz"))
    back = export.read_occupancy(str(tmp_path / "occupancy.npz"))
    assert back.state.tobytes() == state.tobytes() and back.state.shape == state.shape and back.state.dtype == np.uint8
    assert back.index_origin.tolist() == [-3, 2, 7] and back.index_origin.dtype == np.int64 and back.cell == 0.125
    assert back.clearance.tobytes() == clear.tobytes() and back.counts == g.counts and back.settings == g.settings
    assert back.origin.tolist() == g.origin.tolist()
    bare = OccupancyGrid(state, np.zeros(3, np.int64), 0.1)
    export.write_occupancy(bare, str(tmp_path / "bare.npz"))
    back = export.read_occupancy(str(tmp_path / "bare.npz"))
    assert back.clearance is None and back.counts is None and back.settings is None and back.cell == 0.1
    np.savez(tmp_path / "other.npz", points=np.zeros(3))
    with pytest.raises(ValueError, match="not an occupancy grid"):
        export.read_occupancy(str(tmp_path / "other.npz"))


def test_router_arguments():
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.grid_route import GridRouter
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            GridRouter(radius=bad)
    r = GridRouter()
    assert r.radius == 0.0 and r.through_unknown is False and r.clearance_cells(0.1) == (None, 0)
    assert GridRouter(0.5).clearance_cells(0.25) == (2, 4) and GridRouter(0.625).clearance_cells(0.25) == (3, 7)
    assert GridRouter(0.2).clearance_cells(0.1) == (2, 4) and GridRouter(0.01).clearance_cells(0.1) == (1, 1)
    assert GridRouter(25.5).clearance_cells(0.1)[0] == ops.EDT_MAX_RADIUS
    with pytest.raises(ValueError, match=r"256 cells: at most 255 \(radius <= 25.5 or a larger cell\)"):
        GridRouter(25.6).clearance_cells(0.1)
    # world -> cell: floor(p / cell) - index_origin; linear: -1 outside
    g = OccupancyGrid(np.ones((2, 3, 4), np.uint8), np.array([-2, 0, 1], np.int64), 0.5)
    cells = GridRouter.world_cells([[-1.0, 0.0, 0.5], [-0.01, 1.49, 1.2], [0.99, 1.5, 0.49]], g)
    assert cells.tolist() == [[0, 0, 0], [1, 2, 1], [3, 3, -1]]
    assert GridRouter.linear(cells, (2, 3, 4)).tolist() == [0, (1 * 3 + 2) * 4 + 1, -1]
    with pytest.raises(ValueError, match="not finite"):
        GridRouter.world_cells([[0.0, np.nan, 0.0]], g)
    # refused before anything reaches the device
    huge = OccupancyGrid(np.broadcast_to(np.ones(1, np.uint8), (1 << 9, 1 << 9, (1 << 9) + 1)), np.zeros(3, np.int64), 0.1)
    with pytest.raises(ValueError, match="at most 2\\^27"):
        GridRouter().field(huge, [[0.0, 0.0, 0.0]], "cpu")
    with pytest.raises(ValueError, match="not empty"):
        GridRouter().field(OccupancyGrid(np.zeros((0, 3, 4), np.uint8), np.zeros(3, np.int64), 0.1), [[0, 0, 0]], "cpu")


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pi3slam_hip.h")).read()
    for name, n_args in (("pi3_grid_route_init", 13), ("pi3_grid_route_sweep", 7), ("pi3_grid_route_trace", 10)):
        assert len(lib.SIGNATURES[name]) == n_args
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args
    assert "grid_route.hip" in open(os.path.join(root, "pi3_slam_amd", "csrc", "Makefile")).read()


def test_route_parser(tmp_path):
    from pi3_slam_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--start", "1", "2.5", "-3"])
    assert a.command == "route" and a.start == [1.0, 2.5, -3.0] and a.goal is None and a.from_trajectory is None
    assert a.radius == 0.0 and a.through_unknown is False and a.device == "cuda"
    a = p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--from-trajectory", "t.tum", "--goal", "0", "0",
                      "1", "--radius", "0.3", "--through-unknown"])
    assert a.from_trajectory == "t.tum" and a.goal == [0.0, 0.0, 1.0] and a.radius == 0.3 and a.through_unknown
    for argv in (["route", "--output", "out", "--start", "0", "0", "0"], ["route", "--occupancy", "o.npz"],
                 ["route", "--occupancy", "o.npz", "--output", "out", "--start", "0", "0"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    # one kind of source, refused before the file is read
    for extra in ([], ["--start", "0", "0", "0", "--from-trajectory", "t.tum"]):
        with pytest.raises(SystemExit, match="--start X Y Z or --from-trajectory"):
            cli.main(["route", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path)] + extra)
    with pytest.raises(SystemExit, match="route: .*missing.npz"):          # a file that is not there: one line, no traceback
        cli.main(["route", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path), "--start", "0", "0", "0"])
    with pytest.raises(SystemExit, match="radius"):
        cli.main(["route", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path), "--start", "0", "0",
                  "0", "--radius", "-1"])


def test_trajectory_positions(tmp_path):
    from pi3_slam_amd.grid_route import read_tum_positions
    path = tmp_path / "t.tum"
    path.write_text("# timestamp tx ty tz qx qy qz qw\n0 1.5 -2.0 0.25 0 0 0 1\n\n1 3 4 5 0 0 0 1  # note\n")
    assert read_tum_positions(str(path)).tolist() == [[1.5, -2.0, 0.25], [3.0, 4.0, 5.0]]
    path.write_text("# nothing\n")
    with pytest.raises(ValueError, match="no poses"):
        read_tum_positions(str(path))


def test_route_files(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.grid_route import Route, RouteField
    cost = np.array([[[0, 12, ref.FAR]]], np.uint32)
    f = RouteField(np.array([[[0.0, 0.5, np.inf]]], np.float32), cost, np.array([[[1, 1, 0]]], np.uint8),
                   np.array([1, 2, 3], np.int64), 0.5, np.array([[[1, 1, 2]]], np.uint8), None,
                   {"reachable": 2, "sweeps": 2}, {"radius": 0.0})
    export.write_route(f, None, str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["route.npz"]
    with np.load(tmp_path / "a" / "route.npz") as z:
        assert z["cost"].tobytes() == cost.tobytes() and z["cost"].dtype == np.uint32 and z["distance"].dtype == np.float32
        assert z["index_origin"].tolist() == [1, 2, 3] and z["origin"].tolist() == [0.5, 1.0, 1.5] and float(z["cell"]) == 0.5
        assert json.loads(str(z["counts"])) == {"reachable": 2, "sweeps": 2} and json.loads(str(z["settings"])) == {"radius": 0.0}
    way = np.array([[0.75, 1.25, 1.75], [1.25, 1.25, 1.75]])
    export.write_route(f, Route(way, np.array([0, 1]), 12, 0.5, 0.25, {"radius": 0.2}), str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "b")) == ["route.json", "route.npz", "route.ply"]
    rec = json.load(open(tmp_path / "b" / "route.json"))
    assert rec == {"waypoints": way.tolist(), "cost": 12, "length_m": 0.5, "min_clearance_m": 0.25, "settings": {"radius": 0.2}}
    from pi3_slam_amd import map_eval
    pts, cols = map_eval.read_ply_points(str(tmp_path / "b" / "route.ply"))
    assert pts.tolist() == way.astype(np.float32).tolist()
