"""Line of sight and taut ways on the GPU (csrc/grid_sight.hip), byte for byte against the oracle
(tests/grid_sight_ref.py): the two kernels over the shapes of the route tests, spans around the 64-bit word, ways of one
and two cells and several ways in one launch, the argument checks, GridRouter.sees / .taut on the door room, the
serpentine and the box room, plan_tour(taut=True) on the box room's cover, and `cli route --taut` / `cli views --cover
--tour --taut` on a two-chunk sequence.  Every output is filled with 0xFF bytes before each call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_route_ref as rref               # noqa: E402
import grid_sight_ref as sref               # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_gpu as view_gpu       # noqa: E402
from test_grid_view_gpu import reconstructed  # noqa: E402,F401  (the two-chunk sequence's reconstruction, a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = [(1, 1, 1), (1, 1, 300), (300, 2, 3), (9, 8, 7), (17, 9, 20), (65, 67, 66)]       # (nx, ny, nz)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _walks(dims):
    """The four walks of a shape: mazes at 0.3 and 0.45 blocked, all free, all blocked."""
    shape = dims[::-1]
    return {"maze30": rref.walk_mask(rref.maze(shape, 0.3, 1)), "maze45": rref.walk_mask(rref.maze(shape, 0.45, 2)),
            "free": np.ones(shape, np.uint8), "blocked": np.zeros(shape, np.uint8)}


def _wander(rng, dims, n, stride=1):
    """n cells of a lattice walk with steps in {-stride .. stride}^3, held inside the grid: linear indices."""
    hi = np.asarray(dims, np.int64) - 1
    at = rng.integers(0, hi + 1)
    out = []
    for _ in range(n):
        out.append(int((at[2] * dims[1] + at[1]) * dims[0] + at[0]))
        at = np.clip(at + rng.integers(-stride, stride + 1, 3), 0, hi)
    return np.asarray(out, np.int64)


def _paths_device(walk, cells, offsets, span):
    from pi3_slam_amd import ops
    vis = torch.full((len(cells), ops.grid_sight_words(span)), -1, dtype=torch.int64, device=DEV)
    ops.grid_route_sight_paths(_dev(walk), _dev(np.asarray(cells, np.int64)), _dev(np.asarray(offsets, np.int64)), span, vis)
    return vis.cpu().numpy().view(np.uint64)


def _pairs_device(walk, d2, a, b, low_fill=-1):
    from pi3_slam_amd import ops
    N = len(a)
    sees = torch.full((N,), 0xFF, dtype=torch.uint8, device=DEV)
    touched = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    low = torch.full((N,), low_fill, dtype=torch.int16, device=DEV)
    ops.grid_route_sight_pairs(_dev(walk), None if d2 is None else _dev(np.asarray(d2, np.uint16).view(np.int16)),
                               _dev(np.asarray(a, np.int64)), _dev(np.asarray(b, np.int64)), sees, touched, low)
    return sees.cpu().numpy(), touched.cpu().numpy(), low.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_paths_and_pairs_match_the_oracle_byte_for_byte(dims):
    """Four ways in one launch (1, 2, 70 and 77 cells; the third holds indices outside the grid) at span 65, so that a
    row has a second word with one live bit, and 300 pairs with their special cases, on all four walks of the shape."""
    rng = np.random.default_rng(sum(dims))
    n_cells = dims[0] * dims[1] * dims[2]
    legs = [_wander(rng, dims, 1), _wander(rng, dims, 2), _wander(rng, dims, 70), _wander(rng, dims, 77, 2)]
    legs[2][[5, 40]] = (-1, n_cells)
    cells = np.concatenate(legs)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in legs])])
    a = np.concatenate([_wander(rng, dims, 150, 3), rng.integers(0, n_cells, 150)])
    b = np.concatenate([_wander(rng, dims, 150, 3), rng.integers(0, n_cells, 150)])
    a[:4], b[:4] = (-1, 0, n_cells, -7), (0, n_cells, 0, n_cells + 9)      # ends outside the grid
    b[4:8] = a[4:8]                                                         # a == b
    d2 = rng.integers(0, 0xFFFF, dims[::-1]).astype(np.uint16)
    d2.reshape(-1)[rng.integers(0, n_cells, max(n_cells // 8, 1))] = 0xFFFF
    some_bits = 0
    for name, walk in _walks(dims).items():
        exp_bits = sref.vis_bits(walk, cells, offsets, 65)
        got = _paths_device(walk, cells, offsets, 65)
        assert got.shape == (150, 2) and got.tobytes() == sref.pack_words(exp_bits).tobytes(), name
        # no bit crosses a way's end, and the bits past it stay 0
        for l in range(4):
            for p in range(offsets[l], offsets[l + 1]):
                assert not exp_bits[p, offsets[l + 1] - p - 1:].any()
        assert not exp_bits[[0, 2]].any() and not exp_bits[3 + 5].any()     # last cells of a way, an index outside
        if name == "free":
            assert exp_bits[1, 0] and exp_bits[3, :4].all()
        if name == "blocked":
            assert not exp_bits.any()
        some_bits += int(exp_bits.sum())
        for field in (d2, None):
            exp = sref.sight_pairs(walk, field, a, b)
            got = _pairs_device(walk, field, a, b, -1 if field is not None else 0x5555)   # 0xFFFF is the answer there
            for g, e, what in zip(got, exp, ("sees", "touched", "min_d2")):
                assert g.dtype == e.dtype and g.tobytes() == e.tobytes(), (name, what, field is None)
        assert exp[0][:4].tolist() == [0] * 4 and exp[1][:8].tolist() == [0] * 4 + [1] * 4
    assert some_bits > 0


@pytest.mark.parametrize("span", [1, 63, 64, 65, 256])
def test_spans_around_the_word(span):
    """Ways of 300, 1, 2 and 130 cells through a thin maze: rows with up to four words, partners in every one."""
    dims = (17, 9, 20)
    walk = rref.walk_mask(rref.maze(dims[::-1], 0.05, 7))
    rng = np.random.default_rng(span)
    legs = [_wander(rng, dims, 300), _wander(rng, dims, 1), _wander(rng, dims, 2), _wander(rng, dims, 130)]
    cells = np.concatenate(legs)
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in legs])])
    bits = sref.vis_bits(walk, cells, offsets, span)
    got = _paths_device(walk, cells, offsets, span)
    assert got.shape == (433, (span + 63) // 64) and got.tobytes() == sref.pack_words(bits).tobytes()
    assert bits[:, span - 1].any() and not bits.all()               # the last bit of the span is used
    if span == 65:
        assert (got[:, 1] <= 1).all() and (got[:, 1] == 1).any()    # the second word's bits past the span are 0
    if span == 63:
        assert (got[:, 0] >> np.uint64(63) == 0).all()


def test_nothing_to_do_launches_nothing():
    from pi3_slam_amd import ops
    walk = _dev(np.ones((3, 4, 5), np.uint8))
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    ops.grid_route_sight_paths(walk, none, _dev(np.array([0, 0], np.int64)), 64, torch.zeros((0, 1), dtype=torch.int64, device=DEV))
    vis = torch.full((3, 1), -1, dtype=torch.int64, device=DEV)
    ops.grid_route_sight_paths(walk, _dev(np.array([0, 1, 2], np.int64)), _dev(np.array([0], np.int64)), 64, vis)   # no way
    ops.grid_route_sight_pairs(walk, None, none, none, torch.zeros(0, dtype=torch.uint8, device=DEV),
                               torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int16, device=DEV))
    torch.cuda.synchronize()
    assert vis.tolist() == [[-1]] * 3


def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L, ops
    lib = L.load()
    shape = (3, 4, 5)
    walk = torch.ones(shape, dtype=torch.uint8, device=DEV)
    cells = torch.arange(6, dtype=torch.int64, device=DEV)
    offsets = _dev(np.array([0, 6], np.int64))
    vis = torch.full((6, 64), -1, dtype=torch.int64, device=DEV)
    sees = torch.full((6,), 0xFF, dtype=torch.uint8, device=DEV)
    touched = torch.full((6,), -1, dtype=torch.int32, device=DEV)
    low = torch.full((6,), -1, dtype=torch.int16, device=DEV)
    sp = L.stream_ptr()
    w, c, o, v, s, t, m = (x.data_ptr() for x in (walk, cells, offsets, vis, sees, touched, low))
    big = (513, 261633, 1)                                          # 2^27 + 1 cells, every dimension below 2^21
    calls = [lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, o, 1, 0, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, o, 1, -64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, o, 1, 4097, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 0, 3, c, 6, o, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, *big, c, 6, o, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(None, 5, 4, 3, c, 6, o, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, None, 6, o, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, None, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, o, 1, 64, None, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, -1, o, 1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_paths(w, 5, 4, 3, c, 6, o, -1, 64, v, sp),
             lambda: lib.pi3_grid_route_sight_pairs(None, None, 5, 4, 3, c, c, 6, s, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, -3, c, c, 6, s, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, *big, c, c, 6, s, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, None, c, 6, s, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, c, None, 6, s, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, c, c, 6, None, t, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, c, c, 6, s, None, m, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, c, c, 6, s, t, None, sp),
             lambda: lib.pi3_grid_route_sight_pairs(w, None, 5, 4, 3, c, c, -6, s, t, m, sp)]
    for i, call in enumerate(calls):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert b"pi3_grid_route_sight_" in err and b"2^27" in err, (i, err)
        assert i > 2 or b"span=" in err and b"(1 .. 4096)" in err
    with pytest.raises(L.Pi3HipError, match=r"span=5000 \(1 \.\. 4096\)"):
        ops.grid_route_sight_paths(walk, cells, offsets, 5000, vis)
    torch.cuda.synchronize()
    assert bool((vis == -1).all()) and bool((sees == 0xFF).all()) and bool((touched == -1).all()) and bool((low == -1).all())


# ------------------------------------------------------------------------------------------------ 2. the router
def _oracle_taut(walk, cells, span, d2=None):
    """-> (indices, length in cells, the smallest d2 over the touched cells) of the trace's taut way."""
    cells = np.asarray(cells, np.int64)
    nz, ny, nx = walk.shape
    xyz = np.stack([cells % nx, (cells // nx) % ny, cells // (nx * ny)], 1)
    reach = max(1, min(span, len(cells) - 1))
    idx, length = sref.taut(sref.vis_bits(walk, cells, [0, len(cells)], reach), xyz, reach)
    sees, _, low = sref.sight_pairs(walk, d2, cells[idx[:-1]], cells[idx[1:]])
    assert sees.all()
    if d2 is None:
        return idx, length, None
    return idx, length, int(low.min()) if len(low) else int(np.asarray(d2).reshape(-1)[cells[0]])


def test_door_room_and_serpentine_through_the_router():
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.grid_route import GridRouter
    r = rref.door_room()
    nx, ny, cell = 24, 16, r["cell"]
    origin = np.array([-4, -3, 0], np.int64)

    def centre(x, y, z):
        return cell * (np.array([x, y, z]) + origin + 0.5)
    router = GridRouter()
    field = router.field(OccupancyGrid(r["state"], origin, cell), centre(2, 1, 1), DEV)
    route = router.path(field, centre(21, 14, 1))
    taut = router.taut(field, route)
    walk = rref.walk_mask(r["state"])
    idx, length, _ = _oracle_taut(walk, route.cells, 256)
    print(f"door room: {len(route.cells)} cells, {route.length_m:.4f} m, taut {taut.length_m:.4f} m over {taut.indices.tolist()}")
    assert len(route.cells) == 20 and abs(route.length_m - 6.0962) < 5e-5 and abs(taut.length_m - 5.7554) < 5e-5
    assert taut.indices.tolist() == idx == [0, 19] and taut.length_m == cell * length and taut.span == 256
    assert taut.cells.tolist() == route.cells[[0, 19]].tolist() and taut.waypoints.tolist() == route.waypoints[[0, 19]].tolist()
    assert taut.min_clearance_m is None and route.min_clearance_m is None and taut.settings["taut_span"] == 256
    one = router.taut(field, route, span=1)
    assert one.indices.tolist() == list(range(20)) and abs(one.length_m - route.length_m) < 1e-12
    assert router.sees(field, centre(3, 7, 1), centre(20, 7, 1)) is True        # through the gap
    assert router.sees(field, centre(2, 1, 1), centre(21, 14, 1)) is True
    assert router.sees(field, centre(3, 1, 1), centre(20, 1, 1)) is False       # through the wall
    assert router.sees(field, centre(11, 0, 1), centre(11, 0, 1)) is False      # a wall cell does not see itself
    assert router.sees(field, centre(5, 5, 0), centre(5, 5, 0)) is True
    with pytest.raises(ValueError, match="the goal .* lies outside the grid"):
        router.sees(field, centre(3, 1, 1), [100.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="the start .* lies outside the grid"):
        router.sees(field, [100.0, 0.0, 0.0], centre(3, 1, 1))
    with pytest.raises(ValueError, match="the span of a taut way is 1 .. 4096"):
        router.taut(field, route, span=0)
    # the serpentine: a vertex at either side of every gap; a short span costs length
    state, src, goal = rref.serpentine()
    grid = OccupancyGrid(state, np.zeros(3, np.int64), 1.0)
    field = router.field(grid, [0.5, 0.5, 0.5], DEV)
    route = router.path(field, [32.5, 32.5, 0.5])
    walk = rref.walk_mask(state)
    for span, metres in ((256, 304.4683), (32, 304.4683), (8, 305.848)):
        taut = router.taut(field, route, span)
        idx, length, _ = _oracle_taut(walk, route.cells, span)
        assert taut.indices.tolist() == idx and taut.length_m == length and abs(length - metres) < 5e-4
    assert len(route.cells) == 305 and router.taut(field, route, 4096).indices.tolist() == [0] + [
        v for k in range(32, 273, 34) for v in (k, k + 2)] + [304]


@pytest.fixture(scope="module")
def box_room():
    from pi3_slam_amd.dense_map import OccupancyGrid
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    d2a = oref.edt_ref(state, R, False)                          # the planner's: clearance against occupied cells only
    return grid, centres, (walk_u, d2u), (rref.walk_mask(state, d2a, min_d2), d2a)


def _metres(cell, d2):
    return float("inf") if d2 == 0xFFFF else float(np.float32(cell * np.sqrt(np.float64(d2))))


def test_box_room_between_opposite_cameras(box_room):
    from pi3_slam_amd.grid_route import GridRouter
    grid, centres, (walk, d2), _ = box_room
    router = GridRouter(radius=route_cases.BOX_RADIUS)
    field = router.field(grid, centres[0], DEV)
    route = router.path(field, centres[6])
    taut = router.taut(field, route)
    idx, length, low = _oracle_taut(walk, route.cells, 256, d2)       # re-checks every chosen segment
    print(f"box room: {len(route.cells)} cells, {route.length_m:.4f} m, taut {taut.length_m:.4f} m over "
          f"{taut.indices.tolist()}, clearance {taut.min_clearance_m} (the trace's {route.min_clearance_m})")
    assert taut.indices.tolist() == idx and taut.length_m == float(grid.cell) * length
    assert taut.min_clearance_m == _metres(float(grid.cell), low) and taut.min_clearance_m >= route_cases.BOX_RADIUS
    straight = float(np.linalg.norm(route.waypoints[-1] - route.waypoints[0]))
    assert straight - 1e-9 <= taut.length_m <= route.length_m and len(idx) < len(route.cells)


def test_box_room_tour_with_taut_legs(box_room):
    from pi3_slam_amd.view_planner import ViewPlanner
    grid, centres, _, (walk, d2) = box_room
    cell = float(grid.cell)
    ten = ViewPlanner(route_cases.BOX_RADIUS, view_gpu.BOX_RANGE_CELLS * cell, 90, 4, 10).cover(grid, centres, DEV)
    plain, tour = ten.tour(), ten.tour(taut=True, taut_span=64)
    assert tour.order == plain.order and tour.matrix.tolist() == plain.matrix.tolist() and tour.cost == plain.cost
    assert tour.counts == plain.counts and tour.settings == plain.settings and tour.length_m == plain.length_m
    assert [c.tolist() for c in tour.leg_cells] == [c.tolist() for c in plain.leg_cells]
    assert [s._record() for s in tour.stops] == [s.record() for s in plain.stops]
    assert plain.taut_length_m is None and plain.taut_leg_cells is None and plain.stops[0].taut_length_m is None
    total = 0.0
    for stop, leg, way, t_cells, t_way, t_idx in zip(tour.stops, tour.leg_cells, tour.leg_waypoints, tour.taut_leg_cells,
                                                     tour.taut_leg_waypoints, tour.taut_leg_indices):
        idx, length, low = _oracle_taut(walk, leg, 64, d2)
        assert t_idx.tolist() == idx and t_cells.tolist() == leg[idx].tolist() and len(t_way) == len(idx)
        assert stop.taut_length_m == cell * length <= stop.length_m
        assert stop.taut_min_clearance_m == _metres(cell, low) >= route_cases.BOX_RADIUS
        assert t_way.tolist() == way[idx].tolist() and t_way[-1].tolist() == stop.position.tolist()
        total += stop.taut_length_m
    print(f"box room tour: {tour.length_m:.3f} m, taut {tour.taut_length_m:.3f} m over {tour.taut_vertices} vertices")
    assert abs(tour.taut_length_m - total) < 1e-9 and tour.taut_length_m <= tour.length_m and tour.taut_span == 64


# ------------------------------------------------------------------------------------------------ 3. end to end
def _same_files(a, b, names):
    for name in names:
        assert open(a / name, "rb").read() == open(b / name, "rb").read(), name


def test_cli_route_taut_on_a_reconstruction(reconstructed, capsys):   # noqa: F811
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    pos = read_tum_positions(tum)
    cell = float(grid.cell)
    d2 = oref.edt_ref(grid.state, 1, True)
    walk = rref.walk_mask(grid.state, d2, 1)
    base = (["route", "--occupancy", occ, "--start"] + [repr(float(v)) for v in pos[0]] + ["--goal"]
            + [repr(float(v)) for v in pos[-1]] + ["--radius", str(view_gpu.ROUTE_RADIUS), "--device", DEV])
    cli.main(base + ["--output", str(tmp / "r_off")])
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp / "r_on"), "--taut", "--taut-span", "32"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("route: ")]
    assert sorted(os.listdir(tmp / "r_on")) == ["route.json", "route.npz", "route.ply", "route_taut.ply"]
    assert sorted(os.listdir(tmp / "r_off")) == ["route.json", "route.npz", "route.ply"]
    _same_files(tmp / "r_on", tmp / "r_off", ["route.npz", "route.ply"])
    off, on = json.load(open(tmp / "r_off" / "route.json")), json.load(open(tmp / "r_on" / "route.json"))
    assert {k: on[k] for k in off} == off
    way = np.asarray(off["waypoints"])
    cells = GridRouter.linear(GridRouter.world_cells(way, grid), grid.state.shape)
    idx, length, low = _oracle_taut(walk, cells, 32, d2)
    clear = _metres(cell, low)
    assert {k: on[k] for k in on if k not in off} == {
        "taut_waypoints": way[idx].tolist(), "taut_indices": idx, "taut_length_m": cell * length,
        "taut_min_clearance_m": "inf" if np.isinf(clear) else clear, "taut_span": 32}
    assert on["taut_length_m"] <= off["length_m"] + 1e-12
    assert len(line) == 1 and f"; taut {on['taut_length_m']:.3f} m over {len(idx)} vertices" in line[0]
    print(line[0])


def test_cli_views_tour_taut_on_a_reconstruction(reconstructed, capsys):   # noqa: F811
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    cell = float(grid.cell)
    d2 = oref.edt_ref(grid.state, 1, False)
    walk = rref.walk_mask(grid.state, d2, 1)
    poses = read_tum_positions(tum)
    src = GridRouter.linear(GridRouter.world_cells(poses, grid), grid.state.shape)
    good = [i for i, s in enumerate(src) if s >= 0 and walk.reshape(-1)[s]]
    assert good
    extra = []
    if good[-1] != len(src) - 1:                                # the last pose stands on no traversable cell: say where
        extra = ["--tour-from"] + [f"{v:.6f}" for v in poses[good[-1]]]
    base = ["views", "--occupancy", occ, "--from-trajectory", tum, "--radius", str(view_gpu.ROUTE_RADIUS), "--range",
            "0.8", "--stride", "2", "--count", "5", "--device", DEV, "--cover", "--tour", "--route-to", "0"] + extra
    cli.main(base + ["--output", str(tmp / "t_off")])
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp / "t_on"), "--taut"])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("views: ")]
    assert sorted(set(os.listdir(tmp / "t_on")) - set(os.listdir(tmp / "t_off"))) == ["route_taut.ply"]
    _same_files(tmp / "t_on", tmp / "t_off", ["views.json", "views.npz", "views.ply", "route.npz", "route.ply", "tour.ply"])
    off, on = json.load(open(tmp / "t_off" / "tour.json")), json.load(open(tmp / "t_on" / "tour.json"))
    with np.load(tmp / "t_off" / "tour.npz") as z:
        old = {k: z[k].copy() for k in z.files}
    with np.load(tmp / "t_on" / "tour.npz") as z:
        new = {k: z[k].copy() for k in z.files}
    assert all(new[k].tobytes() == old[k].tobytes() for k in old)
    assert sorted(set(new) - set(old)) == ["taut_offsets", "taut_waypoint_cells", "taut_waypoints"]
    legs = [old["waypoint_cells"][a:b] for a, b in zip(old["offsets"][:-1], old["offsets"][1:])]
    t_cells, t_offsets, total, vertices = [], [0], 0.0, 0
    assert len(on["stops"]) == len(legs) == len(off["stops"]) >= 1
    for stop_on, stop_off, leg in zip(on["stops"], off["stops"], legs):
        idx, length, low = _oracle_taut(walk, leg, 256, d2)
        clear = _metres(cell, low)
        assert stop_on.pop("taut_length_m") == cell * length <= stop_off["length_m"] + 1e-12
        assert stop_on.pop("taut_min_clearance_m") == ("inf" if np.isinf(clear) else clear)
        assert stop_on == stop_off
        t_cells += leg[idx].tolist()
        t_offsets.append(len(t_cells))
        total += cell * length
        vertices += len(idx)
    assert abs(on.pop("taut_length_m") - total) < 1e-9 and (on.pop("taut_span"), on.pop("taut_vertices")) == (256, vertices)
    assert on == off
    assert new["taut_waypoint_cells"].tolist() == t_cells and new["taut_offsets"].tolist() == t_offsets
    shape = grid.state.shape
    assert GridRouter.linear(GridRouter.world_cells(new["taut_waypoints"], grid), shape).tolist() == t_cells
    # the way to the best view, pulled taut as `route` does it
    r_off, r_on = json.load(open(tmp / "t_off" / "route.json")), json.load(open(tmp / "t_on" / "route.json"))
    assert {k: r_on[k] for k in r_off} == r_off
    cells = GridRouter.linear(GridRouter.world_cells(np.asarray(r_off["waypoints"]), grid), shape)
    idx, length, low = _oracle_taut(walk, cells, 256, d2)
    assert r_on["taut_indices"] == idx and r_on["taut_length_m"] == cell * length and r_on["taut_span"] == 256
    assert len(line) == 1 and f", taut {total:.2f} m of {off['length_m']:.2f} m over {vertices} vertices" in line[0]
    assert f"; taut {r_on['taut_length_m']:.3f} m over {len(idx)} vertices" in line[0]
    print(line[0])
