"""Routes through the occupancy grid on the GPU (csrc/grid_route.hip), byte for byte against the oracle
(tests/grid_route_ref.py): the init, sweep and trace kernels, the number of sweeps a tile-relaxing kernel may need, the
door and box-room scenes, and reconstruct -> occupancy.npz -> `cli route` on a two-chunk sequence.  Every output is
filled with a poison value before each call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_route_ref as ref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as cpu_cases         # noqa: E402  (the box-room case and its conditions)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON8, POISON32, POISON64 = 7, -5, 11


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _init_device(state, d2, min_d2, through_unknown, sources):
    from pi3_slam_amd import ops
    st = _dev(state)
    walk = torch.full(st.shape, POISON8, dtype=torch.uint8, device=DEV)
    dist = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_init(st, None if d2 is None else _dev(np.asarray(d2, np.uint16).view(np.int16)), min_d2,
                        through_unknown, _dev(np.asarray(sources, np.int64).reshape(-1)), walk, dist, counters)
    return walk, dist, counters.tolist()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _settle(walk, dist):
    """-> the sweeps the device ran, the quiet one included (GridRouter's own loop)."""
    from pi3_slam_amd.grid_route import GridRouter
    return GridRouter().relax(walk, dist, int(walk.sum().item()))


def _trace_device(walk, dist, goal, cap):
    from pi3_slam_amd import ops
    path = torch.full((cap,), POISON64, dtype=torch.int64, device=DEV)
    length = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_trace(walk, dist, goal, path, length)
    return path.cpu().numpy(), int(length.item())


def _check_path(path, walk, dist, goal):
    """The conditions of a route that do not need the oracle's trace."""
    shape = np.asarray(walk).shape
    ok = ref.allowed_moves(walk)
    walk, dist = np.asarray(walk).reshape(-1), np.asarray(dist).reshape(-1)
    assert path[0] == goal and dist[path[-1]] == 0 and walk[path].all()
    total = 0
    nz, ny, nx = shape
    for a, b in zip(path, path[1:]):
        w = ref.step_cost(int(a), int(b), shape)
        assert w, (a, b)
        d = (int(b % nx - a % nx), int((b // nx) % ny - (a // nx) % ny), int(b // (nx * ny) - a // (nx * ny)))
        k = ref.MOVES.index((d[0], d[1], d[2], w))
        assert ok[k].reshape(-1)[a], (a, b)
        total += w
    assert total == dist[goal]


# ------------------------------------------------------------------------------------------------ 1. init
@pytest.mark.parametrize("through_unknown", [False, True])
@pytest.mark.parametrize("with_d2", [False, True])
def test_init_matches_oracle_byte_for_byte(with_d2, through_unknown):
    shape = (5, 9, 67)
    state = ref.maze(shape, 0.4, 11)
    assert {0, 1, 2} == set(np.unique(state).tolist())
    d2 = oref.edt_ref(state, 2, not through_unknown) if with_d2 else None
    min_d2 = 2 if with_d2 else 0
    w = ref.walk_mask(state, d2, min_d2, through_unknown).reshape(-1)
    on, off = np.flatnonzero(w), np.flatnonzero(w == 0)
    occupied = np.flatnonzero(state.reshape(-1) == 2)
    sources = [on[0], on[5], on[5], on[-1], off[0], occupied[3], occupied[3], -1, state.size, state.size + 7, -(1 << 40),
               1 << 40, on[len(on) // 2]]
    for src in (sources, [], [on[1]]):
        exp = ref.init(state, d2, min_d2, through_unknown, src)
        walk, dist, counters = _init_device(state, d2, min_d2, through_unknown, src)
        assert walk.cpu().numpy().tobytes() == exp["walk"].tobytes()
        assert _u32(dist).tobytes() == exp["dist"].tobytes()
        assert counters == exp["counters"], (counters, exp["counters"])
    exp = ref.init(state, d2, min_d2, through_unknown, sources)
    assert exp["counters"][1:] == [5, 3, 5] and 0 < exp["counters"][0] < state.size
    none = ref.init(state, d2, min_d2, through_unknown, [])
    assert (none["dist"] == ref.FAR).all()                      # Ns = 0: an all-far field


# ------------------------------------------------------------------------------------------------ 2. sweep and trace
def _open_field(shape, sources):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    best = None
    for s in sources:
        off = np.sort(np.stack([abs(x - s % nx), abs(y - (s // nx) % ny), abs(z - s // (nx * ny))], -1), -1)
        d = 12 * (off[..., 2] - off[..., 1]) + 17 * (off[..., 1] - off[..., 0]) + 21 * off[..., 0]
        best = d if best is None else np.minimum(best, d)
    return best.astype(np.uint32)


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 300), (300, 2, 3), (9, 8, 7), (17, 9, 20), (65, 67, 66)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_sweeps_reach_the_oracles_field_byte_for_byte(dims):
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    states = {"0.3": ref.maze(shape, 0.3, nx + ny + nz), "0.45": ref.maze(shape, 0.45, nx + 2 * ny + 3 * nz),
              "free": np.ones(shape, np.uint8), "blocked": np.full(shape, 2, np.uint8)}
    for name, state in states.items():
        w = ref.walk_mask(state)
        on = np.flatnonzero(w.reshape(-1))
        first, last = (int(on[0]), int(on[-1])) if len(on) else (0, state.size - 1)
        for sources in ([first], [first, last]):
            if name == "free":
                exp = _open_field(shape, sources)               # the closed form (test_grid_route.py: it is Dijkstra's)
            else:
                exp = ref.distances(w, sources)
            walk, dist, counters = _init_device(state, None, 0, False, sources)
            sweeps = _settle(walk, dist)
            got = _u32(dist)
            assert got.tobytes() == exp.tobytes(), (name, sources, int((got != exp).sum()))
            assert sweeps >= 1 and (name != "blocked" or sweeps == 1)
            again = _settle(walk, dist)                         # a settled field: one quiet sweep, nothing moves
            assert again == 1 and _u32(dist).tobytes() == exp.tobytes()
            # the way back from the farthest reachable cell
            flat = exp.reshape(-1)
            reach = np.flatnonzero(flat != ref.FAR)
            if not len(reach):
                continue
            goal = int(reach[np.argmax(flat[reach])])
            cap = int(flat[goal]) // 12 + 1
            path, length = _trace_device(walk, dist, goal, cap)
            assert length >= 1 and (path[length:] == POISON64).all()
            assert path[:length].tolist() == ref.trace(w, exp, goal), (name, sources)
            _check_path(path[:length], w, exp, goal)
        print(f"{dims} {name}: {int((exp != ref.FAR).sum())} of {exp.size} cells reached in {sweeps} sweeps")


def test_a_launch_relaxes_whole_tiles():
    """A sweep that moved the front by one cell per launch would need 300 and 311 launches here."""
    walk_np = np.ones((1, 1, 300), np.uint8)
    exp, launches, changing = ref.tile_sweeps(walk_np, [0])
    walk, dist, _ = _init_device(walk_np, None, 0, False, [0])
    sweeps = _settle(walk, dist)
    print(f"line: {sweeps} sweeps on the device, {launches} in the emulation")
    assert _u32(dist).tobytes() == exp.tobytes()
    assert sweeps - 1 <= 38 and sweeps <= launches              # it changes something once per tile it crosses at most
    state, src, corner = ref.serpentine()
    exp, launches, changing = ref.tile_sweeps(ref.walk_mask(state), [src])
    assert launches == 38
    walk, dist, _ = _init_device(state, None, 0, False, [src])
    sweeps = _settle(walk, dist)
    print(f"serpentine: {sweeps} sweeps on the device, {launches} in the emulation")
    assert _u32(dist).tobytes() == exp.tobytes() and _u32(dist).reshape(-1)[corner] == 3728
    assert sweeps <= launches


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", [(5, 17, 19), (17, 9, 20), (3, 24, 24)], ids=lambda s: "%dx%dx%d" % s)
def test_mazes_settle_within_the_emulations_sweeps(shape, seed):
    state = ref.maze(shape, 0.3, seed)
    w = ref.walk_mask(state)
    src = int(np.flatnonzero(w.reshape(-1))[0])
    exp, launches, _ = ref.tile_sweeps(w, [src])
    walk, dist, _ = _init_device(state, None, 0, False, [src])
    sweeps = _settle(walk, dist)
    assert _u32(dist).tobytes() == exp.tobytes() and sweeps <= launches
    flat = exp.reshape(-1)
    reach = np.flatnonzero(flat != ref.FAR)
    for goal in (int(reach[np.argmax(flat[reach])]), int(reach[len(reach) // 2]), src):
        cap = int(flat[goal]) // 12 + 1
        path, length = _trace_device(walk, dist, goal, cap)
        exp_path = ref.trace(w, exp, goal)
        assert path[:length].tolist() == exp_path and (path[length:] == POISON64).all()
        _check_path(path[:length], w, exp, goal)
        if goal == src:
            assert length == 1 and path[0] == src               # the goal is a source
        if length > 1:                                          # one too short: the needed length, path untouched
            short, needed = _trace_device(walk, dist, goal, length - 1)
            assert needed == -length and (short == POISON64).all()
    # a goal that is not traversable, and one that no source reaches
    blocked = int(np.flatnonzero(w.reshape(-1) == 0)[0])
    path, length = _trace_device(walk, dist, blocked, 4)
    assert length == 0 and (path == POISON64).all()
    cut = np.flatnonzero((flat == ref.FAR) & (w.reshape(-1) == 1))
    if len(cut):
        path, length = _trace_device(walk, dist, int(cut[0]), 4)
        assert length == 0 and (path == POISON64).all()


# ------------------------------------------------------------------------------------------------ 3. door and box room
@pytest.mark.parametrize("radius,cells,min_d2,reachable", [(0.25, 1, 1, True), (0.5, 2, 4, True), (0.625, 3, 7, False)])
def test_the_door_lets_through_what_fits(radius, cells, min_d2, reachable):
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.grid_route import GridRouter
    r = ref.door_room()
    nx, ny, nz = 24, 16, 3
    router = GridRouter(radius)
    assert router.clearance_cells(r["cell"]) == (cells, min_d2)
    st = _dev(r["state"])
    d2 = torch.full(st.shape, POISON32, dtype=torch.int16, device=DEV)
    ops.grid_edt(st, cells, True, d2, torch.empty_like(d2))
    d2_np = d2.cpu().numpy().view(np.uint16)
    assert d2_np.tobytes() == oref.edt_ref(r["state"], cells, True).tobytes()
    walk, dist, counters = _init_device(r["state"], d2_np, min_d2, False, [r["start"]])
    _settle(walk, dist)
    w = ref.walk_mask(r["state"], d2_np, min_d2)
    exp = ref.distances(w, [r["start"]])
    assert walk.cpu().numpy().tobytes() == w.tobytes() and _u32(dist).tobytes() == exp.tobytes()
    path, length = _trace_device(walk, dist, r["goal"], 64)
    if not reachable:
        assert length == 0 and (path == POISON64).all() and exp.reshape(-1)[r["goal"]] == ref.FAR
    else:
        assert path[:length].tolist() == ref.trace(w, exp, r["goal"]) and path[length - 1] == r["start"]
        in_wall = [int((p // nx) % ny) for p in path[:length] if p % nx == r["wall_x"]]
        assert in_wall and (radius != 0.5 or set(in_wall) == {7})
    # the same through the router, in world coordinates
    grid = OccupancyGrid(r["state"], np.array([-4, -3, 0], np.int64), r["cell"])

    def centre(i):
        return r["cell"] * (np.array([i % nx - 4, (i // nx) % ny - 3, i // (nx * ny)]) + 0.5)
    field = router.field(grid, centre(r["start"]), DEV)
    assert field.cost.tobytes() == exp.tobytes() and field.walk.tobytes() == w.tobytes()
    route = router.path(field, centre(r["goal"]))
    if not reachable:
        assert route is None and np.isinf(field.distance.reshape(-1)[r["goal"]])
    else:
        assert route.cells.tolist() == path[:length][::-1].tolist() and route.cost == exp.reshape(-1)[r["goal"]]
        assert route.waypoints[0].tolist() == centre(r["start"]).tolist()
        assert route.waypoints[-1].tolist() == centre(r["goal"]).tolist()
        assert route.min_clearance_m >= radius and route.length_m >= r["cell"] * 17
        assert field.distance.reshape(-1)[r["goal"]] == np.float32(r["cell"] * route.cost / 12.0)
    with pytest.raises(ValueError, match=r"the goal is not traversable: cell \(11, 0, 1\) is occupied with a clearance of 0 m"):
        router.path(field, centre((1 * ny + 0) * nx + 11))
    with pytest.raises(ValueError, match=r"the start is not traversable: cell \(11, 0, 1\) is occupied"):
        router.field(grid, centre((1 * ny + 0) * nx + 11), DEV)
    with pytest.raises(ValueError, match="outside the grid"):
        router.path(field, [100.0, 0.0, 0.0])


def test_box_room_through_the_router():
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.grid_route import GridRouter
    room, state, cams, d2, w, (R, min_d2) = cpu_cases.box_room_case()
    grid = OccupancyGrid(state, np.asarray(room["origin"], np.int64), room["cell"])
    router = GridRouter(radius=cpu_cases.BOX_RADIUS)
    centres = room["cell"] * ((cams + np.asarray(room["origin"])).astype(np.float64) + 0.5)
    field = router.field(grid, centres, DEV)
    lin = [int((c[2] * state.shape[1] + c[1]) * state.shape[2] + c[0]) for c in cams]
    exp = ref.distances(w, lin)
    assert field.walk.tobytes() == w.tobytes() and field.cost.tobytes() == exp.tobytes()
    assert field.counts["sources_accepted"] == 12 and field.counts["reachable"] == int((exp != ref.FAR).sum())
    assert field.clearance.tobytes() == oref.clearance(d2, room["cell"]).tobytes()
    one = router.field(grid, centres[0], DEV)
    route = router.path(one, centres[6])
    print(f"box room: {field.counts}, route {len(route.waypoints)} waypoints, {route.length_m:.2f} m, clearance "
          f"{route.min_clearance_m}")
    cpu_cases.check_box_room(room, state, cams, d2, w, one.cost, route.cells[::-1].tolist(), 0, 6)
    assert route.min_clearance_m >= cpu_cases.BOX_RADIUS and route.cost == one.cost.reshape(-1)[lin[6]]
    assert route.cells[::-1].tolist() == ref.trace(w, one.cost, lin[6])


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    shape = (3, 4, 5)
    state = torch.ones(shape, dtype=torch.uint8, device=DEV)
    d2 = torch.full(shape, 9, dtype=torch.int16, device=DEV)
    walk = torch.full(shape, POISON8, dtype=torch.uint8, device=DEV)
    dist = torch.full(shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    sources = torch.zeros(2, dtype=torch.int64, device=DEV)
    changed = torch.full((1,), POISON32, dtype=torch.int32, device=DEV)
    path = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    length = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    sp = L.stream_ptr()
    s, d, w, ds, c, so = (t.data_ptr() for t in (state, d2, walk, dist, counters, sources))
    ch, pa, le = changed.data_ptr(), path.data_ptr(), length.data_ptr()
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    assert big[0] * big[1] * big[2] == (1 << 27) + 1
    calls = [lambda: lib.pi3_grid_route_init(None, d, 4, 0, 5, 4, 3, so, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 4, 3, so, 2, None, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 4, 3, so, 2, w, None, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 4, 3, so, 2, w, ds, None, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 4, 3, None, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, None, 4, 0, 5, 4, 3, so, 2, w, ds, c, sp),          # min_d2 without d2
             lambda: lib.pi3_grid_route_init(s, d, -1, 0, 5, 4, 3, so, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 65026, 0, 5, 4, 3, so, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 0, 3, so, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, 5, 4, 3, so, -1, w, ds, c, sp),
             lambda: lib.pi3_grid_route_init(s, d, 4, 0, *big, so, 2, w, ds, c, sp),
             lambda: lib.pi3_grid_route_sweep(None, 5, 4, 3, ds, ch, sp),
             lambda: lib.pi3_grid_route_sweep(w, 5, 4, 3, None, ch, sp),
             lambda: lib.pi3_grid_route_sweep(w, 5, 4, 3, ds, None, sp),
             lambda: lib.pi3_grid_route_sweep(w, 5, 4, -3, ds, ch, sp),
             lambda: lib.pi3_grid_route_sweep(w, *big, ds, ch, sp),
             lambda: lib.pi3_grid_route_trace(None, ds, 5, 4, 3, 0, pa, 8, le, sp),
             lambda: lib.pi3_grid_route_trace(w, None, 5, 4, 3, 0, pa, 8, le, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, 0, None, 8, le, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, 0, pa, 8, None, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, 60, pa, 8, le, sp),                   # goal outside the grid
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, -1, pa, 8, le, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, 0, pa, 0, le, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, 5, 4, 3, 0, pa, -8, le, sp),
             lambda: lib.pi3_grid_route_trace(w, ds, *big, 0, pa, 8, le, sp)]
    for i, call in enumerate(calls):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert b"pi3_grid_route_" in err and b"2^27" in err, (i, err)
    torch.cuda.synchronize()
    assert bool((walk == POISON8).all()) and bool((dist == POISON32).all()) and counters.tolist() == [POISON64] * 4
    assert changed.tolist() == [POISON32] and path.tolist() == [POISON64] * 8 and length.tolist() == [POISON64]


# ------------------------------------------------------------------------------------------------ 5. end to end
OCC_CELL, ROUTE_RADIUS = 0.1, 0.1


@pytest.fixture(scope="module")
def reconstructed(tmp_path_factory):
    import synth_sequence as ss
    import test_dense_follow_gpu as follow_gpu
    tmp = tmp_path_factory.mktemp("route")
    seq = ss.SyntheticSequence(follow_gpu.GT, noise=dict(ss.NOISE_NONE), **dict(follow_gpu.SCENE, n_frames=50))
    assert len(seq.chunks) == 2
    follow_gpu._create(seq, str(tmp / "chunks"))
    follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "rec"), bundle_adjust=False, occupancy_cell=OCC_CELL)
    return tmp


def test_cli_route_on_a_reconstruction(reconstructed, capsys):
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    pos = read_tum_positions(tum)
    shape = grid.state.shape
    nz, ny, nx = shape
    src = GridRouter.linear(GridRouter.world_cells(pos, grid), shape)
    d2 = oref.edt_ref(grid.state, 1, True)
    w = ref.walk_mask(grid.state, d2, 1)
    # every pose a source, the goal at the last pose
    capsys.readouterr()
    cli.main(["route", "--occupancy", occ, "--output", str(tmp / "all"), "--from-trajectory", tum, "--goal"]
             + [repr(float(v)) for v in pos[-1]] + ["--radius", str(ROUTE_RADIUS), "--device", DEV])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("route: ")]
    exp = ref.distances(w, src)
    init = ref.init(grid.state, d2, 1, False, src)
    with np.load(tmp / "all" / "route.npz") as z:
        assert z["cost"].tobytes() == exp.tobytes() and z["cost"].shape == shape
        counts = json.loads(str(z["counts"]))
        assert z["distance"].tobytes() == np.where(exp != ref.FAR, OCC_CELL * exp.astype(np.float64) / 12.0,
                                                   np.inf).astype(np.float32).tobytes()
        assert z["index_origin"].tolist() == grid.index_origin.tolist() and float(z["cell"]) == OCC_CELL
    assert [counts[k] for k in ("traversable", "sources_accepted", "sources_blocked", "sources_outside")] == init["counters"]
    assert counts["reachable"] == int((exp != ref.FAR).sum()) > 1000 and counts["sources_accepted"] >= 1
    assert len(line) == 1 and f"{counts['reachable']} reachable" in line[0] and f"{counts['sweeps']} sweeps" in line[0]
    print(line[0])

    def waypoints(cells):
        c = np.asarray(cells, np.int64)
        xyz = np.stack([c % nx, (c // nx) % ny, c // (nx * ny)], 1) + grid.index_origin[None, :]
        return (OCC_CELL * (xyz.astype(np.float64) + 0.5)).tolist()
    rec = json.load(open(tmp / "all" / "route.json"))
    assert rec["waypoints"] == waypoints(ref.trace(w, exp, int(src[-1]))[::-1]) and rec["cost"] == 0
    assert os.path.exists(tmp / "all" / "route.ply")
    # from the first pose to the last: a route with steps
    cli.main(["route", "--occupancy", occ, "--output", str(tmp / "one"), "--start"] + [repr(float(v)) for v in pos[0]]
             + ["--goal"] + [repr(float(v)) for v in pos[-1]] + ["--radius", str(ROUTE_RADIUS), "--device", DEV])
    one = ref.distances(w, src[:1])
    way = ref.trace(w, one, int(src[-1]))
    with np.load(tmp / "one" / "route.npz") as z:
        assert z["cost"].tobytes() == one.tobytes()
    assert len(way) > 1 or src[0] == src[-1]
    rec = json.load(open(tmp / "one" / "route.json"))
    assert rec["waypoints"] == waypoints(way[::-1]) and rec["cost"] == int(one.reshape(-1)[src[-1]])
    assert rec["min_clearance_m"] == "inf" or rec["min_clearance_m"] >= ROUTE_RADIUS
    # without a goal: the field alone
    cli.main(["route", "--occupancy", occ, "--output", str(tmp / "field"), "--from-trajectory", tum, "--device", DEV])
    assert sorted(os.listdir(tmp / "field")) == ["route.npz"]
    with np.load(tmp / "field" / "route.npz") as z:
        assert z["cost"].tobytes() == ref.distances(ref.walk_mask(grid.state), src).tobytes()
