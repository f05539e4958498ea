"""The tour of the views on the GPU (csrc/grid_route.hip: pi3_grid_route_fields_init, pi3_grid_route_sweep_many,
pi3_grid_route_trace_many; view_tour.plan_tour), byte for byte against the oracle (tests/grid_tour_ref.py): the fields of
several sources at once under every grouping, sweeps of a part of the fields, the number of sweeps a field may need, legs
traced together into neighbouring slots, the argument checks, the box room through ViewSet.tour and `cli views --tour` on
a two-chunk sequence.  Every output is filled with a poison value before each call."""
import functools
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
import grid_tour_ref as tref                # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_gpu as view_gpu       # noqa: E402
from test_grid_view_gpu import reconstructed  # noqa: E402,F401  (the two-chunk sequence's reconstruction, a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON32, POISON64 = -5, 11
HD = vref.headings26()
F90 = vref.cos2(90)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _init(walk_np, sources):
    """-> (walk, dist (K,nz,ny,nx) after the init, the counters)."""
    from pi3_slam_amd import ops
    walk = _dev(walk_np)
    dist = torch.full((len(sources),) + walk_np.shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((3,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_fields_init(walk, _dev(np.asarray(sources, np.int64)), dist, counters)
    return walk, dist, counters.tolist()


def _settle(walk, dist, group, per_read=4):
    """-> the sweeps per field, the quiet one included (the product's own loop)."""
    from pi3_slam_amd import ops
    K = int(dist.shape[0])
    return ops.sweep_many_until_quiet(lambda active, flags: ops.grid_route_sweep_many(walk, dist, active, group, flags),
                                      torch.device(DEV), K, int(walk.sum().item()) + 1, "no {sweeps}", per_read)


@functools.lru_cache(maxsize=None)
def _maze(dims, blocked):
    nx, ny, nz = dims
    state = rref.maze((nz, ny, nx), blocked, nx + 2 * ny + 3 * nz + int(100 * blocked))
    return rref.walk_mask(state)


@functools.lru_cache(maxsize=None)
def _field(dims, blocked, source):
    return rref.distances(_maze(dims, blocked), [source])


# ------------------------------------------------------------------------------------------------ 1. the fields
@pytest.mark.parametrize("blocked", [0.3, 0.45])
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 300), (9, 8, 7), (17, 9, 20), (65, 67, 66)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_fields_match_the_oracle_byte_for_byte(dims, blocked):
    walk_np = _maze(dims, blocked)
    cells = walk_np.size
    on, off = np.flatnonzero(walk_np.reshape(-1)), np.flatnonzero(walk_np.reshape(-1) == 0)
    first, last, mid = (int(on[0]), int(on[-1]), int(on[len(on) // 2])) if len(on) else (0, 0, 0)
    shut = int(off[0]) if len(off) else -7
    seven = [first, last, first, shut, -1, cells, mid]           # a duplicate, a blocked cell, two outside indices
    far = np.full(walk_np.shape, rref.FAR, np.uint32)
    for K in (1, 3, 7):
        src = seven[:K]
        ok = [0 <= s < cells and bool(walk_np.reshape(-1)[s]) for s in src]
        exp = np.stack([_field(dims, blocked, s) if good else far for s, good in zip(src, ok)])
        counters = [sum(ok), sum(0 <= s < cells and not good for s, good in zip(src, ok)),
                    sum(not 0 <= s < cells for s in src)]
        for group in sorted({1, 2, 4, K}):
            walk, dist, got = _init(walk_np, src)
            assert got == counters, (K, got, counters)
            start = _u32(dist)
            assert [(f == rref.FAR).sum() for f in start] == [cells - good for good in ok]
            assert all(f.reshape(-1)[s] == 0 for f, s, good in zip(start, src, ok) if good)
            sweeps = _settle(walk, dist, group)
            assert _u32(dist).tobytes() == exp.tobytes(), (K, group, [int((a != b).sum()) for a, b in zip(_u32(dist), exp)])
            assert all(n >= 1 for n in sweeps) and all(n == 1 for n, good in zip(sweeps, ok) if not good)
            assert _settle(walk, dist, group) == [1] * K and _u32(dist).tobytes() == exp.tobytes()
        if K == 7 and len(on):
            assert counters[1:] == [1 if len(off) else 0, 2 if len(off) else 3]
            assert exp[0].tobytes() == exp[2].tobytes() and (exp[3] == rref.FAR).all() and (exp[5] == rref.FAR).all()
    print(f"{dims} {blocked}: {int((exp[0] != rref.FAR).sum())} of {cells} cells reached from the first source, {sweeps} sweeps")


# ------------------------------------------------------------------------------------------------ 2. the sweep
def test_fields_that_are_not_listed_are_not_touched():
    from pi3_slam_amd import ops
    dims, blocked = (17, 9, 20), 0.3
    walk_np = _maze(dims, blocked)
    first = int(np.flatnonzero(walk_np.reshape(-1))[0])
    on = np.flatnonzero(_field(dims, blocked, first).reshape(-1) != rref.FAR)     # one component: every source has a way to go
    assert len(on) > 1000
    src = [int(on[i]) for i in (0, len(on) // 5, len(on) // 3, len(on) // 2, -2, -1)]
    walk, dist, _ = _init(walk_np, src)
    before = _u32(dist).copy()
    listed = [4, 1, 2]
    changed = torch.full((6,), POISON32, dtype=torch.int32, device=DEV)
    for group in (1, 2, 3):
        ops.grid_route_sweep_many(walk, dist, _dev(np.asarray(listed, np.int32)), group, changed)
    after, flags = _u32(dist), changed.tolist()
    for f in range(6):
        if f in listed:
            assert flags[f] == 1 and (after[f] <= before[f]).all() and (after[f] < before[f]).any()
        else:
            assert flags[f] == POISON32 and after[f].tobytes() == before[f].tobytes()
    # a list of none, and entries that are no field, sweep nothing
    now = _u32(dist).copy()
    ops.grid_route_sweep_many(walk, dist, torch.zeros(0, dtype=torch.int32, device=DEV), 2, changed)
    ops.grid_route_sweep_many(walk, dist, _dev(np.asarray([-1, 6, 1 << 20], np.int32)), 2, changed)
    assert _u32(dist).tobytes() == now.tobytes() and changed.tolist() == flags
    # settled fields: a sweep leaves their flags 0 and their bytes alone
    _settle(walk, dist, 4)
    exp = np.stack([_field(dims, blocked, s) for s in src])
    assert _u32(dist).tobytes() == exp.tobytes()
    changed.zero_()
    ops.grid_route_sweep_many(walk, dist, _dev(np.arange(6, dtype=np.int32)), 4, changed)
    assert changed.tolist() == [0] * 6 and _u32(dist).tobytes() == exp.tobytes()


@pytest.mark.parametrize("group", [1, 2, 4])
def test_fields_settle_within_the_emulations_sweeps(group):
    state, src, corner = rref.serpentine()
    walk_np = rref.walk_mask(state)
    sources = [src, corner, 16 * 33 + 16]
    walk, dist, _ = _init(walk_np, sources)
    sweeps = _settle(walk, dist, group)
    launches = [rref.tile_sweeps(walk_np, [s])[1] for s in sources]
    print(f"serpentine, group {group}: {sweeps} sweeps on the device, {launches} in the emulation")
    assert _u32(dist).tobytes() == tref.fields(walk_np, sources).tobytes()
    assert all(got <= exp for got, exp in zip(sweeps, launches)) and launches[0] == 38
    assert _u32(dist)[0].reshape(-1)[corner] == 3728 == _u32(dist)[1].reshape(-1)[src]
    line = np.ones((1, 1, 300), np.uint8)
    walk, dist, _ = _init(line, [0, 299, 150])
    sweeps = _settle(walk, dist, group)
    launches = [rref.tile_sweeps(line, [s])[1] for s in (0, 299, 150)]
    print(f"line, group {group}: {sweeps} sweeps on the device, {launches} in the emulation")
    assert launches[0] == 39 and all(got <= exp for got, exp in zip(sweeps, launches))
    assert _u32(dist)[0].reshape(-1).tolist() == (12 * np.arange(300)).tolist()
    assert _u32(dist)[2].reshape(-1).tolist() == (12 * np.abs(np.arange(300) - 150)).tolist()


# ------------------------------------------------------------------------------------------------ 3. the trace
SENTINEL = -(1 << 40)


def test_legs_traced_together_match_the_oracle():
    from pi3_slam_amd import ops
    dims, blocked = (17, 9, 20), 0.3
    walk_np = _maze(dims, blocked)
    flat_walk = walk_np.reshape(-1)
    on = np.flatnonzero(flat_walk)
    src = [int(on[0]), int(on[len(on) // 2]), int(on[-1])]
    exp = np.stack([_field(dims, blocked, s) for s in src])
    walk, dist, _ = _init(walk_np, src)
    _settle(walk, dist, 2)
    flat = exp.reshape(3, -1)
    reach = [np.flatnonzero(f != rref.FAR) for f in flat]
    far_goal = [int(r[np.argmax(f[r])]) for f, r in zip(flat, reach)]
    cut = np.flatnonzero((flat[0] == rref.FAR) & (flat_walk == 1))
    shut = int(np.flatnonzero(flat_walk == 0)[0])
    # (field, goal, slot): mixed lengths, a goal that is its field's source, one no source reaches, one that is not
    # traversable, a slot one short, a field and a goal that are none
    legs = [(0, far_goal[0], None), (1, src[1], None), (2, far_goal[2], None), (0, int(reach[0][len(reach[0]) // 2]), None),
            (1, far_goal[1], "short"), (0, shut, 3), (2, int(reach[2][1]), None), (7, src[0], 2), (0, -1, 2),
            (0, walk_np.size, 2), (1, int(reach[1][-1]), None)]
    if len(cut):
        legs.insert(3, (0, int(cut[0]), 3))
    paths = [rref.trace(walk_np, exp[f], g) if 0 <= f < 3 and 0 <= g < walk_np.size else [] for f, g, _ in legs]
    slots = [len(p) - 1 if s == "short" else (int(flat[f][g]) // 12 + 1 if s is None else s)
             for p, (f, g, s) in zip(paths, legs)]
    offsets = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
    path = torch.full((int(offsets[-1]) + 4,), SENTINEL, dtype=torch.int64, device=DEV)
    length = torch.full((len(legs),), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_trace_many(walk, dist, _dev(np.asarray([f for f, _, _ in legs], np.int32)),
                              _dev(np.asarray([g for _, g, _ in legs], np.int64)), _dev(offsets), path, length)
    got, lengths = path.cpu().numpy(), length.tolist()
    for l, ((f, g, s), p) in enumerate(zip(legs, paths)):
        slot = got[offsets[l]:offsets[l + 1]]
        if s == "short":
            assert len(p) > 1 and lengths[l] == -len(p) and (slot == SENTINEL).all(), (l, lengths[l])
        else:
            assert lengths[l] == len(p), (l, lengths[l], len(p))
            assert slot[:len(p)].tolist() == p and (slot[len(p):] == SENTINEL).all(), l
    assert (got[offsets[-1]:] == SENTINEL).all()
    assert lengths[1] == 1 and lengths[0] > 5 and paths[0][-1] == src[0] and paths[2][-1] == src[2]
    assert [lengths[l] for l, (f, g, s) in enumerate(legs) if s in (2, 3)] == [0] * (5 if len(cut) else 4)
    # the single trace walks the same way: one function
    one = torch.full((slots[0],), SENTINEL, dtype=torch.int64, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.grid_route_trace(walk, dist[0], legs[0][1], one, n)
    assert int(n.item()) == lengths[0] and one.cpu().numpy()[:lengths[0]].tolist() == paths[0]
    # no leg: nothing is launched
    ops.grid_route_trace_many(walk, dist, torch.zeros(0, dtype=torch.int32, device=DEV),
                              torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                              path, torch.zeros(0, dtype=torch.int64, device=DEV))
    assert path.cpu().numpy().tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ 4. the arguments
def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    shape = (3, 4, 5)
    walk = torch.ones(shape, dtype=torch.uint8, device=DEV)
    dist = torch.full((2,) + shape, POISON32, dtype=torch.int32, device=DEV)
    sources = torch.zeros(2, dtype=torch.int64, device=DEV)
    counters = torch.full((3,), POISON64, dtype=torch.int64, device=DEV)
    active = torch.zeros(2, dtype=torch.int32, device=DEV)
    changed = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
    field_of = torch.zeros(2, dtype=torch.int32, device=DEV)
    goal = torch.zeros(2, dtype=torch.int64, device=DEV)
    offset = torch.tensor([0, 4, 8], dtype=torch.int64, device=DEV)
    path = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    length = torch.full((2,), POISON64, dtype=torch.int64, device=DEV)
    sp = L.stream_ptr()
    w, d, so, c, ac, ch, fo, go, of, pa, le = (t.data_ptr() for t in (walk, dist, sources, counters, active, changed,
                                                                     field_of, goal, offset, path, length))
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    I, S, T = lib.pi3_grid_route_fields_init, lib.pi3_grid_route_sweep_many, lib.pi3_grid_route_trace_many
    calls = [lambda: I(None, 5, 4, 3, so, 2, d, c, sp),
             lambda: I(w, 5, 4, 3, None, 2, d, c, sp),
             lambda: I(w, 5, 4, 3, so, 2, None, c, sp),
             lambda: I(w, 5, 4, 3, so, 2, d, None, sp),
             lambda: I(w, 5, 4, 3, so, 0, d, c, sp),
             lambda: I(w, 5, 4, 3, so, -2, d, c, sp),
             lambda: I(w, 5, 4, 3, so, 65536, d, c, sp),
             lambda: I(w, 5, 0, 3, so, 2, d, c, sp),
             lambda: I(w, *big, so, 2, d, c, sp),
             lambda: S(None, 5, 4, 3, d, 2, ac, 2, 1, ch, sp),
             lambda: S(w, 5, 4, 3, None, 2, ac, 2, 1, ch, sp),
             lambda: S(w, 5, 4, 3, d, 2, None, 2, 1, ch, sp),
             lambda: S(w, 5, 4, 3, d, 2, ac, 2, 1, None, sp),
             lambda: S(w, 5, 4, 3, d, 0, ac, 0, 1, ch, sp),
             lambda: S(w, 5, 4, 3, d, 2, ac, -1, 1, ch, sp),
             lambda: S(w, 5, 4, 3, d, 2, ac, 3, 1, ch, sp),                                        # more listed than fields
             lambda: S(w, 5, 4, 3, d, 2, ac, 2, 0, ch, sp),
             lambda: S(w, 5, 4, 3, d, 2, ac, 2, -4, ch, sp),
             lambda: S(w, 5, 4, -3, d, 2, ac, 2, 1, ch, sp),
             lambda: S(w, *big, d, 2, ac, 2, 1, ch, sp),
             lambda: T(None, d, 5, 4, 3, 2, fo, go, of, pa, le, 2, sp),
             lambda: T(w, None, 5, 4, 3, 2, fo, go, of, pa, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, None, go, of, pa, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, fo, None, of, pa, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, fo, go, None, pa, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, fo, go, of, None, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, fo, go, of, pa, None, 2, sp),
             lambda: T(w, d, 5, 4, 3, 0, fo, go, of, pa, le, 2, sp),
             lambda: T(w, d, 5, 4, 3, 2, fo, go, of, pa, le, -1, sp),
             lambda: T(w, d, 5, -4, 3, 2, fo, go, of, pa, le, 2, sp),
             lambda: T(w, d, *big, 2, fo, go, of, pa, le, 2, sp)]
    names = [b"fields_init"] * 9 + [b"sweep_many"] * 11 + [b"trace_many"] * 11
    assert len(calls) == len(names)
    for i, (call, name) in enumerate(zip(calls, names)):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert err.startswith(b"pi3_grid_route_" + name + b":") and b"2^27" in err, (i, err)
    torch.cuda.synchronize()
    assert counters.tolist() == [POISON64] * 3 and bool((dist == POISON32).all()) and changed.tolist() == [POISON32] * 2
    assert bool((path == POISON64).all()) and length.tolist() == [POISON64] * 2
    # the bindings refuse what the entry points cannot see
    from pi3_slam_amd import ops
    with pytest.raises(AssertionError):
        ops.grid_route_fields_init(walk, sources[:1], dist, counters)
    with pytest.raises(AssertionError):
        ops.grid_route_sweep_many(walk, dist, active, 1, changed[:1])
    with pytest.raises(AssertionError):
        ops.grid_route_sweep_many(walk, dist.view(torch.float32), active, 1, changed)
    with pytest.raises(AssertionError):
        ops.grid_route_trace_many(walk, dist, field_of, goal, offset[:2], path, length)


# ------------------------------------------------------------------------------------------------ 5. the box room
BOX_RANGE_CELLS = 8


@pytest.fixture(scope="module")
def box_room():
    from pi3_slam_amd.dense_map import OccupancyGrid
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    walk = rref.walk_mask(state, d2a, min_d2)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    return grid, centres, walk, oref.clearance(d2a, cell)


def _check_tour(tour, vset, walk, clearance, radius):
    """The conditions of a tour that do not need the oracle."""
    shape = walk.shape
    ok = rref.allowed_moves(walk)
    nz, ny, nx = shape
    cells, D = tour.cells, tour.matrix
    assert (D == D.T).all() and not np.diagonal(D).any() and cells[0] == tour.start_cell
    assert sorted(tour.order + tour.unreachable) == list(range(len(cells) - 1))
    assert sorted(r for s in tour.stops for r in s.ranks) == list(range(len(vset.views))) or tour.unreachable
    at, running, covered = 0, 0, 0
    for stop, leg, way in zip(tour.stops, tour.leg_cells, tour.leg_waypoints):
        node = stop.number + 1
        assert leg[0] == cells[at] and leg[-1] == cells[node] == stop.cell and walk.reshape(-1)[leg].all()
        total = 0
        for a, b in zip(leg, leg[1:]):
            w = rref.step_cost(int(a), int(b), shape)
            assert w, (a, b)
            d = (int(b % nx - a % nx), int((b // nx) % ny - (a // nx) % ny), int(b // (nx * ny) - a // (nx * ny)))
            assert ok[rref.MOVES.index((d[0], d[1], d[2], w))].reshape(-1)[a], (a, b)
            total += w
        assert total == D[at, node] == stop.leg_cost
        running += total
        assert stop.cumulative_cost == running and len(way) == len(leg) and way[-1].tolist() == stop.position.tolist()
        assert all(vset.views[r].cell == stop.cell for r in stop.ranks) and stop.ranks == sorted(stop.ranks)
        assert stop.position.tolist() == vset.views[stop.ranks[0]].position.tolist()
        assert clearance.reshape(-1)[leg].min() >= radius and stop.min_clearance_m >= radius
        for n, c in zip(stop.tour_new, stop.tour_covered):
            covered += n
            assert c == covered
        at = node
    assert running == tour.cost and covered == tour.covered
    assert abs(tour.length_m - sum(s.length_m for s in tour.stops)) < 1e-9 and tour.length_m <= tour.distance_m + 1e-9


def test_box_room_through_the_tour(box_room):
    from pi3_slam_amd.view_planner import ViewPlanner
    grid, centres, walk, clearance = box_room
    cell = float(grid.cell)
    args = (route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4)
    ten = ViewPlanner(*args, 10).cover(grid, centres, DEV)
    tour = ten.tour()
    print(f"box room, the cover's ten: {tour.counts}, cost {tour.cost}, {tour.distance_m:.2f} m")
    assert tour.start_cell == 34781 and tour.order == [8, 0, 6, 4, 2, 3, 5, 7, 1, 9] and tour.method == "exact"
    assert (tour.rank_order_cost, tour.nn_cost, tour.cost, tour.moves) == (2232, 1422, 1422, 0)
    assert abs(tour.distance_m - 11.85) < 1e-9 and abs(tour.rank_order_length_m - 18.6) < 1e-9
    assert tour.covered == 3016 == ten.counts["covered"] and tour.unreachable == []
    _check_tour(tour, ten, walk, clearance, route_cases.BOX_RADIUS)
    exp = tref.tour(walk, [v.cell for v in ten.views], 34781)
    assert tour.matrix.tolist() == exp["matrix"].tolist() and tour.cells.tolist() == exp["cells"]
    assert [leg.tolist() for leg in tour.leg_cells] == exp["legs"]
    c = tour.counts
    assert c["fields"] == 11 and c["stops"] == 10 and c["views"] == 10 and c["unreachable"] == 0
    assert 1 <= c["sweeps_min"] <= c["sweeps_max"] and c["launches"] >= c["sweeps_max"] and c["traced_cells"] == sum(len(leg) for leg in exp["legs"])
    assert tour.settings["start_cell"] == 34781 and tour.settings["view_mode"] == "cover" and tour.settings["open_path"]
    # in tour order the views add other amounts than in rank order, and the same total
    seen = np.zeros(cref.seen_words(walk.size), np.uint32)
    news = [cref.mark(grid.state, seen, [ten.views[s].cell], [ten.views[s].heading], 8, HD, *F90)["counters"][4]
            for s in tour.order]
    assert [n for s in tour.stops for n in s.tour_new] == news
    # from camera 0, given as a point
    other = ten.tour(centres[0])
    assert other.start_cell == 35032 and (other.rank_order_cost, other.cost) == (2264, 1433)
    _check_tour(other, ten, walk, clearance, route_cases.BOX_RADIUS)
    # find's ten
    plain = ViewPlanner(*args, 10).find(grid, centres, DEV)
    tour = plain.tour()
    assert tour.order == [8, 0, 2, 9, 3, 7, 6, 4, 5, 1] and tour.method == "exact" and tour.covered == 2024
    assert (tour.rank_order_cost, tour.nn_cost, tour.cost) == (1922, 1256, 1221) and tour.settings["view_mode"] == "gain"
    _check_tour(tour, plain, walk, clearance, route_cases.BOX_RADIUS)
    # the memory limit names the views and the bytes
    with pytest.raises(ValueError, match=r"the tour of 10 views needs 11 distance fields of 70000 cells, 3080000 bytes: "
                                         r"more than the limit of 3000000 bytes"):
        plain.tour(max_field_bytes=3000000)
    with pytest.raises(ValueError, match="the start is not traversable: cell"):
        plain.tour(grid.origin + 0.5 * cell)


def test_box_room_the_first_forty_pan_and_take_two_opt(box_room):
    from pi3_slam_amd.view_planner import ViewPlanner
    grid, centres, walk, clearance = box_room
    cell = float(grid.cell)
    forty = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4, 40).cover(grid, centres, DEV)
    tour = forty.tour(group=2)
    assert len(tour.stops) == 38 and tour.counts["views"] == 40 and tour.method == "2-opt"
    assert (tour.rank_order_cost, tour.nn_cost, tour.cost, tour.moves) == (8994, 3526, 3208, 6)
    assert sorted(len(s.ranks) for s in tour.stops)[-2:] == [2, 2] and tour.covered == forty.counts["covered"]
    _check_tour(tour, forty, walk, clearance, route_cases.BOX_RADIUS)
    exact = forty.tour(exact_max=0)
    assert exact.order == tour.order and forty.tour(group=39).matrix.tolist() == tour.matrix.tolist()


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_cli_views_tour_on_a_reconstruction(reconstructed, capsys):   # noqa: F811
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    walk = rref.walk_mask(grid.state, oref.edt_ref(grid.state, 1, False), 1)
    poses = read_tum_positions(tum)
    src = GridRouter.linear(GridRouter.world_cells(poses, grid), grid.state.shape)
    good = [i for i, s in enumerate(src) if s >= 0 and walk.reshape(-1)[s]]
    assert good
    start, extra = int(src[good[-1]]), []
    if good[-1] != len(src) - 1:                                # the last pose stands on no traversable cell: say where
        point = [float(f"{v:.6f}") for v in poses[good[-1]]]
        start = int(GridRouter.linear(GridRouter.world_cells(point, grid), grid.state.shape)[0])
        assert start >= 0 and walk.reshape(-1)[start]
        extra = ["--tour-from"] + [f"{v:.6f}" for v in point]
    base = ["views", "--occupancy", occ, "--from-trajectory", tum, "--radius", str(view_gpu.ROUTE_RADIUS), "--range",
            "0.8", "--stride", "2", "--count", "5", "--device", DEV, "--cover"]
    cli.main(base + ["--output", str(tmp / "tour_off")])
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp / "tour_on"), "--tour", "--route-to", "0"] + extra)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("views: ")]
    assert sorted(os.listdir(tmp / "tour_off")) == ["views.json", "views.npz", "views.ply"]
    assert sorted(os.listdir(tmp / "tour_on")) == ["route.json", "route.npz", "route.ply", "tour.json", "tour.npz", "tour.ply",
                                                   "views.json", "views.npz", "views.ply"]
    for name in ("views.json", "views.ply"):                   # the views do not know about the tour
        assert open(tmp / "tour_on" / name, "rb").read() == open(tmp / "tour_off" / name, "rb").read()
    views = json.load(open(tmp / "tour_on" / "views.json"))["views"]
    rec = json.load(open(tmp / "tour_on" / "tour.json"))
    exp = tref.tour(walk, [v["cell"] for v in views], start)
    assert rec["start"]["cell"] == start and rec["order"] == [s - 1 for s in exp["seq"]] and rec["method"] == exp["method"]
    assert (rec["cost"], rec["rank_order_cost"], rec["nn_cost"]) == (exp["cost"], exp["rank_order_cost"], exp["nn_cost"])
    assert rec["unreachable"] == [s - 1 for s in exp["unreachable"]] and rec["counts"]["fields"] == len(exp["cells"])
    assert [s["cell"] for s in rec["stops"]] == [exp["cells"][s] for s in exp["seq"]]
    assert [[v["rank"] for v in s["views"]] for s in rec["stops"]] == [exp["ranks"][s - 1] for s in exp["seq"]]
    assert [s["position"] for s in rec["stops"]] == [views[s["views"][0]["rank"]]["position"] for s in rec["stops"]]
    if not exp["unreachable"]:
        assert rec["covered"] == views[-1]["covered"]
    with np.load(tmp / "tour_on" / "tour.npz") as z:
        assert z["matrix"].tolist() == exp["matrix"].tolist() and z["cells"].tolist() == exp["cells"]
        legs = [z["waypoint_cells"][a:b].tolist() for a, b in zip(z["offsets"][:-1], z["offsets"][1:])]
    assert legs == exp["legs"]
    assert len(line) == 1 and (f"; tour: {len(rec['stops'])} stops, {rec['distance_m']:.2f} m "
                               f"({rec['rank_order_length_m']:.2f} m in rank order), {rec['method']}") in line[0]
    print(line[0])
    with pytest.raises(SystemExit, match="views: --tour-from needs --tour"):
        cli.main(base + ["--output", str(tmp / "w"), "--tour-from", "0", "0", "0"])
    with pytest.raises(SystemExit, match="views: the start .* lies outside the grid"):
        cli.main(base + ["--output", str(tmp / "w"), "--tour", "--tour-from", "1000", "0", "0"])
