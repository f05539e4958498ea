"""Frontiers of the occupancy grid on the GPU (csrc/grid_frontier.hip), byte for byte against the oracle
(tests/grid_frontier_ref.py): the mark, sweep, roots and stats kernels, the number of sweeps a tile-relaxing kernel may
need, the box room through FrontierFinder, and reconstruct -> occupancy.npz -> `cli frontiers` on a two-chunk sequence.
Every output is filled with a poison value before each call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_frontier_ref as fref            # noqa: E402
import grid_route_ref as rref               # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON32, POISON64 = -5, 11


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _mark_device(state):
    from pi3_slam_amd import ops
    st = _dev(state)
    label = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_frontier_mark(st, label, counters)
    return st, label, counters.tolist()


def _settle(label, frontier_cells):
    """-> the sweeps the device ran, the quiet one included (FrontierFinder's own loop)."""
    from pi3_slam_amd.frontier import FrontierFinder
    return FrontierFinder().settle(label, frontier_cells)


def _roots_device(label, cap):
    from pi3_slam_amd import ops
    roots = torch.full((cap,), POISON64, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_frontier_roots(label, roots, count)
    return roots.cpu().numpy(), int(count.item())


def _stats_device(st, label, dist, roots_sorted):
    from pi3_slam_amd import ops
    K = len(roots_sorted)
    stats = torch.full((K, 12), POISON64, dtype=torch.int64, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    d = None if dist is None else _dev(np.asarray(dist, np.uint32).view(np.int32))
    ops.grid_frontier_stats(st, label, d, _dev(np.asarray(roots_sorted, np.int64)), stats, counters)
    return stats.cpu().numpy(), counters.tolist()


# ------------------------------------------------------------------------------------------------ 1. the four kernels
def _open_field(shape, sources):
    """The route field of an all-free grid: 12 (p - q) + 17 (q - r) + 21 r for the sorted offsets p >= q >= r."""
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
def test_kernels_match_the_oracle_byte_for_byte(dims):
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    states = {"0.5/0.4/0.1": fref.three_state(shape, 0.5, 0.1, nx + ny + nz),
              "0.1/0.8/0.1": fref.three_state(shape, 0.1, 0.1, nx + 2 * ny + 3 * nz),
              "0.2/0.1/0.7": fref.three_state(shape, 0.2, 0.7, 2 * nx + ny + nz),       # many small clusters
              "free": np.ones(shape, np.uint8), "unknown": np.zeros(shape, np.uint8)}
    for name, state in states.items():
        m = fref.mark(state)
        st, label, counters = _mark_device(state)
        assert _u32(label).tobytes() == m["label"].tobytes(), (name, "mark")
        assert counters == m["counters"], (name, counters, m["counters"])
        n = m["counters"][0]
        exp = fref.labels(state)
        sweeps = _settle(label, n)
        got = _u32(label)
        assert got.tobytes() == exp.tobytes(), (name, "fixed point", int((got != exp).sum()))
        assert _settle(label, n) == 1 and _u32(label).tobytes() == exp.tobytes()       # settled: one quiet sweep
        r = fref.roots(exp)
        K = len(r)
        assert (name != "unknown" or K == 0) and (name != "free" or K == 1) and (state.size < 100 or name == "unknown" or K)
        roots, count = _roots_device(label, K + 3)
        assert count == K and sorted(roots[:K].tolist()) == r.tolist() and (roots[K:] == POISON64).all()
        # stats: a settled route field from the first free cells, no field, a field that reaches no frontier cell
        walk = rref.walk_mask(state)
        on = np.flatnonzero(walk.reshape(-1))
        if name == "free":
            settled = _open_field(shape, on[:2])                 # the closed form (test_grid_route.py: it is Dijkstra's)
        else:
            settled = rref.distances(walk, on[:2]) if len(on) else np.full(shape, rref.FAR, np.uint32)
        nowhere = np.where(m["faces"] > 0, rref.FAR, 0).astype(np.uint32)
        for what, dist in (("settled", settled), ("none", None), ("nowhere", nowhere)):
            e = fref.stats(state, exp, dist, r)
            stats, counters = _stats_device(st, label, dist, r)
            assert stats.tobytes() == e["stats"].tobytes(), (name, what)
            assert counters == e["counters"] and counters[0] == n and counters[1] == 0, (name, what, counters)
            if what != "settled":
                assert counters[2] == 0 and (K == 0 or (stats[:, 11] == -1).all())
        reach = int(((settled != rref.FAR) & (m["faces"] > 0)).sum())
        assert name == "unknown" or state.size < 100 or reach >= 1       # the settled field does reach frontier cells
        print(f"{dims} {name}: {n} frontier cells, {K} clusters, {sweeps} sweeps, {reach} cells reachable")


def test_stats_counts_cells_whose_root_is_missing():
    state = fref.three_state((7, 8, 9), 0.2, 0.7, 5)
    exp = fref.labels(state)
    r = fref.roots(exp)
    assert len(r) >= 3
    st, label, _ = _mark_device(state)
    _settle(label, int((exp != fref.NONE).sum()))
    part = np.delete(r, 1)                                       # a wrong caller: one root withheld
    e = fref.stats(state, exp, None, part)
    stats, counters = _stats_device(st, label, None, part)
    assert stats.tobytes() == e["stats"].tobytes() and counters == e["counters"]
    assert counters[1] == int((exp == r[1]).sum()) > 0


# ------------------------------------------------------------------------------------------------ 2. per-tile propagation
def test_a_launch_relaxes_whole_tiles():
    """A sweep that moved a label by one cell per launch would need 300 launches for the line."""
    line = np.ones((1, 1, 300), np.uint8)
    exp, launches, changing = fref.tile_sweeps(fref.mark(line)["label"])
    assert changing == 38
    st, label, counters = _mark_device(line)
    assert counters[:2] == [300, 300 * 4 + 2]
    sweeps = _settle(label, 300)
    print(f"line: {sweeps} sweeps on the device, {launches} in the emulation")
    assert _u32(label).tobytes() == exp.tobytes() and (exp == 0).all()
    assert sweeps - 1 <= 38 and sweeps <= launches
    state = fref.serpentine()
    exp, launches, changing = fref.tile_sweeps(fref.mark(state)["label"])
    st, label, counters = _mark_device(state)
    sweeps = _settle(label, counters[0])
    print(f"serpentine: {sweeps} sweeps on the device, {launches} in the emulation")
    assert _u32(label).tobytes() == exp.tobytes() and exp.tobytes() == fref.labels(state).tobytes()
    assert sweeps <= launches < 60


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("shape", [(5, 17, 19), (17, 9, 20), (3, 24, 24)], ids=lambda s: "%dx%dx%d" % s)
def test_random_grids_settle_within_the_emulations_sweeps(shape, seed):
    state = fref.three_state(shape, 0.15, 0.3, seed)
    exp, launches, _ = fref.tile_sweeps(fref.mark(state)["label"])
    st, label, counters = _mark_device(state)
    sweeps = _settle(label, counters[0])
    assert _u32(label).tobytes() == exp.tobytes() and sweeps <= launches


# ------------------------------------------------------------------------------------------------ 3. roots and arguments
def test_roots_reports_the_full_count_when_cap_is_short():
    state = fref.three_state((9, 20, 33), 0.2, 0.7, 3)           # mostly occupied: many small clusters
    exp = fref.labels(state)
    r = fref.roots(exp)
    K = len(r)
    assert K >= 8
    st, label, counters = _mark_device(state)
    _settle(label, counters[0])
    for cap in (0, 1, K // 2, K - 1):
        roots, count = _roots_device(label, cap)
        assert count == K
        assert len(set(roots.tolist())) == cap and set(roots.tolist()) <= set(r.tolist())
    roots, count = _roots_device(label, K)
    assert count == K and sorted(roots.tolist()) == r.tolist()
    # before the fixed point every frontier cell is its own root
    st, label, counters = _mark_device(state)
    roots, count = _roots_device(label, 4)
    assert count == counters[0] == int((exp != fref.NONE).sum())


def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    shape = (3, 4, 5)
    state = torch.ones(shape, dtype=torch.uint8, device=DEV)
    label = torch.full(shape, POISON32, dtype=torch.int32, device=DEV)
    dist = torch.zeros(shape, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    changed = torch.full((1,), POISON32, dtype=torch.int32, device=DEV)
    roots = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    stats = torch.full((2, 12), POISON64, dtype=torch.int64, device=DEV)
    sp = L.stream_ptr()
    s, la, d, c, ch, ro, co, sa = (t.data_ptr() for t in (state, label, dist, counters, changed, roots, count, stats))
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    assert big[0] * big[1] * big[2] == (1 << 27) + 1
    calls = [lambda: lib.pi3_grid_frontier_mark(None, 5, 4, 3, la, c, sp),
             lambda: lib.pi3_grid_frontier_mark(s, 5, 4, 3, None, c, sp),
             lambda: lib.pi3_grid_frontier_mark(s, 5, 4, 3, la, None, sp),
             lambda: lib.pi3_grid_frontier_mark(s, 0, 4, 3, la, c, sp),
             lambda: lib.pi3_grid_frontier_mark(s, 5, -4, 3, la, c, sp),
             lambda: lib.pi3_grid_frontier_mark(s, 5, 4, 1 << 21, la, c, sp),
             lambda: lib.pi3_grid_frontier_mark(s, *big, la, c, sp),
             lambda: lib.pi3_grid_frontier_sweep(5, 4, 3, None, ch, sp),
             lambda: lib.pi3_grid_frontier_sweep(5, 4, 3, la, None, sp),
             lambda: lib.pi3_grid_frontier_sweep(5, 4, 0, la, ch, sp),
             lambda: lib.pi3_grid_frontier_sweep(-5, 4, 3, la, ch, sp),
             lambda: lib.pi3_grid_frontier_sweep(*big, la, ch, sp),
             lambda: lib.pi3_grid_frontier_roots(None, 5, 4, 3, ro, 8, co, sp),
             lambda: lib.pi3_grid_frontier_roots(la, 5, 4, 3, None, 8, co, sp),
             lambda: lib.pi3_grid_frontier_roots(la, 5, 4, 3, ro, 8, None, sp),
             lambda: lib.pi3_grid_frontier_roots(la, 5, 4, 3, ro, -1, co, sp),
             lambda: lib.pi3_grid_frontier_roots(la, 5, 0, 3, ro, 8, co, sp),
             lambda: lib.pi3_grid_frontier_roots(la, *big, ro, 8, co, sp),
             lambda: lib.pi3_grid_frontier_stats(None, la, d, 5, 4, 3, ro, 2, sa, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, None, d, 5, 4, 3, ro, 2, sa, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, 3, None, 2, sa, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, 3, ro, 2, None, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, 3, ro, 2, sa, None, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, 3, ro, -1, sa, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, 3, ro, 61, sa, c, sp),             # more rows than cells
             lambda: lib.pi3_grid_frontier_stats(s, la, d, 5, 4, -3, ro, 2, sa, c, sp),
             lambda: lib.pi3_grid_frontier_stats(s, la, d, *big, ro, 2, sa, c, sp)]
    for i, call in enumerate(calls):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert b"pi3_grid_frontier_" in err and b"2^27" in err, (i, err)
    names = [b"mark"] * 7 + [b"sweep"] * 5 + [b"roots"] * 6 + [b"stats"] * 9
    for call, name in zip(calls, names):
        assert call() == -1 and lib.pi3_last_error().startswith(b"pi3_grid_frontier_" + name + b":")
    torch.cuda.synchronize()
    assert bool((label == POISON32).all()) and counters.tolist() == [POISON64] * 4 and changed.tolist() == [POISON32]
    assert roots.tolist() == [POISON64] * 8 and count.tolist() == [POISON64] and bool((stats == POISON64).all())


# ------------------------------------------------------------------------------------------------ 4. the box room
def test_box_room_through_the_finder():
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.frontier import FrontierFinder
    from pi3_slam_amd.grid_route import GridRouter
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    shape = state.shape
    nz, ny, nx = shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    walk_a = rref.walk_mask(state, d2a, min_d2)
    dist_a = rref.distances(walk_a, lin)
    exp = fref.frontier_set(state, dist_a)
    found = FrontierFinder(radius=route_cases.BOX_RADIUS).find(grid, centres, DEV)
    c = found.counts
    print(f"box room: {c}")
    assert c["frontier_cells"] == 4292 and c["clusters"] == c["clusters_found"] == 1 and c["clusters_dropped"] == 0
    assert c["reachable_clusters"] == 1 and c["reachable_cells"] == 3748 and c["unknown_faces"] == fref.mark(state)["counters"][1]
    assert c["sweeps"] <= fref.tile_sweeps(fref.mark(state)["label"])[1]
    assert found.rank.dtype == np.int32 and found.rank.tobytes() == exp["rank"].tobytes()
    assert found.field.cost.tobytes() == dist_a.tobytes() and found.field.walk.tobytes() == walk_a.tobytes()
    assert found.settings["router"]["approach_unknown"] is True and found.settings["radius"] == route_cases.BOX_RADIUS
    front = fref.faces(state) > 0
    for got, e, row in zip(found.clusters, exp["clusters"], exp["keep"]):
        assert (got.root, got.cells, got.unknown_faces, got.cost, got.goal_cell) == (e["root"], e["cells"], e["faces"],
                                                                                     e["cost"], e["goal"])
        assert got.reachable is True and front.reshape(-1)[got.goal_cell] and dist_a.reshape(-1)[got.goal_cell] == got.cost
        assert got.cost != rref.FAR and got.distance_m == cell * got.cost / 12.0
        s = exp["stats"][row]
        assert got.centroid.tolist() == (cell * (origin + s[2:5] / float(s[0]) + 0.5)).tolist()
        assert got.bbox_min.tolist() == (cell * (origin + s[5:8] + 0.5)).tolist()
        assert got.bbox_max.tolist() == (cell * (origin + s[8:11] + 0.5)).tolist()
        g = got.goal_cell
        assert got.goal.tolist() == (cell * (origin + np.array([g % nx, (g // nx) % ny, g // (nx * ny)]) + 0.5)).tolist()
    # the way to the nearest cluster
    best = found.clusters[0]
    route = found.route_to(0)
    path = route.cells.tolist()
    assert path[-1] == best.goal_cell and dist_a.reshape(-1)[path[0]] == 0 and route.cost == best.cost
    ok = rref.allowed_moves(walk_a)
    total = 0
    for a, b in zip(path, path[1:]):
        w = rref.step_cost(a, b, shape)
        d = (b % nx - a % nx, (b // nx) % ny - (a // nx) % ny, b // (nx * ny) - a // (nx * ny))
        assert w and ok[rref.MOVES.index((d[0], d[1], d[2], w))].reshape(-1)[a], (a, b)
        total += w
    assert total == best.cost and walk_a.reshape(-1)[path].all()
    assert oref.clearance(d2a, cell).reshape(-1)[path].min() >= route_cases.BOX_RADIUS
    assert route.min_clearance_m >= route_cases.BOX_RADIUS
    assert route.waypoints[-1].tolist() == best.goal.tolist()
    # the reason for the switch: the router as it was reaches none of the goals
    plain = GridRouter(route_cases.BOX_RADIUS).field(grid, centres, DEV)
    for got in found.clusters:
        assert plain.cost.reshape(-1)[got.goal_cell] == rref.FAR and plain.walk.reshape(-1)[got.goal_cell] == 0
    assert not (plain.walk.astype(bool) & front).any() and plain.counts["reachable"] == 10612
    # without sources: the same clusters, ordered by size, nothing about reachability
    bare = FrontierFinder().find(grid, None, DEV)
    assert bare.field is None and [(k.root, k.cells, k.reachable, k.cost, k.goal) for k in bare.clusters] == [
        (exp["clusters"][0]["root"], 4292, None, None, None)]
    assert bare.rank.tobytes() == exp["rank"].tobytes() and bare.counts["reachable_clusters"] == 0
    with pytest.raises(ValueError, match="no route without sources"):
        bare.route_to(0)


def test_finder_ranks_and_drops_like_the_oracle():
    import test_grid_frontier as cpu_cases
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.frontier import FrontierFinder
    state, src, expect, dropped_root = cpu_cases.ranking_plan()
    nz, ny, nx = state.shape
    grid = OccupancyGrid(state, np.array([3, -2, 1], np.int64), 0.25)
    start = 0.25 * (np.array([src % nx + 3, (src // nx) % ny - 2, src // (nx * ny) + 1]) + 0.5)
    found = FrontierFinder(0.0, 3).find(grid, start, DEV)
    exp = fref.frontier_set(state, rref.distances(rref.walk_mask(state), [src]), 3)
    assert [(c.root, c.cells, c.cost) for c in found.clusters] == expect
    assert [c.rank for c in found.clusters] == [0, 1, 2, 3] and [c.reachable for c in found.clusters] == [True] * 3 + [False]
    assert found.rank.tobytes() == exp["rank"].tobytes() and found.rank.reshape(-1)[dropped_root] == -1
    assert found.counts["clusters"] == 4 and found.counts["clusters_dropped"] == 1 and found.counts["cells_dropped"] == 2
    assert found.counts["reachable_clusters"] == 3 and found.counts["clusters_found"] == 5
    with pytest.raises(ValueError, match="cluster 3 .* cannot be reached"):
        found.route_to(3)
    assert found.route_to(1).cells.tolist()[-1] == exp["clusters"][1]["goal"]
    nothing = FrontierFinder().find(OccupancyGrid(np.zeros((4, 5, 6), np.uint8), np.zeros(3, np.int64), 0.1), None, DEV)
    assert nothing.clusters == [] and (nothing.rank == -1).all() and nothing.counts["sweeps"] == 0
    assert nothing.counts["frontier_cells"] == 0 and nothing.counts["clusters"] == 0


# ------------------------------------------------------------------------------------------------ 5. end to end
OCC_CELL, ROUTE_RADIUS = 0.1, 0.1


@pytest.fixture(scope="module")
def reconstructed(tmp_path_factory):
    import synth_sequence as ss
    import test_dense_follow_gpu as follow_gpu
    tmp = tmp_path_factory.mktemp("frontiers")
    seq = ss.SyntheticSequence(follow_gpu.GT, noise=dict(ss.NOISE_NONE), **dict(follow_gpu.SCENE, n_frames=50))
    assert len(seq.chunks) == 2
    follow_gpu._create(seq, str(tmp / "chunks"))
    follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "rec"), bundle_adjust=False, occupancy_cell=OCC_CELL)
    return tmp


def test_cli_frontiers_on_a_reconstruction(reconstructed, capsys):
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    shape = grid.state.shape
    src = GridRouter.linear(GridRouter.world_cells(read_tum_positions(tum), grid), shape)
    d2 = oref.edt_ref(grid.state, 1, False)
    w = rref.walk_mask(grid.state, d2, 1)
    exp = fref.frontier_set(grid.state, rref.distances(w, src))
    capsys.readouterr()
    cli.main(["frontiers", "--occupancy", occ, "--output", str(tmp / "f"), "--from-trajectory", tum, "--radius",
              str(ROUTE_RADIUS), "--device", DEV])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("frontiers: ")]
    rec = json.load(open(tmp / "f" / "frontiers.json"))
    counts = rec["counts"]
    assert [(c["root"], c["cells"], c["unknown_faces"], c["cost"], c["goal_cell"]) for c in rec["clusters"]] == [
        (e["root"], e["cells"], e["faces"], e["cost"], e["goal"]) for e in exp["clusters"]]
    assert [c["rank"] for c in rec["clusters"]] == list(range(len(exp["clusters"])))
    with np.load(tmp / "f" / "frontiers.npz") as z:
        assert z["rank"].tobytes() == exp["rank"].tobytes() and z["rank"].shape == shape
        assert z["index_origin"].tolist() == grid.index_origin.tolist() and float(z["cell"]) == OCC_CELL
    assert counts["clusters"] == len(exp["clusters"]) >= 1 and counts["frontier_cells"] == int((exp["label"] != fref.NONE).sum())
    reachable = sum(1 for e in exp["clusters"] if e["cost"] is not None)
    assert counts["reachable_clusters"] == reachable and rec["settings"]["radius"] == ROUTE_RADIUS
    assert len(line) == 1 and f"{counts['frontier_cells']} frontier cells in {counts['clusters']} clusters" in line[0]
    assert f"{counts['reachable_clusters']} reachable, {counts['sweeps']} sweeps" in line[0]
    print(line[0])
    print(f"two-chunk reconstruction: {reachable} of {counts['clusters']} clusters reachable at {ROUTE_RADIUS} m; "
          f"sizes {[e['cells'] for e in exp['clusters']][:12]}")
    from pi3_slam_amd import map_eval
    assert len(map_eval.read_ply_points(str(tmp / "f" / "frontiers.ply"))[0]) == counts["frontier_cells"]
    assert sorted(os.listdir(tmp / "f")) == ["frontiers.json", "frontiers.npz", "frontiers.ply"]
    if reachable:                                               # and the way to the nearest one, as `route` writes it
        cli.main(["frontiers", "--occupancy", occ, "--output", str(tmp / "g"), "--from-trajectory", tum, "--radius",
                  str(ROUTE_RADIUS), "--route-to", "0", "--device", DEV])
        way = json.load(open(tmp / "g" / "route.json"))
        assert way["cost"] == exp["clusters"][0]["cost"] and way["waypoints"][-1] == rec["clusters"][0]["goal"]
        assert way["settings"]["approach_unknown"] is True
        # a point `route --approach-unknown --goal` accepts as it stands
        cli.main(["route", "--occupancy", occ, "--output", str(tmp / "h"), "--from-trajectory", tum, "--radius",
                  str(ROUTE_RADIUS), "--approach-unknown", "--goal"] + [repr(v) for v in rec["clusters"][0]["goal"]]
                 + ["--device", DEV])
        assert json.load(open(tmp / "h" / "route.json"))["waypoints"] == way["waypoints"]
    # without a source: ordered by size
    cli.main(["frontiers", "--occupancy", occ, "--output", str(tmp / "s"), "--device", DEV])
    plain = fref.frontier_set(grid.state)
    rec = json.load(open(tmp / "s" / "frontiers.json"))
    assert [(c["root"], c["cells"], c["reachable"]) for c in rec["clusters"]] == [(e["root"], e["cells"], None)
                                                                                   for e in plain["clusters"]]
