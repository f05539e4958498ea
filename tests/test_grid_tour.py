"""The tour of the views without a GPU: view_tour.order_stops against the oracle (tests/grid_tour_ref.py: brute force over
all permutations, nearest neighbour and 2-opt written a second time), the nodes and the matrix at their edges,
ops.sweep_many_until_quiet driven by the oracle's emulation of the batched sweep, the box room's figures of DESIGN §7k from
the oracle alone, the header, the flags and tour.json / tour.npz / tour.ply."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_cover_ref as cref               # noqa: E402
import grid_route_ref as rref               # noqa: E402
import grid_tour_ref as tref                # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

HD = vref.headings26()
F90 = vref.cos2(90)


def _random_matrix(n, seed, values=(1, 2, 3)):
    """Symmetric, zero diagonal, entries from `values`: ties are the rule."""
    rng = np.random.default_rng(seed)
    D = rng.choice(np.asarray(values, np.int64), size=(n + 1, n + 1))
    D = np.triu(D, 1)
    return D + D.T


# ------------------------------------------------------------------------------------------------ 1. the order
@pytest.mark.parametrize("n", [0, 1, 2, 5, 7])
def test_the_exact_order_is_the_brute_forces(n):
    from pi3_slam_amd.view_tour import order_stops
    for seed in range(6 if n < 7 else 3):
        D = _random_matrix(n, 100 * n + seed)
        seq, cost = tref.brute_force(D)
        got = order_stops(D)
        assert got.method == "exact" and got.moves == 0
        assert (got.seq, got.cost) == (seq, cost), (n, seed, D.tolist())
        assert got.rank_order_cost == tref.path_cost(D, range(1, n + 1)) >= cost
        assert got.nn_cost == tref.path_cost(D, tref.nearest_neighbour(D)) >= cost
    if n == 0:
        assert order_stops(np.zeros((1, 1), np.int64)) == ([], 0, "exact", 0, 0, 0)


def test_the_exact_order_beyond_permutations():
    """Ten and twelve stops, where 10! permutations are out of reach: the oracle's top-down recursion."""
    from pi3_slam_amd.view_tour import order_stops
    for n, seed in ((10, 1), (12, 2)):
        D = _random_matrix(n, seed, values=(3, 4, 5, 6))
        got = order_stops(D)
        assert got.method == "exact" and (got.seq, got.cost) == tref.held_karp(D)
    D = _random_matrix(6, 5)
    assert tref.held_karp(D) == tuple(tref.brute_force(D))


@pytest.mark.parametrize("n", [2, 5, 7, 13, 30])
def test_two_opt_is_the_oracles_and_a_local_optimum(n):
    from pi3_slam_amd.view_tour import order_stops, two_opt_delta
    for seed in range(3):
        D = _random_matrix(n, 7 * n + seed, values=(1, 2, 3) if seed else tuple(range(1, 40)))
        exp = tref.nn_two_opt(D)
        got = order_stops(D, exact_max=0)
        assert got.method == "2-opt"
        assert (got.seq, got.cost, got.nn_cost, got.moves) == (exp["seq"], exp["cost"], exp["nn_cost"], exp["moves"])
        assert sorted(got.seq) == list(range(1, n + 1)) and got.cost == tref.path_cost(D, got.seq) <= got.nn_cost
        for i in range(n):                                      # no reversal lowers it
            for j in range(i + 1, n):
                assert two_opt_delta(D, got.seq, i, j) >= 0
                flipped = got.seq[:i] + got.seq[i:j + 1][::-1] + got.seq[j + 1:]
                assert tref.path_cost(D, flipped) - got.cost == two_opt_delta(D, got.seq, i, j)
        if n <= 7:
            assert got.cost >= order_stops(D).cost == tref.brute_force(D)[1]
    # above exact_max the default takes this branch
    D = _random_matrix(13, 3)
    assert order_stops(D).method == "2-opt" and order_stops(D, exact_max=13).method == "exact"
    assert order_stops(D, exact_max=13).cost <= order_stops(D).cost


def test_stops_along_a_line_cost_the_span():
    from pi3_slam_amd.view_tour import order_stops
    at = np.array([0, 7, 3, 12, 1, 9, 30, 4, 18, 2, 25, 11, 6, 21, 15], np.int64)       # node 0 at one end
    D = 12 * np.abs(at[:, None] - at[None, :])
    for exact_max in (0, 14):
        got = order_stops(D, exact_max=exact_max)
        assert got.cost == 12 * 30 and [int(at[s]) for s in got.seq] == sorted(at[1:].tolist())


# ------------------------------------------------------------------------------------------------ 2. the edges
def test_matrices_that_are_refused():
    from pi3_slam_amd.view_tour import order_stops, reachable_nodes
    D = _random_matrix(4, 1)
    D[1, 3] += 1
    with pytest.raises(ValueError, match=r"not symmetric: D\[1\]\[3\]"):
        order_stops(D)
    with pytest.raises(ValueError, match="not symmetric"):
        reachable_nodes(D)
    with pytest.raises(ValueError, match="square"):
        order_stops(np.zeros((2, 3), np.int64))
    D = _random_matrix(3, 2)
    D[2, 2] = 5
    with pytest.raises(ValueError, match="diagonal"):
        order_stops(D)
    D = _random_matrix(3, 2)
    D[0, 2] = D[2, 0] = tref.FAR
    with pytest.raises(ValueError, match="far entry"):
        order_stops(D)


def test_stops_that_cannot_be_reached_are_left_out_and_counted():
    from pi3_slam_amd.view_tour import order_stops, reachable_nodes
    # two components: the start with stops 1, 3, 4, and stops 2, 5 on the other side of a wall
    walk = np.ones((1, 3, 9), np.uint8)
    walk[0, :, 4] = 0
    lin = lambda x, y: y * 9 + x                                # noqa: E731
    cells, ranks = tref.nodes([lin(3, 0), lin(6, 1), lin(0, 2), lin(2, 1), lin(8, 2)], lin(1, 1))
    D = tref.matrix(tref.fields(walk, cells), cells)
    assert D[0, 2] == D[2, 0] == tref.FAR and D[2, 5] == D[5, 2] != tref.FAR and (D == D.T).all()
    keep, out = reachable_nodes(D)
    assert keep == [0, 1, 3, 4] and out == [2, 5]
    got = order_stops(D[np.ix_(keep, keep)])
    exp = tref.tour(walk, cells[1:], cells[0])
    assert [keep[s] for s in got.seq] == exp["seq"] and got.cost == exp["cost"] and exp["unreachable"] == [2, 5]
    assert keep == exp["keep"]


def test_nodes_of_views_that_share_a_cell_or_stand_on_the_start():
    from pi3_slam_amd.view_tour import order_stops, tour_nodes
    cells, ranks = tour_nodes([50, 20, 50, 7, 20, 50], 7)
    assert cells == [7, 50, 20, 7] and ranks == [[0, 2, 5], [1, 4], [3]]          # a view on the start cell is a stop
    assert (cells, ranks) == tref.nodes([50, 20, 50, 7, 20, 50], 7)
    assert tour_nodes([], 3) == ([3], [])
    walk = np.ones((1, 1, 60), np.uint8)
    D = tref.matrix(tref.fields(walk, cells), cells)
    assert D[0, 3] == D[3, 0] == 0 and D[0, 2] == 12 * 13
    got = order_stops(D)
    assert got.seq == [3, 2, 1] and got.cost == 12 * 43          # the stop on the start first, at a leg of cost 0
    assert got.rank_order_cost == 12 * (43 + 30 + 13)


# ------------------------------------------------------------------------------------------------ 3. the host loop
def test_the_sweep_loop_drops_each_field_when_it_is_quiet():
    from pi3_slam_amd import ops
    state, src, corner = rref.serpentine()
    walk = rref.walk_mask(state)
    blocked = int(np.flatnonzero(walk.reshape(-1) == 0)[0])
    sources = [src, corner, 16 * 33 + 16, blocked]                # two ends, the middle, and a field that stays all far
    single = [rref.tile_sweeps(walk, [s])[1] for s in sources]
    assert single[0] == 38 and single[3] == 1 and len(set(single)) >= 3
    for per_read in (1, 4, 5):
        emu = tref.SweepEmulation(walk, sources)
        sweeps = ops.sweep_many_until_quiet(emu.launch, torch.device("cpu"), len(sources), int(walk.sum()) + 1,
                                            "no {sweeps}", per_read)
        assert sweeps == single                                 # every field its own count, the quiet one included
        assert emu.settled().tobytes() == tref.fields(walk, sources).tobytes()
        for f, n in enumerate(single):                          # listed in whole batches, never after its quiet sweep
            batches = -(-n // per_read)
            listed = [f in h for h in emu.history]
            assert listed == [True] * (batches * per_read) + [False] * (len(emu.history) - batches * per_read)
            assert emu.swept[f] == batches * per_read
        assert all(h == sorted(set(h)) and h for h in emu.history)
        assert len(emu.history) == -(-max(single) // per_read) * per_read


def test_the_sweep_loop_with_one_field_is_the_single_loop():
    from pi3_slam_amd import ops
    walk = np.ones((1, 1, 300), np.uint8)
    for per_read in (1, 4):
        emu = tref.SweepEmulation(walk, [0])
        many = ops.sweep_many_until_quiet(emu.launch, torch.device("cpu"), 1, 301, "no {sweeps}", per_read)
        one = tref.SweepEmulation(walk, [0])

        def launch(flag):
            one.launch(torch.zeros(1, dtype=torch.int32), flag)
        assert many == [ops.sweep_until_quiet(launch, torch.device("cpu"), 301, "no {sweeps}", per_read)] == [39]
        assert len(emu.history) == len(one.history)
    # the bound: the line needs 39 launches
    emu = tref.SweepEmulation(walk, [0, 299])
    with pytest.raises(RuntimeError, match="the tour field did not settle in 8 sweeps over 5 cells"):
        ops.sweep_many_until_quiet(emu.launch, torch.device("cpu"), 2, 6,
                                   "the tour field did not settle in {sweeps} sweeps over 5 cells", 4)
    with pytest.raises(RuntimeError, match="single did not settle in 8"):
        one = tref.SweepEmulation(walk, [0])
        ops.sweep_until_quiet(lambda flag: one.launch(torch.zeros(1, dtype=torch.int32), flag), torch.device("cpu"), 6,
                              "single did not settle in {sweeps}", 4)


# ------------------------------------------------------------------------------------------------ 4. the box room
@pytest.fixture(scope="module")
def box_room():
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    walk = rref.walk_mask(state, oref.edt_ref(state, R, False), min_d2)      # clearance against occupied cells only
    dist = rref.distances(walk, lin)
    cand = vref.candidates(dist, room["origin"], 4)
    cost = dist.reshape(-1)[cand].astype(np.int64)
    forty = cref.cover(state, cand, cost, 8, HD, *F90, count=40)
    found = vref.view_set(state, dist, room["origin"], 8, 4, 90, 10, 4)
    return dict(state=state, walk=walk, cams=lin, cover=forty, find=found["views"])


def _covered(state, views):
    seen = np.zeros(cref.seen_words(state.size), np.uint32)
    news = [cref.mark(state, seen, [c], [h], 8, HD, *F90)["counters"][4] for c, h in views]
    return news, cref.popcount(seen)


def test_the_box_room_figures(box_room):
    b = box_room
    start = b["cams"][-1]
    assert start == 34781 and b["cams"][0] == 35032
    picks = [(c, h) for c, h, _ in b["cover"]["picks"]]
    ten = tref.tour(b["walk"], [c for c, _ in picks[:10]], start)
    assert len(ten["cells"]) == 11 and ten["unreachable"] == [] and ten["method"] == "exact"
    assert (ten["rank_order_cost"], ten["nn_cost"], ten["cost"]) == (2232, 1422, 1422)
    assert [s - 1 for s in ten["seq"]] == [8, 0, 6, 4, 2, 3, 5, 7, 1, 9]
    assert tref.nn_two_opt(ten["matrix"])["moves"] == 0
    for leg, (a, c) in zip(ten["legs"], zip([0] + ten["seq"][:-1], ten["seq"])):
        assert leg[0] == ten["cells"][a] and leg[-1] == ten["cells"][c]
        assert sum(rref.step_cost(p, q, b["state"].shape) for p, q in zip(leg, leg[1:])) == ten["matrix"][a, c]
    in_tour = [picks[s - 1] for s in ten["seq"]]
    news, total = _covered(b["state"], in_tour)
    assert total == 3016 == sum(news) and sorted(news) != news
    # from camera 0
    other = tref.tour(b["walk"], [c for c, _ in picks[:10]], b["cams"][0])
    assert (other["rank_order_cost"], other["cost"]) == (2264, 1433)
    # find's ten
    views = [(v["cell"], v["heading"]) for v in b["find"]]
    plain = tref.tour(b["walk"], [c for c, _ in views], start)
    assert (plain["rank_order_cost"], plain["nn_cost"], plain["cost"]) == (1922, 1256, 1221)
    assert [s - 1 for s in plain["seq"]] == [8, 0, 2, 9, 3, 7, 6, 4, 5, 1]
    assert _covered(b["state"], [views[s - 1] for s in plain["seq"]])[1] == 2024


def test_the_box_rooms_first_forty(box_room):
    from pi3_slam_amd.view_tour import order_stops, reachable_nodes
    b = box_room
    cells = [c for c, _, _ in b["cover"]["picks"]]
    assert len(cells) == 40
    forty = tref.tour(b["walk"], cells, b["cams"][-1])
    assert len(forty["cells"]) == 39 and forty["method"] == "2-opt"                    # 38 stops: two cells pan
    assert (forty["rank_order_cost"], forty["nn_cost"], forty["cost"], forty["moves"]) == (8994, 3526, 3208, 6)
    keep, out = reachable_nodes(forty["matrix"])
    got = order_stops(forty["matrix"])
    assert out == [] and got.seq == forty["seq"] and (got.cost, got.moves, got.nn_cost) == (3208, 6, 3526)


# ------------------------------------------------------------------------------------------------ 5. the host side
def test_signatures_header_and_ops_agree():
    from pi3_slam_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    for name, n_args in (("pi3_grid_route_fields_init", 9), ("pi3_grid_route_sweep_many", 11),
                         ("pi3_grid_route_trace_many", 13)):
        assert len(lib.SIGNATURES[name]) == n_args
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args
        assert callable(getattr(ops, name[len("pi3_"):]))
    assert ops.ROUTE_FIELDS_COUNTERS == ("sources_accepted", "sources_blocked", "sources_outside")
    source = open(os.path.join(ROOT, "pi3_slam_amd", "csrc", "grid_route.hip")).read()
    for name in ("pi3_grid_route_fields_init", "pi3_grid_route_sweep_many", "pi3_grid_route_trace_many"):
        assert f'extern "C" int {name}(' in source
    assert source.count("__device__ __forceinline__ void trace_walk(") == 1 and source.count("trace_walk(walk") == 2


def test_views_parser_of_the_tour(tmp_path):
    from pi3_slam_amd import cli
    base = ["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"]
    a = cli.build_parser().parse_args(base)
    assert a.tour is False and a.tour_from is None
    a = cli.build_parser().parse_args(base + ["--cover", "--tour", "--tour-from", "0.5", "-1", "2", "--route-to", "0"])
    assert a.tour is True and a.tour_from == [0.5, -1.0, 2.0] and a.cover is True and a.route_to == 0
    with pytest.raises(SystemExit, match="views: --tour-from needs --tour"):
        cli.main(base + ["--tour-from", "0", "0", "0"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--tour", "--tour-from", "0", "0"])
    with pytest.raises(SystemExit, match="views: .*missing.npz"):                 # refused flags first, then the file
        cli.main(["views", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path), "--start", "0", "0",
                  "0", "--tour"])
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert "--tour-from X Y Z" in text and "--tour " in text


def test_plan_tour_refuses_before_the_device():
    from pi3_slam_amd.grid_route import RouteField
    from pi3_slam_amd.view_planner import View, ViewSet
    from pi3_slam_amd.view_tour import plan_tour
    shape = (1, 2, 5)
    state = np.ones(shape, np.uint8)
    state[0, 0, 4] = 2
    walk = (state == 1).astype(np.uint8)
    origin = np.array([-1, 0, 2], np.int64)
    f = RouteField(None, None, walk, origin, 0.5, state, None, {"traversable": 9}, {"radius": 0.0},
                   {"walk": torch.from_numpy(walk)})
    views = [View(r, c, np.zeros(3), 0, HD[0].copy(), HD[0] / 1.0, 1, 1, 0, 0.0) for r, c in enumerate((1, 3, 1, 7))]
    vset = ViewSet(views, None, None, HD, origin, 0.5, {}, {"range_cells": 2, "cos2_num": 1, "cos2_den": 2}, f, None)
    with pytest.raises(ValueError, match="carries no sources: give the tour a start"):
        plan_tour(vset)
    vset.sources = np.array([[0.1, 0.1, 1.1], [1.6, 0.2, 1.2]])                   # the last: cell (4, 0, 0), occupied
    with pytest.raises(ValueError, match=r"the start is not traversable: cell \(4, 0, 0\) is occupied"):
        plan_tour(vset)
    with pytest.raises(ValueError, match="lies outside the grid"):
        plan_tour(vset, [9.0, 0.0, 1.1])
    with pytest.raises(ValueError, match="one point"):
        plan_tour(vset, [[0.0, 0.0, 1.1], [0.0, 0.0, 1.1]])
    with pytest.raises(ValueError, match=r"the tour of 4 views needs 4 distance fields of 10 cells, 160 bytes: more than "
                                         r"the limit of 159 bytes"):
        plan_tour(vset, [-0.4, 0.1, 1.1], max_field_bytes=159)
    with pytest.raises(ValueError, match="carries no route field"):
        plan_tour(ViewSet(views, None, None, HD, origin, 0.5))


def test_tour_files(tmp_path):
    from pi3_slam_amd import export, map_eval
    from pi3_slam_amd.view_tour import Tour, TourStop
    D = np.array([[0, 24, 12], [24, 0, 12], [12, 12, 0]], np.int64)
    legs = [np.array([5, 6]), np.array([6, 7, 8])]
    ways = [np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]]), np.array([[0.75, 0.25, 0.25], [1.25, 0.25, 0.25],
                                                                          [1.75, 0.25, 0.25]])]
    stops = [TourStop(1, 6, ways[0][-1], [1], 12, 12, 0.5, None, [7], [7]),
             TourStop(0, 8, ways[1][-1], [0, 2], 12, 24, 1.0, float("inf"), [9, 2], [16, 18])]
    tour = Tour(stops, [1, 0], 5, ways[0][0], D, np.array([5, 8, 6]), legs, ways, 24, 1.5, 36, 24, 0, "exact", [], 18,
                {"fields": 3, "stops": 2, "sweeps_min": 1, "sweeps_max": 2, "launches": 4, "traced_cells": 5,
                 "unreachable": 0}, {"cell": 0.5, "radius": 0.0})
    assert tour.distance_m == 1.0 and tour.rank_order_length_m == 1.5
    assert export.write_tour(tour, str(tmp_path)) == 2
    assert sorted(os.listdir(tmp_path)) == ["tour.json", "tour.npz", "tour.ply"]
    rec = json.load(open(tmp_path / "tour.json"))
    assert rec["order"] == [1, 0] and rec["cost"] == 24 and rec["rank_order_cost"] == 36 and rec["method"] == "exact"
    assert rec["distance_m"] == 1.0 and rec["length_m"] == 1.5 and rec["rank_order_length_m"] == 1.5 and rec["covered"] == 18
    assert rec["counts"] == tour.counts and rec["settings"] == tour.settings and rec["unreachable"] == []
    assert rec["start"] == {"cell": 5, "position": [0.25, 0.25, 0.25]}
    assert [(s["number"], s["cell"], s["leg_cost"], s["cumulative_cost"], s["length_m"]) for s in rec["stops"]] == [
        (1, 6, 12, 12, 0.5), (0, 8, 12, 24, 1.0)]
    assert rec["stops"][1]["views"] == [{"rank": 0, "tour_new": 9, "tour_covered": 16},
                                        {"rank": 2, "tour_new": 2, "tour_covered": 18}]
    assert rec["stops"][0]["min_clearance_m"] is None and rec["stops"][1]["min_clearance_m"] == "inf"
    assert rec["stops"][1]["position"] == [1.75, 0.25, 0.25]
    with np.load(tmp_path / "tour.npz") as z:
        assert sorted(z.files) == ["cells", "matrix", "offsets", "order", "waypoint_cells", "waypoints"]
        assert z["order"].tolist() == [1, 0] and z["matrix"].tolist() == D.tolist() and z["cells"].tolist() == [5, 8, 6]
        assert z["offsets"].tolist() == [0, 2, 5] and z["waypoint_cells"].tolist() == [5, 6, 6, 7, 8]
        assert z["waypoints"].tolist() == np.concatenate(ways).tolist() and z["matrix"].dtype == np.int64
    pts, cols = map_eval.read_ply_points(str(tmp_path / "tour.ply"))
    assert pts.tolist() == np.concatenate(ways).astype(np.float32).tolist()
    assert cols[0].tolist() == cols[1].tolist() == list(export.FRONTIER_PALETTE[0]) and cols[4].tolist() == list(
        export.FRONTIER_PALETTE[1])
    # a tour of nothing
    empty = Tour([], [], 5, ways[0][0], np.zeros((1, 1), np.int64), np.array([5]), [], [], 0, 0.0, 0, 0, 0, "exact", [],
                 0, {}, {"cell": 0.5})
    assert export.write_tour(empty, str(tmp_path / "e")) == 0
    with np.load(tmp_path / "e" / "tour.npz") as z:
        assert z["offsets"].tolist() == [0] and z["waypoints"].shape == (0, 3)
