"""Frontiers of the occupancy grid without a GPU: the oracle (tests/grid_frontier_ref.py) against scipy.ndimage, closed
forms and its own emulation of the kernel's tile schedule, the box room's figures, the ranking on a hand-built plan,
argument checks, the `frontiers` parser and the file writers."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grid_frontier_ref as fref        # noqa: E402
import grid_route_ref as rref           # noqa: E402
import occupancy_ref as oref            # noqa: E402


def _lin(x, y, z, shape):
    nz, ny, nx = shape
    return (z * ny + y) * nx + x


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("mix", [(0.5, 0.1), (0.1, 0.1), (0.03, 0.3)], ids=lambda m: "%g-%g" % m)
def test_labels_are_scipys_partition_named_by_the_smallest_index(mix, seed):
    from scipy import ndimage
    shape = (11, 13, 17)
    state = fref.three_state(shape, mix[0], mix[1], seed)
    lab = fref.labels(state)
    front = fref.faces(state) > 0
    assert ((lab != fref.NONE) == front).all() and front.sum() > 100
    theirs, n = ndimage.label(front, structure=np.ones((3, 3, 3)))
    flat, tflat = lab.reshape(-1), theirs.reshape(-1)
    cells = np.flatnonzero(front.reshape(-1))
    pairs = set(zip(flat[cells].tolist(), tflat[cells].tolist()))
    assert len(pairs) == n == len(set(flat[cells].tolist()))    # a bijection between the two namings
    for name in set(flat[cells].tolist()):
        assert name == cells[flat[cells] == name].min()
    assert fref.roots(lab).tolist() == sorted(set(flat[cells].tolist()))
    m = fref.mark(state)
    assert m["counters"] == [int(front.sum()), int(fref.faces(state).sum()), 0, 0]
    assert (m["label"].reshape(-1)[cells] == cells).all() and (m["label"][~front] == fref.NONE).all()


def test_faces_by_hand():
    state = np.array([[[1, 1, 0, 1, 2, 1]]], np.uint8)           # one line: above, below and beside it lies outside
    assert fref.faces(state).tolist() == [[[5, 5, 0, 5, 0, 5]]]  # 4 outside + the line's end or the unknown cell
    state = np.ones((3, 3, 3), np.uint8)
    f = fref.faces(state)
    assert f[1, 1, 1] == 0 and f[0, 0, 0] == 3 and f[0, 1, 1] == 1 and f[0, 0, 1] == 2 and f.sum() == 54
    state[1, 1, 1] = 0                                          # an unknown cell inside: its 6 neighbours gain a face
    assert fref.faces(state).sum() == 60 and fref.faces(state)[1, 1, 1] == 0
    state[1, 1, 1] = 2                                          # an occupied one: none
    assert fref.faces(state).sum() == 54


def _cuboid(shape, lo, size):
    state = np.zeros(shape, np.uint8)
    (x, y, z), (a, b, c) = lo, size
    state[z:z + c, y:y + b, x:x + a] = 1
    return state


@pytest.mark.parametrize("lo", [(2, 3, 1), (0, 0, 0), (4, 3, 2)], ids=["inside", "low-corner", "high-corner"])
def test_a_free_cuboid_in_unknown_space(lo):
    shape, (a, b, c) = (7, 9, 10), (6, 5, 4)                    # the grid: x 10, y 9, z 7; high-corner ends on its border
    state = _cuboid(shape, lo, (a, b, c))
    s = fref.frontier_set(state)
    assert s["roots"].tolist() == [_lin(*lo, shape)] and s["keep"] == [0] and s["dropped"] == []
    row = s["stats"][0]
    cells = a * b * c - (a - 2) * (b - 2) * (c - 2)
    assert row[0] == cells and row[1] == 2 * (a * b + b * c + c * a)
    # the shell's coordinate sums: the cuboid's minus the inner cuboid's
    def sums(n0, n, m):                                         # sum over n cells from n0, each counted m times
        return m * (n * n0 + n * (n - 1) // 2)
    inner = (a - 2) * (b - 2) * (c - 2)
    assert row[2] == sums(lo[0], a, b * c) - sums(lo[0] + 1, a - 2, inner // (a - 2))
    assert row[3] == sums(lo[1], b, a * c) - sums(lo[1] + 1, b - 2, inner // (b - 2))
    assert row[4] == sums(lo[2], c, a * b) - sums(lo[2] + 1, c - 2, inner // (c - 2))
    assert row[5:8].tolist() == list(lo) and row[8:11].tolist() == [lo[0] + a - 1, lo[1] + b - 1, lo[2] + c - 1]
    assert row[11] == -1 and s["counters"] == [cells, 0, 0, 0]  # no dist: best stays all ones
    assert (s["rank"] >= 0).sum() == cells and set(np.unique(s["rank"]).tolist()) == {-1, 0}


def test_corner_contact_joins_and_a_gap_separates():
    shape = (10, 10, 10)
    one = _cuboid(shape, (1, 1, 1), (3, 3, 3)) | _cuboid(shape, (4, 4, 4), (3, 3, 3))     # (3,3,3) and (4,4,4) touch
    s = fref.frontier_set(one)
    assert s["roots"].tolist() == [_lin(1, 1, 1, shape)] and s["stats"][0, 0] == 2 * 26
    two = _cuboid(shape, (1, 1, 1), (3, 3, 3)) | _cuboid(shape, (5, 5, 5), (3, 3, 3))
    s = fref.frontier_set(two)
    assert s["roots"].tolist() == [_lin(1, 1, 1, shape), _lin(5, 5, 5, shape)] and s["stats"][:, 0].tolist() == [26, 26]


def test_grids_without_a_frontier():
    room = np.zeros((8, 9, 10), np.uint8)
    room[1:7, 1:8, 1:9] = 2
    room[2:6, 2:7, 2:8] = 1                                     # closed by occupied walls, fully free inside
    for state in (room, np.zeros((5, 6, 7), np.uint8), np.full((5, 6, 7), 2, np.uint8)):
        s = fref.frontier_set(state)
        assert (s["label"] == fref.NONE).all() and len(s["roots"]) == 0 and s["stats"].shape == (0, 12)
        assert s["counters"] == [0, 0, 0, 0] and (s["rank"] == -1).all() and s["clusters"] == []
        assert fref.mark(state)["counters"] == [0, 0, 0, 0]
        assert fref.tile_sweeps(fref.mark(state)["label"])[1:] == (1, 0)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("shape", [(5, 17, 19), (17, 9, 20), (3, 24, 24)], ids=lambda s: "%dx%dx%d" % s)
def test_the_tile_schedule_reaches_the_component_minima(shape, seed):
    state = fref.three_state(shape, 0.15, 0.3, seed)
    lab, launches, changing = fref.tile_sweeps(fref.mark(state)["label"])
    assert lab.tobytes() == fref.labels(state).tobytes() and launches == changing + 1 and 2 <= launches <= 12
    print(f"{shape} seed {seed}: {launches} launches, {len(fref.roots(lab))} clusters")


def test_tiles_relax_to_their_own_fixed_point():
    line = np.ones((1, 1, 300), np.uint8)                       # all frontier: label 0 travels 299 cells
    lab, launches, changing = fref.tile_sweeps(fref.mark(line)["label"])
    assert (lab == 0).all() and changing == 38 and launches == 39
    state = fref.serpentine()
    lab, launches, changing = fref.tile_sweeps(fref.mark(state)["label"])
    assert lab.tobytes() == fref.labels(state).tobytes() and fref.roots(lab).tolist() == [0]
    assert (lab[state == 1] == 0).all() and 20 <= launches <= 60
    print(f"serpentine: {launches} launches")


@pytest.fixture(scope="module")
def box_room():
    import test_grid_route as cases
    room, state, cams, d2u, walk_u, (R, min_d2) = cases.box_room_case()
    lin = [_lin(*c, state.shape) for c in cams]
    walk_a = rref.walk_mask(state, oref.edt_ref(state, R, False), min_d2)
    return dict(room=room, state=state, cams=cams, lin=lin, R=R, min_d2=min_d2, walk_u=walk_u, walk_a=walk_a,
                dist_u=rref.distances(walk_u, lin), dist_a=rref.distances(walk_a, lin),
                dist_0=rref.distances(rref.walk_mask(state), lin))


def test_box_room_frontiers_need_approach_unknown(box_room):
    b = box_room
    assert b["state"].shape == (35, 40, 50) and len(b["lin"]) == 12
    front = fref.faces(b["state"]) > 0
    s = fref.frontier_set(b["state"], b["dist_a"])
    assert front.sum() == 4292 and len(s["roots"]) == 1
    for dist, cells, frontier_cells in ((b["dist_u"], 10612, 0), (b["dist_a"], 15896, 3748), (b["dist_0"], None, 4292)):
        reach = dist != rref.FAR
        assert cells is None or reach.sum() == cells
        assert (front & reach).sum() == frontier_cells
        assert fref.stats(b["state"], s["label"], dist, s["roots"])["counters"] == [4292, 0, frontier_cells, 0]
    c = s["clusters"][0]
    assert c["cells"] == 4292 and c["cost"] is not None and front.reshape(-1)[c["goal"]]
    assert c["cost"] == b["dist_a"].reshape(-1)[c["goal"]] == b["dist_a"][front].min()
    assert fref.frontier_set(b["state"], b["dist_u"])["clusters"][0]["cost"] is None


def ranking_plan():
    """x 29, y 9, z 3: an occupied floor, ceiling and border, free inside, an occupied wall at x = 21 that closes a
    room; single unknown cells make the frontiers.  -> (state, source, expectation per cluster in rank order at
    min_cells = 3: (root, cells, cost or None), the dropped root)."""
    shape = (3, 9, 29)
    state = np.full(shape, 2, np.uint8)
    state[1, 1:8, 1:28] = 1
    state[1, :, 21] = 2
    for x, y in ((5, 4), (15, 4), (10, 1), (25, 3), (25, 5), (1, 1)):
        state[1, y, x] = 0
    lin = lambda x, y: _lin(x, y, 1, shape)                     # noqa: E731
    expect = [(lin(9, 1), 3, 24),                               # under (10, 1): (10, 2) is two cells from the source
              (lin(5, 3), 4, 48), (lin(15, 3), 4, 48),          # a tie of 4 cells each way: the smaller root first
              (lin(25, 2), 7, None)]                            # behind the wall: two holes that share (25, 4)
    return state, lin(10, 4), expect, lin(2, 1)


def test_ranking_on_a_hand_built_plan():
    from pi3_slam_amd.frontier import order_clusters
    state, src, expect, dropped_root = ranking_plan()
    dist = rref.distances(rref.walk_mask(state), [src])
    s = fref.frontier_set(state, dist, min_cells=3)
    assert [(c["root"], c["cells"], c["cost"]) for c in s["clusters"]] == expect
    assert [int(s["roots"][k]) for k in s["dropped"]] == [dropped_root] and s["stats"][s["dropped"][0], 0] == 2
    assert s["clusters"][1]["goal"] == _lin(6, 4, 1, state.shape) and s["clusters"][2]["goal"] == _lin(14, 4, 1, state.shape)
    flat = s["rank"].reshape(-1)
    assert [flat[c[0]] for c in expect] == [0, 1, 2, 3] and flat[dropped_root] == -1
    assert (flat >= 0).sum() == 3 + 4 + 4 + 7
    # the product's own ordering on the same rows
    keep, dropped = order_clusters(s["stats"], s["roots"], 3, True)
    assert keep.tolist() == s["keep"] and dropped.tolist() == s["dropped"]
    # nothing dropped: the two-cell cluster is reachable too and takes its place by its cost
    everything = fref.frontier_set(state, dist, min_cells=1)
    keep, dropped = order_clusters(everything["stats"], everything["roots"], 1, True)
    assert keep.tolist() == everything["keep"] and len(keep) == 5 and len(dropped) == 0
    costs = [c["cost"] for c in everything["clusters"]]
    assert costs[:-1] == sorted(costs[:-1]) and costs[-1] is None
    # without sources: by size, ties by root, nothing reachable
    plain = fref.frontier_set(state, None, min_cells=3)
    assert [(c["root"], c["cells"], c["cost"]) for c in plain["clusters"]] == [
        (expect[3][0], 7, None), (expect[1][0], 4, None), (expect[2][0], 4, None), (expect[0][0], 3, None)]
    keep, _ = order_clusters(plain["stats"], plain["roots"], 3, False)
    assert keep.tolist() == plain["keep"]
    keep, _ = order_clusters(s["stats"], s["roots"], 3, False)  # a field's `best` is ignored without sources
    assert keep.tolist() == plain["keep"]


def test_arguments():
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.frontier import FrontierCluster, FrontierFinder, FrontierSet
    from pi3_slam_amd.grid_route import GridRouter, RouteField
    with pytest.raises(ValueError, match="exclude each other"):
        GridRouter(0.2, through_unknown=True, approach_unknown=True)
    r = GridRouter(0.2, approach_unknown=True)
    assert r.approach_unknown is True and r.through_unknown is False
    assert r.settings() == {"radius": 0.2, "through_unknown": False, "approach_unknown": True, "costs": [12, 17, 21]}
    assert GridRouter().settings()["approach_unknown"] is False and GridRouter().approach_unknown is False
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="min_cells"):
            FrontierFinder(min_cells=bad)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            FrontierFinder(radius=bad)
    f = FrontierFinder(0.2, 5)
    assert f.router.approach_unknown and f.router.radius == 0.2 and f.settings()["min_cells"] == 5
    assert FrontierFinder().min_cells == 1 and FrontierFinder().radius == 0.0
    # refused before anything reaches the device
    huge = OccupancyGrid(np.broadcast_to(np.ones(1, np.uint8), (1 << 9, 1 << 9, (1 << 9) + 1)), np.zeros(3, np.int64), 0.1)
    with pytest.raises(ValueError, match="at most 2\\^27"):
        FrontierFinder().find(huge, None, "cpu")
    with pytest.raises(ValueError, match="not empty"):
        FrontierFinder().find(OccupancyGrid(np.zeros((0, 3, 4), np.uint8), np.zeros(3, np.int64), 0.1), None, "cpu")
    # route_to
    z3 = np.zeros(3)
    near = FrontierCluster(0, 7, 4, 4, z3, z3, z3, True, 24, 0.2, 9, z3)
    far = FrontierCluster(1, 30, 9, 9, z3, z3, z3, False)
    rank = np.full((1, 1, 40), -1, np.int32)
    bare = FrontierSet([near, far], rank, np.zeros(3, np.int64), 0.1)
    with pytest.raises(ValueError, match="no route without sources"):
        bare.route_to(0)
    field = RouteField(None, None, np.ones((1, 1, 40), np.uint8), np.zeros(3, np.int64), 0.1, np.ones((1, 1, 40), np.uint8))
    ranked = FrontierSet([near, far], rank, np.zeros(3, np.int64), 0.1, {}, {"radius": 0.2}, field, GridRouter(0.2))
    with pytest.raises(ValueError, match=r"cluster 1 \(root 30, 9 cells\) cannot be reached at a radius of 0.2"):
        ranked.route_to(1)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="no cluster of rank"):
            ranked.route_to(bad)


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pi3slam_hip.h")).read()
    for name, n_args in (("pi3_grid_frontier_mark", 7), ("pi3_grid_frontier_sweep", 6), ("pi3_grid_frontier_roots", 8),
                         ("pi3_grid_frontier_stats", 11)):
        assert len(lib.SIGNATURES[name]) == n_args
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args
        assert hasattr(ops, name[len("pi3_"):])
    assert "grid_frontier.hip" in open(os.path.join(root, "pi3_slam_amd", "csrc", "Makefile")).read()
    assert len(ops.FRONTIER_STATS_FIELDS) == 12 and ops.FRONTIER_KEY_SHIFT == fref.KEY_SHIFT
    assert ops.FRONTIER_NONE == fref.NONE


def test_frontiers_parser(tmp_path):
    from pi3_slam_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["frontiers", "--occupancy", "o.npz", "--output", "out"])
    assert a.command == "frontiers" and a.start is None and a.from_trajectory is None and a.radius == 0.0
    assert a.min_cells == 1 and a.route_to is None and a.device == "cuda"
    a = p.parse_args(["frontiers", "--occupancy", "o.npz", "--output", "out", "--from-trajectory", "t.tum", "--radius",
                      "0.1", "--min-cells", "20", "--route-to", "0"])
    assert a.from_trajectory == "t.tum" and a.radius == 0.1 and a.min_cells == 20 and a.route_to == 0
    a = p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--start", "0", "0", "0", "--approach-unknown"])
    assert a.approach_unknown is True and a.through_unknown is False
    assert p.parse_args(["route", "--occupancy", "o.npz", "--output", "out", "--start", "0", "0", "0"]).approach_unknown is False
    for argv in (["frontiers", "--output", "out"], ["frontiers", "--occupancy", "o.npz"],
                 ["frontiers", "--occupancy", "o.npz", "--output", "out", "--min-cells", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    missing = ["frontiers", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path)]
    with pytest.raises(SystemExit, match="--route-to needs a source"):
        cli.main(missing + ["--route-to", "0"])
    with pytest.raises(SystemExit, match="not both"):
        cli.main(missing + ["--start", "0", "0", "0", "--from-trajectory", "t.tum"])
    with pytest.raises(SystemExit, match="frontiers: .*min_cells"):
        cli.main(missing + ["--min-cells", "-1"])
    with pytest.raises(SystemExit, match="frontiers: .*missing.npz"):       # one line, no traceback
        cli.main(missing)
    with pytest.raises(SystemExit, match="route: .*exclude each other"):
        cli.main(["route", "--occupancy", str(tmp_path / "missing.npz"), "--output", str(tmp_path), "--start", "0", "0",
                  "0", "--through-unknown", "--approach-unknown"])


def test_frontier_files(tmp_path):
    from pi3_slam_amd import export, map_eval
    from pi3_slam_amd.frontier import FrontierCluster, FrontierSet
    rank = np.full((2, 2, 3), -1, np.int32)
    rank[0, 0, :2] = 0
    rank[1, 1, 2] = 1
    origin, cell = np.array([1, -2, 3], np.int64), 0.5
    centre = lambda i: cell * (origin + np.asarray(i, np.float64) + 0.5)   # noqa: E731
    near = FrontierCluster(0, 0, 2, 7, centre([0.5, 0, 0]), centre([0, 0, 0]), centre([1, 0, 0]), True, 24, 1.0, 1,
                           centre([1, 0, 0]))
    far = FrontierCluster(1, 11, 1, 3, centre([2, 1, 1]), centre([2, 1, 1]), centre([2, 1, 1]), False)
    counts = {"frontier_cells": 3, "clusters": 2, "clusters_dropped": 0, "reachable_clusters": 1, "sweeps": 2}
    fs = FrontierSet([near, far], rank, origin, cell, counts, {"radius": 0.2, "min_cells": 1})
    assert export.write_frontiers(fs, str(tmp_path / "a")) == 3
    assert sorted(os.listdir(tmp_path / "a")) == ["frontiers.json", "frontiers.npz", "frontiers.ply"]
    rec = json.load(open(tmp_path / "a" / "frontiers.json"))
    assert rec["counts"] == counts and rec["settings"] == {"radius": 0.2, "min_cells": 1} and len(rec["clusters"]) == 2
    assert rec["clusters"][0] == {"rank": 0, "root": 0, "cells": 2, "unknown_faces": 7, "centroid": [1.0, -0.75, 1.75],
                                  "bbox_min": [0.75, -0.75, 1.75], "bbox_max": [1.25, -0.75, 1.75], "reachable": True,
                                  "cost": 24, "distance_m": 1.0, "goal_cell": 1, "goal": [1.25, -0.75, 1.75]}
    assert rec["clusters"][1]["reachable"] is False and rec["clusters"][1]["goal"] is None and rec["clusters"][1]["cost"] is None
    with np.load(tmp_path / "a" / "frontiers.npz") as z:
        assert z["rank"].tobytes() == rank.tobytes() and z["rank"].dtype == np.int32 and z["rank"].shape == (2, 2, 3)
        assert z["index_origin"].tolist() == [1, -2, 3] and z["origin"].tolist() == [0.5, -1.0, 1.5] and float(z["cell"]) == 0.5
    pts, cols = map_eval.read_ply_points(str(tmp_path / "a" / "frontiers.ply"))
    assert pts.tolist() == [centre([0, 0, 0]).tolist(), centre([1, 0, 0]).tolist(), centre([2, 1, 1]).tolist()]
    if cols is not None:
        assert np.asarray(cols).reshape(-1, 3)[2].tolist() in ([128, 128, 128], [128 / 255.0] * 3)
    unranked = FrontierSet([FrontierCluster(0, 0, 2, 7, centre([0.5, 0, 0]), centre([0, 0, 0]), centre([1, 0, 0]))],
                           np.where(rank == 0, 0, -1).astype(np.int32), origin, cell, {}, {})
    assert export.write_frontiers(unranked, str(tmp_path / "b")) == 2
    assert json.load(open(tmp_path / "b" / "frontiers.json"))["clusters"][0]["reachable"] is None
    empty = FrontierSet([], np.full((1, 1, 2), -1, np.int32), origin, cell, {"clusters": 0}, {})
    assert export.write_frontiers(empty, str(tmp_path / "c")) == 0
    assert len(map_eval.read_ply_points(str(tmp_path / "c" / "frontiers.ply"))[0]) == 0
