"""Views of the occupancy grid on the GPU (csrc/grid_view.hip), byte for byte against the oracle (tests/grid_view_ref.py):
the gain and candidates kernels, their argument checks, the box room through ViewPlanner, and reconstruct ->
occupancy.npz -> `cli views` on a two-chunk sequence.  Every output is filled with a poison value before each call."""
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
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON32, POISON64 = -5, 11
HD = vref.headings26()
FOVS = (vref.cos2(90), vref.cos2(180))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gain_device(state, cand, R, headings, num, den):
    from pi3_slam_amd import ops
    V, H = len(cand), len(headings)
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_gain(state, _dev(np.asarray(cand, np.int64)), R, headings, num, den, gain, visible, best, counters)
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _same(got, exp, what):
    assert got["counters"] == exp["counters"], (what, got["counters"], exp["counters"])
    assert got["visible"].tobytes() == exp["visible"].tobytes(), (what, "visible")
    assert got["gain"].tobytes() == exp["gain"].tobytes(), (what, "gain", int((got["gain"] != exp["gain"]).sum()))
    assert got["best"].dtype == np.int32 and got["best"].tobytes() == exp["best"].tobytes(), (what, "best")


def _states(dims):
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    return {"0.5/0.4/0.1": vref.three_state(shape, 0.5, 0.1, nx + ny + nz),
            "0.1/0.8/0.1": vref.three_state(shape, 0.1, 0.1, nx + 2 * ny + 3 * nz),
            "0.2/0.1/0.7": vref.three_state(shape, 0.2, 0.7, 2 * nx + ny + nz),
            "unknown": np.zeros(shape, np.uint8), "free": np.ones(shape, np.uint8)}


def _candidates(dims, seed):
    """Every cell of a small grid; of a large one the 8 corners, 64 seeded cells and one index outside."""
    nx, ny, nz = dims
    cells = nx * ny * nz
    if cells <= 600:
        return np.arange(cells, dtype=np.int64)
    corners = [(z * ny + y) * nx + x for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)]
    rng = np.random.default_rng(seed)
    return np.concatenate([corners, rng.integers(0, cells, 64), [cells]]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. the gain kernel
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 300), (9, 8, 7), (17, 9, 20), (65, 67, 66)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_gain_matches_the_oracle_byte_for_byte(dims):
    cand = _candidates(dims, sum(dims))
    nums, dens = [f[0] for f in FOVS], [f[1] for f in FOVS]
    for name, state in _states(dims).items():
        st = _dev(state)
        for R in (1, 2, 7):
            exp = vref.gain(state, cand, R, HD, nums, dens)
            for e, (num, den) in zip(exp, FOVS):
                _same(_gain_device(st, cand, R, HD, num, den), e, (dims, name, R, num))
            c = exp[0]["counters"]
            assert c[0] == len(cand) - (state.size > 600) and c[1] == c[2] + c[3]
            assert name != "free" or c[1] == 0
            assert name != "unknown" or c[2] == 0
            if state.size > 600 and "/" in name and R == 7:
                assert c[2] > 0 and c[3] > 0 and len(set(exp[0]["best"].tolist())) > 3       # the case says something
                assert exp[0]["best"][-1] == -1 and not exp[0]["gain"][-1].any()


def test_gain_at_the_largest_range():
    dims = (65, 67, 66)
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    centre = (33 * ny + 33) * nx + 32                            # 32 cells from every border
    open_space = np.zeros(shape, np.uint8)
    got = _gain_device(_dev(open_space), [centre], 32, HD, *FOVS[0])
    assert got["visible"].tolist() == [137064] and got["counters"] == [1, 137064, 0, 137064]
    _same(got, vref.gain(open_space, [centre], 32, HD, *FOVS[0]), "open")
    mixed = vref.three_state(shape, 0.5, 0.02, 9)
    cand = np.concatenate([[centre], np.random.default_rng(5).integers(0, mixed.size, 7)]).astype(np.int64)
    exp = vref.gain(mixed, cand, 32, HD, *FOVS[0])
    assert exp["counters"][2] > 1000 and exp["counters"][3] > 1000
    _same(_gain_device(_dev(mixed), cand, 32, HD, *FOVS[0]), exp, "mixed")


def test_gain_with_other_headings_and_no_candidate():
    state = vref.three_state((7, 8, 9), 0.5, 0.1, 3)
    st = _dev(state)
    cand = np.arange(0, state.size, 5, dtype=np.int64)
    axes = np.array([(1, 0, 0), (3, -2, 1), (0, 0, -7), (1024, 1024, -1024), (1, 1, 0), (-1, -1, 0)] + [(1, 2, 3)] * 26)
    assert len(axes) == 32
    for num, den in ((1 << 19, 1 << 20), (3, 4), (0, 1), (1, 1), ((1 << 31) - 2, (1 << 31) - 1)):
        _same(_gain_device(st, cand, 5, axes, num, den), vref.gain(state, cand, 5, axes, num, den), (num, den))
    _same(_gain_device(st, cand, 5, axes[:1], 1, 2), vref.gain(state, cand, 5, axes[:1], 1, 2), "one heading")
    got = _gain_device(st, [], 5, HD, *FOVS[0])
    assert got["counters"] == [0, 0, 0, 0] and got["gain"].shape == (0, 26)
    got = _gain_device(st, [-1, state.size, 1 << 40], 5, HD, *FOVS[0])
    assert got["counters"] == [0, 0, 0, 0] and got["best"].tolist() == [-1] * 3 and not got["gain"].any()
    assert got["visible"].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 2. the candidates
def _candidates_device(dist, origin, stride, max_cost, cap):
    from pi3_slam_amd import ops
    cells = torch.full((cap,), POISON64, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_candidates(dist, origin, stride, max_cost, cells, count)
    return cells.cpu().numpy(), int(count.item())


def test_candidates_match_the_oracle():
    shape = (20, 9, 17)
    rng = np.random.default_rng(4)
    dist_np = rng.integers(0, 400, shape).astype(np.uint32)
    dist_np[rng.random(shape) < 0.3] = vref.FAR
    dist = _dev(dist_np.view(np.int32))
    for origin in ((0, 0, 0), (-5, 3, -1), (-1000003, 7, -8)):
        for stride in (1, 3, 4):
            for max_cost in (vref.FAR - 1, 200, 0):
                exp = vref.candidates(dist_np, origin, stride, max_cost)
                K = len(exp)
                got, count = _candidates_device(dist, origin, stride, max_cost, K + 3)
                assert count == K and sorted(got[:K].tolist()) == exp.tolist() and (got[K:] == POISON64).all()
                for cap in {0, 1, max(K - 1, 0)}:
                    got, count = _candidates_device(dist, origin, stride, max_cost, cap)
                    w = min(cap, K)                             # the slots written; the rest keeps the poison
                    assert count == K and len(set(got[:w].tolist())) == w and set(got[:w].tolist()) <= set(exp.tolist())
                    assert (got[w:] == POISON64).all()
            assert len(vref.candidates(dist_np, origin, stride)) >= 20
    # more than one workgroup, and a cost of the far mark never passes
    big = np.zeros((30, 31, 33), np.uint32)
    big[::2] = vref.FAR
    got, count = _candidates_device(_dev(big.view(np.int32)), (1, -2, 3), 1, 1 << 40, big.size)
    assert count == 15 * 31 * 33 and sorted(got[:count].tolist()) == vref.candidates(big, (1, -2, 3), 1).tolist()


def test_argument_errors_launch_nothing():
    import ctypes
    from pi3_slam_amd import lib as L
    lib = L.load()
    shape = (3, 4, 5)
    state = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    dist = torch.zeros(shape, dtype=torch.int32, device=DEV)
    cells = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    count = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
    cand = torch.zeros(2, dtype=torch.int64, device=DEV)
    gain = torch.full((2, 2), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((2,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    sp = L.stream_ptr()
    s, d, ce, co, ca, g, v, b, c = (t.data_ptr() for t in (state, dist, cells, count, cand, gain, visible, best, counters))
    axes = lambda *a: (ctypes.c_int * len(a))(*a)               # noqa: E731
    hd = axes(1, 0, 0, 0, 0, -1)
    big = (513, 261633, 1)                                      # 2^27 + 1 cells, every dimension below 2^21
    far = vref.FAR
    calls = [lambda: lib.pi3_grid_view_candidates(None, 5, 4, 3, 0, 0, 0, 4, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, 4, far, None, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, 4, far, ce, 8, None, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, 4, far, ce, -1, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, 0, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, -4, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 3, 0, 0, 0, 4, -1, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 0, 4, 3, 0, 0, 0, 4, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, 5, 4, 1 << 21, 0, 0, 0, 4, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_candidates(d, *big, 0, 0, 0, 4, far, ce, 8, co, sp),
             lambda: lib.pi3_grid_view_gain(None, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, None, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, None, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, None, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, None, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, None, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, None, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, -1, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 0, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 33, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 0, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, axes(*([1, 0, 0] * 33)), 33, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, axes(1, 0, 0, 0, 0, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, axes(1, 0, 0, 0, 1025, 0), 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 0, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, -2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 1, 1 << 31, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, -1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, 4, 3, ca, 2, 4, hd, 2, 3, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, 5, -4, 3, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp),
             lambda: lib.pi3_grid_view_gain(s, *big, ca, 2, 4, hd, 2, 1, 2, g, v, b, c, sp)]
    names = [b"candidates"] * 10 + [b"gain"] * 21
    assert len(calls) == len(names)
    for i, (call, name) in enumerate(zip(calls, names)):
        assert call() == -1, i
        err = lib.pi3_last_error()
        assert err.startswith(b"pi3_grid_view_" + name + b":") and b"2^27" in err, (i, err)
    torch.cuda.synchronize()
    assert cells.tolist() == [POISON64] * 8 and count.tolist() == [POISON64] and counters.tolist() == [POISON64] * 4
    assert bool((gain == POISON32).all()) and bool((visible == POISON32).all()) and bool((best == POISON32).all())


# ------------------------------------------------------------------------------------------------ 3. the box room
BOX_RANGE_CELLS = 8


def test_box_room_through_the_planner():
    from pi3_slam_amd.dense_map import OccupancyGrid
    from pi3_slam_amd.view_planner import ViewPlanner
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    walk_a = rref.walk_mask(state, d2a, min_d2)
    dist_a = rref.distances(walk_a, lin)
    planner = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4, 10)
    Rv, sep, max_cost = planner.cells_of(cell)
    assert (Rv, sep, max_cost) == (BOX_RANGE_CELLS, 4, vref.FAR - 1)
    exp = vref.view_set(state, dist_a, origin, Rv, 4, 90, 10, sep)
    found = planner.find(grid, centres, DEV)
    c = found.counts
    print(f"box room: {c}")
    assert c["candidates"] == 230 and c["reachable"] == 15896 and c["best_gain"] == 316
    assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == exp["gain"]["counters"]
    assert c["views"] == len(exp["views"]) == len(found.views) and c["low_gain"] == exp["low_gain"]
    assert found.gain.dtype == np.int32 and found.gain.tobytes() == exp["gain_map"].tobytes()
    assert found.heading.dtype == np.int8 and found.heading.tobytes() == exp["heading_map"].tobytes()
    assert found.field.cost.tobytes() == dist_a.tobytes() and found.headings.tolist() == HD.tolist()
    assert found.settings["cos2_num"] == 1 << 19 and found.settings["cos2_den"] == 1 << 20
    assert found.settings["range_cells"] == 8 and found.settings["router"]["approach_unknown"] is True
    for rank, (got, e) in enumerate(zip(found.views, exp["views"])):
        assert (got.rank, got.cell, got.heading, got.gain, got.visible, got.cost) == (
            rank, e["cell"], e["heading"], e["gain"], e["visible"], e["cost"])
        assert got.axis.tolist() == e["axis"] and got.distance_m == cell * got.cost / 12.0
        k = got.cell
        assert got.position.tolist() == (cell * (origin + np.array([k % nx, (k // nx) % ny, k // (nx * ny)]) + 0.5)).tolist()
        assert abs(float((got.direction ** 2).sum()) - 1.0) < 1e-12 and (np.sign(got.direction) == np.sign(got.axis)).all()
    first = found.views[0]
    assert (first.cell % nx, (first.cell // nx) % ny, first.cell // (nx * ny)) == (21, 13, 9)
    assert first.axis.tolist() == [1, 1, -1] and first.gain == 316
    route = found.route_to(0)
    assert route.cells.tolist()[-1] == first.cell and route.cost == first.cost == int(dist_a.reshape(-1)[first.cell])
    assert dist_a.reshape(-1)[route.cells[0]] == 0 and route.waypoints[-1].tolist() == first.position.tolist()
    with pytest.raises(ValueError, match=f"no view of rank {len(found.views)}"):
        found.route_to(len(found.views))
    # a short candidate buffer asks again; a distance limit and a gain limit drop candidates
    small = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4, 3, max_distance_m=1.0, min_gain=200)
    small.CANDIDATES_FIRST_CAP = 7
    near = small.find(grid, centres, DEV)
    e2 = vref.view_set(state, dist_a, origin, Rv, 4, 90, 3, sep, 200, 120)
    assert near.settings["max_cost"] == 120 and 7 < near.counts["candidates"] == len(e2["cells"]) < 230
    assert [(v.cell, v.heading, v.gain) for v in near.views] == [(v["cell"], v["heading"], v["gain"]) for v in e2["views"]]
    assert near.counts["low_gain"] == e2["low_gain"] > 0 and len(near.views) == 3


# ------------------------------------------------------------------------------------------------ 4. end to end
OCC_CELL, ROUTE_RADIUS = 0.1, 0.1


@pytest.fixture(scope="module")
def reconstructed(tmp_path_factory):
    import synth_sequence as ss
    import test_dense_follow_gpu as follow_gpu
    tmp = tmp_path_factory.mktemp("views")
    seq = ss.SyntheticSequence(follow_gpu.GT, noise=dict(ss.NOISE_NONE), **dict(follow_gpu.SCENE, n_frames=50))
    assert len(seq.chunks) == 2
    follow_gpu._create(seq, str(tmp / "chunks"))
    follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "rec"), bundle_adjust=False, occupancy_cell=OCC_CELL)
    return tmp


def test_cli_views_on_a_reconstruction(reconstructed, capsys):
    from pi3_slam_amd import cli, export, map_eval
    from pi3_slam_amd.grid_route import GridRouter, read_tum_positions
    tmp = reconstructed
    occ, tum = str(tmp / "rec" / "occupancy.npz"), str(tmp / "rec" / "trajectory_tum.txt")
    grid = export.read_occupancy(occ)
    shape = grid.state.shape
    src = GridRouter.linear(GridRouter.world_cells(read_tum_positions(tum), grid), shape)
    d2 = oref.edt_ref(grid.state, 1, False)
    dist = rref.distances(rref.walk_mask(grid.state, d2, 1), src)
    exp = vref.view_set(grid.state, dist, grid.index_origin, 8, 2, 90, 5, 4)
    capsys.readouterr()
    cli.main(["views", "--occupancy", occ, "--output", str(tmp / "v"), "--from-trajectory", tum, "--radius",
              str(ROUTE_RADIUS), "--range", "0.8", "--stride", "2", "--count", "5", "--route-to", "0", "--device", DEV])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("views: ")]
    rec = json.load(open(tmp / "v" / "views.json"))
    counts = rec["counts"]
    assert len(exp["views"]) >= 1 and len(exp["cells"]) >= 10
    assert [(v["cell"], v["heading"], v["axis"], v["gain"], v["visible"], v["cost"]) for v in rec["views"]] == [
        (e["cell"], e["heading"], e["axis"], e["gain"], e["visible"], e["cost"]) for e in exp["views"]]
    assert [v["rank"] for v in rec["views"]] == list(range(len(exp["views"])))
    assert [counts[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == exp["gain"]["counters"]
    assert rec["settings"]["range_cells"] == 8 and rec["settings"]["stride"] == 2 and rec["settings"]["radius"] == ROUTE_RADIUS
    with np.load(tmp / "v" / "views.npz") as z:
        assert z["gain"].tobytes() == exp["gain_map"].tobytes() and z["gain"].shape == shape
        assert z["heading"].tobytes() == exp["heading_map"].tobytes() and z["headings"].tolist() == HD.tolist()
        assert z["index_origin"].tolist() == grid.index_origin.tolist() and float(z["cell"]) == OCC_CELL
    best = rec["views"][0]
    assert len(line) == 1 and f"views: {counts['candidates']} candidates, {counts['rays']} rays" in line[0]
    assert f"{counts['views']} views kept" in line[0] and f"the best: {best['gain']} cells at {best['distance_m']:.3f} m" in line[0]
    print(line[0])
    assert len(map_eval.read_ply_points(str(tmp / "v" / "views.ply"))[0]) == counts["views"]
    assert sorted(os.listdir(tmp / "v")) == ["route.json", "route.npz", "route.ply", "views.json", "views.npz", "views.ply"]
    way = json.load(open(tmp / "v" / "route.json"))
    assert way["cost"] == best["cost"] and way["waypoints"][-1] == best["position"]
    assert way["settings"]["approach_unknown"] is True
    with pytest.raises(SystemExit, match="views: no view of rank 99"):
        cli.main(["views", "--occupancy", occ, "--output", str(tmp / "w"), "--from-trajectory", tum, "--range", "0.8",
                  "--route-to", "99", "--device", DEV])
    with pytest.raises(SystemExit, match="views: a range of 4.0 at cells of 0.1 is 40 cells: at most 32"):
        cli.main(["views", "--occupancy", occ, "--output", str(tmp / "w"), "--from-trajectory", tum, "--range", "4.0",
                  "--device", DEV])
