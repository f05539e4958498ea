"""Unknown space that ends a ray, on the GPU (csrc/grid_view.hip: pi3_grid_view_gain_depth, pi3_grid_view_mark_depth),
byte for byte against tests/grid_view_depth_ref.py, against the transparent entry points at depth 255, and through the
planner, the tour and the command line.  Every output is filled with a poison value before each call, and every mask
has two guard words behind it.  Near ranges 31 and 32 and far ranges 33 and 64 lie on both sides of the 64 KB of LDS a
kernel has without asking, so the opt-in is exercised."""
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
import grid_view_depth_ref as dref          # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_cover_gpu as cover_gpu     # noqa: E402  (its guarded mask)
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_far_gpu as far_gpu    # noqa: E402  (its calls of the transparent entry points)
import test_grid_view_gpu as view_gpu       # noqa: E402  (its candidates and comparison)

pytestmark = pytest.mark.gpu
DEV = view_gpu.DEV
POISON32, POISON64, POISON16 = view_gpu.POISON32, view_gpu.POISON64, cover_gpu.POISON16
HD = vref.headings26()
F90 = vref.cos2(90)
Mask = cover_gpu.Mask
_dev = view_gpu._dev
_same = view_gpu._same
DEPTHS = (0, 1, 2, 5)
SMALL = (20, 9, 70)                         # test_grid_view_far_gpu's grid and candidates
SMALL_CAND = [0, 69, 6615, 12599]


def _gain(state, cand, R, depth, far=False, mask=None, headings=HD):
    """ops.grid_view_gain, or with a mask ops.grid_view_gain_unseen, at unknown_depth = depth into poisoned outputs."""
    from pi3_slam_amd import ops
    V, H = len(cand), len(headings)
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    cells = _dev(np.asarray(cand, np.int64))
    if mask is None:
        ops.grid_view_gain(state, cells, R, headings, *F90, gain, visible, best, counters, far=far, unknown_depth=depth)
    else:
        before = mask.host()
        ops.grid_view_gain_unseen(state, mask.words, cells, R, headings, *F90, gain, visible, best, counters, far=far,
                                  unknown_depth=depth)
        assert mask.host().tobytes() == before.tobytes()        # read only
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _mark(state, mask, cells, heading_of, R, depth, owner=None, tag=0, far=False):
    from pi3_slam_amd import ops
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_mark(state, mask.words, _dev(np.asarray(cells, np.int64)), heading_of, R, HD, *F90, counters, owner, tag,
                       far=far, unknown_depth=depth)
    return counters.tolist()


def _rising(figures, transparent):
    """The depths tell: each sees strictly more than the one before and less than the transparent rule."""
    assert all(a < b for a, b in zip(figures, figures[1:])) and figures[-1] < transparent, (figures, transparent)


def _edge_candidates(shape):
    """The 8 corners, the 6 face centres, a cell inside, and one index on either side of [0, cells)."""
    nz, ny, nx = shape
    lin = lambda z, y, x: (z * ny + y) * nx + x                 # noqa: E731
    corners = [lin(z, y, x) for z in sorted({0, nz - 1}) for y in sorted({0, ny - 1}) for x in sorted({0, nx - 1})]
    faces = [lin(0, ny // 2, nx // 2), lin(nz - 1, ny // 2, nx // 2), lin(nz // 2, 0, nx // 2),
             lin(nz // 2, ny - 1, nx // 2), lin(nz // 2, ny // 2, 0), lin(nz // 2, ny // 2, nx - 1)]
    return np.array(sorted(set(corners + faces)) + [lin(nz // 2, ny // 2, nx // 3), -1, nz * ny * nx], np.int64)


# ------------------------------------------------------------------------------------------------ 1. the gain
@pytest.mark.parametrize("dims,R", [((9, 8, 7), 1), ((9, 8, 7), 8), ((17, 9, 20), 8), ((17, 9, 20), 31), ((17, 9, 20), 32)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "R%d" % v)
def test_near_gain_matches_the_oracle(dims, R):
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.02 if R > 1 else 0.1, 5)
    st = _dev(state)
    cand = _edge_candidates(state.shape)                        # corners, faces, one inside, two outside
    if R <= 8:
        cand = np.concatenate([view_gpu._candidates(dims, sum(dims)), cand])
    plain = vref.gain(state, cand, R, HD, *F90)
    seen = []
    for depth in DEPTHS:
        exp = dref.gain(state, cand, R, depth, HD, *F90)
        got = _gain(st, cand, R, depth)
        _same(got, exp, (dims, R, depth))
        assert got["counters"][1] == plain["counters"][1] and got["counters"][0] == plain["counters"][0]
        seen.append(got["counters"][3])
    print(dims, R, seen, plain["counters"])
    if R > 1:
        _rising(seen, plain["counters"][3])
    else:
        assert seen == [plain["counters"][3]] * 4 > [0] * 4    # nothing lies between neighbours


# The oracle's visible rays per depth on the SMALL grid, and under the transparent rule (at 64 cells the figure
# test_grid_view_far_gpu.TABLE pins): a case per depth keeps each one short, and the table shows that the depths tell.
FAR_SEEN = {8: None, 33: ((444, 1388, 2814, 9328), 41666), 64: ((95, 293, 568, 1847), 9247)}


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("R", [8, 33, 64])
def test_far_gain_matches_the_oracle(R, depth):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    cand = np.concatenate([SMALL_CAND, _edge_candidates(SMALL)]) if R < 64 else np.array(
        SMALL_CAND + [-1, state.size], np.int64)                # two corners, a face, the last cell, two outside
    exp = dref.gain(state, cand, R, depth, HD, *F90)
    got = _gain(_dev(state), cand, R, depth, far=True)
    print(R, depth, got["counters"])
    _same(got, exp, (R, depth))
    if FAR_SEEN[R] is None:
        seen = [dref.gain(state, cand, R, d, HD, *F90)["counters"][3] for d in DEPTHS]
        _rising(seen, vref.gain(state, cand, R, HD, *F90)["counters"][3])
    else:
        figures, transparent = FAR_SEEN[R]
        _rising(list(figures), transparent)
        assert exp["counters"][3] == figures[DEPTHS.index(depth)]


@pytest.mark.parametrize("shape,R,far", [((1, 70, 70), 32, False), ((1, 70, 70), 33, True), ((70, 1, 70), 33, True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_flat_grids(shape, R, far):
    state = vref.three_state(shape, 0.5, 0.02, sum(shape))
    cand = _edge_candidates(shape)
    seen = []
    for depth in (0, 2, 5):
        exp = dref.gain(state, cand, R, depth, HD, *F90)
        _same(_gain(_dev(state), cand, R, depth, far=far), exp, (shape, depth))
        seen.append(exp["counters"][3])
    _rising(seen, vref.gain(state, cand, R, HD, *F90)["counters"][3])


# ------------------------------------------------------------------------------------------------ 2. depth 255
@pytest.mark.parametrize("R,far", [(8, False), (32, False), (8, True), (33, True), (64, True)])
def test_depth_255_gives_the_transparent_bytes(R, far):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    st = _dev(state)
    cand = np.concatenate([SMALL_CAND, [6000, 3333, -1]]).astype(np.int64)
    plain = far_gpu._gain(st, cand, R, HD, *F90, far=far)
    assert plain["counters"][2] > 100 and plain["counters"][3] > 100
    _same(_gain(st, cand, R, 255, far=far), plain, (R, far, "gain"))
    _same(_gain(st, cand, R, 110, far=far), plain, (R, far, "gain at 110"))
    words = cref.pack(np.random.default_rng(R).random(state.size) < 0.5)
    plain = far_gpu._gain(st, cand, R, HD, *F90, far=far, mask=Mask(state.size, words))
    _same(_gain(st, cand, R, 255, far=far, mask=Mask(state.size, words)), plain, (R, far, "unseen"))
    hof = [3, -1, 25, 13, 0, -1, 7]
    a, b = Mask(state.size, words), Mask(state.size, words)
    assert _mark(st, b, cand, hof, R, 255, far=far) == far_gpu._mark(st, a, cand, hof, R, HD, *F90, far=far)
    assert a.host().tobytes() == b.host().tobytes() != words.tobytes()


# ------------------------------------------------------------------------------------------------ 3. unseen and mark
@pytest.mark.parametrize("R,far,depth", [(8, False, 1), (32, False, 2), (33, True, 1), (64, True, 5)])
def test_unseen_and_mark(R, far, depth):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    st = _dev(state)
    cand = np.array(SMALL_CAND + [6000, -1], np.int64)
    casts = dref.cast_depth(state, cand, R, depth)
    rng = np.random.default_rng(R + depth)
    # the unseen gain: a zero mask gives the plain depth bytes, a half-set one the oracle's
    plain = _gain(st, cand, R, depth, far=far)
    _same(_gain(st, cand, R, depth, far=far, mask=Mask(state.size)), plain, "zero mask")
    words = cref.pack(rng.random(state.size) < 0.5)
    exp = cref.gain_unseen(state, words, cand, R, HD, *F90, casts=casts)
    assert 0 < exp["counters"][1] < plain["counters"][1] and exp["counters"][3] > 50 and exp["counters"][2] > 50
    _same(_gain(st, cand, R, depth, far=far, mask=Mask(state.size, words)), exp, "half-set mask")
    # marks: any heading, and a heading per row (mixed, -1 among them)
    for hof in ([-1] * 6, [25, -1, 13, 0, 7, 3]):
        words = cref.pack(rng.random(state.size) < 0.2)
        mask = Mask(state.size, words)
        exp = cref.mark(state, words, cand, hof, R, HD, *F90, casts=casts)
        assert _mark(st, mask, cand, hof, R, depth, far=far) == exp["counters"] and exp["counters"][4] > 50
        assert mask.host().tobytes() == words.tobytes() and int(exp["new"].sum()) == exp["counters"][4]
    # one row with an owner
    words = cref.pack(rng.random(state.size) < 0.2)
    mask = Mask(state.size, words)
    owner_np = np.full(state.shape, POISON16, np.int16)
    owner = _dev(owner_np)
    one = dref.cast_depth(state, cand[2:3], R, depth)
    exp = cref.mark(state, words, cand[2:3], [13], R, HD, *F90, owner_np, 77, casts=one)["counters"]
    assert _mark(st, mask, cand[2:3], [13], R, depth, owner, 77, far=far) == exp and exp[4] > 20
    assert mask.host().tobytes() == words.tobytes() and owner.cpu().numpy().tobytes() == owner_np.tobytes()
    # rows that race for the same cells: neighbours looking the same way, and one row twice
    rows = np.array([cand[2], cand[2] + 1, cand[2] + 70, cand[2], cand[2] + 71], np.int64)
    hof = [13, 13, -1, 13, -1]
    words = np.zeros(cref.seen_words(state.size), np.uint32)
    mask = Mask(state.size)
    exp = cref.mark(state, words, rows, hof, R, HD, *F90, casts=dref.cast_depth(state, rows, R, depth))
    got = _mark(st, mask, rows, hof, R, depth, far=far)
    assert got == exp["counters"] and got[3] > got[4] == int(exp["new"].sum()) == cref.popcount(mask.host()) > 50
    assert mask.host().tobytes() == words.tobytes()


def test_no_candidate_launches_nothing_and_zeroes_the_counters():
    state = _dev(vref.three_state((7, 8, 9), 0.5, 0.1, 3))
    got = _gain(state, [], 4, 1)
    assert got["counters"] == [0, 0, 0, 0]
    mask = Mask(7 * 8 * 9)
    assert _mark(state, mask, [], [], 4, 1) == [0, 0, 0, 0, 0] and not mask.host().any()


# ------------------------------------------------------------------------------------------------ 4. planner, tour, cli
BOX_RANGE_CELLS = 8


def _box_room():
    from pi3_slam_amd.dense_map import OccupancyGrid
    room, state, cams, d2u, walk_u, (Rb, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    grid = OccupancyGrid(state, origin, cell)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    dist = rref.distances(rref.walk_mask(state, oref.edt_ref(state, Rb, False), min_d2), lin)
    return state, grid, centres, dist, cell, origin


def _views(found):
    return [(v.cell, v.heading, v.gain, v.visible, v.cost) for v in found.views]


def test_box_room_through_the_planner_and_the_tour():
    from pi3_slam_amd.view_planner import ViewPlanner
    state, grid, centres, dist, cell, origin = _box_room()
    args = (route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, 90, 4)
    planner = ViewPlanner(*args, 10, unknown_depth=1)
    R, sep, _ = planner.cells_of(cell)
    assert R == BOX_RANGE_CELLS
    # find
    exp = dref.view_set(state, dist, origin, R, 1, 4, 90, 10, sep)
    found = planner.find(grid, centres, DEV)
    c = found.counts
    print(f"box room at depth 1: {c}")
    assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == exp["gain"]["counters"]
    assert found.gain.tobytes() == exp["gain_map"].tobytes() and found.heading.tobytes() == exp["heading_map"].tobytes()
    assert _views(found) == [(e["cell"], e["heading"], e["gain"], e["visible"], e["cost"]) for e in exp["views"]]
    assert len(found.views) >= 3 and c["low_gain"] == exp["low_gain"]
    assert found.settings["unknown_depth"] == 1 and found.settings["unknown_is_transparent"] is False
    plain = vref.view_set(state, dist, origin, R, 4, 90, 10, sep)
    assert exp["gain"]["counters"][3] < plain["gain"]["counters"][3] and exp["gain_map"].tobytes() != plain["gain_map"].tobytes()
    # cover
    cand = vref.candidates(dist, origin, 4)
    cost = dist.reshape(-1)[cand].astype(np.int64)
    full = dref.cover(state, cand, cost, R, 1, HD, *F90, count=4)
    four = ViewPlanner(*args, 4, unknown_depth=1).cover(grid, centres, DEV)
    assert [(v.cell, v.heading, v.gain) for v in four.views] == full["picks"] and len(full["picks"]) == 4
    assert [v.new for v in four.views] == full["new"] and [v.covered for v in four.views] == full["covered"]
    assert [v.visible for v in four.views] == full["visible"] and four.counts["seeable"] == full["seeable"]
    assert four.seen_by.tobytes() == full["seen_by"].tobytes() and four.settings["unknown_depth"] == 1
    assert full["seeable"] < cref.cover(state, cand, cost, R, HD, *F90, count=1)["seeable"]
    # the tour replays the marks in its own order, by the same rule
    tour = four.tour()
    order = [r for stop in tour.stops for r in stop.ranks]
    assert sorted(order) == [0, 1, 2, 3] and tour.settings["unknown_depth"] == 1
    replay = dref.replay(state, [(four.views[r].cell, four.views[r].heading) for r in order], R, 1, HD, *F90)
    assert [n for stop in tour.stops for n in stop.tour_new] == replay
    assert tour.covered == sum(replay) == full["covered"][-1]
    if order != [0, 1, 2, 3]:                                   # in another order the shares differ, the sum does not
        assert replay != full["new"]


def test_box_room_through_the_far_planner():
    from pi3_slam_amd.view_planner import ViewPlanner
    state, grid, centres, dist, cell, origin = _box_room()
    planner = ViewPlanner(route_cases.BOX_RADIUS, (33 - 0.1) * cell, 90, 8, 10, far=True, unknown_depth=1)
    R, sep, _ = planner.cells_of(cell)
    assert R == 33
    exp = dref.view_set(state, dist, origin, R, 1, 8, 90, 10, sep)
    found = planner.find(grid, centres, DEV)
    c = found.counts
    assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == exp["gain"]["counters"]
    assert _views(found) == [(e["cell"], e["heading"], e["gain"], e["visible"], e["cost"]) for e in exp["views"]]
    assert len(found.views) >= 1 and found.settings["far"] is True and found.settings["unknown_depth"] == 1


def _files(folder):
    """What a run wrote, comparable between runs: text files by their bytes, archives by their arrays."""
    out = {}
    for name in sorted(os.listdir(folder)):
        path = os.path.join(folder, name)
        if name.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                out[name] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
        else:
            out[name] = open(path, "rb").read()
    return out


def test_cli_views_with_and_without_the_flag(tmp_path, capsys):
    from pi3_slam_amd import cli, export
    state, grid, centres, dist, cell, origin = _box_room()
    occ = str(tmp_path / "occupancy.npz")
    export.write_occupancy(grid, occ)
    base = ["views", "--occupancy", occ, "--start"] + [repr(float(v)) for v in centres[0]] + [
        "--radius", str(route_cases.BOX_RADIUS), "--range", repr(BOX_RANGE_CELLS * cell), "--count", "4", "--cover", "--tour",
        "--device", DEV]
    capsys.readouterr()
    cli.main(base + ["--output", str(tmp_path / "d1"), "--unknown-depth", "1"])
    assert "rays end after 1 unknown cells" in capsys.readouterr().out
    rec = json.load(open(tmp_path / "d1" / "views.json"))
    assert rec["settings"]["unknown_depth"] == 1 and rec["settings"]["unknown_is_transparent"] is False
    assert json.load(open(tmp_path / "d1" / "tour.json"))["settings"]["unknown_depth"] == 1
    # without the flag: no new key, the same files run after run, and the views depth 255 picks
    cli.main(base + ["--output", str(tmp_path / "a")])
    assert "rays end after" not in capsys.readouterr().out
    cli.main(base + ["--output", str(tmp_path / "b")])
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert a == b and {"views.json", "views.npz", "views.ply", "tour.json", "tour.npz", "tour.ply"} <= set(a)
    plain = json.loads(a["views.json"])
    assert "unknown_depth" not in plain["settings"] and plain["settings"]["unknown_is_transparent"] is True
    assert b"unknown_depth" not in a["views.json"] and b"unknown_depth" not in a["tour.json"]
    cli.main(base + ["--output", str(tmp_path / "t"), "--unknown-depth", "255"])
    deep = json.load(open(tmp_path / "t" / "views.json"))
    assert deep["views"] == plain["views"] != rec["views"]
    assert _files(tmp_path / "t")["views.ply"] == a["views.ply"]
    with pytest.raises(SystemExit, match="views: unknown_depth must be an integer in 0 .. 255"):
        cli.main(base + ["--output", str(tmp_path / "w"), "--unknown-depth", "256"])
    assert not os.path.exists(tmp_path / "w")
