"""Routes for a body that stands on the GPU (csrc/grid_stand.hip and route_init_stand_kernel of grid_route.hip), byte for
byte against the oracle (tests/grid_stand_ref.py): the height scan in all six directions, the standing init, the
floor-following candidates, a wall with a door and a window, a staircase, the box room through the view planner, and
`cli views --stand`.  Every output is filled with a poison value before each call."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_frontier_ref as fref            # noqa: E402
import grid_route_ref as rref               # noqa: E402
import grid_sight_ref as sref               # noqa: E402
import grid_stand_ref as ref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON8, POISON32, POISON64 = 7, -5, 11


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _height_device(state, up_axis, up_sign, through_unknown):
    from pi3_slam_amd import ops
    st = _dev(state)
    out = torch.full(st.shape, POISON8, dtype=torch.uint8, device=DEV)
    ops.grid_stand_height(st, up_axis, up_sign, through_unknown, out)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. height
def _states(shape):
    slab = np.ones(shape, np.uint8)                 # one occupied cell in from every face: long runs above a floor
    for ax in range(3):
        if shape[ax] > 2:
            sl = [slice(None)] * 3
            sl[ax] = 1
            slab[tuple(sl)] = 2
            sl[ax] = shape[ax] - 2
            slab[tuple(sl)] = 2
    return {"occupied 0.05": ref.random_state(shape, 0.05, 1), "occupied 0.3": ref.random_state(shape, 0.3, 2),
            "free": np.ones(shape, np.uint8), "occupied": np.full(shape, 2, np.uint8), "unknown": np.zeros(shape, np.uint8),
            "slab": slab}


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 300), (1, 300, 2), (300, 2, 3), (9, 8, 7), (65, 67, 66)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_height_matches_the_oracle_in_all_six_directions(shape):
    for name, state in _states(shape).items():
        for up_axis, up_sign in ref.UPS:
            for tu in (False, True):
                exp = ref.height(state, up_axis, up_sign, tu)
                got = _height_device(state, up_axis, up_sign, tu)
                assert got.tobytes() == exp.tobytes(), (name, up_axis, up_sign, tu, np.argwhere(got != exp)[:4].tolist())
    if max(shape) == 300:                           # the 255 mark is reached along the long axis
        k = 2 - shape.index(300)
        far = ref.height(np.ones(shape, np.uint8), k, 1)
        assert (far == 255).sum() == (300 - 254) * (np.prod(shape) // 300) and (far == 0).sum() == 254 * (np.prod(shape) // 300)


def test_height_of_rows_that_cross_several_waves_segments():
    """x rows of 700 cells: eleven 64-cell chunks, three segments of four; stops placed so that the carry is looked for
    one, two, three and four chunks back and at the border, for both signs."""
    state = np.ones((2, 3, 700), np.uint8)
    state[0, 0, 255] = 2                            # the segment at 256 finds it in the chunk before, at the last lane
    state[0, 1, 0] = 2                              # 255 cells before 256: beyond the four chunks
    state[0, 1, 258] = 0                            # an unknown stop inside the second segment
    state[0, 2, 130] = 2                            # two chunks back
    state[0, 2, 699] = 2                            # -x: the border chunk is a part chunk with a stop in its last lane
    state[1, 0, 3] = 0                              # kinds: unknown first, then occupied further down
    state[1, 0, 1] = 2
    state[1, 1, 511] = 2                            # exactly at a segment's end
    state[1, 1, 512] = 0
    state[1, 2, 64] = 2                             # three chunks back from 256
    for up_sign in (1, -1):
        for tu in (False, True):
            exp = ref.height(state, 0, up_sign, tu)
            got = _height_device(state, 0, up_sign, tu)
            assert got.tobytes() == exp.tobytes(), (up_sign, tu, np.argwhere(got != exp)[:4].tolist())
    assert set(np.unique(ref.height(state, 0, 1))) >= {0, 1, 254, 255}


# ------------------------------------------------------------------------------------------------ 2. the standing init
def _init_device(state, d2, min_d2, through_unknown, height, band, sources):
    from pi3_slam_amd import ops
    st = _dev(state)
    walk = torch.full(st.shape, POISON8, dtype=torch.uint8, device=DEV)
    dist = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_init_stand(st, None if d2 is None else _dev(np.asarray(d2, np.uint16).view(np.int16)), min_d2,
                              through_unknown, _dev(height), band[0], band[1],
                              _dev(np.asarray(sources, np.int64).reshape(-1)), walk, dist, counters)
    return walk.cpu().numpy(), _u32(dist), counters.tolist()


@pytest.mark.parametrize("through_unknown", [False, True])
@pytest.mark.parametrize("with_d2", [False, True])
@pytest.mark.parametrize("band", [(1, 1), (3, 5), (1, 254)], ids=lambda b: "%d..%d" % b)
def test_init_stand_matches_the_oracle(band, with_d2, through_unknown):
    shape = (12, 9, 67)
    state = ref.random_state(shape, 0.1, 4)
    state[0] = 2                                    # a floor under everything, so that plenty of cells stand
    assert {0, 1, 2} == set(np.unique(state).tolist())
    d2 = oref.edt_ref(state, 2, not through_unknown) if with_d2 else None
    min_d2 = (1 if band == (1, 1) else 2) if with_d2 else 0      # right above a floor d2 is 1
    h = ref.height(state, 2, 1, through_unknown)
    w = ref.walk_stand(state, h, *band, d2, min_d2, through_unknown).reshape(-1)
    plain = rref.walk_mask(state, d2, min_d2, through_unknown).reshape(-1)
    on, off_band = np.flatnonzero(w), np.flatnonzero((plain != 0) & (w == 0))
    occupied = np.flatnonzero(state.reshape(-1) == 2)
    assert len(on) > 8 and (len(off_band) > 3 or band == (1, 254))
    blocked = [off_band[0], off_band[2], off_band[2]] if len(off_band) > 3 else [occupied[0], occupied[1], occupied[1]]
    sources = [on[0], on[5], on[5], on[-1]] + blocked + [occupied[3], -1, state.size, state.size + 7, -(1 << 40), 1 << 40]
    for src in (sources, [], [on[1]]):
        exp = ref.init_stand(state, d2, min_d2, through_unknown, h, *band, src)
        walk, dist, counters = _init_device(state, d2, min_d2, through_unknown, h, band, src)
        assert walk.tobytes() == exp["walk"].tobytes() and dist.tobytes() == exp["dist"].tobytes()
        assert counters == exp["counters"], (counters, exp["counters"])
    exp = ref.init_stand(state, d2, min_d2, through_unknown, h, *band, sources)
    assert exp["counters"][1:4] == [4, 4, 5] and exp["counters"][0] == len(on) and exp["counters"][4] == len(off_band)


def test_the_widest_band_over_a_floored_grid_is_the_plain_init():
    from pi3_slam_amd import ops
    state = ref.random_state((10, 9, 70), 0.0, 6)   # free and unknown cells only
    state[:, -1, :] = 2                             # up = -y: the floor is the last row, and through unknown space every
    h = ref.height(state, 1, -1, True)              # cell above it has one
    src = [3, 4, state.size - 1]
    walk, dist, counters = _init_device(state, None, 0, True, h, (1, 254), src)
    st = _dev(state)
    pw = torch.full(st.shape, POISON8, dtype=torch.uint8, device=DEV)
    pd = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    pc = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_route_init(st, None, 0, True, _dev(np.asarray(src, np.int64)), pw, pd, pc)
    assert walk.tobytes() == pw.cpu().numpy().tobytes() and dist.tobytes() == _u32(pd).tobytes()
    assert counters == pc.tolist() + [0] and counters[0] == int((state != 2).sum())


# ------------------------------------------------------------------------------------------------ 3. candidates
@pytest.mark.parametrize("stride", [1, 3, 4])
def test_candidates_stand_match_the_oracle(stride):
    from pi3_slam_amd import ops
    rng = np.random.default_rng(8)
    shape = (20, 23, 70)
    for up_axis, up_sign in ref.UPS:
        state = np.ones(shape, np.uint8)
        lv = ref._scan_first(state, up_axis, up_sign)
        floors = rng.integers(0, 3, lv.shape[1:])         # neighbours' bands 3 .. 5 always overlap
        for t in range(3):
            lv[t][floors >= t] = 2
        h = ref.height(state, up_axis, up_sign)
        walk = ref.walk_stand(state, h, 3, 5)
        src = int(np.flatnonzero(walk.reshape(-1))[0])
        dist = rref.distances(walk, [src])
        origin = (-3, 2, 5)
        for max_cost in (rref.FAR - 1, 400):
            exp = ref.candidates_stand(dist, h, origin, stride, max_cost, up_axis, 3)
            assert len(exp) > 2
            count = torch.full((1,), POISON64, dtype=torch.int64, device=DEV)
            cells = torch.full((len(exp) + 3,), -1, dtype=torch.int64, device=DEV)
            ops.grid_view_candidates_stand(_dev(dist.view(np.int32)), _dev(h), origin, stride, max_cost, up_axis, 3, cells,
                                           count)
            assert int(count.item()) == len(exp)
            got = cells.cpu().numpy()
            assert np.sort(got[:len(exp)]).tolist() == exp.tolist() and (got[len(exp):] == -1).all()
            # a buffer that is too small: the count is still the whole number, nothing is written past the end
            small = torch.full((2,), -1, dtype=torch.int64, device=DEV)
            ops.grid_view_candidates_stand(_dev(dist.view(np.int32)), _dev(h), origin, stride, max_cost, up_axis, 3,
                                           small, count)
            assert int(count.item()) == len(exp) and set(small.tolist()) <= set(exp.tolist())


# ------------------------------------------------------------------------------------------------ 4. end to end
def _grid(state, cell=0.1, origin=(0, 0, 0)):
    from pi3_slam_amd.dense_map import OccupancyGrid
    return OccupancyGrid(state, np.asarray(origin, np.int64), cell)


def _centre(lin, shape, cell=0.1, origin=(0, 0, 0)):
    nz, ny, nx = shape
    c = np.array([lin % nx, (lin // nx) % ny, lin // (nx * ny)], np.int64) + np.asarray(origin, np.int64)
    return cell * (c.astype(np.float64) + 0.5)


@pytest.mark.parametrize("up", [(0, -1, 0), (0, 0, 1), (1, 0, 0)], ids=str)
def test_the_flyer_takes_the_window_and_the_walker_the_door(up):
    from pi3_slam_amd.grid_route import GridRouter, up_axes
    s, _, _, k = up_axes(up)
    room = ref.wall_room(k, s)
    state, shape = room["state"], room["state"].shape
    grid = _grid(state)
    start, goal = _centre(room["start"], shape), _centre(room["goal"], shape)

    def in_wall(cells):
        c = room["coords"](cells)
        return c[c[:, 1] == room["wall"]]

    flyer = GridRouter()
    f = flyer.field(grid, [start], DEV)
    way = flyer.path(f, goal)
    assert f.height is None and "height" not in f.device_arrays and "stand" not in f.settings
    through = in_wall(way.cells)
    assert len(through) and (through[:, 2] >= room["window"][0]).all() and (through[:, 0] >= 20).all()
    assert way.cost == int(rref.distances(rref.walk_mask(state), [room["start"]]).reshape(-1)[room["goal"]])

    walker = GridRouter(stand=(0.6, 0.8), up=up)
    f = walker.field(grid, [start], DEV)
    h = ref.height(state, k, s)
    exp = ref.init_stand(state, None, 0, False, h, 6, 8, [room["start"]])
    assert f.settings["stand_cells"] == [6, 8] and f.settings["stand"] == [0.6, 0.8] and f.settings["up"] == list(up)
    assert f.height.tobytes() == h.tobytes() and f.walk.tobytes() == exp["walk"].tobytes()
    assert f.device_arrays["height"].cpu().numpy().tobytes() == h.tobytes()
    assert [f.counts[n] for n in ("traversable", "sources_accepted", "sources_blocked", "sources_outside", "off_band")] == exp["counters"]
    dist = rref.distances(exp["walk"], [room["start"]])
    assert f.cost.tobytes() == dist.tobytes()
    way = walker.path(f, goal)
    assert way.cost == int(dist.reshape(-1)[room["goal"]]) > 1000           # exactly the oracle's Dijkstra over walk_stand
    through = in_wall(way.cells)
    assert len(through) and (through[:, 2] < room["door"][1]).all() and (through[:, 0] <= 10).all()
    hs = h.reshape(-1)
    assert ((hs[way.cells] >= 6) & (hs[way.cells] <= 8)).all()
    taut = walker.taut(f, way)
    assert taut.length_m <= way.length_m and taut.cells[0] == way.cells[0] and taut.cells[-1] == way.cells[-1]
    nz, ny, nx = shape
    for a, b in zip(taut.cells, taut.cells[1:]):
        for x, y, z in sref.supercover(sref._xyz(int(a), nx, ny), sref._xyz(int(b), nx, ny)):
            assert 6 <= h[z, y, x] <= 8 and exp["walk"][z, y, x]
    assert walker.sees(f, start, _centre(room["lin"](7, 3, 50), shape)) and not walker.sees(f, start, goal)
    # a refused goal says what is wrong with it
    with pytest.raises(ValueError, match=r"is free, 12 cells above its floor \(band 6 .. 8\)"):
        walker.path(f, _centre(room["lin"](12, 14, 55), shape))
    with pytest.raises(ValueError, match=r"the start is not traversable: .* is free, 22 cells above its floor \(band 6 .. 8\)"):
        walker.field(grid, [_centre(room["lin"](22, 3, 6), shape)], DEV)


def test_the_staircase_needs_a_band_wider_than_its_step():
    from pi3_slam_amd.grid_route import GridRouter
    st = ref.staircase()
    state, shape = st["state"], st["state"].shape
    grid = _grid(state)
    h = ref.height(state, 1, -1)
    start, top = _centre(st["start"], shape), _centre(st["top"], shape)
    for (lo, hi), band in (((0.3, 0.5), (3, 5)), ((0.4, 0.4), (4, 4))):
        walk = ref.walk_stand(state, h, *band)
        dist = rref.distances(walk, [st["start"]])
        router = GridRouter(stand=(lo, hi))
        f = router.field(grid, [start], DEV)
        assert f.settings["stand_cells"] == list(band) and f.walk.tobytes() == walk.tobytes()
        assert f.cost.tobytes() == dist.tobytes() and walk.reshape(-1)[st["top"]] == 1
        way = router.path(f, top)
        if band == (3, 5):                          # climbed
            assert way is not None and way.cost == int(dist.reshape(-1)[st["top"]]) < rref.FAR
            assert ((h.reshape(-1)[way.cells] >= 3) & (h.reshape(-1)[way.cells] <= 5)).all()
        else:                                       # the no-corner rule needs the cell above, which is off the band
            assert way is None and dist.reshape(-1)[st["top"]] == rref.FAR and f.counts["reachable"] == int((dist != rref.FAR).sum())


# ------------------------------------------------------------------------------------------------ 5. planner, finder, cli
BOX_STAND = (0.6, 2.0)          # the observed box room has walls, not a floor, under most cells: up = -y stands on a wall
BOX_RANGE_CELLS = 12


def _box_room():
    room, state, cams, d2u, walk_u, (Rb, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    cell, origin = room["cell"], np.asarray(room["origin"], np.int64)
    centres = cell * ((cams + origin).astype(np.float64) + 0.5)
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    h = ref.height(state, 1, -1)
    band = ref.band_cells(*BOX_STAND, cell)
    walk = ref.walk_stand(state, h, *band, oref.edt_ref(state, Rb, False), min_d2)
    dist = rref.distances(walk, lin)
    return state, _grid(state, cell, origin), centres, lin, h, band, walk, dist, cell, origin


def test_box_room_through_the_standing_planner_finder_and_tour():
    from pi3_slam_amd.frontier import FrontierFinder
    from pi3_slam_amd.view_planner import ViewPlanner
    state, grid, centres, lin, h, band, walk, dist, cell, origin = _box_room()
    assert band == (6, 20) and int(walk.reshape(-1)[lin].sum()) >= 2 and int((dist != rref.FAR).sum()) > 300
    stands = walk.reshape(-1)
    for kw in (dict(), dict(frustum=(90, 67.5), unknown_depth=2)):
        planner = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, stride=4, count=6, stand=BOX_STAND, **kw)
        found = planner.find(grid, centres, DEV)
        exp = ref.candidates_stand(dist, h, origin, 4, rref.FAR - 1, 1, band[0])
        assert found.field.walk.tobytes() == walk.tobytes() and found.field.cost.tobytes() == dist.tobytes()
        assert found.counts["candidates"] == len(exp) > 10 and np.flatnonzero(found.gain.reshape(-1) >= 0).tolist() == exp.tolist()
        assert len(found.views) >= 1 and all(stands[v.cell] and band[0] <= h.reshape(-1)[v.cell] <= band[1] for v in found.views)
        assert found.settings["stand"] == list(BOX_STAND) and found.settings["stand_cells"] == list(band)
        assert found.field.counts["off_band"] == int(rref.walk_mask(state, oref.edt_ref(state, 2, False), 4).sum() - walk.sum())
        assert found.route_to(0).cost == found.views[0].cost
    cover = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, stride=4, count=4, stand=BOX_STAND).cover(grid, centres, DEV)
    assert len(cover.views) >= 1 and all(stands[v.cell] for v in cover.views)
    assert cover.counts["candidates"] == len(exp)
    # the tour leaves from a camera that stands and reaches the best view: the band cuts the room into several parts,
    # and the views of the others are left out, as the oracle's field from that camera says
    fields = {i: rref.distances(walk, [lin[i]]).reshape(-1) for i in np.flatnonzero(stands[lin])}
    first = next(i for i, d in fields.items() if d[cover.views[0].cell] != rref.FAR)
    tour = cover.tour(centres[first], taut=True)
    within = [v.rank for v in cover.views if fields[first][v.cell] != rref.FAR]
    assert sorted(r for stop in tour.stops for r in stop.ranks) == within and 0 in within
    assert tour.counts["unreachable"] == len({v.cell for v in cover.views if v.rank not in within})
    assert tour.settings["stand"] == list(BOX_STAND) and tour.settings["router"]["up"] == [0, -1, 0]
    assert all(stands[c] for leg in tour.leg_cells for c in leg)
    # the world lattice alone would offer other cells: the floor-following rule is the one in use
    from pi3_slam_amd import ops
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    cells = torch.empty(dist.size, dtype=torch.int64, device=DEV)
    ops.grid_view_candidates(_dev(dist.view(np.int32)), origin, 4, rref.FAR - 1, cells, count)
    assert sorted(cells[:int(count.item())].tolist()) != exp.tolist()
    # the frontiers ranked by a walkable route
    ranked = FrontierFinder(route_cases.BOX_RADIUS, 1, stand=BOX_STAND).find(grid, centres, DEV)
    assert ranked.field.walk.tobytes() == walk.tobytes() and ranked.settings["router"]["stand"] == list(BOX_STAND) and ranked.settings["stand_cells"] == list(band)
    expf = fref.frontier_set(state, dist)           # the oracle's clusters over the standing field
    assert [(c.root, c.cells, c.cost, c.goal_cell) for c in ranked.clusters] == \
        [(c["root"], c["cells"], c["cost"], c["goal"]) for c in expf["clusters"]] and len(ranked.clusters) >= 1
    assert ranked.counts["reachable_cells"] == expf["counters"][2] == int(((dist != rref.FAR) & (fref.faces(state) > 0)).sum())
    assert all(stands[c.goal_cell] for c in ranked.clusters if c.reachable)


def _files(folder):
    out = {}
    for name in sorted(os.listdir(folder)):
        path = os.path.join(folder, name)
        if name.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                out[name] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
        else:
            out[name] = open(path, "rb").read()
    return out


def test_cli_with_and_without_the_flag(tmp_path, capsys):
    from pi3_slam_amd import cli, export
    state, grid, centres, lin, h, band, walk, dist, cell, origin = _box_room()
    first = int(np.flatnonzero(walk.reshape(-1)[lin])[0])          # a camera that stands
    occ = str(tmp_path / "occupancy.npz")
    export.write_occupancy(grid, occ)
    where = [repr(float(v)) for v in centres[first]]
    base = ["views", "--occupancy", occ, "--start"] + where + ["--radius", str(route_cases.BOX_RADIUS), "--range",
                                                              repr(BOX_RANGE_CELLS * cell), "--count", "4", "--cover",
                                                              "--tour", "--device", DEV]
    flag = ["--stand", repr(BOX_STAND[0]), repr(BOX_STAND[1])]
    capsys.readouterr()
    cli.main(base + flag + ["--output", str(tmp_path / "s")])
    out = capsys.readouterr().out
    assert "standing 6 .. 20 cells above a floor (" in out and "cells off the band)" in out
    for name in ("views.json", "tour.json"):
        st = json.load(open(tmp_path / "s" / name))["settings"]
        assert st["stand"] == list(BOX_STAND) and st["up"] == [0, -1, 0]
        assert st["router"]["stand"] == list(BOX_STAND) and st["stand_cells"] == [6, 20] and st["router"]["up"] == [0, -1, 0]
    rec = json.load(open(tmp_path / "s" / "views.json"))
    assert len(rec["views"]) >= 1 and all(walk.reshape(-1)[v["cell"]] for v in rec["views"])
    # route: the height array and the settings; frontiers: the settings
    goal = [repr(float(v)) for v in _centre(rec["views"][0]["cell"], state.shape, cell, origin)]
    cli.main(["route", "--occupancy", occ, "--start"] + where + ["--goal"] + goal + [
        "--radius", str(route_cases.BOX_RADIUS), "--approach-unknown", "--device", DEV, "--output", str(tmp_path / "r")] + flag)
    out = capsys.readouterr().out
    assert f"standing 6 .. 20 cells above a floor ({int(rref.walk_mask(state, oref.edt_ref(state, 2, False), 4).sum() - walk.sum())} cells off the band)" in out
    with np.load(tmp_path / "r" / "route.npz") as z:
        assert z["height"].dtype == np.uint8 and z["height"].tobytes() == h.tobytes()
        st = json.loads(str(z["settings"]))
        assert st["stand"] == list(BOX_STAND) and st["stand_cells"] == [6, 20] and st["up"] == [0, -1, 0]
        assert json.loads(str(z["counts"]))["off_band"] > 0
    route = json.load(open(tmp_path / "r" / "route.json"))
    assert route["settings"]["stand_cells"] == [6, 20] and route["cost"] == rec["views"][0]["cost"]
    cli.main(["frontiers", "--occupancy", occ, "--start"] + where + ["--radius", str(route_cases.BOX_RADIUS), "--device", DEV,
                                                                      "--output", str(tmp_path / "f")] + flag + ["--up", "0", "-1", "0"])
    assert "standing 6 .. 20 cells" in capsys.readouterr().out
    assert json.load(open(tmp_path / "f" / "frontiers.json"))["settings"]["stand_cells"] == [6, 20]
    # without the flag: no new key, and the same files run after run
    for cmd, extra in ((base, []), (["route", "--occupancy", occ, "--start"] + where + ["--device", DEV], []),
                       (["frontiers", "--occupancy", occ, "--start"] + where + ["--device", DEV], [])):
        a_dir, b_dir = tmp_path / (cmd[0] + "_a"), tmp_path / (cmd[0] + "_b")
        cli.main(cmd + ["--output", str(a_dir)])
        assert "standing" not in capsys.readouterr().out
        cli.main(cmd + ["--output", str(b_dir), "--up", "0", "0", "1"])         # --up alone changes nothing
        a, b = _files(a_dir), _files(b_dir)
        assert a == b and len(a) >= 1
        for name, blob in a.items():
            if name.endswith(".json"):
                assert b"stand" not in blob and b'"up"' not in blob and b"off_band" not in blob, name
            elif name == "route.npz":
                with np.load(a_dir / name) as z:
                    assert "height" not in z.files and "stand" not in str(z["settings"]) and "off_band" not in str(z["counts"])
    with pytest.raises(SystemExit, match="views: a standing band of lo = 0.61 .. hi = 0.69 at cells of 0.1 is 7 .. 6 cells"):
        cli.main(base + ["--stand", "0.61", "0.69", "--output", str(tmp_path / "w")])
    with pytest.raises(SystemExit, match="route: the start is not traversable: .*(has no verified floor below it|above its floor)"):
        cli.main(["route", "--occupancy", occ, "--start"] + [repr(float(v)) for v in centres[_not_standing(walk, lin)]] + [
            "--radius", str(route_cases.BOX_RADIUS), "--approach-unknown", "--device", DEV, "--output", str(tmp_path / "w")] + flag)
    assert not os.path.exists(tmp_path / "w")


def _not_standing(walk, lin):
    return int(np.flatnonzero(walk.reshape(-1)[lin] == 0)[0])
