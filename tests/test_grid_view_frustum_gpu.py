"""Views through a camera on the GPU (csrc/grid_view.hip: pi3_grid_view_gain_frustum, pi3_grid_view_mark_frustum), byte
for byte against tests/grid_view_frustum_ref.py, against the shipped cone entry points where the two rules coincide (the
half space) or contain each other, under the 48 signed axis permutations, and through the planner, the tour and the
command line.  Every output is filled with a poison value before each call, and every mask has two guard words behind
it.  Near ranges 31 and 32 and far ranges 62 and 63 lie on both sides of the 64 KB of LDS the depth form may have
without asking.  The oracle casts its rays once per grid, range and depth; the frames, fractions and masks share them."""
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
import grid_view_frustum_ref as fref        # noqa: E402
import grid_view_ref as vref                # noqa: E402
import test_grid_cover_gpu as cover_gpu     # noqa: E402  (its guarded mask)
import test_grid_route as route_cases       # noqa: E402  (the box-room case)
import test_grid_view_depth_gpu as depth_gpu  # noqa: E402  (its candidates, the box room, the files of a run)
import test_grid_view_far_gpu as far_gpu    # noqa: E402  (the signed permutations)
import test_grid_view_gpu as view_gpu       # noqa: E402  (its comparison)

pytestmark = pytest.mark.gpu
DEV = view_gpu.DEV
POISON32, POISON64, POISON16 = view_gpu.POISON32, view_gpu.POISON64, cover_gpu.POISON16
Mask = cover_gpu.Mask
_dev = view_gpu._dev
_same = view_gpu._same
_edge_candidates = depth_gpu._edge_candidates
BIG = 1 << 20
T90, T67 = fref.tan2(90), fref.tan2(67.5)   # 4096 / 4096 and 1829 / 4096
HD = vref.headings26()
SMALL = far_gpu.SMALL                       # (20, 9, 70)
SMALL_CAND = far_gpu.SMALL_CAND


def _frames_of(axes):
    """A frame per axis: r = f x (0, -1, 0), or f x (0, 0, 1) where f is vertical, divided by nothing (within +-64)."""
    rows = []
    for f in np.asarray(axes, np.int64).reshape(-1, 3):
        up = (0, 0, 1) if f[0] == 0 and f[2] == 0 else (0, -1, 0)
        rows.append(np.concatenate([f, np.cross(f, up)]))
    return np.array(rows, np.int64)


AXES6 = _frames_of([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
F26 = _frames_of(HD)


def _f32():
    from pi3_slam_amd.view_planner import view_frames
    return view_frames(8, (-40, -15, 15, 40))                   # components up to 64


# (frames, tan^2 horizontal, tan^2 vertical): H = 1 on the faces, 26, and 32 with a portrait's fractions
def _shapes():
    return {"1": (AXES6[:1], (1, 1), (1, 1)), "26": (F26, T90, T67), "32": (_f32(), T67, T90)}


def _frustum(shape):
    from pi3_slam_amd import ops
    frames, th, tv = shape
    return ops.ViewFrustum(frames, *th, *tv)


def _gain(state, cand, R, shape, depth=None, far=False, mask=None):
    """ops.grid_view_gain, or with a mask ops.grid_view_gain_unseen, with frustum= into poisoned outputs."""
    from pi3_slam_amd import ops
    V, H = len(cand), len(shape[0])
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    cells = _dev(np.asarray(cand, np.int64))
    kw = dict(far=far, unknown_depth=depth, frustum=_frustum(shape))
    if mask is None:
        ops.grid_view_gain(state, cells, R, None, None, None, gain, visible, best, counters, **kw)
    else:
        before = mask.host()
        ops.grid_view_gain_unseen(state, mask.words, cells, R, None, None, None, gain, visible, best, counters, **kw)
        assert mask.host().tobytes() == before.tobytes()        # read only
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _mark(state, mask, cells, heading_of, R, shape, depth=None, owner=None, tag=0, far=False):
    from pi3_slam_amd import ops
    counters = torch.full((5,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_mark(state, mask.words, _dev(np.asarray(cells, np.int64)), heading_of, R, None, None, None, counters,
                       owner, tag, far=far, unknown_depth=depth, frustum=_frustum(shape))
    return counters.tolist()


def _cone_gain(state, cand, R, headings, num, den, depth=None, far=False):
    """The shipped entry points: pi3_grid_view_gain, _far or _depth."""
    from pi3_slam_amd import ops
    V, H = len(cand), len(headings)
    gain = torch.full((V, H), POISON32, dtype=torch.int32, device=DEV)
    visible = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    best = torch.full((V,), POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.grid_view_gain(state, _dev(np.asarray(cand, np.int64)), R, headings, num, den, gain, visible, best, counters,
                       far=far, unknown_depth=depth)
    return dict(gain=gain.cpu().numpy().view(np.uint32), visible=visible.cpu().numpy().view(np.uint32),
                best=best.cpu().numpy(), counters=counters.tolist())


def _all_ways(state, cand, R, far, depths, what):
    """Every depth x (H = 1 / every cell, H = 26 / a half-set mask, H = 32 / an empty mask) against the oracle."""
    st = _dev(state)
    shapes = _shapes()
    half = cref.pack(np.random.default_rng(R).random(state.size) < 0.5)
    none = np.zeros(cref.seen_words(state.size), np.uint32)
    seen = 0
    for depth in depths:
        casts = fref.casts_of(state, cand, R, depth)            # the rays, once
        for key, words in (("1", None), ("26", half), ("32", none)):
            frames, th, tv = shapes[key]
            exp = fref.gain_unseen(state, none if words is None else words, cand, R, frames, th, tv, casts=casts)
            got = _gain(st, cand, R, shapes[key], depth, far, None if words is None else Mask(state.size, words))
            _same(got, exp, (what, R, depth, key))
            seen += int(got["gain"].sum())
    return seen


# ------------------------------------------------------------------------------------------------ 1. the gain
@pytest.mark.parametrize("dims,R", [((9, 7, 5), 1), ((9, 7, 5), 2), ((9, 7, 5), 7), ((33, 20, 17), 2), ((33, 20, 17), 7),
                                    ((33, 20, 17), 31), ((33, 20, 17), 32), ((41, 40, 39), 32)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "R%d" % v)
def test_near_gain_matches_the_oracle(dims, R):
    nx, ny, nz = dims
    state = vref.three_state((nz, ny, nx), 0.5, 0.02 if R > 2 else 0.1, 5)
    cand = _edge_candidates(state.shape)                        # the 8 corners, the face centres, one inside, two outside
    if R < 31:
        cand = np.concatenate([view_gpu._candidates(dims, sum(dims)), cand])
    depths = (None, 0, 3, 255) if dims != (41, 40, 39) else (None, 3)
    assert _all_ways(state, cand, R, False, depths, dims) > 100


@pytest.mark.parametrize("R", [7, 33, 62, 63, 64])
def test_far_gain_matches_the_oracle(R):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    cand = np.concatenate([SMALL_CAND, _edge_candidates(SMALL)]) if R < 62 else np.array(
        SMALL_CAND + [-1, state.size], np.int64)                # two corners, a face, the last cell, two outside
    assert _all_ways(state, cand, R, True, (None, 0, 3, 255) if R != 62 else (None, 3), "far") > 100


@pytest.mark.parametrize("fill", [0, 2])
def test_all_unknown_and_all_occupied(fill):
    state = np.full((5, 7, 9), fill, np.uint8)
    cand = np.arange(state.size + 1)
    total = sum(_all_ways(state, cand, R, far, (None, 0), fill) for R, far in ((2, False), (7, False), (7, True)))
    assert (total > 10000) if fill == 0 else (total == 0)


def test_the_faces_are_inclusive():
    """Axis frames at tan^2 = 1 / 1: the cells with |o_y| = o_x or |o_z| = o_x lie on a face, those with both on an edge."""
    n, c, R = 15, 7, 7
    state = np.zeros((n, n, n), np.uint8)
    centre = [(c * n + c) * n + c]
    shape = (AXES6, (1, 1), (1, 1))
    got = _gain(_dev(state), centre, R, shape)
    ball = vref.ball_offsets(R)
    x, y, z = ball.T
    pyramid = int(((x > 0) & (np.abs(y) <= x) & (np.abs(z) <= x)).sum())
    on_a_face = int(((x > 0) & ((np.abs(y) == x) | (np.abs(z) == x)) & (np.abs(y) <= x) & (np.abs(z) <= x)).sum())
    assert got["gain"].tolist() == [[pyramid] * 6] and on_a_face > 50 and got["visible"].tolist() == [len(ball)]
    _same(got, fref.gain(state, centre, R, *shape), "open")
    mixed = vref.three_state((n, n, n), 0.6, 0.03, 3)
    cand = np.concatenate([centre, _edge_candidates(mixed.shape)])
    for depth, far in ((None, False), (1, False), (None, True), (1, True)):
        _same(_gain(_dev(mixed), cand, R, shape, depth, far), fref.gain(mixed, cand, R, *shape, depth), (depth, far))


# ------------------------------------------------------------------------------------------------ 2. against the cones
@pytest.mark.parametrize("R,far,depth", [(7, False, None), (32, False, None), (40, True, None), (64, True, None),
                                         (7, False, 2), (32, False, 2), (64, True, 2)])
def test_the_widest_frustum_is_the_cones_half_space(R, far, depth):
    """tan^2 = 2^20 / 1 on both sides leaves o.f > 0 within 64 cells; so does a cone with cos^2 = 0."""
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    st = _dev(state)
    cand = np.array(SMALL_CAND + [6000, 3333, -1], np.int64)
    cone = _cone_gain(st, cand, R, AXES6[:, :3], 0, BIG, depth, far)
    assert cone["counters"][3] > 100 and len(set(cone["gain"][2].tolist())) > 3
    _same(_gain(st, cand, R, (AXES6, (BIG, 1), (BIG, 1)), depth, far), cone, (R, far, depth))


def test_cones_and_frusta_contain_each_other():
    """A cone of 45 degrees (cos^2 = 1 / 2, tan^2 = 1) on the 26 axes: inside the frustum tan^2 = (1, 2), whose smaller
    half angle is the cone's, and around the frustum tan^2 = (1 / 2, 1 / 2), whose corner lies on the cone."""
    state = vref.three_state((17, 20, 33), 0.5, 0.02, 5)
    st = _dev(state)
    cand = _edge_candidates(state.shape)[:-2]
    for R, far in ((7, False), (20, True)):
        cone = _cone_gain(st, cand, R, HD, 1, 2, far=far)["gain"].astype(np.int64)
        wide = _gain(st, cand, R, (F26, (1, 1), (2, 1)), far=far)["gain"].astype(np.int64)
        slim = _gain(st, cand, R, (F26, (1, 2), (1, 2)), far=far)["gain"].astype(np.int64)
        assert (cone <= wide).all() and (slim <= cone).all() and (cone < wide).any() and (slim < cone).any()
        assert slim.sum() > 1000


def test_the_48_signed_axis_permutations_see_the_same():
    n, c, R = 67, 33, 33
    state = vref.three_state((n, n, n), 0.5, 0.02, 17)
    centre = [far_gpu._lin(state.shape, c, c, c)]
    frames, th, tv = _f32()[[0, 1, 9, 10, 18, 27]], T90, T67
    z, y, x = np.meshgrid(*[np.arange(n) - c] * 3, indexing="ij")           # every cell's offset from the centre
    first = _gain(_dev(state), centre, R, (frames, th, tv))
    _same(first, fref.gain(state, centre, R, frames, th, tv), "the first orientation")
    assert first["counters"][2] > 1000 and first["counters"][3] > 1000 and len(set(first["gain"][0].tolist())) == 6
    moves = far_gpu._signed_permutations()
    assert len(moves) == 48
    for perm, flips in moves:
        # where the moved grid has the offset a, the first one had M a: a frame v of the first grid is M^T v there
        mx, my, mz = (far_gpu._moved(k, perm, flips) for k in (x, y, z))
        M = np.array([[int(m[c + a[2], c + a[1], c + a[0]]) for a in np.eye(3, dtype=int)] for m in (mx, my, mz)], np.int64)
        assert sorted(np.abs(M).sum(0)) == [1, 1, 1] and abs(round(np.linalg.det(M))) == 1
        moved = np.concatenate([frames[:, :3] @ M, frames[:, 3:] @ M], 1)
        got = _gain(_dev(far_gpu._moved(state, perm, flips)), centre, R, (moved, th, tv))
        assert got["visible"].tolist() == first["visible"].tolist() and got["counters"] == first["counters"], (perm, flips)
        assert got["gain"].tolist() == first["gain"].tolist(), (perm, flips)


# ------------------------------------------------------------------------------------------------ 3. the marks
@pytest.mark.parametrize("R,far,depth", [(7, False, None), (32, False, 3), (33, True, None), (63, True, 3)])
def test_marks(R, far, depth):
    state = vref.three_state(SMALL, 0.5, 0.02, 5)
    st = _dev(state)
    cand = np.array(SMALL_CAND + [6000, -1], np.int64)
    shape = _shapes()["26"]
    casts = fref.casts_of(state, cand, R, depth)
    rng = np.random.default_rng(R)
    # any frame's frustum (-1 in every row), and a frame per row (mixed, -1 among them)
    for hof in ([-1] * 6, [25, -1, 13, 0, 7, 3]):
        words = cref.pack(rng.random(state.size) < 0.2)
        mask = Mask(state.size, words)
        exp = fref.mark(state, words, cand, hof, R, *shape, casts=casts)
        assert _mark(st, mask, cand, hof, R, shape, depth, far=far) == exp["counters"] and exp["counters"][4] > 50
        assert mask.host().tobytes() == words.tobytes() and int(exp["new"].sum()) == exp["counters"][4]
    # one row with an owner; what it turns is its gain under the same mask ("only when the bit reads clear")
    words = cref.pack(rng.random(state.size) < 0.2)
    under = _gain(st, cand[2:3], R, shape, depth, far, Mask(state.size, words))
    mask = Mask(state.size, words)
    owner_np = np.full(state.shape, POISON16, np.int16)
    owner = _dev(owner_np)
    exp = fref.mark(state, words, cand[2:3], [13], R, *shape, depth, owner_np, 77)["counters"]
    assert _mark(st, mask, cand[2:3], [13], R, shape, depth, owner, 77, far=far) == exp and exp[4] > 20
    assert mask.host().tobytes() == words.tobytes() and owner.cpu().numpy().tobytes() == owner_np.tobytes()
    assert exp[4] == int(under["gain"][0, 13]) and int((owner_np == 77).sum()) == exp[4]


def test_more_rows_than_one_launch_takes():
    """Mixed frames over more than 1024 rows: several launches, rows that race for the same cells, one count per cell."""
    state = vref.three_state((5, 7, 9), 0.6, 0.05, 11)
    st = _dev(state)
    shape = _shapes()["32"]
    rng = np.random.default_rng(4)
    rows = np.concatenate([np.tile(np.arange(state.size), 4), [-1, state.size]]).astype(np.int64)
    assert len(rows) > 1024 + 200
    hof = rng.integers(-1, 32, len(rows))
    for R, far, depth in ((2, False, None), (3, True, 1)):
        words = cref.pack(rng.random(state.size) < 0.3)
        mask = Mask(state.size, words)
        exp = fref.mark(state, words, rows, hof, R, *shape, depth)
        got = _mark(st, mask, rows, hof, R, shape, depth, far=far)
        assert got == exp["counters"] and got[3] > got[4] > 20 and got[0] == len(rows) - 2
        assert mask.host().tobytes() == words.tobytes()


def test_no_candidate_launches_nothing_and_zeroes_the_counters():
    state = _dev(vref.three_state((7, 8, 9), 0.5, 0.1, 3))
    shape = _shapes()["26"]
    mask = Mask(7 * 8 * 9)
    for depth, far in ((None, False), (1, False), (None, True), (255, True)):
        assert _gain(state, [], 4, shape, depth, far)["counters"] == [0, 0, 0, 0]
        assert _gain(state, [], 4, shape, depth, far, mask)["counters"] == [0, 0, 0, 0]
        assert _mark(state, mask, [], [], 4, shape, depth, far=far) == [0, 0, 0, 0, 0] and not mask.host().any()


# ------------------------------------------------------------------------------------------------ 4. planner, tour, cli
BOX_RANGE_CELLS = 8
CAMERA = dict(frustum=(90, 67.5), yaw_steps=8, pitches_deg=(-30, 0, 30))


def _expected_find(state, dist, origin, R, frames, th, tv, count, sep, depth=None):
    """grid_view_ref.view_set with the frusta's gain."""
    cells = vref.candidates(dist, origin, 4)
    g = fref.gain(state, cells, R, frames, th, tv, depth)
    best_gain = g["gain"][np.arange(len(cells)), np.maximum(g["best"], 0)].astype(np.int64)
    cost = np.asarray(dist, np.uint32).reshape(-1)[cells].astype(np.int64)
    kept, low = vref.select(cells, best_gain, cost, state.shape, count, sep, 1)
    views = [(int(cells[i]), int(g["best"][i]), int(best_gain[i]), int(g["visible"][i]), int(cost[i])) for i in kept]
    return g, views, low


def test_box_room_through_the_planner_and_the_tour():
    from pi3_slam_amd.view_planner import ViewPlanner, view_frames, view_pose
    state, grid, centres, dist, cell, origin = depth_gpu._box_room()
    frames = view_frames(8, (-30, 0, 30))
    th, tv = T90, T67
    for depth in (None, 1):
        planner = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, stride=4, count=10, unknown_depth=depth,
                              **CAMERA)
        R, sep, _ = planner.cells_of(cell)
        assert R == BOX_RANGE_CELLS
        g, views, low = _expected_find(state, dist, origin, R, frames, th, tv, 10, sep, depth)
        found = planner.find(grid, centres, DEV)
        c = found.counts
        print(f"box room through the frusta at depth {depth}: {c}")
        assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == g["counters"]
        assert [(v.cell, v.heading, v.gain, v.visible, v.cost) for v in found.views] == views and c["low_gain"] == low
        assert len(found.views) >= 3 and found.views[0].gain > 0
        assert found.frames.tobytes() == frames.tobytes() and found.headings.tolist() == frames[:, :3].tolist()
        for v in found.views:                                   # every view: its gain at its cell and frame, its camera
            one = fref.gain(state, [v.cell], R, frames[v.heading:v.heading + 1], th, tv, depth)
            assert int(one["gain"][0, 0]) == v.gain and v.axis.tolist() == frames[v.heading, :3].tolist()
            assert v.frame.tolist() == frames[v.heading].reshape(2, 3).tolist()
            assert v.pose.tobytes() == view_pose(frames[v.heading], v.position).tobytes()
            assert np.abs(v.pose[:3, :3].T @ v.pose[:3, :3] - np.eye(3)).max() < 1e-12
        fr = found.settings["frustum"]
        assert fr["tan2_h"] == list(th) and fr["tan2_v"] == list(tv) and found.settings["headings"] == 24
    # cover (transparent), and the tour with taut legs: it replays the marks in its own order, by the same rule
    cand = vref.candidates(dist, origin, 4)
    cost = dist.reshape(-1)[cand].astype(np.int64)
    full = fref.cover(state, cand, cost, R, frames, th, tv, None, count=4)
    four = ViewPlanner(route_cases.BOX_RADIUS, BOX_RANGE_CELLS * cell, stride=4, count=4, **CAMERA).cover(grid, centres, DEV)
    assert [(v.cell, v.heading, v.gain) for v in four.views] == full["picks"] and len(full["picks"]) == 4
    assert [v.new for v in four.views] == full["new"] and [v.covered for v in four.views] == full["covered"]
    assert [v.visible for v in four.views] == full["visible"] and four.counts["seeable"] == full["seeable"]
    assert four.seen_by.tobytes() == full["seen_by"].tobytes() and all(v.pose is not None for v in four.views)
    marks = np.zeros(cref.seen_words(state.size), np.uint32)
    for k, v in enumerate(four.views):                          # the cover's `new` against the marks
        assert int(fref.mark(state, marks, [v.cell], [v.heading], R, frames, th, tv)["counters"][4]) == v.new == full["new"][k]
    tour = four.tour(taut=True)
    order = [r for stop in tour.stops for r in stop.ranks]
    assert sorted(order) == [0, 1, 2, 3] and tour.settings["frustum"]["tan2_v"] == list(tv)
    replay = fref.replay(state, [(four.views[r].cell, four.views[r].heading) for r in order], R, frames, th, tv)
    assert [n for stop in tour.stops for n in stop.tour_new] == replay
    assert tour.covered == sum(replay) == full["covered"][-1]


def test_box_room_through_the_far_planner():
    from pi3_slam_amd.view_planner import ViewPlanner, view_frames
    state, grid, centres, dist, cell, origin = depth_gpu._box_room()
    frames = view_frames(4, (0,), (0, -1, 0), True)
    planner = ViewPlanner(route_cases.BOX_RADIUS, (33 - 0.1) * cell, stride=8, count=10, far=True, unknown_depth=1,
                          frustum=(90, 67.5), yaw_steps=4, portrait=True)
    R, sep, _ = planner.cells_of(cell)
    assert R == 33
    cells = vref.candidates(dist, origin, 8)
    g = fref.gain(state, cells, R, frames, T67, T90, 1)         # portrait: the fractions change places
    found = planner.find(grid, centres, DEV)
    c = found.counts
    assert [c[k] for k in ("candidates", "rays", "rays_blocked", "rays_visible")] == g["counters"]
    assert found.gain.reshape(-1)[cells].tolist() == g["gain"].max(1).tolist() and len(found.views) >= 1
    assert found.settings["frustum"]["portrait"] is True and found.settings["far"] is True


def test_cli_views_with_and_without_the_flag(tmp_path, capsys):
    from pi3_slam_amd import cli, export
    from pi3_slam_amd.view_planner import view_frames
    state, grid, centres, dist, cell, origin = depth_gpu._box_room()
    occ = str(tmp_path / "occupancy.npz")
    export.write_occupancy(grid, occ)
    base = ["views", "--occupancy", occ, "--start"] + [repr(float(v)) for v in centres[0]] + [
        "--radius", str(route_cases.BOX_RADIUS), "--range", repr(BOX_RANGE_CELLS * cell), "--count", "4", "--cover", "--tour",
        "--taut", "--device", DEV]
    camera = ["--frustum", "90", "67.5", "--yaw-steps", "8", "--pitch", "-30", "0", "30"]
    capsys.readouterr()
    cli.main(base + camera + ["--output", str(tmp_path / "f")])
    assert "24 frusta of 90 x 67.5 degrees" in capsys.readouterr().out
    rec = json.load(open(tmp_path / "f" / "views.json"))
    frames = view_frames(8, (-30, 0, 30))
    fr = rec["settings"]["frustum"]
    assert (fr["hfov_deg"], fr["vfov_deg"], fr["yaw_steps"], fr["pitches_deg"], fr["up"]) == (90, 67.5, 8, [-30, 0, 30], [0, -1, 0])
    assert fr["intrinsics"]["W"] == 640 and fr["intrinsics"]["H"] == 428 and len(fr["realised"]) == 24
    assert len(rec["views"]) == 4 and rec["views"][0]["gain"] > 0
    R = rec["settings"]["range_cells"]
    for v in rec["views"]:
        assert v["frame"] == frames[v["heading"]].reshape(2, 3).tolist() and v["axis"] == v["frame"][0]
        pose = np.array(v["pose"])
        assert pose.shape == (4, 4) and np.abs(pose[:3, :3].T @ pose[:3, :3] - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.det(pose[:3, :3]) - 1) < 1e-12 and pose[:3, 3].tolist() == v["position"]
    # the run has one source, so its costs are its own: every view's gain and `new` against the oracle's marks in order
    marks, owner = np.zeros(cref.seen_words(state.size), np.uint32), np.full(state.shape, -1, np.int16)
    for k, v in enumerate(rec["views"]):
        under = fref.gain_unseen(state, marks, [v["cell"]], R, frames[v["heading"]:v["heading"] + 1], T90, T67)
        new = fref.mark(state, marks, [v["cell"]], [v["heading"]], R, frames, T90, T67, None, owner, k)["counters"][4]
        assert int(under["gain"][0, 0]) == v["gain"] == v["new"] == new > 0
    assert rec["views"][-1]["covered"] == sum(v["new"] for v in rec["views"]) == cref.popcount(marks)
    with np.load(tmp_path / "f" / "views.npz") as z:
        assert z["frames"].dtype == np.int64 and z["frames"].tolist() == frames.tolist()
        assert z["headings"].tolist() == frames[:, :3].tolist() and z["seen_by"].tobytes() == owner.tobytes()
    tour = json.load(open(tmp_path / "f" / "tour.json"))
    assert tour["settings"]["frustum"] == fr and tour["covered"] == rec["views"][-1]["covered"]
    assert {"views.ply", "tour.npz", "tour.ply"} <= set(os.listdir(tmp_path / "f"))
    # without the flag: no new key, and the same files run after run (the unchanged path)
    cli.main(base + ["--output", str(tmp_path / "a")])
    assert "frusta" not in capsys.readouterr().out
    cli.main(base + ["--output", str(tmp_path / "b"), "--fov", "90"])
    a, b = depth_gpu._files(tmp_path / "a"), depth_gpu._files(tmp_path / "b")
    assert a == b and {"views.json", "views.npz", "views.ply", "tour.json", "tour.npz", "tour.ply"} <= set(a)
    plain = json.loads(a["views.json"])
    assert "frustum" not in plain["settings"] and plain["settings"]["fov_deg"] == 90.0
    assert plain["settings"]["cos2_num"] == vref.cos2(90)[0] and "frames" not in a["views.npz"]
    for name in ("views.json", "tour.json"):
        assert b"frustum" not in a[name] and b"pose" not in a[name] and b"frame" not in a[name]
    assert a["views.npz"]["headings"][2] == HD.tobytes()
    with pytest.raises(SystemExit, match="views: a frustum has its own two angles: leave fov_deg out"):
        cli.main(base + camera + ["--output", str(tmp_path / "w"), "--fov", "90"])
    with pytest.raises(SystemExit, match="views: each angle of the frustum must lie in"):
        cli.main(base + ["--frustum", "90", "171", "--output", str(tmp_path / "w")])
    assert not os.path.exists(tmp_path / "w")
