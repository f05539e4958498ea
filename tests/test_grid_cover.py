"""Views that cover, on the CPU: the oracle (tests/grid_cover_ref.py) against grid_view_ref.py and against properties it
does not use, the planner's loop (view_planner.cover_views) driven by the oracle's gain and mark, the box room's figures,
and the host side (settings, signatures, files, flags).  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_cover_ref as cref               # noqa: E402
import grid_route_ref as rref               # noqa: E402
import grid_view_ref as vref                # noqa: E402
import occupancy_ref as oref                # noqa: E402
import test_grid_route as route_cases       # noqa: E402  (the box-room case)

HD = vref.headings26()
F90, F180, F30 = vref.cos2(90), vref.cos2(180), vref.cos2(30)
GRIDS = {(9, 8, 7): vref.three_state((7, 8, 9), 0.5, 0.1, 24), (17, 9, 20): vref.three_state((20, 9, 17), 0.5, 0.1, 46)}


def _zeros(state):
    return np.zeros(cref.seen_words(state.size), np.uint32)


# ------------------------------------------------------------------------------------------------ the mask and the gain
@pytest.mark.parametrize("dims", list(GRIDS), ids=lambda d: "%dx%dx%d" % d)
def test_a_zero_mask_is_the_plain_gain_and_a_full_one_sees_nothing(dims):
    state = GRIDS[dims]
    cand = np.concatenate([np.arange(0, state.size, 3), [-1, state.size]]).astype(np.int64)
    for R, (num, den) in ((2, F90), (5, F180)):
        exp = vref.gain(state, cand, R, HD, num, den)
        got = cref.gain_unseen(state, _zeros(state), cand, R, HD, num, den)
        assert got["counters"] == exp["counters"] and exp["counters"][3] > 0
        for k in ("gain", "visible", "best"):
            assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), k
        full = cref.gain_unseen(state, cref.pack(np.ones(state.size, bool)), cand, R, HD, num, den)
        assert full["counters"] == [len(cand) - 2, 0, 0, 0] and not full["gain"].any() and not full["visible"].any()
        assert full["best"].tolist() == [0] * (len(cand) - 2) + [-1, -1]
    # half a mask: exactly the targets whose bit is clear are counted
    half = np.random.default_rng(1).random(state.size) < 0.5
    got = cref.gain_unseen(state, cref.pack(half), cand, 5, HD, *F90)
    hidden = state.copy().reshape(-1)
    hidden[half & (hidden == 0)] = 1                            # a seen unknown cell counts like a free one
    exp = vref.gain(hidden.reshape(state.shape), cand, 5, HD, *F90)
    assert got["counters"] == exp["counters"] and got["gain"].tobytes() == exp["gain"].tobytes()
    assert got["best"].tobytes() == exp["best"].tobytes()
    assert 0 < exp["counters"][1] < vref.gain(state, cand, 5, HD, *F90)["counters"][1]


@pytest.mark.parametrize("cells", [1, 31, 32, 33, 300, 504])
def test_the_mask_layout_and_its_last_word(cells):
    state = np.zeros((7, 8, 9) if cells == 504 else (1, 1, cells), np.uint8)
    assert state.size == cells and cref.seen_words(cells) == (cells + 31) // 32
    bits = np.random.default_rng(cells).random(cells) < 0.5
    words = cref.pack(bits)
    assert words.dtype == np.uint32 and len(words) == cref.seen_words(cells) and cref.popcount(words) == bits.sum()
    assert cref.unpack(words, cells).tolist() == bits.tolist()
    for c in np.flatnonzero(bits)[:5]:
        assert (int(words[c >> 5]) >> (c & 31)) & 1
    # every cell of an open grid sees every other within two cells: all `cells` bits and none above
    total, seen = cref.seeable(state, np.arange(cells), 2, HD, *F180)
    assert total == (cells if cells > 1 else 0) == cref.popcount(seen)
    if cells & 31:
        assert int(seen[-1]) >> (cells & 31) == 0
    assert cref.unpack(seen, cells).all() or cells == 1


# ------------------------------------------------------------------------------------------------ the mark
@pytest.mark.parametrize("dims", list(GRIDS), ids=lambda d: "%dx%dx%d" % d)
def test_a_mark_turns_the_bits_the_gain_counted(dims):
    state = GRIDS[dims]
    seen = cref.pack(np.random.default_rng(3).random(state.size) < 0.2)
    owner = np.full(state.shape, -1, np.int16)
    rng = np.random.default_rng(4)
    turned = 0
    for tag, (v, h) in enumerate(zip(rng.integers(0, state.size, 12), rng.integers(0, 26, 12))):
        before = cref.gain_unseen(state, seen, [v], 4, HD, *F90)
        was, held = cref.popcount(seen), owner.copy()
        c = cref.mark(state, seen, [v], [h], 4, HD, *F90, owner, tag)["counters"]
        assert c[4] == before["gain"][0][h] == cref.popcount(seen) - was and c[0] == 1 and c[4] <= c[3] <= c[2] <= c[1]
        assert (owner == tag).sum() == c[4] and ((owner == held) | (owner == tag)).all()
        after = cref.gain_unseen(state, seen, [v], 4, HD, *F90)
        assert after["gain"][0][h] == 0 and after["visible"][0] == before["visible"][0] - c[4]
        again = cref.mark(state, seen, [v], [h], 4, HD, *F90, owner, 99)["counters"]
        assert again[4] == 0 and again[:4] == c[:4] and not (owner == 99).any()
        turned += c[4]
    assert turned > 50
    assert cref.mark(state, seen.copy(), [-1, state.size], [0, -1], 4, HD, *F90)["counters"] == [0, 0, 0, 0, 0]


def test_any_heading_is_the_visible_set_at_180_degrees_and_less_at_30():
    state = GRIDS[(17, 9, 20)]
    for v in (0, 1234, state.size - 1):
        seen = _zeros(state)
        c = cref.mark(state, seen, [v], [-1], 5, HD, *F180)["counters"]
        g = cref.gain_unseen(state, _zeros(state), [v], 5, HD, *F180)
        assert c[4] == c[3] == c[2] == g["visible"][0] > 0
        k = cref.cast(state, [v], 5)
        assert sorted(np.flatnonzero(cref.unpack(seen, state.size)).tolist()) == sorted(k["u"][k["arrived"]].tolist())
    # an open grid: the offset (2, 1, 0) is 26.6 degrees off (1, 0, 0) and 18.4 off (1, 1, 0), in no cone of 30 degrees
    free = np.zeros((9, 9, 9), np.uint8)
    centre = (4 * 9 + 4) * 9 + 4
    seen = _zeros(free)
    c = cref.mark(free, seen, [centre], [-1], 4, HD, *F30)["counters"]
    bits = cref.unpack(seen, free.size)
    assert 0 < c[4] == c[3] < c[2] == len(vref.ball_offsets(4))
    assert bits[centre + 1] and bits[centre + 9 + 1] and bits[centre - 81 - 9 - 1] and not bits[centre + 9 + 2]
    wide = _zeros(free)
    cref.mark(free, wide, [centre], [-1], 4, HD, *F180)
    assert not (seen & ~wide).any() and cref.popcount(wide) == c[2]


# ------------------------------------------------------------------------------------------------ the cover
def _case(dims):
    state = GRIDS[dims]
    cand = np.arange(1, state.size, 7, dtype=np.int64)
    cost = np.random.default_rng(sum(dims)).integers(0, 4, len(cand)).astype(np.int64)      # many ties
    return state, cand, cost, 3


def _oracle_kernels(state, cand, R, num, den):
    """mark and regain for cover_views, from the oracle, with what they were asked."""
    seen = _zeros(state)
    owner = np.full(state.shape, -1, np.int16)
    asked = []

    def mark(k, row, h):
        return cref.mark(state, seen, cand[row:row + 1], [h], R, HD, num, den, owner, k)["counters"][4]

    def regain(rows):
        asked.append(np.asarray(rows).copy())
        return cref.gain_unseen(state, seen, cand[rows], R, HD, num, den)["gain"]
    return mark, regain, seen, owner, asked


@pytest.mark.parametrize("dims", list(GRIDS), ids=lambda d: "%dx%dx%d" % d)
def test_cover_on_seeded_grids_and_the_incremental_loop(dims):
    from pi3_slam_amd.view_planner import cover_views
    state, cand, cost, R = _case(dims)
    exp = cref.cover(state, cand, cost, R, HD, *F90)
    m = [p[2] for p in exp["picks"]]
    assert len(m) > 5 and m == sorted(m, reverse=True) and m[-1] >= 1 and m == exp["new"]
    assert exp["covered"] == np.cumsum(m).tolist() and exp["covered"][-1] == cref.popcount(exp["seen"]) == exp["seeable"]
    assert exp["seeable"] == cref.seeable(state, cand, R, HD, *F90)[0] <= int((state == 0).sum())
    by = exp["seen_by"].reshape(-1)
    assert np.bincount(by[by >= 0], minlength=len(m)).tolist() == exp["new"] and by.min() == -1
    assert ((by >= 0) == cref.unpack(exp["seen"], state.size)).all() and (state.reshape(-1)[by >= 0] == 0).all()
    assert len({p[0] for p in exp["picks"]}) < len(exp["picks"])            # a cell is kept with several headings
    assert all(v >= g for v, g in zip(exp["visible"], m)) and len(exp["visible"]) == len(m)
    # the planner's loop, asking only for the rows within 2 R, gives the same list
    mark, regain, seen, owner, asked = _oracle_kernels(state, cand, R, *F90)
    picks, recomputed = cover_views(cand, cost, state.shape, exp["first"]["gain"], 2 * R, None, 1, mark, regain)
    assert [(int(cand[r]), h, g) for r, h, g, _, _ in picks] == exp["picks"]
    assert [p[3] for p in picks] == exp["new"] and [p[4] for p in picks] == exp["covered"]
    assert seen.tobytes() == exp["seen"].tobytes() and owner.tobytes() == exp["seen_by"].tobytes()
    assert recomputed == sum(len(a) for a in asked) and len(asked) == len(picks)
    if dims == (17, 9, 20):
        assert recomputed < len(picks) * len(cand)                          # the short list is shorter
    nz, ny, nx = state.shape
    xyz = np.stack([cand % nx, (cand // nx) % ny, cand // (nx * ny)], 1)
    for (r, *_), rows in zip(picks, asked):
        d2 = ((xyz - xyz[r]) ** 2).sum(1)
        assert sorted(rows.tolist()) == np.flatnonzero(d2 <= (2 * R) ** 2).tolist()
    # stops: a count, a gain, a fraction
    assert cref.cover(state, cand, cost, R, HD, *F90, count=3)["picks"] == exp["picks"][:3]
    n = sum(g >= m[2] for g in m)
    assert cref.cover(state, cand, cost, R, HD, *F90, min_gain=m[2])["picks"] == exp["picks"][:n]
    goal = cref.until_target(0.5, exp["seeable"])
    n = int(np.argmax(np.array(exp["covered"]) >= goal)) + 1
    assert cref.cover(state, cand, cost, R, HD, *F90, until=0.5)["picks"] == exp["picks"][:n]
    mark, regain, *_ = _oracle_kernels(state, cand, R, *F90)
    assert len(cover_views(cand, cost, state.shape, exp["first"]["gain"], 2 * R, 1000, 1, mark, regain, exp["seeable"],
                           0.5)[0]) == n


class _Sets:
    """A hand-built cover problem: (row, heading) sees a set of elements; gains, mark and regain follow from it."""

    def __init__(self, sets, rows, headings):
        self.sets, self.done, self.asked = sets, set(), []
        self.shape = (rows, headings)

    def table(self, rows=None):
        rows = range(self.shape[0]) if rows is None else rows
        return np.array([[len(self.sets.get((r, h), set()) - self.done) for h in range(self.shape[1])] for r in rows])

    def mark(self, k, row, h):
        new = self.sets[(row, h)] - self.done
        self.done |= new
        return len(new)

    def regain(self, rows):
        self.asked.append(list(rows))
        return self.table(rows)


def _span(lo, n):
    return set(range(lo, lo + n))


def test_cover_views_on_hand_built_tables():
    from pi3_slam_amd.view_planner import cover_target, cover_views
    shape = (1, 1, 100)
    # a gain tie goes to the smaller cost, then the smaller cell, then the smaller heading
    s = _Sets({(0, 1): _span(0, 5), (1, 0): _span(10, 5), (2, 0): _span(20, 5), (2, 2): _span(30, 5), (3, 0): _span(40, 6)},
              4, 3)
    cells, cost = np.array([10, 30, 20, 50]), np.array([3, 2, 2, 9])
    picks, rec = cover_views(cells, cost, shape, s.table(), 100, None, 1, s.mark, s.regain)
    assert [(r, h, m) for r, h, m, _, _ in picks] == [(3, 0, 6), (2, 0, 5), (2, 2, 5), (1, 0, 5), (0, 1, 5)]
    assert [p[3] for p in picks] == [6, 5, 5, 5, 5] and [p[4] for p in picks] == [6, 11, 16, 21, 26] and rec == 20
    # only the rows within reach are asked for, the pick among them
    s = _Sets({(0, 0): _span(0, 5), (1, 0): _span(3, 5), (2, 0): _span(20, 4)}, 3, 1)
    picks, rec = cover_views(np.array([10, 12, 40]), np.zeros(3), shape, s.table(), 2, None, 1, s.mark, s.regain)
    assert [(r, m) for r, _, m, _, _ in picks] == [(0, 5), (2, 4), (1, 3)] and s.asked == [[0, 1], [2], [0, 1]] and rec == 5
    # overlapping headings of one cell: the same cell is kept twice, the second time with what is left
    s = _Sets({(0, 0): _span(0, 6), (0, 1): _span(4, 6), (1, 0): _span(20, 3)}, 2, 2)
    picks, _ = cover_views(np.array([5, 6]), np.array([1, 0]), shape, s.table(), 9, None, 1, s.mark, s.regain)
    assert [(r, h, m) for r, h, m, _, _ in picks] == [(0, 0, 6), (0, 1, 4), (1, 0, 3)]

    # gains 5, 4, 3, 2, 1 of 15 seeable: each condition stops one round before the next one would
    def run(count, min_gain, until):
        s = _Sets({(r, 0): _span(10 * r, 5 - r) for r in range(5)}, 5, 1)
        return len(cover_views(np.arange(5), np.zeros(5), shape, s.table(), 9, count, min_gain, s.mark, s.regain, 15,
                               until)[0])
    assert cover_target(0.6, 15) == 9 and cover_target(0.61, 15) == 10 and cover_target(1.0, 15) == 15
    assert run(2, 3, 0.8) == 2 and run(4, 3, 1.0) == 3 and run(4, 1, 0.6) == 2
    assert run(None, 1, None) == 5 and run(4, 1, None) == 4 and run(None, 2, 1.0) == 4 and run(None, 1, 0.61) == 3
    assert run(9, 0, 1.0) == 5 and run(7, 0, None) == 7          # min_gain 0 keeps empty views until the count
    with pytest.raises(ValueError, match="min_gain >= 1"):
        run(None, 0, None)
    with pytest.raises(RuntimeError, match="marked 0 cells, its gain was 5"):
        s = _Sets({(0, 0): _span(0, 5)}, 1, 1)
        cover_views(np.arange(1), np.zeros(1), shape, s.table(), 9, 3, 1, lambda k, r, h: 0, s.regain)
    assert cover_views(np.zeros(0), np.zeros(0), shape, np.zeros((0, 26)), 9, 3, 1, None, None) == ([], 0)


# ------------------------------------------------------------------------------------------------ the box room
@pytest.fixture(scope="module")
def box_room():
    room, state, cams, d2u, walk_u, (R, min_d2) = route_cases.box_room_case()
    nz, ny, nx = state.shape
    lin = [int((c[2] * ny + c[1]) * nx + c[0]) for c in cams]
    d2a = oref.edt_ref(state, R, False)                          # clearance against occupied cells only
    dist = rref.distances(rref.walk_mask(state, d2a, min_d2), lin)
    cells = vref.candidates(dist, room["origin"], 4)
    cost = dist.reshape(-1)[cells].astype(np.int64)
    return room, state, dist, cells, cost, cref.cover(state, cells, cost, 8, HD, *F90)


def test_the_box_room_figures(box_room):
    room, state, dist, cells, cost, full = box_room
    assert len(cells) == 230 and int((state == 0).sum()) == 46000
    assert full["seeable"] == 13828 and len(full["picks"]) == 267 and full["covered"][-1] == 13828
    assert len({p[0] for p in full["picks"]}) == 145
    assert full["picks"][:3] == [(18671, 8, 316), (50671, 25, 316), (19283, 0, 314)]
    assert full["new"][:10] == [316, 316, 314, 314, 312, 312, 299, 299, 267, 267] and full["covered"][9] == 3016
    ten = cref.cover(state, cells, cost, 8, HD, *F90, count=10)
    assert ten["picks"] == full["picks"][:10] and ten["covered"][-1] == 3016 == cref.popcount(ten["seen"])
    covered = np.array(full["covered"])
    assert [int(np.argmax(covered >= cref.until_target(f, 13828))) + 1 for f in (0.5, 0.9, 0.99)] == [29, 104, 195]
    assert len(cref.cover(state, cells, cost, 8, HD, *F90, until=0.5)["picks"]) == 29
    low = cref.cover(state, cells, cost, 8, HD, *F90, min_gain=50)
    assert len(low["picks"]) == 79 and low["covered"][-1] == 11511
    # what find's ten views see together
    s = vref.view_set(state, dist, room["origin"], 8, 4, 90, 10, 4)
    assert [v["gain"] for v in s["views"]] == [316] * 8 + [315] * 2
    seen = _zeros(state)
    for v in s["views"]:
        cref.mark(state, seen, [v["cell"]], [v["heading"]], 8, HD, *F90)
    assert cref.popcount(seen) == 2024


# ------------------------------------------------------------------------------------------------ the host side
def test_planner_arguments_of_the_cover():
    from pi3_slam_amd import ops
    from pi3_slam_amd.view_planner import ViewPlanner
    assert ops.VIEW_MARK_COUNTERS == ("views", "rays", "rays_visible", "in_cone", "new") and ops.VIEW_MAX_TAG == 32767
    assert [ops.grid_view_seen_words(c) for c in (1, 31, 32, 33, 300, 504)] == [1, 1, 1, 2, 10, 16]
    p = ViewPlanner(0.2, 1.6)
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="fraction to cover must lie in \\(0, 1\\]"):
            p.cover(None, [[0.0, 0.0, 0.0]], until=bad)
    with pytest.raises(ValueError, match="separation has no meaning"):
        ViewPlanner(0.2, 1.6, separation_m=0.8).cover(None, [[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="views need a source"):
        p.cover(None, None)
    assert p.separation_m == 0.8 and p.settings()["separation_m"] == 0.8        # find's default stays


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    assert len(lib.SIGNATURES["pi3_grid_view_gain_unseen"]) == 17 and len(lib.SIGNATURES["pi3_grid_view_mark"]) == 17
    for name in ("pi3_grid_view_gain_unseen", "pi3_grid_view_mark"):
        assert f"int {name}(" in text


def test_view_files_of_a_cover(tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.view_planner import View, ViewSet
    shape = (3, 4, 5)
    gain = np.full(shape, -1, np.int32)
    heading = np.full(shape, -1, np.int8)
    gain[1, 2, 3], heading[1, 2, 3] = 40, 13
    origin = np.array([-2, 1, 0], np.int64)
    at = 0.5 * (origin + [3, 2, 1] + 0.5)
    plain = [View(0, 33, at, 13, HD[13].copy(), HD[13] / 1.0, 40, 90, 24, 1.0)]
    plain_set = ViewSet(plain, gain, heading, HD, origin, 0.5, {"candidates": 1, "views": 1}, {"range_m": 1.0})
    assert plain[0].new == -1 and plain[0].covered == -1 and plain_set.seen_by is None and plain_set.mode == "gain"
    seen_by = np.full(shape, -1, np.int16)
    seen_by[0, 0, :3], seen_by[2, 3, 4] = 0, 1
    views = [View(0, 33, at, 13, HD[13].copy(), HD[13] / 1.0, 3, 90, 24, 1.0, 3, 3),
             View(1, 33, at, 25, HD[25].copy(), HD[25] / np.sqrt(3.0), 1, 87, 24, 1.0, 1, 4)]
    cover_set = ViewSet(views, gain, heading, HD, origin, 0.5, {"candidates": 1, "views": 2}, {"mode": "cover"}, None,
                        None, seen_by, "cover")
    assert export.write_views(plain_set, str(tmp_path / "p")) == 1 and export.write_views(cover_set, str(tmp_path / "c")) == 2
    for d in ("p", "c"):
        assert sorted(os.listdir(tmp_path / d)) == ["views.json", "views.npz", "views.ply"]
    rec = json.load(open(tmp_path / "p" / "views.json"))
    assert sorted(rec["views"][0]) == sorted(["rank", "cell", "position", "heading", "axis", "direction", "gain", "visible",
                                              "cost", "distance_m"])
    with np.load(tmp_path / "p" / "views.npz") as z:
        assert sorted(z.files) == ["cell", "gain", "heading", "headings", "index_origin", "origin"]
    rec = json.load(open(tmp_path / "c" / "views.json"))
    assert [(v["rank"], v["cell"], v["heading"], v["gain"], v["new"], v["covered"]) for v in rec["views"]] == [
        (0, 33, 13, 3, 3, 3), (1, 33, 25, 1, 1, 4)]
    with np.load(tmp_path / "c" / "views.npz") as z:
        assert z["seen_by"].dtype == np.int16 and z["seen_by"].tobytes() == seen_by.tobytes() and z["seen_by"].shape == shape
        assert z["gain"].tobytes() == gain.tobytes()


def test_views_parser_of_the_cover():
    from pi3_slam_amd import cli
    base = ["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"]
    a = cli.build_parser().parse_args(base)
    assert a.cover is False and a.cover_until is None and a.separation is None and a.count == 10 and a.min_gain == 1
    a = cli.build_parser().parse_args(base + ["--cover", "--cover-until", "0.9", "--count", "40"])
    assert a.cover is True and a.cover_until == 0.9 and a.count == 40
    with pytest.raises(SystemExit, match="views: --separation has no meaning with --cover"):
        cli.main(base + ["--cover", "--separation", "0.5"])
    with pytest.raises(SystemExit, match="views: --cover-until needs --cover"):
        cli.main(base + ["--cover-until", "0.5"])
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert "--cover-until FRACTION" in text and text.count("a starting point, not a measured optimum") == 3
