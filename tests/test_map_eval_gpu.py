"""The cloud search on the GPU (csrc/cloud_nn.hip through map_eval.CloudIndex) against the brute-force oracle
(tests/cloud_nn_ref.py), byte for byte: every d2, every index, every counter, and the index build's table and rows;
then compare_clouds against itself driven by the oracle, and creator -> reconstruct -> evaluate-map on a small
synthetic room."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_nn_ref as nnref            # noqa: E402
import dense_map_ref as mref            # noqa: E402
import test_dense_carve_gpu as carve_gpu                # noqa: E402  (_reconstruct)
import test_dense_consistency_gpu as cons_gpu           # noqa: E402  (_items)
import test_map_eval as cpu             # noqa: E402  (the planted clouds, the oracle as compare_clouds' search)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GT = cpu.GT
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """voxel_table.h's hash of a key (splitmix64's finaliser)."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def neighbour_evaluations(p_keys, p_ok, q_keys, q_ok):
    """What the kernel's evaluation counter must read: per query that is not dropped, the rows of the existing cells
    among the 27 around its own."""
    cells, counts = np.unique(p_keys[p_ok], return_counts=True)
    size = dict(zip(cells.tolist(), counts.tolist()))
    total = 0
    for key in q_keys[q_ok].tolist():
        k = [(key >> 42) & 0x1FFFFF, (key >> 21) & 0x1FFFFF, key & 0x1FFFFF]
        for c in range(27):
            f = [k[0] + c // 9 - 1, k[1] + (c // 3) % 3 - 1, k[2] + c % 3 - 1]
            if all(1 <= v <= 0x1FFFFF for v in f):
                total += size.get((f[0] << 42) | (f[1] << 21) | f[2], 0)
    return total, size


def check_search(p, q, max_dist, expect_capacity=None):
    """Index p, query q, compare everything with the oracle; -> (oracle result, build stats, query stats)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.map_eval import CloudIndex
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    n, m = len(p), len(q)
    exp = nnref.nearest(p, q, max_dist)
    index = CloudIndex(p, max_dist, DEV)
    d2, idx = index.nearest(torch.from_numpy(q).to(DEV))
    assert d2.dtype == torch.float64 and idx.dtype == torch.int64 and d2.is_cuda and idx.is_cuda
    assert d2.shape == (m,) and idx.shape == (m,)
    got_d2, got_idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert got_d2.tobytes() == exp["d2"].tobytes()
    assert np.array_equal(got_idx, exp["idx"].astype(np.int64))
    assert not np.isnan(got_d2).any()
    qs, bs = dict(index.last_stats), dict(index.build_stats)
    assert {k: qs[k] for k in ("dropped", "matched", "beyond")} == exp["counters"]
    assert qs["dropped"] + qs["matched"] + qs["beyond"] == m == qs["queries"]
    # the index itself: table and rows
    inv = nnref.inv_cell(max_dist)
    assert index.inv_cell == inv and ops.cloud_inv_cell(max_dist) == inv
    cap = index.table.numel() // 8
    assert cap == ops.voxel_capacity(n) and (expect_capacity is None or cap == expect_capacity)
    p_ok, p_keys, _ = mref.quantise(p, inv) if n else (np.zeros(0, bool), np.zeros(0, np.uint64), None)
    q_ok, q_keys, _ = mref.quantise(q, inv) if m else (np.zeros(0, bool), np.zeros(0, np.uint64), None)
    evals, size = neighbour_evaluations(p_keys, p_ok, q_keys, q_ok) if n else (0, {})
    assert bs == dict(dropped=int((~p_ok).sum()), cells=len(size), no_slot=0, largest_cell=max(size.values(), default=0),
                      points=n)
    assert bs["dropped"] == exp["ref_dropped"] and qs["evaluations"] == evals
    table = index.table.cpu().numpy().view(np.uint64).reshape(cap, 8)
    rows = index.cells.cpu().numpy()
    occ = table[:, 0] != EMPTY
    kept = int(p_ok.sum())
    assert int(occ.sum()) == len(size) and int(table[0, 4]) == kept               # the cursor: rows handed out
    assert not table[~occ][:, 1:4].any() and not table[:, 5:].any() and not table[1:, 4].any()
    assert np.array_equal(table[occ, 1], table[occ, 3])                            # every claimed row was filled
    spans = sorted(zip(table[occ, 2].tolist(), table[occ, 1].tolist(), table[occ, 0].tolist()))
    at = 0
    for start, count, key in spans:                                                # contiguous, disjoint, complete
        assert start == at and count == size[key]
        orig = rows[start:start + count, 3]
        assert np.all(p_keys[orig] == np.uint64(key)) and np.all(p_ok[orig])
        assert rows[start:start + count, :3].tobytes() == p[orig].tobytes()
        at += count
    assert at == kept and sorted(rows[:kept, 3].tolist()) == np.flatnonzero(p_ok).tolist()
    # again: the same bytes, whatever order the atomics landed in
    again = CloudIndex(p, max_dist, DEV)
    d2b, idxb = again.nearest(q)
    assert d2b.cpu().numpy().tobytes() == got_d2.tobytes() and torch.equal(idxb, idx)
    return exp, bs, qs


# ------------------------------------------------------------------------------------------------ a. sizes
@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (1, 1), (1, 300), (300, 1), (5000, 5000)])
def test_sizes(n, m):
    rng = np.random.default_rng(1000 * n + m)
    p, q = rng.random((n, 3)).astype(np.float32), rng.random((m, 3)).astype(np.float32)
    if n and m and min(n, m) == 1:
        q[0] = p[n // 2] + np.float32(0.01)              # the single point / single query has a neighbour
    exp, bs, qs = check_search(p, q, 0.05)
    print(f"n={n} m={m}: {bs} {qs}")
    if n == 0:
        assert qs["beyond"] == m and qs["evaluations"] == 0
    if n and m:
        assert qs["matched"] > 0
    if n == m == 5000:
        assert qs["beyond"] > 0 and bs["cells"] > 2000


# ------------------------------------------------------------------------------------------------ b. ties, boundaries
def test_ties_and_the_inclusive_radius():
    R = np.float32(5.0 / 128.0)                          # max_dist; 3-4-5 over 128: every square and sum below is exact
    a, b = np.float32(3.0 / 128.0), np.float32(4.0 / 128.0)
    up, down = np.nextafter(R, np.float32(1)), np.nextafter(R, np.float32(0))
    p = np.array([[0.5, 0.5, 0.5], [2, 2, 2], [0.5, 0.5, 0.5], [2, 2, 2],              # duplicates, interleaved
                  [4, 0, 0], [4 + 2 * a, 0, 0],                                        # a query half way between
                  [6 + 2 * a, 1, 1], [6, 1, 1],                                        # the same, the farther index first
                  [0, 0, 0]], np.float32)
    q = np.array([[0.5, 0.5, 0.5], [2, 2, 2 + a], [4 + a, 0, 0], [6 + a, 1, 1],
                  [R, 0, 0], [a, -b, 0], [0, a, b],                                    # exactly max_dist away: inside
                  [up, 0, 0], [0, -up, 0],                                             # one ulp more: beyond
                  [down, 0, 0]], np.float32)
    assert float(q[7, 0]) > 5 / 128 == float(q[4, 0]) > float(q[9, 0])
    exp, bs, qs = check_search(p, q, float(R))
    assert exp["idx"].tolist() == [0, 1, 4, 6, 8, 8, 8, -1, -1, 8]
    r2 = float(R) * float(R)
    assert exp["d2"][4:7].tolist() == [r2, r2, r2] and exp["d2"][9] < r2 and exp["d2"][2] == float(a) ** 2
    assert qs["matched"] == 8 and qs["beyond"] == 2


# ------------------------------------------------------------------------------------------------ c. cell borders
def test_cell_borders():
    md = 0.05
    cell = 1.25 * md
    assert cell == 0.0625
    g = np.arange(-3, 4, dtype=np.float64) * cell
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)         # on the cells' corners
    ps, qs_ = [lattice], [lattice, lattice + 0.03, lattice - 0.03]
    axis, diag = np.array([1.0, 0, 0]), np.ones(3) / np.sqrt(3.0)
    j = 0
    for u in (axis, axis[[1, 0, 2]], axis[[2, 1, 0]], diag, diag * [1, -1, 1], -diag):
        for border in (-2 * cell, 0.0, 3 * cell):
            for reach in (0.0499, 0.0501):                                             # just inside, just outside
                for back in (0.001, 0.02, 0.045):
                    j += 1                                                             # every pair alone, 4 cells from the next
                    base = np.full(3, border) + cell * 4 * (j + 1) * (-1) ** j         # a corner of cells, either sign
                    ps.append((base - back * u)[None])
                    qs_.append((base + (reach - back) * u)[None])
    p, q = np.concatenate(ps).astype(np.float32), np.concatenate(qs_).astype(np.float32)
    exp, bs, qs = check_search(p, q, md)
    pairs = exp["idx"][3 * len(lattice):]
    assert (pairs >= 0).sum() == (pairs < 0).sum() == len(pairs) // 2                  # every 0.0499 pair, no 0.0501 pair
    assert (exp["idx"][: len(lattice)] == np.arange(len(lattice))).all() and (exp["d2"][: len(lattice)] == 0).all()
    assert (p < 0).any() and (q < 0).any()


# ------------------------------------------------------------------------------------------------ d. long lists, probing
def test_three_thousand_points_in_one_cell():
    md = 0.05
    rng = np.random.default_rng(9)
    inside = (0.0625 * (2.0 + rng.random((3000, 3)))).astype(np.float32)               # all in cell (2, 2, 2)
    inside = np.clip(inside, np.float32(0.125), np.nextafter(np.float32(0.1875), np.float32(0)))
    others = (rng.random((40, 3)) * 0.4).astype(np.float32)
    p = np.concatenate([others[:20], inside, others[20:]])
    q = np.concatenate([(0.0625 * (1.0 + 3.0 * rng.random((300, 3)))).astype(np.float32), inside[::50]])
    exp, bs, qs = check_search(p, q, md)
    assert bs["largest_cell"] >= 3000 and qs["matched"] > 200 and qs["evaluations"] > 300 * 1000


def test_tiny_table_where_probing_wraps():
    md = 0.05
    inv = nnref.inv_cell(md)
    # four cells whose hash lands on the last slot of an 8-slot table: they fill slots 7, 0, 1, 2
    cells = []
    for k in range(1, 4000):
        key = ((k + mref.BIAS) << 42) | ((3 + mref.BIAS) << 21) | (5 + mref.BIAS)
        if mix64(key) & 7 == 7:
            cells.append(k)
        if len(cells) == 4:
            break
    assert len(cells) == 4
    p = np.array([[(k + 0.5) / inv, 3.5 / inv, 5.5 / inv] for k in cells], np.float32)
    q = np.concatenate([p + np.float32(0.01), p - np.float32(0.02), p + np.float32(0.2)])
    exp, bs, qs = check_search(p, q, md, expect_capacity=8)
    assert bs["cells"] == 4 and exp["idx"][:8].tolist() == [0, 1, 2, 3] * 2 and qs["matched"] >= 8


def test_a_table_without_a_free_slot():
    """Nine cells into a table of eight slots: the arm of the shared slot claim (voxel_table.h, slot_claim) that gives
    up after `capacity` probes, and the lookups of a table that has no empty slot to stop at.  The fusion entry points
    refuse capacity < 2 n, so only the cloud index gets there.  Which point loses its slot depends on scheduling;
    nothing asserted here does."""
    from pi3_slam_amd import ops
    md, cap, sentinel = 0.05, 8, -7
    inv = ops.cloud_inv_cell(md)
    p = np.array([[(3 * j + 0.5) / inv, 3.5 / inv, 5.5 / inv] for j in range(9)], np.float32)   # 3 cells apart on x
    ok, keys, _ = mref.quantise(p, inv)
    assert ok.all() and np.diff(np.sort(keys >> np.uint64(42)).astype(np.int64)).min() >= 3
    pts = torch.from_numpy(p).to(DEV)
    seen = []
    for _ in range(2):
        table = torch.full((cap * 8,), 5, dtype=torch.int64, device=DEV)
        cells = torch.full((9, 4), sentinel, dtype=torch.int32, device=DEV)
        built = torch.full((4,), 11, dtype=torch.int64, device=DEV)
        ops.cloud_index_build(pts, inv, table, cells, built)
        d2 = torch.full((9,), 5.0, dtype=torch.float64, device=DEV)
        idx = torch.full((9,), 5, dtype=torch.int32, device=DEV)
        asked = torch.full((4,), 11, dtype=torch.int64, device=DEV)
        ops.cloud_nearest(table, cells, inv, pts, md, d2, idx, asked)
        torch.cuda.synchronize()
        bs = dict(zip(ops.CLOUD_INDEX_COUNTERS, built.tolist()))
        assert bs == dict(dropped=0, cells=8, no_slot=1, largest_cell=1)
        t = table.cpu().numpy().view(np.uint64).reshape(cap, 8)
        assert (t[:, 0] != EMPTY).all() and int(t[0, 4]) == 8                          # full; the cursor: 8 rows
        assert (t[:, 1] == 1).all() and (t[:, 3] == 1).all() and sorted(t[:, 2].tolist()) == list(range(8))
        rows = cells.cpu().numpy()
        orig = rows[:8, 3]
        assert sorted(set(orig.tolist())) == sorted(orig.tolist()) and set(orig.tolist()) < set(range(9))
        assert rows[:8, :3].tobytes() == p[orig].tobytes() and (rows[8] == sentinel).all()
        assert set(keys[orig].tolist()) == set(t[:, 0].tolist())
        lost = (set(range(9)) - set(orig.tolist())).pop()
        got_d2, got_idx = d2.cpu().numpy(), idx.cpu().numpy()
        exp_d2, exp_idx = np.zeros(9), np.arange(9, dtype=np.int32)
        exp_d2[lost], exp_idx[lost] = np.inf, -1
        assert got_d2.tobytes() == exp_d2.tobytes() and np.array_equal(got_idx, exp_idx)
        qs = dict(zip(ops.CLOUD_NEAREST_COUNTERS, asked.tolist()))
        assert {k: qs[k] for k in ("matched", "beyond", "dropped")} == dict(matched=8, beyond=1, dropped=0)
        seen.append((bs, qs))
    assert seen[0] == seen[1]


# ------------------------------------------------------------------------------------------------ e. large coordinates
def test_large_coordinates():
    rng = np.random.default_rng(1000 * 5000 + 5000)
    shift = np.array([9000.0, -9000.0, 4000.0])
    p = (rng.random((5000, 3)) + shift).astype(np.float32)
    q = (rng.random((5000, 3)) + shift).astype(np.float32)
    inv = nnref.inv_cell(0.05)
    s = np.abs(p[:, 0] * np.float32(inv))
    assert 1.4e5 < s.min() and np.spacing(s.max()) == np.float32(2.0 ** -6)            # 6 fraction bits left
    exp, bs, qs = check_search(p, q, 0.05)
    print(f"large coordinates: {bs} {qs}")
    assert qs["matched"] > 1000 and qs["beyond"] > 100 and qs["dropped"] == 0


# ------------------------------------------------------------------------------------------------ f. drops
def test_dropped_points_and_queries():
    md = 0.05
    edge = 65536.0                                                                     # 2^20 cells of 1 / 16
    rng = np.random.default_rng(13)
    good = rng.random((200, 3)).astype(np.float32)
    last = np.nextafter(np.float32(edge), np.float32(0))                               # the last coordinate inside
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [edge, 0, 0], [0, -edge - 1, 0], [1e30, 0, 0],
                    [0.5, 0.5, 3e38]], np.float32)
    rim = np.array([[last, 0.5, 0.5], [-edge, 0.5, 0.5], [0.5, -edge, last]], np.float32)        # in range: |k| = 2^20 - 1 and k = -2^20?
    p = np.concatenate([good[:100], bad, rim, good[100:]])
    q = np.concatenate([bad, rim, rim + np.float32([0, 0.01, 0]), good[:50] + np.float32(0.01), bad[::-1]])
    exp, bs, qs = check_search(p, q, md)
    ok = mref.quantise(rim, nnref.inv_cell(md))[0]
    assert ok.tolist() == [True, False, False]                                         # k = -2^20 is out: |k| < 2^20
    assert bs["dropped"] == len(bad) + 2 and qs["dropped"] == 2 * len(bad) + 4
    assert exp["idx"][len(bad)] == 100 + len(bad) and qs["matched"] >= 50


# ------------------------------------------------------------------------------------------------ the entry points' checks
def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    n, m, cap = 100, 50, 256
    pts = torch.rand(n, 3, device=DEV)
    table = torch.full((cap * 8,), 5, dtype=torch.int64, device=DEV)
    cells = torch.full((n, 4), 5, dtype=torch.int32, device=DEV)
    d2 = torch.full((m,), 5.0, dtype=torch.float64, device=DEV)
    idx = torch.full((m,), 5, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    inf, nan = float("inf"), float("nan")

    def build(n_=n, inv=16.0, cap_=cap, **null):
        a = dict(points=pts.data_ptr(), table=table.data_ptr(), cells=cells.data_ptr(), counters=counters.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_cloud_index_build(a["points"], n_, inv, a["table"], cap_, a["cells"], a["counters"], L.stream_ptr())

    def query(n_=n, m_=m, inv=16.0, md=0.05, cap_=cap, **null):
        a = dict(table=table.data_ptr(), cells=cells.data_ptr(), queries=pts.data_ptr(), d2=d2.data_ptr(), idx=idx.data_ptr(),
                 counters=counters.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_cloud_nearest(a["table"], cap_, a["cells"], n_, inv, a["queries"], m_, md, a["d2"], a["idx"],
                                     a["counters"], L.stream_ptr())

    for kw in [dict(n_=-1), dict(n_=1 << 31), dict(inv=0.0), dict(inv=-1.0), dict(inv=inf), dict(inv=nan), dict(cap_=0),
               dict(cap_=cap - 1), dict(points=1), dict(table=1), dict(cells=1), dict(counters=1)]:
        assert build(**kw) == -1, kw
        assert b"pi3_cloud_index_build" in lib.pi3_last_error()
    for kw in [dict(n_=-1), dict(n_=1 << 31), dict(m_=-1), dict(inv=0.0), dict(inv=inf), dict(inv=nan), dict(md=0.0),
               dict(md=-1.0), dict(md=inf), dict(md=nan), dict(md=0.0625), dict(cap_=0), dict(cap_=cap + 1), dict(table=1),
               dict(cells=1), dict(queries=1), dict(d2=1), dict(idx=1), dict(counters=1)]:
        assert query(**kw) == -1, kw
        assert b"pi3_cloud_nearest" in lib.pi3_last_error()
    torch.cuda.synchronize()
    assert bool((table == 5).all()) and bool((cells == 5).all()) and bool((d2 == 5).all()) and bool((idx == 5).all())
    assert counters.tolist() == [11] * 4
    assert build() == 0 and query(m_=0, queries=1, d2=1, idx=1) == 0                   # no query: counters zeroed, no output
    torch.cuda.synchronize()
    assert counters.tolist() == [0] * 4 and bool((d2 == 5).all()) and int(table[4]) == n
    assert query() == 0
    torch.cuda.synchronize()
    assert counters.tolist()[1] == m and bool((d2 == 0).all()) and idx.tolist() == list(range(m))


# ------------------------------------------------------------------------------------------------ g. compare_clouds
def _same_result(got, exp):
    from pi3_slam_amd.map_eval import public
    a, b = public(got), public(exp)
    a.pop("search"), b.pop("search")
    assert a == b
    for k in ("estimate", "reference"):
        assert got["_distances"][k].tobytes() == exp["_distances"][k].tobytes()
        assert got["_points"][k].tobytes() == exp["_points"][k].tobytes()


def test_compare_clouds_equals_itself_driven_by_the_oracle():
    from scipy.spatial.transform import Rotation
    from pi3_slam_amd.map_eval import compare_clouds, tau_key
    rng = np.random.default_rng(21)
    ref = rng.random((4000, 3)).astype(np.float32) * np.float32([2, 1, 1])
    est = (ref[:3000] + 0.02 * rng.standard_normal((3000, 3))).astype(np.float32)
    est[::97] = np.nan                                                                 # dropped points take part
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 1.3 * Rotation.from_rotvec([0.2, -0.4, 0.7]).as_matrix(), [0.5, -1.0, 2.0]
    moved = ((est.astype(np.float64) - M[:3, 3]) @ M[:3, :3] / 1.3 ** 2).astype(np.float32)      # M moved = est, nearly
    ths = [0.01, 0.03, 0.05]
    for kw in (dict(), dict(max_dist=0.07), dict(voxel_size=0.04), dict(transform=M), dict(transform=M, voxel_size=0.04)):
        e = moved if "transform" in kw else est
        got = compare_clouds(e, ref, ths, device=DEV, **kw)
        exp = compare_clouds(e, ref, ths, device=DEV, _nearest=cpu.oracle_search, **kw)
        _same_result(got, exp)
        st = got["accuracy"]
        assert st["matched"] + st["beyond"] == got["points"]["estimate_used"] == st["points"]
        assert got["completeness"]["points"] == got["points"]["reference_used"]
        assert got["search"]["accuracy"]["evaluations"] > 0 and got["search"]["accuracy"]["cells"] > 0
        if "voxel_size" in kw:
            assert got["points"]["estimate_used"] < 3000 and got["points"]["reference_used"] < 4000
        else:
            assert got["dropped"] == {"estimate": len(est[::97]), "reference": 0}
            assert 0.5 < got["precision"][tau_key(0.05)] < 1.0
        print(kw.keys(), {k: got[k] for k in ("points", "precision", "recall", "fscore")})


def test_planted_identity_and_a_cloud_against_itself_on_the_device():
    from pi3_slam_amd.map_eval import compare_clouds, tau_key
    V, K, md = 600, 37, 0.1
    ref, est, far = cpu.planted(V, K, md)
    res = compare_clouds(est, ref, [0.0, 0.05], max_dist=md, device=DEV)
    _same_result(res, compare_clouds(est, ref, [0.0, 0.05], max_dist=md, device=DEV, _nearest=cpu.oracle_search))
    for t in (0.0, 0.05):
        k = tau_key(t)
        assert res["precision"][k] == V / (V + K) and res["recall"][k] == 1.0
    assert res["accuracy"]["beyond"] == K and res["completeness"]["beyond"] == 0
    same = compare_clouds(ref, ref, [0.0, 0.05], device=DEV)
    for t in (0.0, 0.05):
        k = tau_key(t)
        assert same["precision"][k] == same["recall"][k] == same["fscore"][k] == 1.0
    assert not same["_distances"]["estimate"].any() and not same["_distances"]["reference"].any()
    assert same["accuracy"]["max"] == 0.0 and same["completeness"]["beyond"] == 0


# ------------------------------------------------------------------------------------------------ h. end to end
H, W, FRAMES, CHUNK, OVERLAP = 48, 64, 24, 12, 4
VOXEL, EVAL_VOXEL, THRESHOLDS, MAX_DIST = 0.05, 0.1, (0.1, 0.2), 0.4


def _create(seq, out_dir):
    """Stage 1 of the small room through the real creator, the scene in the network's place."""
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=True, num_loader_workers=0, dense_voxel_size=VOXEL)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    _, manifest, _ = cr.write_chunks(cr.process_chunks(cons_gpu._items(seq, cr.device, range(len(seq.chunks)))))
    cr.write_run_metadata(manifest)


@pytest.mark.parametrize("noise", ["NOISE_NONE", "NOISE_BF16"])
def test_creator_reconstruct_evaluate_map(noise, tmp_path, capsys):
    """24 frames of 48 x 64 in chunks of 12 / 4 -> dense_points.ply (5 cm voxels, no bundle adjustment), scored
    against the room's reference cloud after the trajectory pair's alignment, both resampled at 10 cm.  The scores
    are printed, not bounded: nothing exists yet to hold them against (DESIGN.md 7d records them)."""
    import synth_sequence as ss
    from pi3_slam_amd import cli, map_eval
    from pi3_slam_amd.export import write_ply
    seq = ss.SyntheticSequence(GT, H=H, W=W, chunk_length=CHUNK, overlap=OVERLAP, n_frames=FRAMES, max_kp=100,
                               noise=dict(getattr(ss, noise)))
    assert len(seq.chunks) == 3
    _create(seq, str(tmp_path / "chunks"))
    carve_gpu._reconstruct(str(tmp_path / "chunks"), str(tmp_path / "rec"))
    est_ply, est_tum = str(tmp_path / "rec" / "dense_points.ply"), str(tmp_path / "rec" / "trajectory_tum.txt")
    ref_ply = str(tmp_path / "reference.ply")
    cloud = seq.reference_cloud().numpy()
    write_ply(cloud, np.full((len(cloud), 3), 200, np.uint8), ref_ply)
    capsys.readouterr()
    argv = ["evaluate-map", "--estimate", est_ply, "--reference", ref_ply, "--thresholds"] + [str(t) for t in THRESHOLDS] + \
           ["--max-dist", str(MAX_DIST), "--voxel-size", str(EVAL_VOXEL), "--estimate-trajectory", est_tum,
            "--reference-trajectory", GT, "--device", DEV]
    cli.main(argv + ["--json", "--error-ply", str(tmp_path / "error.ply")])
    said = capsys.readouterr().out.strip().splitlines()
    assert len(said) == 1
    from_cli = json.loads(said[0])
    est, _ = map_eval.read_ply_points(est_ply)
    ref, _ = map_eval.read_ply_points(ref_ply)
    assert ref.tobytes() == cloud.tobytes() and len(est) > 1000
    T = map_eval.trajectory_alignment(est_tum, GT)
    res = map_eval.compare_clouds(est, ref, THRESHOLDS, max_dist=MAX_DIST, transform=T, voxel_size=EVAL_VOXEL, device=DEV)
    assert from_cli == json.loads(json.dumps(map_eval.public(res))) == map_eval.public(res)
    # the device's distances are the oracle's, byte for byte, on the clouds that were compared
    pe, pr = res["_points"]["estimate"], res["_points"]["reference"]
    for queries, indexed, who in ((pe, pr, "estimate"), (pr, pe, "reference")):
        exp = nnref.nearest(indexed, queries, MAX_DIST)
        assert np.sqrt(exp["d2"]).tobytes() == res["_distances"][who].tobytes()
        st = res["accuracy" if who == "estimate" else "completeness"]
        assert st["matched"] == exp["counters"]["matched"] and st["beyond"] == len(queries) - st["matched"]
        assert st["points"] == len(queries) == res["points"][who + "_used"] and res["dropped"][who] == 0
    assert res["points"]["estimate"] == len(est) and res["points"]["reference"] == len(ref)
    # the error PLY: the compared estimate, coloured by the fixed ramp
    ep, ec = map_eval.read_ply_points(str(tmp_path / "error.ply"))
    assert ep.tobytes() == pe.tobytes()
    assert ec.tobytes() == map_eval.error_colors(res["_distances"]["estimate"], MAX_DIST).tobytes()
    # the table
    cli.main(argv)
    table = capsys.readouterr().out
    assert "accuracy" in table and "completeness" in table and "fscore" in table
    print(f"{noise}: {res['points']}")
    print(table)
