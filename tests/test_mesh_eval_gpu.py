"""The mesh search and the surface sampler on the GPU (csrc/mesh_nn.hip, csrc/mesh_sample.hip through map_eval.MeshIndex
and sample_surface) against the brute-force oracle (tests/mesh_eval_ref.py), byte for byte: every d2, face, closest
point and counter, the index's table and rows, every sample; then compare_clouds with mesh sides against itself driven
by the oracle, the planted room as a 22-triangle reference, and evaluate-map --mesh-surface end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_icp_ref as icpref          # noqa: E402
import dense_map_ref as mref            # noqa: E402
import mesh_eval_ref as meshref         # noqa: E402
import test_map_eval as cloud_cpu       # noqa: E402  (the point oracle as compare_clouds' search)
import test_mesh_eval as cpu            # noqa: E402  (the meshes, the oracle as compare_clouds' hooks)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
M64 = (1 << 64) - 1
CELL = 0.0625                            # 1.25 * 0.05


def mix64(x: int) -> int:
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def boxes(v, f, ok, inv):
    """Per kept triangle the biased cell indices lo, hi (T,3) of its bounding box, from the quantiser alone."""
    corners = v[f[ok]].reshape(-1, 3)
    good, keys, _ = mref.quantise(corners, inv)
    assert good.all()
    k = np.stack([(keys >> np.uint64(42 - 21 * a)) & np.uint64(0x1FFFFF) for a in range(3)], 1).astype(np.int64)
    k = k.reshape(-1, 3, 3)
    return k.min(1), k.max(1)


def cells_of(lo, hi, faces_kept):
    """cell key -> sorted faces with a row there, by enumerating every box."""
    keys, who = [], []
    for (l, h, face) in zip(lo, hi, faces_kept):
        g = np.stack(np.meshgrid(*[np.arange(l[a], h[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
        keys.append((g[:, 0] << 42) | (g[:, 1] << 21) | g[:, 2])
        who.append(np.full(len(g), face, np.int64))
    if not keys:
        return {}
    keys, who = np.concatenate(keys), np.concatenate(who)
    order = np.lexsort((who, keys))
    keys, who = keys[order], who[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    return {int(keys[s]): who[s:e] for s, e in zip(starts, np.r_[starts[1:], len(keys)])}


def check_mesh(v, f, q, max_dist, table_check=True, **kw):
    """Index the mesh, query q, compare everything with the oracle; -> (oracle result, build stats, query stats)."""
    from pi3_slam_amd.map_eval import MeshIndex
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    F, m = len(f), len(q)
    exp = meshref.nearest(v, f, q, max_dist)
    index = MeshIndex(v, f, max_dist, DEV, **kw)
    d2, face, closest = index.nearest(torch.from_numpy(q).to(DEV))
    assert d2.dtype == torch.float64 and face.dtype == torch.int64 and closest.dtype == torch.float32
    assert d2.shape == (m,) and face.shape == (m,) and closest.shape == (m, 3) and d2.is_cuda
    got_d2, got_face, got_cp = d2.cpu().numpy(), face.cpu().numpy(), closest.cpu().numpy()
    assert not np.isnan(got_d2).any() and not np.isnan(got_cp).any()
    assert np.array_equal(got_face, exp["idx"].astype(np.int64))
    assert got_d2.tobytes() == exp["d2"].tobytes()
    assert got_cp.tobytes() == exp["closest"].tobytes()
    qs, bs = dict(index.last_stats), dict(index.build_stats)
    assert {k: qs[k] for k in ("dropped", "matched", "beyond")} == exp["counters"]
    assert qs["dropped"] + qs["matched"] + qs["beyond"] == m == qs["queries"]
    # the index: rows per box, cells, the evaluation counter
    inv = meshref.inv_cell(max_dist)
    assert index.inv_cell == inv
    ok = meshref.triangle_ok(v, f, inv) if F else np.zeros(0, bool)
    lo, hi = boxes(v, f, ok, inv) if ok.any() else (np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64))
    rows = int(np.prod(hi - lo + 1, axis=1).sum())
    assert bs["dropped"] == exp["ref_dropped"] == int((~ok).sum()) and bs["rows"] == rows == index.rows.numel()
    assert bs["no_slot"] == 0 and bs["faces"] == F
    packed = index.packed.cpu().numpy()
    assert packed[:, 11].view(np.int32).tolist() == np.where(ok, np.arange(F), -1).tolist()
    assert packed[ok][:, :9].tobytes() == v[f[ok]].reshape(-1, 9).tobytes() and not packed[:, 9:11].any()
    q_ok, q_keys, _ = mref.quantise(q, inv) if (m and F) else (np.zeros(m, bool), np.zeros(m, np.uint64), None)
    if q_ok.any() and len(lo):
        kq = np.stack([(q_keys[q_ok] >> np.uint64(42 - 21 * a)) & np.uint64(0x1FFFFF) for a in range(3)], 1).astype(np.int64)
        first = np.maximum(np.maximum(kq - 1, 1)[:, None, :], lo[None])
        last = np.minimum(np.minimum(kq + 1, 0x1FFFFF)[:, None, :], hi[None])
        evals = int(np.prod(np.maximum(last - first + 1, 0), axis=2).sum())
    else:
        evals = 0
    assert qs["evaluations"] == evals
    if table_check:
        cells = cells_of(lo, hi, np.flatnonzero(ok))
        assert bs["cells"] == len(cells) and bs["largest_cell"] == max((len(c) for c in cells.values()), default=0)
        cap = index.table.numel() // 8
        table = index.table.cpu().numpy().view(np.uint64).reshape(cap, 8)
        got_rows = index.rows.cpu().numpy()
        occ = table[:, 0] != EMPTY
        assert int(occ.sum()) == len(cells) and int(table[0, 4]) == rows
        assert np.array_equal(table[occ, 1], table[occ, 3]) and not table[~occ][:, 1:4].any()
        at = 0
        for start, count, key in sorted(zip(table[occ, 2].tolist(), table[occ, 1].tolist(), table[occ, 0].tolist())):
            assert start == at and np.array_equal(np.sort(got_rows[start:start + count]), cells[key])
            at += count
        assert at == rows
    # again: the same bytes, whatever order the atomics landed in
    again = MeshIndex(v, f, max_dist, DEV, **kw)
    d2b, faceb, cpb = again.nearest(q)
    assert d2b.cpu().numpy().tobytes() == got_d2.tobytes() and torch.equal(faceb, face) and torch.equal(cpb, closest)
    return exp, bs, qs


def near_surface(v, f, count, rng, spread):
    """count queries: points of random kept triangles moved by `spread` times a normal deviate."""
    t = v[f[rng.integers(0, len(f), count)]].astype(np.float64)
    r = rng.random((count, 2))
    fold = r.sum(1) > 1
    r[fold] = 1 - r[fold]
    p = t[:, 0] + r[:, :1] * (t[:, 1] - t[:, 0]) + r[:, 1:] * (t[:, 2] - t[:, 0])
    return (p + spread * rng.standard_normal((count, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ a. sizes
@pytest.mark.parametrize("F,m", [(0, 5), (5, 0), (1, 1), (1, 300), (300, 1), (2000, 3000)])
def test_sizes(F, m):
    rng = np.random.default_rng(1000 * F + m)
    v, f = cpu.random_triangles(F, rng, 0.5 * CELL, 3 * CELL)
    q = (rng.random((m, 3)) * 1.4 - 0.2).astype(np.float32)                           # around the triangles' cube too
    if F and m:
        k = m if F == 1 else max(m // 2, 1)
        q[:k] = near_surface(v, f, k, rng, 0.01)
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    print(f"F={F} m={m}: {bs} {qs}")
    if F == 0:
        assert qs["beyond"] == m and qs["evaluations"] == 0 and bs["rows"] == 0
    if F and m:
        assert qs["matched"] > 0
    if F == 2000:
        assert qs["beyond"] > 100 and qs["matched"] > 1500 and bs["largest_cell"] > 1 and bs["rows"] > 4 * F
        assert len(set(exp["idx"].tolist())) > 500


# ------------------------------------------------------------------------------------------------ b. regions, radius
def test_seven_regions_and_the_inclusive_radius():
    q = np.array([c[1] for c in cpu.REGION_CASES], np.float32)
    exp, bs, qs = check_mesh(cpu.TRI_V, cpu.TRI_F, q, 8.0)
    assert exp["d2"][:6].tolist() == [c[3] for c in cpu.REGION_CASES[:6]] and qs["matched"] == 7
    on = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [2, 0, 0], [0, 1.5, 0], [2, 1.5, 0], [1, 1, 0]], np.float32)
    R = np.float32(5.0 / 128.0)
    a, b = np.float32(3.0 / 128.0), np.float32(4.0 / 128.0)
    up = np.nextafter(R, np.float32(1))
    edge = np.array([[1, 1, R], [1, 1, -R], [2, -a, b], [-a, -b, 0], [1, 1, up], [-up, 0, 0], [4 + R, 0, 0]], np.float32)
    exp, bs, qs = check_mesh(cpu.TRI_V, cpu.TRI_F, np.concatenate([on, edge]), float(R))
    r2 = float(R) * float(R)
    assert not exp["d2"][:7].any() and exp["closest"][:7].tobytes() == on.tobytes()
    assert exp["d2"][7:].tolist() == [r2, r2, r2, r2, np.inf, np.inf, r2] and bs["rows"] > 3000
    assert exp["idx"].tolist() == [0] * 11 + [-1, -1, 0]


# ------------------------------------------------------------------------------------------------ c. ties
def test_ties_go_to_the_smaller_face_index():
    v = np.array([[0, 0, 0], [0, 1, 0], [1, 0.5, 0], [-1, 0.5, 0]], np.float32)
    q = np.array([[0, 0.5, 0.25], [0.5, 0.5, 0.1], [0, 0.25, 0], [0, 1, 0.1], [-0.5, 0.5, -0.2]], np.float32)
    for faces, want in (([[0, 1, 2], [1, 0, 3]], [0, 0, 0, 0, 1]), ([[1, 0, 3], [0, 1, 2]], [0, 1, 0, 0, 0]),
                        ([[0, 1, 2], [0, 1, 2]], [0, 0, 0, 0, -1]),
                        ([[3, 0, 1], [2, 0, 1], [0, 1, 2], [3, 0, 1]], [0, 1, 0, 0, 0])):
        exp, bs, qs = check_mesh(v, np.array(faces, np.int32), q, 0.3)
        assert exp["idx"].tolist() == want


# ------------------------------------------------------------------------------------------------ d. large triangles
def test_a_wall_of_two_triangles():
    rng = np.random.default_rng(31)
    v = np.array([[-2, -1.5, 0.3], [2, -1.5, 0.3], [2, 1.5, 0.3], [-2, 1.5, 0.3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    q = np.c_[rng.uniform(-2.1, 2.1, 3000), rng.uniform(-1.6, 1.6, 3000), 0.3 + rng.uniform(-0.07, 0.07, 3000)]
    q[:200, 1] = q[:200, 0] * 0.75                                                       # on the shared diagonal
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    print(f"wall: {bs} {qs}")
    assert bs["rows"] > 2 * 3000 and bs["cells"] > 3000 and bs["largest_cell"] == 2
    assert qs["matched"] > 1500 and qs["beyond"] > 300 and set(exp["idx"].tolist()) == {-1, 0, 1}
    inside = (np.abs(q[:, 0]) < 2) & (np.abs(q[:, 1]) < 1.5) & (exp["idx"] >= 0)
    dz = q[inside, 2].astype(np.float32).astype(np.float64) - float(np.float32(0.3))
    assert np.abs(np.sqrt(exp["d2"][inside]) - np.abs(dz)).max() < 1e-12


def test_a_skewed_triangle_over_forty_cells_cubed():
    rng = np.random.default_rng(32)
    v = np.array([[0.01, 0.02, 0.03], [2.49, 0.3, 2.45], [0.2, 2.48, 1.0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    q = np.concatenate([near_surface(v, f, 800, rng, 0.03), rng.random((200, 3)).astype(np.float32) * 2.5])
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    print(f"skewed: {bs} {qs}")
    assert bs["rows"] == bs["cells"] == 40 ** 3 and qs["matched"] > 400 and qs["beyond"] > 200


# ------------------------------------------------------------------------------------------------ e. cell borders
def test_vertices_on_cell_borders():
    rng = np.random.default_rng(33)
    lattice = rng.integers(-6, 7, (60, 3, 3)).astype(np.float64) * CELL                  # every vertex on a cell corner
    v = lattice.reshape(-1, 3).astype(np.float32)
    f = np.arange(180, dtype=np.int32).reshape(60, 3)
    g = np.arange(-6, 7) * CELL
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    q = np.concatenate([grid, grid + 0.03, grid - 0.03, near_surface(v, f[meshref.triangle_ok(v, f, 16.0)], 500, rng, 0.02)])
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    assert qs["matched"] > 1000 and qs["beyond"] > 500 and (exp["d2"] == 0).sum() > 100 and (v < 0).any()


# ------------------------------------------------------------------------------------------------ f. large coordinates
def test_large_coordinates():
    rng = np.random.default_rng(34)
    shift = np.array([9000.0, -9000.0, 4000.0])
    v, f = cpu.random_triangles(1500, rng, 0.5 * CELL, 3 * CELL)
    v = (v.astype(np.float64) + shift).astype(np.float32)
    q = np.concatenate([near_surface(v, f, 1500, rng, 0.03), (rng.random((500, 3)) * 1.6 - 0.3 + shift).astype(np.float32)])
    s = np.abs(v[:, 0] * np.float32(meshref.inv_cell(0.05)))
    assert 1.4e5 < s.min() and np.spacing(s.max()) == np.float32(2.0 ** -6)            # 6 fraction bits left
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    print(f"large coordinates: {bs} {qs}")
    assert qs["matched"] > 1000 and qs["beyond"] > 100 and qs["dropped"] == 0


# ------------------------------------------------------------------------------------------------ g. drops
def test_every_drop_rule():
    rng = np.random.default_rng(35)
    v, f = cpu.random_triangles(100, rng, 0.5 * CELL, 3 * CELL)
    V = len(v)
    extra = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, 7e4], [0.5, 0.5, 0.5], [0.75, 0.75, 0.75],
                      [1.0, 1.0, 1.0], [65535.9, 0.5, 0.5], [65535.9, 0.6, 0.5], [65535.9, 0.5, 0.6]], np.float32)
    v = np.concatenate([v, extra])
    bad = np.array([[0, 1, V + 9], [0, -1, 2], [2 ** 31 - 1, 1, 2], [-2 ** 31, 1, 2],   # index out of range
                    [3, 3, 4], [5, 6, 5],                                               # a repeated index: zero area
                    [0, 1, V], [0, V + 1, 2], [V + 2, 1, 2],                            # NaN, inf, outside the grid
                    [V + 3, V + 4, V + 5]], np.int32)                                   # three points on a line
    rim = np.array([[V + 6, V + 7, V + 8]], np.int32)                                   # the last cells inside: kept
    f = np.concatenate([f[:50], bad, rim, f[50:]]).astype(np.int32)
    q = np.concatenate([near_surface(v[:V], f[:50], 300, rng, 0.02), extra[:3], extra[6:] + np.float32([0, 0.02, 0.02]),
                        [[-65536.0, 0, 0], [65536.0, 0, 0]]]).astype(np.float32)
    exp, bs, qs = check_mesh(v, f, q, 0.05)
    assert bs["dropped"] == len(bad) and qs["dropped"] == 5 and qs["matched"] > 250
    assert not (set(exp["idx"].tolist()) & set(range(50, 50 + len(bad)))) and 50 + len(bad) in exp["idx"].tolist()
    # a mesh of dropped triangles only: queries are still quantised, none finds anything
    exp, bs, qs = check_mesh(v, bad, q, 0.05)
    assert bs["rows"] == 0 and bs["cells"] == 0 and qs["matched"] == 0 and qs["dropped"] == 5


# ------------------------------------------------------------------------------------------------ h. the table
def _one_cell_triangles(cells, inv):
    """One small triangle inside each cell (k, 3, 5)."""
    v = np.array([[[(k + 0.3) / inv, 3.3 / inv, 5.3 / inv], [(k + 0.7) / inv, 3.4 / inv, 5.3 / inv],
                   [(k + 0.4) / inv, 3.7 / inv, 5.6 / inv]] for k in cells], np.float32).reshape(-1, 3)
    return v, np.arange(3 * len(cells), dtype=np.int32).reshape(-1, 3)


def test_tiny_table_where_probing_wraps():
    md = 0.05
    inv = meshref.inv_cell(md)
    cells = []
    for k in range(1, 4000):                    # four cells whose hash lands on the last slot of an 8-slot table
        key = ((k + mref.BIAS) << 42) | ((3 + mref.BIAS) << 21) | (5 + mref.BIAS)
        if mix64(key) & 7 == 7:
            cells.append(k)
        if len(cells) == 4:
            break
    v, f = _one_cell_triangles(cells, inv)
    centre = v.reshape(-1, 3, 3).mean(1)
    q = np.concatenate([centre + np.float32(0.01), centre - np.float32(0.02), centre + np.float32(0.3)])
    exp, bs, qs = check_mesh(v, f, q, md, capacity=8)
    assert bs["cells"] == bs["rows"] == 4 and exp["idx"][:8].tolist() == [0, 1, 2, 3] * 2 and qs["matched"] == 8


def test_a_table_without_a_free_slot_raises():
    from pi3_slam_amd.map_eval import MeshIndex
    v, f = _one_cell_triangles([3 * j for j in range(9)], meshref.inv_cell(0.05))      # nine cells, eight slots
    with pytest.raises(RuntimeError, match="cell table overflow at 8 slots"):
        MeshIndex(v, f, 0.05, DEV, capacity=8)
    index = MeshIndex(v, f, 0.05, DEV, capacity=16)
    assert index.build_stats["cells"] == 9 and index.nearest(v)[1].tolist() == [j // 3 for j in range(27)]
    # sized by default: a first guess, and a second table when the count pass finds the first more than half full
    one = np.array([[0, 1, 2]], np.int32)
    wall = MeshIndex(np.array([[-2, -1.5, 0.3], [2, -1.5, 0.3], [2, 1.5, 0.3]], np.float32), one, 0.05, DEV)
    assert wall.build_stats["cells"] == 65 * 49 and wall.table.numel() // 8 == MeshIndex.FIRST_SLOTS
    skew = MeshIndex(np.array([[0.01, 0.02, 0.03], [2.49, 0.3, 2.45], [0.2, 2.48, 1.0]], np.float32), one, 0.05, DEV)
    assert skew.build_stats["cells"] == 40 ** 3 and skew.table.numel() // 8 == 131072 and skew.build_stats["no_slot"] == 0


def test_max_rows_exceeded_raises():
    from pi3_slam_amd.map_eval import MeshIndex
    wall = np.array([[-2, -1.5, 0.3], [2, -1.5, 0.3], [2, 1.5, 0.3], [np.nan, 0, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    with pytest.raises(RuntimeError, match=r"3\d\d\d rows for 2 triangles \(1 dropped\).*max_rows = 1000"):
        MeshIndex(wall, f, 0.05, DEV, max_rows=1000)
    far = np.array([[-60000, -60000, -60000], [60000, 60000, 60000], [60000, -60000, 0]], np.float32)
    with pytest.raises(RuntimeError, match="exceed max_rows"):                         # 2^32 rows and more: counted, not walked
        MeshIndex(far, f[:1], 0.05, DEV)
    with pytest.raises(ValueError):
        MeshIndex(wall, f, 0.05, DEV, max_rows=0)


# ------------------------------------------------------------------------------------------------ the entry points' checks
def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    V, F, m, cap, n_rows = 30, 10, 20, 64, 200
    verts = torch.rand(V, 3, device=DEV)
    faces = torch.randint(0, V, (F, 3), dtype=torch.int32, device=DEV)
    table = torch.full((cap * 8,), 5, dtype=torch.int64, device=DEV)
    packed = torch.full((F, 12), 5.0, dtype=torch.float32, device=DEV)
    rows = torch.full((n_rows,), 5, dtype=torch.int32, device=DEV)
    d2 = torch.full((m,), 5.0, dtype=torch.float64, device=DEV)
    face = torch.full((m,), 5, dtype=torch.int32, device=DEV)
    closest = torch.full((m, 3), 5.0, dtype=torch.float32, device=DEV)
    counts = torch.full((F,), 5, dtype=torch.int64, device=DEV)
    offsets = torch.arange(F + 1, dtype=torch.int64, device=DEV)
    normals = torch.full((F, 3), 5.0, dtype=torch.float32, device=DEV)
    counters = torch.full((8,), 11, dtype=torch.int64, device=DEV)
    inf, nan = float("inf"), float("nan")
    ptr = dict(vertices=verts, faces=faces, table=table, packed=packed, rows=rows, queries=verts, d2=d2, face=face,
               closest=closest, counts=counts, offsets=offsets, points=closest, normals=normals, counters=counters)

    def args(null):
        a = {k: t.data_ptr() for k, t in ptr.items()}
        a.update({k: None for k in null})
        return a

    def count(V_=V, F_=F, inv=16.0, cap_=cap, mr=1000, **null):
        a = args(null)
        return lib.pi3_mesh_index_count(a["vertices"], V_, a["faces"], F_, inv, a["table"], cap_, a["packed"], mr,
                                        a["counters"], L.stream_ptr())

    def fill(F_=F, inv=16.0, cap_=cap, n_=n_rows, **null):
        a = args(null)
        return lib.pi3_mesh_index_fill(a["table"], cap_, a["packed"], F_, inv, a["rows"], n_, a["counters"], L.stream_ptr())

    def query(F_=F, m_=m, inv=16.0, md=0.05, cap_=cap, n_=n_rows, **null):
        a = args(null)
        return lib.pi3_mesh_nearest(a["table"], cap_, a["rows"], n_, a["packed"], F_, inv, a["queries"], m_, md, a["d2"],
                                    a["face"], a["closest"], a["counters"], L.stream_ptr())

    def scount(V_=V, F_=F, sp=0.1, **null):
        a = args(null)
        return lib.pi3_mesh_sample_counts(a["vertices"], V_, a["faces"], F_, sp, 3, a["counts"], a["counters"],
                                          L.stream_ptr())

    def spoints(V_=V, F_=F, n_=F, **null):
        a = args(null)
        return lib.pi3_mesh_sample_points(a["vertices"], V_, a["faces"], F_, a["offsets"], n_, 3, a["points"], a["face"],
                                          a["normals"], L.stream_ptr())

    size = [dict(F_=-1), dict(F_=1 << 31), dict(V_=-1), dict(V_=1 << 31)]
    grid = [dict(inv=0.0), dict(inv=-1.0), dict(inv=inf), dict(inv=nan), dict(cap_=0), dict(cap_=cap - 1)]
    for fn, name, cases in (
            (count, b"pi3_mesh_index_count", size + grid + [dict(mr=0), dict(mr=1 << 31), dict(vertices=1), dict(faces=1),
                                                            dict(table=1), dict(packed=1), dict(counters=1)]),
            (fill, b"pi3_mesh_index_fill", size[:2] + grid + [dict(n_=-1), dict(n_=1 << 31), dict(table=1), dict(packed=1),
                                                              dict(rows=1), dict(counters=1)]),
            (query, b"pi3_mesh_nearest", size[:2] + grid + [dict(m_=-1), dict(n_=-1), dict(md=0.0), dict(md=-1.0), dict(md=inf),
                                                            dict(md=nan), dict(md=0.0625), dict(table=1), dict(rows=1),
                                                            dict(packed=1), dict(queries=1), dict(d2=1), dict(face=1),
                                                            dict(closest=1), dict(counters=1)]),
            (scount, b"pi3_mesh_sample_counts", size + [dict(sp=0.0), dict(sp=-1.0), dict(sp=inf), dict(sp=nan), dict(sp=1e-200),
                                                        dict(sp=1e200), dict(vertices=1), dict(faces=1), dict(counts=1),
                                                        dict(counters=1)]),
            (spoints, b"pi3_mesh_sample_points", size + [dict(F_=0), dict(n_=-1), dict(n_=1 << 31), dict(vertices=1),
                                                         dict(faces=1), dict(offsets=1), dict(points=1), dict(face=1),
                                                         dict(normals=1)])):
        for kw in cases:
            assert fn(**kw) == -1, (name, kw)
            assert name in lib.pi3_last_error()
    torch.cuda.synchronize()
    for t, val in ((table, 5), (packed, 5), (rows, 5), (d2, 5), (face, 5), (closest, 5), (counts, 5), (normals, 5),
                   (counters, 11)):
        assert bool((t == val).all())
    assert query(m_=0, queries=1, d2=1, face=1, closest=1) == 0                        # no query: counters zeroed, no output
    torch.cuda.synchronize()
    assert counters.tolist() == [0] * 4 + [11] * 4 and bool((d2 == 5).all())


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("F", [0, 1, 300])
def test_sampler_against_the_oracle(F):
    from pi3_slam_amd.map_eval import sample_surface
    rng = np.random.default_rng(40 + F)
    v, f = cpu.random_triangles(F, rng, 0.01, 0.5)
    if F == 300:
        v[f[7, 1]] = np.nan                                                            # dropped faces in between
        f[11] = [4, 4, 9]
        f[12] = [0, 1, len(v)]
    for seed, S in ((0, 0.05), (2 ** 63 + 12345, 0.013)):
        exp = meshref.sample_surface(v, f, S, seed)
        pts, face, nrm = sample_surface(v, f, S, seed, DEV)
        assert pts.dtype == torch.float32 and face.dtype == torch.int32 and nrm.dtype == torch.float32 and pts.is_cuda
        assert pts.shape == (len(exp["points"]), 3) == nrm.shape and face.shape == (len(exp["points"]),)
        assert pts.cpu().numpy().tobytes() == exp["points"].tobytes()
        assert face.cpu().numpy().tobytes() == exp["face"].tobytes()
        assert nrm.cpu().numpy().tobytes() == exp["normals"].tobytes()
        again = sample_surface(v, f, S, seed, DEV)
        assert all(torch.equal(a, b) for a, b in zip(again, (pts, face, nrm)))
        if F == 300:
            assert len(exp["points"]) > 1000 and exp["dropped"] == 3
            other = sample_surface(v, f, S, seed + 1, DEV)[0]
            assert other.shape != pts.shape or not torch.equal(other, pts)
        if F == 1:
            assert abs(len(exp["points"]) - cpu.areas(v, f).sum() / S ** 2) < 1


# ------------------------------------------------------------------------------------------------ compare_clouds
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
    rng = np.random.default_rng(51)
    v, f = cpu.random_triangles(300, rng, 0.05, 0.25)
    cloud = near_surface(v, f, 1500, rng, 0.01)
    cloud[::83] = np.nan                                                               # dropped points take part
    jitter = (v + 0.005 * rng.standard_normal(v.shape)).astype(np.float32)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 1.3 * Rotation.from_rotvec([0.2, -0.4, 0.7]).as_matrix(), [0.5, -1.0, 2.0]
    back = lambda p: ((p.astype(np.float64) - M[:3, 3]) @ M[:3, :3] / 1.3 ** 2).astype(np.float32)      # noqa: E731
    ths = [0.02, 0.04]
    hooks = dict(_nearest=cloud_cpu.oracle_search, _mesh_nearest=cpu.oracle_mesh_search, _sampler=cpu.oracle_sampler)
    for est, kw in ((cloud, dict(ref_faces=f)), (cloud, dict(ref_faces=f, sample_spacing=0.04, sample_seed=9)),
                    (jitter, dict(est_faces=f, ref_faces=f, voxel_size=0.04)),
                    (back(jitter), dict(est_faces=f, transform=M, max_dist=0.05))):
        ref = cloud if "ref_faces" not in kw else v
        got = compare_clouds(est, ref, ths, device=DEV, **kw)
        exp = compare_clouds(est, ref, ths, device=DEV, **kw, **hooks)
        _same_result(got, exp)
        pts, st = got["points"], got["settings"]
        want_s = kw.get("sample_spacing", kw.get("voxel_size", 0.01))
        assert st["mesh_sample_spacing"] == want_s and st["mesh_sample_seed"] == kw.get("sample_seed", 0)
        for side in ("estimate", "reference"):
            if side[:3] + "_faces" in kw:
                assert pts[side + "_faces"] == 300 and pts[side + "_faces_dropped"] == 0 and pts[side] == len(v)
                area = cpu.areas(jitter if side == "estimate" else v, f).sum() / want_s ** 2      # M back(jitter) = jitter, nearly
                assert abs(pts[side + "_samples"] - area) < 300 + 1e-3 * area
                assert pts[side + "_used"] == pts[side + "_samples"] or "voxel_size" in kw
            else:
                assert side + "_faces" not in pts
        assert got["accuracy"]["points"] == pts["estimate_used"] and got["completeness"]["points"] == pts["reference_used"]
        assert 0.3 < got["precision"][tau_key(0.04)] <= 1.0 and got["search"]["accuracy"]["evaluations"] > 0
        print(sorted(kw), {k: got[k] for k in ("points", "precision", "recall")})
    # ICP on the query clouds, the mesh side's samples with their face normals
    icp = dict(mode="plane", iterations=5)
    got = compare_clouds(cloud, v, ths, device=DEV, ref_faces=f, sample_spacing=0.03, icp=icp)
    exp = compare_clouds(cloud, v, ths, device=DEV, ref_faces=f, sample_spacing=0.03, icp=icp, **hooks)
    _same_result(got, exp)
    assert got["icp"]["iterations"] >= 1 and got["icp"]["history"][0]["pairs"] > 1000


def test_the_room_as_a_22_triangle_reference():
    """The planted room of cloud_icp_ref: the estimate is sample_room's points, the reference its 22 triangles.  By its
    16 vertices the reference says nothing; by its surface every point of the estimate lies on it (fp32 rounding of
    coordinates up to 4 m: below 1e-6 m), and the recall is what the oracle finds on the same samples: sample_room
    leaves the floor under the cabinet out, the mesh has it, so some of the reference's samples have no estimate
    near them by construction."""
    from pi3_slam_amd.map_eval import compare_clouds, tau_key
    v, f = cpu.room_mesh()
    est = icpref.sample_room(6000, np.random.default_rng(7))[0].astype(np.float32)
    ths, k = [0.02], tau_key(0.02)
    hooks = dict(_nearest=cloud_cpu.oracle_search, _mesh_nearest=cpu.oracle_mesh_search, _sampler=cpu.oracle_sampler)
    got = compare_clouds(est, v, ths, device=DEV, ref_faces=f, sample_spacing=0.08)
    exp = compare_clouds(est, v, ths, device=DEV, ref_faces=f, sample_spacing=0.08, **hooks)
    _same_result(got, exp)
    print({x: got[x] for x in ("points", "accuracy", "precision", "recall")})
    assert got["accuracy"]["max"] <= 1e-6 and got["accuracy"]["beyond"] == 0 and got["precision"][k] == 1.0
    assert got["recall"][k] == exp["recall"][k] and 0.0 < got["recall"][k] < 1.0
    assert got["points"]["reference"] == 16 and got["points"]["reference_faces"] == 22
    assert abs(got["points"]["reference_samples"] - 60.0 / 0.08 ** 2) < 22
    # without the new arguments: today's vertex scoring, key for key
    old = compare_clouds(est, v, ths, device=DEV)
    _same_result(old, compare_clouds(est, v, ths, device=DEV, _nearest=cloud_cpu.oracle_search))
    assert set(old) == {"points", "dropped", "accuracy", "completeness", "precision", "recall", "fscore", "search",
                        "settings", "_distances", "_points"}
    assert set(old["points"]) == {"estimate", "reference", "estimate_used", "reference_used"}
    assert set(old["settings"]) == {"thresholds", "max_dist", "voxel_size", "transform", "cell"}
    assert set(old["search"]["accuracy"]) == {"evaluations", "cells", "largest_cell"}
    assert old["points"]["reference_used"] == 16 and old["precision"][k] < 0.01


# ------------------------------------------------------------------------------------------------ end to end
def test_cli_evaluate_map_mesh_surface(tmp_path, capsys):
    from pi3_slam_amd import cli, map_eval
    from pi3_slam_amd.export import write_mesh_ply, write_ply
    v, f = cpu.room_mesh()
    est = icpref.sample_room(5000, np.random.default_rng(8))[0].astype(np.float32)
    ref_ply, est_ply, err_ply = str(tmp_path / "room.ply"), str(tmp_path / "est.ply"), str(tmp_path / "error.ply")
    write_mesh_ply(v, np.zeros_like(v), np.full((len(v), 3), 200, np.uint8), f, ref_ply)
    write_ply(est, np.full((len(est), 3), 100, np.uint8), est_ply)
    argv = ["evaluate-map", "--estimate", est_ply, "--reference", ref_ply, "--thresholds", "0.02", "0.05", "--device", DEV]
    mesh = ["--mesh-surface", "--mesh-sample-spacing", "0.1", "--mesh-sample-seed", "3"]
    capsys.readouterr()
    cli.main(argv + mesh + ["--json"])
    said = capsys.readouterr().out.strip().splitlines()
    assert len(said) == 1
    from_cli = json.loads(said[0])
    res = map_eval.compare_clouds(est, v, [0.02, 0.05], device=DEV, ref_faces=f, sample_spacing=0.1, sample_seed=3)
    assert from_cli == json.loads(json.dumps(map_eval.public(res))) == map_eval.public(res)
    assert from_cli["settings"]["mesh_sample_spacing"] == 0.1 and from_cli["settings"]["mesh_sample_seed"] == 3
    assert from_cli["points"]["reference_faces"] == 22 and from_cli["precision"]["0.02"] == 1.0
    # without the flag the same files score by the 16 vertices, and the output has no mesh key
    cli.main(argv + ["--json"])
    plain = json.loads(capsys.readouterr().out.strip())
    assert plain == map_eval.public(map_eval.compare_clouds(est, v, [0.02, 0.05], device=DEV))
    assert "reference_faces" not in plain["points"] and "mesh_sample_spacing" not in plain["settings"]
    # the table; the mesh as the estimate too: the error PLY holds its samples
    cli.main(["evaluate-map", "--estimate", ref_ply, "--reference", ref_ply, "--thresholds", "0.02", "--device", DEV] + mesh +
             ["--error-ply", err_ply])
    table = capsys.readouterr().out
    print(table)
    lines = [ln for ln in table.splitlines() if " mesh " in ln]
    assert len(lines) == 2 and lines[0].startswith("estimate mesh") and lines[1].startswith("reference mesh")
    assert all("22 faces, 0 dropped" in ln and "at spacing 0.1 (seed 3)" in ln for ln in lines)
    both = map_eval.compare_clouds(v, v, [0.02], device=DEV, est_faces=f, ref_faces=f, sample_spacing=0.1, sample_seed=3)
    ep, ec = map_eval.read_ply_points(err_ply)
    assert ep.tobytes() == both["_points"]["estimate"].tobytes() and len(ep) == both["points"]["estimate_samples"]
    assert ec.tobytes() == map_eval.error_colors(both["_distances"]["estimate"], 0.04).tobytes()
    assert both["accuracy"]["max"] <= 1e-6 and both["recall"]["0.02"] == 1.0
