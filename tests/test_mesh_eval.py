"""CPU: the oracle of the mesh search and the surface sampler (tests/mesh_eval_ref.py) against independent checks, the
PLY face reader, and the parsing of evaluate-map's mesh flags.  The meshes and hooks the GPU tests share live here."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_icp_ref as icpref          # noqa: E402
import mesh_eval_ref as meshref         # noqa: E402

# one triangle with a right angle at a, and a query in each of Ericson's seven regions with its closest point and
# squared distance worked out by hand (all but the interior's are exact in f64)
TRI_V = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
REGION_CASES = (("A", (-1, -1, 2), (0, 0, 0), 6.0), ("B", (5, -1, 1), (4, 0, 0), 3.0), ("AB", (2, -2, 1), (2, 0, 0), 5.0),
                ("C", (-1, 4, 0), (0, 3, 0), 2.0), ("AC", (-2, 1, 2), (0, 1, 0), 8.0),
                ("BC", (5, 5.5, 1), (2, 1.5, 0), 26.0), ("interior", (1, 1, 3), (1, 1, 0), 9.0))


def random_triangles(F, rng, lo_edge, hi_edge, box=1.0):
    """F triangles with edges of roughly lo_edge .. hi_edge and a corner uniform in [0, box)^3 -> (vertices f32 (3F,3),
    faces int32 (F,3)), every triangle on vertices of its own, in shuffled vertex order."""
    a = rng.random((F, 3)) * box
    d1 = rng.standard_normal((F, 3))
    d2 = rng.standard_normal((F, 3))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    b = a + d1 * rng.uniform(lo_edge, hi_edge, (F, 1))
    c = a + d2 * rng.uniform(lo_edge, hi_edge, (F, 1))
    v = np.stack([a, b, c], 1).reshape(-1, 3).astype(np.float32)
    order = rng.permutation(3 * F)
    inverse = np.empty(3 * F, np.int64)
    inverse[order] = np.arange(3 * F)
    return np.ascontiguousarray(v[order]), inverse.reshape(F, 3).astype(np.int32)


def room_mesh():
    """The planted room of cloud_icp_ref as a mesh: 16 vertices (the corners of the room, then of the cabinet's box),
    22 triangles: the ceiling and the two far walls, the WHOLE floor (the square under the cabinet included: 60 m^2
    where sample_room covers 59), the two near walls as L shapes around the cabinet, the cabinet's three free faces."""
    lo, hi = -icpref.ROOM / 2.0, icpref.ROOM / 2.0
    cab = lo + icpref.CABINET
    bits = [(i >> 2 & 1, i >> 1 & 1, i & 1) for i in range(8)]
    verts = [[(hi if b else lo)[k] for k, b in enumerate(bb)] for bb in bits] + \
            [[(cab if b else lo)[k] for k, b in enumerate(bb)] for bb in bits]
    at = lambda x, y, z, base=0: base + 4 * x + 2 * y + z                              # noqa: E731
    quad = lambda p: [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]                          # noqa: E731
    faces = []
    faces += quad([at(1, 0, 0), at(1, 1, 0), at(1, 1, 1), at(1, 0, 1)])                # x = hi
    faces += quad([at(0, 1, 0), at(1, 1, 0), at(1, 1, 1), at(0, 1, 1)])                # y = hi
    faces += quad([at(0, 0, 1), at(1, 0, 1), at(1, 1, 1), at(0, 1, 1)])                # z = hi
    faces += quad([at(0, 0, 0), at(1, 0, 0), at(1, 1, 0), at(0, 1, 0)])                # the floor, whole
    # wall x = lo: the rectangle without the cabinet's corner, fanned from the reflex corner (lo, cab, cab)
    r = at(0, 1, 1, 8)
    ring = [at(0, 1, 0, 8), at(0, 1, 0), at(0, 1, 1), at(0, 0, 1), at(0, 0, 1, 8)]
    faces += [[r, ring[i], ring[i + 1]] for i in range(4)]
    # wall y = lo, likewise from (cab, lo, cab)
    r = at(1, 0, 1, 8)
    ring = [at(1, 0, 0, 8), at(1, 0, 0), at(1, 0, 1), at(0, 0, 1), at(0, 0, 1, 8)]
    faces += [[r, ring[i], ring[i + 1]] for i in range(4)]
    faces += quad([at(1, 0, 0, 8), at(1, 1, 0, 8), at(1, 1, 1, 8), at(1, 0, 1, 8)])    # cabinet, x = cab
    faces += quad([at(0, 1, 0, 8), at(1, 1, 0, 8), at(1, 1, 1, 8), at(0, 1, 1, 8)])    # cabinet, y = cab
    faces += quad([at(0, 0, 1, 8), at(1, 0, 1, 8), at(1, 1, 1, 8), at(0, 1, 1, 8)])    # cabinet, z = cab
    return np.array(verts, np.float32), np.array(faces, np.int32)


def oracle_mesh_search(vertices, faces, queries, max_dist):
    """compare_clouds' _mesh_nearest hook, served by the oracle."""
    out = meshref.nearest(np.asarray(vertices.cpu()), np.asarray(faces.cpu()), np.asarray(queries.cpu()), max_dist)
    return dict(d2=out["d2"], idx=out["idx"].astype(np.int64), closest=out["closest"], ref_dropped=out["ref_dropped"],
                counters=out["counters"])


def oracle_sampler(vertices, faces, spacing, seed):
    """compare_clouds' _sampler hook, served by the oracle (device tensors out, as the device sampler gives them)."""
    import torch
    out = meshref.sample_surface(np.asarray(vertices.cpu()), np.asarray(faces.cpu()), spacing, seed)
    dev = vertices.device
    return dict(points=torch.from_numpy(out["points"]).to(dev), face=torch.from_numpy(out["face"]).to(dev),
                normals=torch.from_numpy(out["normals"]).to(dev), dropped=out["dropped"])


def areas(v, f):
    t = v[f].astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_is_never_farther_than_a_dense_set_of_points_of_the_triangle():
    rng = np.random.default_rng(3)
    T, m, n = 120, 150, 60
    v, f = random_triangles(T, rng, 0.05, 0.6)
    q = (rng.random((m, 3)) * 1.4 - 0.2).astype(np.float32)
    tri = v[f].astype(np.float64)
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    bu, bv = i[keep] / n, j[keep] / n                                                  # 1891 barycentric samples
    assert len(bu) == (n + 1) * (n + 2) // 2 == 1891
    a, b, c = ([tri[None, :, k, x] for x in range(3)] for k in range(3))
    p = [q.astype(np.float64)[:, None, x] for x in range(3)]
    cp, d2, region = meshref.closest_points(p, a, b, c)
    assert np.isfinite(d2).all() and np.isfinite(cp).all() and d2.shape == (m, T)
    assert set(np.unique(region).tolist()) == set(range(7))                            # every region is met
    for t in range(T):
        pts = tri[t, 0] + bu[:, None] * (tri[t, 1] - tri[t, 0]) + bv[:, None] * (tri[t, 2] - tri[t, 0])
        best = ((q.astype(np.float64)[:, None, :] - pts[None]) ** 2).sum(2).min(1)
        assert (d2[:, t] <= best * (1 + 1e-12) + 1e-300).all(), t
        # and not much nearer than the samples allow: they are at most an edge / n apart
        edge = max(np.linalg.norm(tri[t, 1] - tri[t, 0]), np.linalg.norm(tri[t, 2] - tri[t, 0]),
                   np.linalg.norm(tri[t, 2] - tri[t, 1]))
        assert (np.sqrt(best) <= np.sqrt(d2[:, t]) + edge / n).all(), t
    # the closest point is a point of the triangle: barycentric coordinates in [0, 1]
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    for t in range(0, T, 7):
        sol = np.linalg.lstsq(np.stack([ab[t], ac[t]], 1), (cp[:, :, t] - tri[t, 0][:, None]), rcond=None)[0]
        assert (sol > -1e-9).all() and (sol.sum(0) < 1 + 1e-9).all()
        assert np.abs(tri[t, 0][:, None] + np.stack([ab[t], ac[t]], 1) @ sol - cp[:, :, t]).max() < 1e-9


def test_oracle_in_each_of_the_seven_regions():
    q = np.array([c[1] for c in REGION_CASES], np.float32)
    out = meshref.nearest(TRI_V, TRI_F, q, 8.0)
    tri = TRI_V.astype(np.float64)
    _, d2, region = meshref.closest_points([q.astype(np.float64)[:, x] for x in range(3)], *[tri[k] for k in range(3)])
    assert [meshref.REGIONS[r] for r in region] == [c[0] for c in REGION_CASES] == list(meshref.REGIONS)
    want_q, want_d2 = np.array([c[2] for c in REGION_CASES], np.float64), np.array([c[3] for c in REGION_CASES])
    assert out["idx"].tolist() == [0] * 7 and out["counters"] == dict(dropped=0, matched=7, beyond=0)
    assert (out["d2"][:6] == want_d2[:6]).all() and abs(out["d2"][6] - 9.0) < 1e-14
    assert (out["closest"][:6] == want_q[:6].astype(np.float32)).all() and np.abs(out["closest"][6] - want_q[6]).max() < 1e-6
    assert d2.tobytes() == out["d2"].tobytes()
    # on a vertex, on an edge, in the plane: zero; the radius is inclusive and one ulp more is beyond
    on = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [2, 0, 0], [0, 1.5, 0], [2, 1.5, 0], [1, 1, 0]], np.float32)
    assert not meshref.nearest(TRI_V, TRI_F, on, 0.5)["d2"].any()
    R = np.float32(5.0 / 128.0)
    above = np.array([[1, 1, R], [1, 1, -R], [1, 1, np.nextafter(R, np.float32(1))], [-R, -1, 0]], np.float32)
    got = meshref.nearest(TRI_V, TRI_F, above, float(R))
    assert got["idx"].tolist() == [0, 0, -1, -1] and got["d2"][:2].tolist() == [float(R) ** 2] * 2
    assert np.isinf(got["d2"][2:]).all() and not got["closest"][2:].any()


def test_oracle_tie_and_drop_rules():
    # two triangles sharing the edge (0,0,0)-(0,1,0), the query above that edge; then the same triangle twice
    v = np.array([[0, 0, 0], [0, 1, 0], [1, 0.5, 0], [-1, 0.5, 0], [np.nan, 0, 0], [0, 0, 7e4]], np.float32)
    q = np.array([[0, 0.5, 0.25], [0.5, 0.5, 0.1]], np.float32)
    for faces, want in (([[0, 1, 2], [1, 0, 3]], [0, 0]), ([[1, 0, 3], [0, 1, 2]], [0, 1]),
                        ([[0, 1, 2], [0, 1, 2]], [0, 0]), ([[3, 0, 1], [2, 0, 1], [0, 1, 2]], [0, 1])):
        assert meshref.nearest(v, np.array(faces), q, 0.5)["idx"].tolist() == want
    # drops: index out of range (either side), a repeated index, a vertex that is not finite, one outside the grid
    # (7e4 / 0.625 > 2^20 cells only for a small max_dist), three points on a line
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    vv = np.concatenate([v, line])
    faces = np.array([[0, 1, 2], [0, 1, 9], [-1, 1, 2], [0, 0, 2], [0, 1, 4], [0, 1, 5], [6, 7, 8], [1, 0, 3]])
    ok = meshref.triangle_ok(vv, faces, meshref.inv_cell(0.05))
    assert ok.tolist() == [True, False, False, False, False, False, False, True]
    assert meshref.triangle_ok(vv, faces, meshref.inv_cell(0.5)).tolist()[5] is True           # 7e4 is inside that grid
    assert meshref.triangle_ok(vv, faces, None).tolist() == [True, False, False, False, False, True, False, True]
    out = meshref.nearest(vv, faces, np.array([[0, 0.5, 7e4 / 2], [0.5, 0.5, 0.01], [np.inf, 0, 0]], np.float32), 0.05)
    assert out["ref_dropped"] == 6 and out["idx"].tolist() == [-1, 0, -1]
    assert out["counters"] == dict(dropped=1, matched=1, beyond=1)
    empty = meshref.nearest(vv, np.zeros((0, 3), np.int32), np.array([[np.nan, 0, 0], [0, 0, 0]], np.float32), 0.05)
    assert empty["counters"] == dict(dropped=0, matched=0, beyond=2)


# ------------------------------------------------------------------------------------------------ the sampler
def test_sampler_properties():
    rng = np.random.default_rng(11)
    v, f = random_triangles(300, rng, 0.01, 0.5)
    f[5] = [0, 0, 1]                                                                   # a dropped face in between
    S = 0.05
    out = meshref.sample_surface(v, f, S, seed=7)
    A = areas(v, f)
    n, F = len(out["points"]), len(f)
    assert out["dropped"] == 1 and out["counts"][5] == 0 and n == out["counts"].sum() > 1000
    assert abs(n - A.sum() / S ** 2) < F                                               # floor(x + u), u in [0, 1)
    assert (np.abs(out["counts"] - A / S ** 2) < 1).all()
    assert (out["counts"][A < S * S] <= 1).all() and 0 < (out["counts"][A < S * S] == 1).sum() < (A < S * S).sum()
    bary = out["bary"]
    assert (bary >= 0).all() and (bary <= 1).all() and (bary.sum(1) <= 1).all()
    assert (np.diff(out["face"]) >= 0).all() and (np.bincount(out["face"], minlength=F) == out["counts"]).all()
    tri = v[f[out["face"]]].astype(np.float64)
    want = tri[:, 0] + bary[:, :1] * (tri[:, 1] - tri[:, 0]) + bary[:, 1:] * (tri[:, 2] - tri[:, 0])
    assert np.abs(want - out["points"]).max() < 1e-6
    nrm = out["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-6
    assert np.abs(np.einsum("ij,ij->i", nrm, tri[:, 1] - tri[:, 0])).max() < 1e-6
    # uniform by area inside a face: the mean of many samples of one big triangle is its centroid
    big = meshref.sample_surface(TRI_V, TRI_F, 0.02, seed=1)
    assert len(big["points"]) in (14999, 15000, 15001)
    assert np.abs(big["points"].mean(0) - TRI_V.mean(0)).max() < 0.03
    # the same seed: the same bytes; another seed: other bytes
    again = meshref.sample_surface(v, f, S, seed=7)
    other = meshref.sample_surface(v, f, S, seed=8)
    for k in ("points", "face", "normals"):
        assert out[k].tobytes() == again[k].tobytes()
    assert out["points"].tobytes() != other["points"].tobytes() and out["counts"].tobytes() != other["counts"].tobytes()
    none = meshref.sample_surface(v, np.zeros((0, 3), np.int32), S)
    assert none["points"].shape == (0, 3) and none["face"].shape == (0,) and none["dropped"] == 0


def test_room_mesh_is_the_room():
    v, f = room_mesh()
    assert v.shape == (16, 3) and f.shape == (22, 3)
    assert abs(areas(v, f).sum() - 60.0) < 1e-9 and meshref.triangle_ok(v, f, meshref.inv_cell(0.04)).all()
    pts, _ = icpref.sample_room(3000, np.random.default_rng(2))
    out = meshref.nearest(v, f, pts.astype(np.float32), 0.04)
    assert out["counters"]["matched"] == 3000 and np.sqrt(out["d2"].max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ PLY faces
def test_ply_faces_round_trip(tmp_path):
    from pi3_slam_amd import map_eval
    from pi3_slam_amd.export import write_mesh_ply, write_ply
    rng = np.random.default_rng(4)
    v = rng.random((40, 3)).astype(np.float32)
    nrm = rng.standard_normal((40, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (40, 3), dtype=np.uint8)
    f = rng.integers(0, 40, (25, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    write_mesh_ply(v, nrm, rgb, f, path)                                               # what dense_mesh.ply is written by
    got = map_eval.read_ply_mesh(path)
    assert got["faces"].dtype == np.int32 and got["faces"].tobytes() == f.tobytes()
    assert got["points"].tobytes() == v.tobytes() and got["normals"].tobytes() == nrm.tobytes()
    assert got["colors"].tobytes() == rgb.tobytes()
    old = map_eval.read_ply_vertices(path)
    assert set(got) == set(old) | {"faces"} and all(np.array_equal(got[k], old[k]) for k in old)
    # no face element: None
    write_ply(v, rgb, path)
    assert map_eval.read_ply_mesh(path)["faces"] is None
    # binary, vertex_index, other types, a scalar property beside the list, a quad and a pentagon among triangles
    polys = [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9], [10, 11, 12, 13, 14], [1, 2]]
    want = [[0, 1, 2], [3, 4, 5], [3, 5, 6], [7, 8, 9], [10, 11, 12], [10, 12, 13], [10, 13, 14]]
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\ncomment made by hand\nelement vertex 40\nproperty double x\n"
                  "property double y\nproperty double z\n"
                  f"element face {len(polys)}\nproperty uchar flags\nproperty list ushort uint vertex_index\n"
                  "end_header\n").encode())
        fh.write(v.astype("<f8").tobytes())
        for p in polys:
            fh.write(np.uint8(3).tobytes() + np.uint16(len(p)).astype("<u2").tobytes() + np.array(p, "<u4").tobytes())
    got = map_eval.read_ply_mesh(path)
    assert got["faces"].tolist() == want and got["points"].tobytes() == v.tobytes()
    # the same with every polygon a quad: the one-view path
    quads = rng.integers(0, 40, (9, 4))
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex 40\nproperty float x\nproperty float y\n"
                  "property float z\nelement face 9\nproperty list uchar short vertex_indices\nend_header\n").encode())
        fh.write(v.tobytes())
        for p in quads:
            fh.write(np.uint8(4).tobytes() + p.astype("<i2").tobytes())
    got = map_eval.read_ply_mesh(path)
    assert got["faces"].tolist() == [t for p in quads.tolist() for t in ([p[0], p[1], p[2]], [p[0], p[2], p[3]])]
    # ascii
    with open(path, "w") as fh:
        fh.write(f"ply\nformat ascii 1.0\nelement vertex 15\nproperty float x\nproperty float y\nproperty float z\n"
                 f"element face {len(polys)}\nproperty list uchar int vertex_indices\nend_header\n")
        for p in v[:15]:
            fh.write(" ".join(repr(float(x)) for x in p) + "\n")
        for p in polys:
            fh.write(" ".join(str(x) for x in [len(p)] + p) + "\n")
    got = map_eval.read_ply_mesh(path)
    assert got["faces"].tolist() == want and got["points"].tobytes() == v[:15].tobytes()
    # a list that is not vertex indices is refused
    with open(path, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar float texcoord\nend_header\n0 0 0\n3 0 0 0\n")
    with pytest.raises(ValueError, match="vertex_indices"):
        map_eval.read_ply_mesh(path)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_parses_the_mesh_flags(tmp_path):
    from pi3_slam_amd import cli
    from pi3_slam_amd.export import write_ply
    base = ["evaluate-map", "--estimate", "e.ply", "--reference", "r.ply", "--thresholds", "0.02"]
    a = cli.build_parser().parse_args(base)
    assert a.mesh_surface is False and a.mesh_sample_spacing is None and a.mesh_sample_seed == 0
    b = cli.build_parser().parse_args(base + ["--mesh-surface", "--mesh-sample-spacing", "0.01", "--mesh-sample-seed", "5"])
    assert b.mesh_surface is True and b.mesh_sample_spacing == 0.01 and b.mesh_sample_seed == 5
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--mesh-sample-spacing", "close"])
    # refused before any device work: the sampling flags without --mesh-surface, --mesh-surface without any faces
    cloud = str(tmp_path / "cloud.ply")
    write_ply(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8), cloud)
    files = ["evaluate-map", "--estimate", cloud, "--reference", cloud, "--thresholds", "0.02"]
    with pytest.raises(SystemExit, match="need --mesh-surface"):
        cli.main(files + ["--mesh-sample-spacing", "0.01"])
    with pytest.raises(SystemExit, match="needs faces"):
        cli.main(files + ["--mesh-surface"])


def test_table_gains_a_line_per_mesh_side():
    from pi3_slam_amd import map_eval
    st = dict(points=3, matched=3, beyond=0, mean=0.0, median=0.0, rmse=0.0, p90=0.0, max=0.0, within={"0.02": 1.0})
    res = dict(points=dict(estimate=3, reference=16, estimate_used=3, reference_used=90, reference_faces=22,
                           reference_faces_dropped=1, reference_samples=90),
               dropped=dict(estimate=0, reference=0), accuracy=st, completeness=st, precision={"0.02": 1.0},
               recall={"0.02": 1.0}, fscore={"0.02": 1.0},
               settings=dict(thresholds=[0.02], max_dist=0.04, voxel_size=None, transform=None, mesh_sample_spacing=0.01,
                             mesh_sample_seed=4))
    table = map_eval.format_table(res)
    assert "reference mesh" in table and "22 faces, 1 dropped, 90 samples at spacing 0.01 (seed 4)" in table
    assert "estimate mesh" not in table
    for k in ("reference_faces", "reference_faces_dropped", "reference_samples"):
        res["points"].pop(k)
    plain = map_eval.format_table(res)
    assert "mesh" not in plain and [ln for ln in table.splitlines() if "mesh" not in ln] == plain.splitlines()
