"""The dense map's surface mesh without a GPU: the numpy oracle (tests/dense_mesh_ref.py) on a sphere and a plane patch
whose right answer is known, the PLY writer, and the option's plumbing."""
import os

import numpy as np
import pytest

import dense_mesh_ref as ref

V = 0.02
CENTRE = np.array([0.0137, 0.0137, 0.0137])         # off the lattice: a sphere centred on a lattice point touches
                                                    # lattice planes tangentially at its poles and does not close

_cache = {}


def sphere(radius):
    """The reference mesh of a densely sampled sphere (fused once per radius, shared by the tests, read only)."""
    if radius not in _cache:
        n = 60000 if radius < 0.1 else 300000
        p, nr, col = ref.sphere_samples(radius, CENTRE, n)
        table, nacc = ref.fused(p, nr, col, V)
        _cache[radius] = (table, nacc, ref.mesh(table, nacc, V))
    return _cache[radius]


def plane():
    if "plane" not in _cache:
        v = 2.0 ** -6
        p, nr, col, (origin, normal) = ref.plane_samples(v)
        table, nacc = ref.fused(p, nr, col, v)
        _cache["plane"] = (table, nacc, ref.mesh(table, nacc, v), v, origin, normal)
    return _cache["plane"]


@pytest.mark.parametrize("radius", [0.083, 0.2])
def test_sphere_is_closed_outward_and_on_the_sphere(radius):
    table, _, m = sphere(radius)
    f, x = m["faces"], m["vertices"].astype(np.float64)
    nv, nf = len(x), len(f)
    edges, uses = ref.edge_uses(f)
    dev = np.abs(np.linalg.norm(x - CENTRE, axis=1) - radius)
    bound = 3.0 * V * V / (2.0 * radius)            # the sag of a tangent plane at sqrt(3) v, the farthest a voxel that
    #                                                 contributes to a corner lies from it
    print(f"R = {radius}: {len(table['keys'])} voxels, {m['cells']} cells, {nv} vertices, {len(edges)} edges, {nf} "
          f"triangles; max | |x - c| - R | = {dev.max() / V:.4f} v (bound {bound / V:.3f} v); {m['ambiguous']} ambiguous")
    assert len(table["keys"]) > (300 if radius < 0.1 else 1800)
    assert nf == 2 * m["quads"] and f.dtype == np.int32 and f.min() >= 0 and f.max() < nv
    assert (uses == 2).all()                                            # closed: every edge on exactly two triangles
    assert nv - len(edges) + nf == 2
    assert len(np.unique(f)) == nv                                      # no unused vertex
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    tri = x[f]
    out = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((out * (tri.mean(1) - CENTRE)).sum(1) > 0).all()            # every triangle faces outward
    assert (dev <= bound).all()
    # the vertex normals face outward too, and the colours follow the samples' (a function of the direction)
    d = (x - CENTRE) / np.linalg.norm(x - CENTRE, axis=1)[:, None]
    assert ((m["normals"].astype(np.float64) * d).sum(1) > 0.95).all()
    assert np.abs(m["colors"].astype(np.float64) - 127.5 * (d + 1.0)).max() < 40


def test_plane_patch_has_its_rim_as_only_boundary_and_lies_on_the_plane():
    table, _, m, v, origin, normal = plane()
    x = m["vertices_f64"]
    edges, uses = ref.edge_uses(m["faces"])
    off = np.abs((x - origin) @ normal)
    rim = ref.plane_rim_distance(x[np.unique(edges[uses == 1])])
    print(f"plane: {len(table['keys'])} voxels, {len(x)} vertices, {len(m['faces'])} triangles, {int((uses == 1).sum())} "
          f"boundary edges at most {rim.max():.3f} voxels from the rim; max distance from the plane {off.max():.3g} v")
    assert len(m["faces"]) > 2000 and set(np.unique(uses)) == {1, 2}
    assert (rim <= 3.0).all()
    assert (off <= 1e-9).all()
    assert len(np.unique(m["faces"])) == len(x)
    tri = x[m["faces"]]
    assert (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) @ normal > 0).all()      # wound towards the normal
    # the fp32 vertices in metres are those positions rounded
    assert np.array_equal(m["vertices"], (v * x).astype(np.float32))
    assert np.abs(m["normals"].astype(np.float64) - normal).max() < 1e-6


def test_keep_mask_cuts_a_hole():
    table, nacc, full, v, origin, _ = plane()
    k = ref.fields(table["keys"]) - ref.BIAS
    keep = ~((np.abs(k[:, 0]) < 4) & (np.abs(k[:, 1]) < 4))
    m = ref.mesh(table, nacc, v, keep)
    edges, uses = ref.edge_uses(m["faces"])
    assert 0 < len(m["faces"]) < len(full["faces"]) and m["sources"] == int(keep.sum())
    inner = ref.plane_rim_distance(m["vertices_f64"][np.unique(edges[uses == 1])]) > 3.0
    assert inner.any()                                                  # a second boundary: the hole's


def test_voxels_without_a_normal_or_with_cancelling_normals_are_no_sources():
    import dense_map_ref as dm
    import dense_normals_ref as dn
    pts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [2.5, 0.5, 0.5]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]], np.float32)
    nw = np.array([1, 0, 1, 1], np.int32)           # voxel 1 has no normal, voxel 2's cancel
    keys, w, wu, wc, _ = dm.contributions_points(pts, None, None, 1.0)
    table = dm.merge(keys, w, wu, wc)
    nacc = dn.accumulate([dn.point_normals(pts, nrm, nw, np.eye(3).reshape(9), 1.0)])
    m = ref.mesh(table, nacc, 1.0)
    assert m["sources"] == 1 and m["cells"] == 27
    # one oriented point: the plane z = 0.5 through the 3 x 3 cells of the middle layer, 4 quads around the voxel's edges
    assert len(m["keys"]) == 9 and m["quads"] == 4
    assert np.array_equal(m["vertices"][:, 2], np.full(9, 0.5, np.float32))


def test_empty_map_gives_an_empty_mesh_and_a_valid_file(tmp_path):
    from pi3_slam_amd.export import write_mesh_ply
    none = dict(keys=np.zeros(0, np.uint64), W=np.zeros(0, np.uint64), U=np.zeros((0, 3), np.uint64),
                C=np.zeros((0, 3), np.uint64))
    m = ref.mesh(none, dict(keys=np.zeros(0, np.uint64), acc=np.zeros((0, 4), np.int64)), V)
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["cells"] == 0
    path = tmp_path / "empty.ply"
    write_mesh_ply(m["vertices"], m["normals"], m["colors"], m["faces"], str(path))
    got = parse_mesh_ply(path)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)


def parse_mesh_ply(path):
    """A hand parser of write_mesh_ply's layout (shared with the GPU tests)."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert lines[2].startswith("element vertex ") and lines[12].startswith("element face ")
    assert lines[3:12] == [f"property float {a}" for a in ("x", "y", "z", "nx", "ny", "nz")] + \
        [f"property uchar {c}" for c in ("red", "green", "blue")]
    assert lines[13:] == ["property list uchar int vertex_indices", ""]
    nv, nf = int(lines[2].split()[-1]), int(lines[12].split()[-1])
    vt = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("v", "<i4", 3)])
    assert vt.itemsize == 27 and ft.itemsize == 13 and len(body) == 27 * nv + 13 * nf
    vert = np.frombuffer(body[:27 * nv], vt)
    face = np.frombuffer(body[27 * nv:], ft)
    assert (face["k"] == 3).all()
    return dict(vertices=vert["xyz"], normals=vert["n"], colors=vert["rgb"], faces=face["v"])


def test_write_mesh_ply_round_trips(tmp_path):
    from pi3_slam_amd.export import write_mesh_ply
    _, _, m = sphere(0.083)
    path = tmp_path / "m.ply"
    write_mesh_ply(m["vertices"], m["normals"], m["colors"], m["faces"], str(path))
    got = parse_mesh_ply(path)
    for k in ("vertices", "normals", "colors", "faces"):
        assert got[k].tobytes() == m[k].tobytes(), k
    with pytest.raises(ValueError):
        write_mesh_ply(m["vertices"], m["normals"], m["colors"], m["faces"] + len(m["vertices"]), str(path))
    with pytest.raises(ValueError):
        write_mesh_ply(m["vertices"], m["normals"][:-1], m["colors"], m["faces"], str(path))


def test_host_faces_match_the_reference_ring():
    """dense_map.quad_faces (key arithmetic on the packed fields) against the oracle's (on the unpacked ones)."""
    from pi3_slam_amd.dense_map import quad_faces
    _, _, m = sphere(0.083)
    assert np.array_equal(quad_faces(m["keys"], m["quad_keys"], m["quad_codes"]), m["faces"])
    assert quad_faces(m["keys"], m["quad_keys"][:0], m["quad_codes"][:0]).shape == (0, 3)
    with pytest.raises(RuntimeError, match="without a vertex"):
        quad_faces(m["keys"][1:], m["quad_keys"], m["quad_codes"])


def test_option_plumbing(tmp_path, monkeypatch):
    import inspect

    from pi3_slam_amd import cli, export
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    p = cli.build_parser()
    base = ["reconstruct", "--chunks", "c", "--output", "o"]
    assert p.parse_args(base).dense_mesh is False and p.parse_args(base + ["--dense-mesh"]).dense_mesh is True
    online = ["online", "--image_dir", "i", "--output_path", "o"]
    assert p.parse_args(online).dense_mesh is False and p.parse_args(online + ["--dense_mesh"]).dense_mesh is True
    assert inspect.signature(OfflineReconstructor.__init__).parameters["dense_mesh"].default is False
    assert inspect.signature(export.write_outputs).parameters["dense_mesh"].default is False
    assert callable(Pi3SLAMOnline.save_dense_mesh)
    assert OfflineReconstructor(str(tmp_path), str(tmp_path), device="cpu").dense_mesh is False
    assert OfflineReconstructor(str(tmp_path), str(tmp_path), device="cpu", dense_mesh=True).dense_mesh is True
    # the CLI hands the switch to the reconstructor
    seen = {}

    class Fake:
        def __init__(self, **kw):
            seen.update(kw)

        def run(self):
            pass
    import pi3_slam_amd.reconstructor as rec
    monkeypatch.setattr(rec, "OfflineReconstructor", Fake)
    cli.main(["reconstruct", "--chunks", str(tmp_path), "--output", str(tmp_path / "o"), "--dense-mesh"])
    assert seen["dense_mesh"] is True
    cli.main(["reconstruct", "--chunks", str(tmp_path), "--output", str(tmp_path / "o")])
    assert seen["dense_mesh"] is False


class NoTable:
    """Stands in for dense_map.VoxelFuser: an empty table, no device."""

    def __init__(self, voxel_size, device="cpu", out_sets=1):
        self.voxel_size, self.device = float(voxel_size), device

    def reserve(self, n):
        pass

    def extract(self, keep=None):
        return dict(keys=np.zeros(0, np.uint64), points=np.zeros((0, 3), np.float32),
                    colors=np.zeros((0, 3), np.uint8), weights=np.zeros(0, np.int32))


def test_clouds_without_normals_give_one_notice_and_no_file(tmp_path, monkeypatch, capsys):
    """write_outputs with dense_mesh on chunks whose clouds carry no normals: the fused map is written as ever, one
    line says why there is no mesh, no dense_mesh.ply, nothing raised.  The clouds are empty and the device table is a
    stand-in, so the real fuse_chunks runs without a GPU."""
    import torch

    from pi3_slam_amd import dense_map, export
    monkeypatch.setattr(dense_map, "VoxelFuser", NoTable)
    cloud = {"points": torch.zeros(0, 3), "colors": torch.zeros(0, 3, dtype=torch.uint8),
             "weights": torch.zeros(0, dtype=torch.int32), "voxel_size": 0.05}
    chunks = [{"dense_cloud": dict(cloud), "camera_poses": torch.eye(4)[None]} for _ in range(2)]
    export.write_outputs(chunks, str(tmp_path), device="cpu", dense_mesh=True)
    text = capsys.readouterr().out
    assert text.count("no dense mesh") == 1 and "Failed to save the dense m" not in text
    assert os.path.exists(tmp_path / "dense_points.ply") and not os.path.exists(tmp_path / "dense_mesh.ply")
    # only some clouds carry normals: the map has none (the line it always printed), and one line for the mesh
    chunks[0]["dense_cloud"].update(normals=torch.zeros(0, 3), normal_weights=torch.zeros(0, dtype=torch.int32))
    export.write_outputs(chunks, str(tmp_path), device="cpu", dense_mesh=True)
    text = capsys.readouterr().out
    assert text.count("Only 1 of 2 dense clouds carry normals") == 1 and text.count("no dense mesh") == 1
    assert not os.path.exists(tmp_path / "dense_mesh.ply")
    # without the option nothing about a mesh is printed
    export.write_outputs(chunks, str(tmp_path), device="cpu")
    assert "mesh" not in capsys.readouterr().out


def test_a_failed_mesh_travels_with_the_map_and_the_points_are_still_written(tmp_path, monkeypatch, capsys):
    """A mesher whose apply() raises: fuse_chunks still returns the map, with mesh None and the exception in
    mesh_error; write_outputs writes dense_points.ply (with the normals) and reports the mesh once.  Empty clouds that
    carry normals, stand-ins for the device table and its normal sums."""
    import torch

    from pi3_slam_amd import dense_map, export

    class NoSums:
        def __init__(self, fuser, out_sets=1):
            pass

        def clear(self):
            pass

        def extract(self, keep=None):
            return dict(keys=np.zeros(0, np.uint64), normals=np.zeros((0, 3), np.float32),
                        normal_weights=np.zeros(0, np.int32))

    boom = RuntimeError("dense mesh: the cell table of 8 slots is too small")

    class FailingMesher:
        calls = 0

        def apply(self, fuser, normals_acc, keep=None):
            assert isinstance(fuser, NoTable) and isinstance(normals_acc, NoSums) and keep is None
            FailingMesher.calls += 1
            raise boom
    monkeypatch.setattr(dense_map, "VoxelFuser", NoTable)
    monkeypatch.setattr(dense_map, "NormalAccumulator", NoSums)
    cloud = {"points": torch.zeros(0, 3), "colors": torch.zeros(0, 3, dtype=torch.uint8),
             "weights": torch.zeros(0, dtype=torch.int32), "voxel_size": 0.05,
             "normals": torch.zeros(0, 3), "normal_weights": torch.zeros(0, dtype=torch.int32)}
    chunks = [{"dense_cloud": dict(cloud), "camera_poses": torch.eye(4)[None]} for _ in range(2)]
    dense = dense_map.fuse_chunks(chunks, "cpu", mesher=FailingMesher())
    assert isinstance(dense, dense_map.DenseMap) and export.DenseMap is dense_map.DenseMap
    assert dense.mesh is None and dense.mesh_error is boom and FailingMesher.calls == 1
    assert dense.voxel_size == 0.05 and dense.normals.shape == (0, 3) and dense.points.shape == (0, 3)
    assert "Dense mesh" not in capsys.readouterr().out
    assert dense_map.fuse_chunks([{"camera_poses": torch.eye(4)[None]}], "cpu", mesher=FailingMesher()) is None

    monkeypatch.setattr(export, "MapMesher", FailingMesher)
    export.write_outputs(chunks, str(tmp_path), device="cpu", dense_mesh=True)
    text = capsys.readouterr().out
    assert text.count("Failed to save the dense mesh") == 1 and "the cell table of 8 slots is too small" in text
    assert "Failed to save the dense map" not in text and "no dense mesh" not in text
    assert "and normals to:" in text and FailingMesher.calls == 2
    assert os.path.exists(tmp_path / "dense_points.ply") and not os.path.exists(tmp_path / "dense_mesh.ply")
    assert b"property float nx" in open(tmp_path / "dense_points.ply", "rb").read()
