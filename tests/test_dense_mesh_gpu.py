"""The dense map's surface mesh on the GPU (csrc/voxel_mesh.hip, dense_map.MapMesher) against the numpy oracle
tests/dense_mesh_ref.py, byte for byte and twice the same bytes; then the option end to end on the tiny engine
configuration (56 x 70 frames): create with normals, reconstruct with dense_mesh, dense_mesh.ply."""
import os

import numpy as np
import pytest
import torch

import dense_map_ref as dm
import dense_mesh_ref as ref
import dense_normals_ref as dn
from test_dense_mesh import CENTRE, V, parse_mesh_ply, plane, sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = ("keys", "vertices", "normals", "colors", "faces")


@pytest.fixture(scope="module", autouse=True)
def _gpu(built_lib):
    assert torch.cuda.is_available()
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)


def _capacity(n):
    from pi3_slam_amd import ops
    return ops.voxel_capacity(n)


def _device_table(pts, nrm, col, w, nw, v, capacity):
    """A voxel table of `capacity` slots with the points fused (colours, weights w or 1) and their normals (weights nw
    or 1) beside it, through the ops entry points in batches that respect their capacity >= 2 n rule -> (a VoxelFuser
    that holds the table, nacc)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import VoxelFuser, inverse_voxel
    fz = VoxelFuser(v, DEV)
    fz.table = torch.empty(capacity * 8, dtype=torch.int64, device=DEV)
    fz.capacity = capacity
    ops.voxel_clear(fz.table, fz.stats)
    nacc = torch.zeros(4 * capacity, dtype=torch.int64, device=DEV)
    nstats = torch.zeros(4, dtype=torch.int64, device=DEV)
    rot = torch.eye(3, dtype=torch.float64, device=DEV).reshape(9).contiguous()
    n, step, inv_v = len(pts), capacity // 2, inverse_voxel(v)
    w = np.ones(n, np.int32) if w is None else w
    nw = np.ones(n, np.int32) if nw is None else nw
    for a in range(0, n, step):
        sl = slice(a, a + step)
        P = torch.from_numpy(pts[sl]).to(DEV).contiguous()
        ops.voxel_fuse_points(fz.table, fz.stats, P, torch.from_numpy(col[sl]).to(DEV).contiguous(),
                              torch.from_numpy(w[sl]).to(DEV).contiguous(), inv_v)
        ops.voxel_fuse_point_normals(fz.table, nacc, nstats, P, torch.from_numpy(nrm[sl]).to(DEV).contiguous(),
                                     torch.from_numpy(nw[sl]).to(DEV).contiguous(), rot, inv_v)
    assert fz.stats.tolist()[:2] == [0, 0] and int(nstats[3]) == 0
    return fz, nacc


def _ref_inputs(pts, nrm, col, w, nw, v):
    inv_v = dm.inv_voxel(v)
    keys, ws, wu, wc, dropped = dm.contributions_points(pts, col, w, inv_v)
    assert dropped == 0
    part = dn.point_normals(pts, nrm, np.ones(len(pts), np.int32) if nw is None else nw, np.eye(3).reshape(9), inv_v)
    return dm.merge(keys, ws, wu, wc), dn.accumulate([part])


def _same(got, exp):
    assert got["keys"].dtype == np.uint64 and got["vertices"].dtype == np.float32 and got["normals"].dtype == np.float32
    assert got["colors"].dtype == np.uint8 and got["faces"].dtype == np.int32
    for k in ROWS:
        assert got[k].shape == exp[k].shape, k
        assert got[k].tobytes() == np.ascontiguousarray(exp[k]).tobytes(), k


def _filler(table, count, seed, v):
    """`count` points in voxels of their own inside the map's bounding box, grown by 2 voxels: they carry no normal."""
    rng = np.random.default_rng(seed)
    k = ref.fields(table["keys"]) - ref.BIAS
    lo, hi = k.min(0) - 2, k.max(0) + 3
    taken = set(map(tuple, k.tolist()))
    out = []
    while len(out) < count:
        c = tuple(int(x) for x in rng.integers(lo, hi))
        if c not in taken:
            taken.add(c)
            out.append(c)
    return ((np.asarray(out, np.float64).reshape(-1, 3) + 0.5) * v).astype(np.float32)


def _samples(case):
    if case == "plane":
        v = 2.0 ** -6
        p, nr, col, _ = ref.plane_samples(v)
        return p, nr, col, v, plane()[2]
    radius = {"sphere_small": 0.083, "sphere_large": 0.2}[case]
    p, nr, col = ref.sphere_samples(radius, CENTRE, 60000 if radius < 0.1 else 300000)
    return p, nr, col, V, sphere(radius)[2]


@pytest.mark.parametrize("fill", ["natural", "half"])
@pytest.mark.parametrize("case", ["sphere_small", "sphere_large", "plane"])
def test_mesh_matches_the_oracle_byte_for_byte(case, fill):
    """The two spheres and the plane patch of the CPU tests.  natural: the table VoxelFuser would allocate for the
    samples (>= 2 slots per point: nearly empty).  half: the smallest table the capacity rule allows for the voxels,
    topped up to exactly half full with voxels that carry no normal (long probe chains; the oracle says they change
    nothing: the mesh is the natural table's)."""
    from pi3_slam_amd.dense_map import MapMesher
    p, nr, col, v, exp = _samples(case)
    nw = None
    if fill == "natural":
        cap = _capacity(len(p))
    else:
        table = _ref_inputs(p, nr, col, None, None, v)[0]
        cap = _capacity(len(table["keys"]))
        extra = _filler(table, cap // 2 - len(table["keys"]), 5, v)
        nw = np.r_[np.ones(len(p), np.int32), np.zeros(len(extra), np.int32)]
        p, nr = np.concatenate([p, extra]), np.concatenate([nr, np.zeros_like(extra)])
        col = np.concatenate([col, np.full((len(extra), 3), 9, np.uint8)])
    fz, nacc = _device_table(p, nr, col, None, nw, v, cap)
    mesher = MapMesher()
    got = mesher.apply(fz, nacc)
    st = mesher.last_stats
    occupied = int((fz.table.view(-1, 8)[:, 0] != -1).sum())
    print(f"{case} / {fill}: table {occupied} / {cap}, {st}")
    if fill == "half":
        assert 2 * occupied == cap
    _same(got, exp)
    assert (st["sources"], st["cells"], st["vertices"], st["quads"], st["ambiguous_faces"], st["overflow"]) == \
        (exp["sources"], exp["cells"], len(exp["keys"]), exp["quads"], exp["ambiguous"], 0)
    assert st["cell_capacity"] >= 2 * st["cells"] and st["cell_table_bytes"] == 40 * st["cell_capacity"]
    _same(mesher.apply(fz, nacc), got)              # twice the same bytes


def test_keep_mask_and_weights():
    """The plane with weighted points, and a keep mask that cuts a hole: the oracle's mesh under the same mask."""
    from pi3_slam_amd.dense_map import MapMesher
    v = 2.0 ** -6
    p, nr, col, _ = ref.plane_samples(v)
    rng = np.random.default_rng(3)
    w, nw = rng.integers(1, 4, len(p)).astype(np.int32), rng.integers(1, 3, len(p)).astype(np.int32)
    table, nsum = _ref_inputs(p, nr, col, w, nw, v)
    fz, nacc = _device_table(p, nr, col, w, nw, v, _capacity(len(table["keys"])))

    def hole(keys):
        k = ref.fields(keys) - ref.BIAS
        return ~((np.abs(k[:, 0]) < 4) & (np.abs(k[:, 1]) < 4))
    slot_keys = fz.table.view(-1, 8)[:, 0].cpu().numpy().view(np.uint64)
    keep = torch.from_numpy((hole(slot_keys) & (slot_keys != np.uint64(2 ** 64 - 1))).astype(np.uint8)).to(DEV)
    exp_all, exp_cut = ref.mesh(table, nsum, v), ref.mesh(table, nsum, v, hole(table["keys"]))
    assert 0 < len(exp_cut["faces"]) < len(exp_all["faces"])
    mesher = MapMesher()
    _same(mesher.apply(fz, nacc), exp_all)
    _same(mesher.apply(fz, nacc, keep), exp_cut)
    assert mesher.last_stats["sources"] == exp_cut["sources"]
    # an all-ones mask is no mask
    _same(mesher.apply(fz, nacc, torch.ones(fz.capacity, dtype=torch.uint8, device=DEV)), exp_all)


def test_voxels_that_must_not_contribute_change_nothing():
    """Voxels without normals and voxels whose normal sums cancel, in between and next to the small sphere's voxels."""
    from pi3_slam_amd.dense_map import MapMesher
    p, nr, col, v, exp = _samples("sphere_small")
    table = sphere(0.083)[0]
    extra = _filler(table, 600, 1, v)               # 600 voxels of their own
    bare = extra[:300]
    pair = np.repeat(extra[300:], 2, 0)             # two points per voxel with opposite normals
    pn = np.tile(np.array([[0.6, 0.0, 0.8], [-0.6, 0.0, -0.8]], np.float32), (300, 1))
    P = np.concatenate([p, bare, pair])
    N = np.concatenate([nr, np.zeros_like(bare), pn])
    C = np.concatenate([col, np.full((len(bare) + len(pair), 3), 255, np.uint8)])
    nw = np.r_[np.ones(len(p), np.int32), np.zeros(len(bare), np.int32), np.ones(len(pair), np.int32)]
    tab2, nsum2 = _ref_inputs(P, N, C, None, nw, v)
    assert len(tab2["keys"]) == len(table["keys"]) + 600
    cancelled = (nsum2["acc"][:, 3] == 2) & ~nsum2["acc"][:, :3].any(1)
    assert cancelled.sum() == 300
    fz, nacc = _device_table(P, N, C, None, nw, v, _capacity(len(P)))
    mesher = MapMesher()
    _same(mesher.apply(fz, nacc), exp)
    assert mesher.last_stats["sources"] == exp["sources"]


def test_index_range():
    """Source voxels at k = +-(2^20 - 1) on every axis (voxel size 1): slabs of 3 x 3 voxels on the six faces of the
    representable cube, each reaching its corner, facing outward.  No cell outside the range is created, no key carries
    into the neighbouring field, and the rows are the oracle's."""
    from pi3_slam_amd.dense_map import MapMesher
    K = 2 ** 20 - 1
    pts, nrm = [], []
    for axis in range(3):
        for sign in (1, -1):
            for i in range(3):
                for j in range(3):
                    k = [0, 0, 0]
                    k[axis], k[(axis + 1) % 3], k[(axis + 2) % 3] = sign * K, sign * (K - i), sign * (K - j)
                    pts.append([c + 0.5 for c in k])
                    e = [0.0, 0.0, 0.0]
                    e[axis] = float(sign)
                    nrm.append(e)
    pts, nrm = np.asarray(pts, np.float32), np.asarray(nrm, np.float32)
    assert np.array_equal(pts.astype(np.float64), np.floor(pts.astype(np.float64)) + 0.5)       # exact in fp32
    col = np.full((len(pts), 3), 77, np.uint8)
    table, nsum = _ref_inputs(pts, nrm, col, None, None, 1.0)
    assert len(table["keys"]) == 38                 # 2 corners x (3 slabs of 9 that share 8 voxels)
    exp = ref.mesh(table, nsum, 1.0)
    fz, nacc = _device_table(pts, nrm, col, None, None, 1.0, _capacity(len(pts)))
    mesher = MapMesher()
    got = mesher.apply(fz, nacc)
    print(f"index range: {mesher.last_stats}")
    _same(got, exp)
    assert len(got["faces"]) > 0 and mesher.last_stats["cells"] == exp["cells"]
    f = ref.fields(got["keys"])
    assert f.min() >= 1 and f.max() <= 2 ** 21 - 1 and (f == 1).any() and (f == 2 ** 21 - 1).any()
    assert np.abs(got["vertices"]).max() <= 2.0 ** 20


def test_undersized_cell_table_is_an_error_not_a_fault():
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapMesher
    p, nr, col, v, exp = _samples("sphere_small")
    fz, nacc = _device_table(p, nr, col, None, None, v, _capacity(len(p)))
    small = _capacity(exp["cells"]) // 4            # the power of two below the number of cells: one size too small
    assert small < exp["cells"] <= 2 * small
    cells = torch.empty(small, dtype=torch.int64, device=DEV)
    stats = torch.zeros(12, dtype=torch.int64, device=DEV)
    ops.voxel_mesh_cells(fz.table, nacc, None, cells, stats)
    sources, used, overflow = stats[:3].tolist()
    print(f"undersized: {small} slots for {exp['cells']} cells: {used} inserted, {overflow} inserts without a slot")
    assert sources == exp["sources"] and 0 < used <= small and overflow > 0
    assert int((cells != -1).sum()) == used         # what was inserted is there, the rest was counted, not written
    with pytest.raises(RuntimeError, match="too small"):
        MapMesher(cell_capacity=small).apply(fz, nacc)
    # the size it grows to on its own is enough
    m = MapMesher()
    _same(m.apply(fz, nacc), exp)
    _same(MapMesher(cell_capacity=m.last_stats["cell_capacity"]).apply(fz, nacc), exp)
    with pytest.raises(ValueError):
        MapMesher(cell_capacity=1000)


def test_isolated_voxels_grow_the_cell_table_to_its_bound():
    """Voxels 4 apart have 27 cells each, far more than the 8 slots per voxel the first table has: the table doubles
    (an insert without a slot, then more than half full) up to its bound, and the mesh is the oracle's: a 3 x 3 patch
    of 4 quads around every oriented point."""
    from pi3_slam_amd.dense_map import MapMesher
    g = np.arange(6, dtype=np.float64) * 4.0
    pts = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 0.25).astype(np.float32)
    nrm = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (len(pts), 1))
    col = np.full((len(pts), 3), 50, np.uint8)
    table, nsum = _ref_inputs(pts, nrm, col, None, None, 1.0)
    exp = ref.mesh(table, nsum, 1.0)
    assert exp["sources"] == 216 and exp["cells"] == 27 * 216
    fz, nacc = _device_table(pts, nrm, col, None, None, 1.0, _capacity(len(pts)))
    mesher = MapMesher()
    _same(mesher.apply(fz, nacc), exp)
    print(f"isolated voxels: {mesher.last_stats}")
    assert mesher.last_stats["cell_capacity"] == _capacity(27 * 216) > _capacity(MapMesher.FIRST_CELLS_PER_SOURCE * 216)


def test_empty_table():
    from pi3_slam_amd.dense_map import MapMesher, NormalAccumulator, VoxelFuser
    fz = VoxelFuser(0.05, DEV)
    acc = NormalAccumulator(fz)
    acc.clear()
    m = MapMesher()
    got = m.apply(fz, acc)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["keys"].shape == (0,)
    assert m.last_stats["sources"] == 0 and m.last_stats["vertices"] == 0


# ------------------------------------------------------------------------------------------------------ end to end
def _create(tmp, eng, items, normals):
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cc = OfflineCreatorConfig(model_path="recipe", output_dir=str(tmp), chunk_length=4, overlap=1, device=DEV,
                              do_metric_depth=False, keypoint_type="grid", max_num_keypoints=20,
                              estimate_camera_params=True, num_loader_workers=0, dense_voxel_size=0.05,
                              dense_conf_threshold=0.05, dense_normals=normals)
    cr = OfflineChunkCreator(cc, model=eng)
    cr.target_size = (56, 70)
    saved, manifest, _ = cr.write_chunks(cr.process_chunks(iter(items)))
    cr.write_run_metadata(manifest)
    return saved


def test_option_end_to_end_on_the_tiny_engine(tmp_path, capsys):
    """Two chunks of 56 x 70 frames created with dense_normals: reconstruct with dense_mesh writes a dense_mesh.ply that
    parses, indexes valid vertices and equals MapMesher on the same fused table; without the option the output
    directory and dense_points.ply are what they were.  Chunks without normals: one line, no file."""
    from pi3_slam_amd.dense_map import MapMesher, fuse_chunks
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    from pi3_slam_amd.weights import Pi3Config
    eng = Pi3Engine(Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5), DEV)
    with torch.no_grad():     # non-empty masks (the edit bench.py makes to plain recipe weights: one depth per patch)
        w_, b_ = eng.w["point_head.proj.weight"], eng.w["point_head.proj.bias"]
        w_[392:588] = 0.05 * w_[392:393].clone()
        b_[392:588] = b_[392].clone()
        eng.w["conf_head.proj.bias"][:196] -= 2.2
    g = torch.Generator().manual_seed(9)
    frames = torch.rand(7, 3, 56, 70, generator=g)
    names = [f"f{i:03d}.png" for i in range(7)]
    items = [{"frames": frames[s:s + 4].unsqueeze(0).contiguous(), "paths": names[s:s + 4],
              "meta": {"chunk_index": i, "start_idx": s, "end_idx": s + 4}} for i, s in enumerate((0, 3))]
    assert len(_create(tmp_path / "on", eng, items, True)) == 2
    saved_off = _create(tmp_path / "off", eng, items, False)
    assert len(saved_off) == 2
    capsys.readouterr()

    out_mesh, out_plain, out_default = tmp_path / "r_mesh", tmp_path / "r_plain", tmp_path / "r_default"
    rec = OfflineReconstructor(str(tmp_path / "on"), str(out_mesh), device=DEV, bundle_adjust=False, dense_mesh=True)
    rec.run()
    text_mesh = capsys.readouterr().out
    OfflineReconstructor(str(tmp_path / "on"), str(out_plain), device=DEV, bundle_adjust=False, dense_mesh=False).run()
    text_plain = capsys.readouterr().out
    OfflineReconstructor(str(tmp_path / "on"), str(out_default), device=DEV, bundle_adjust=False).run()
    capsys.readouterr()
    assert set(os.listdir(out_mesh)) == set(os.listdir(out_plain)) | {"dense_mesh.ply"}
    assert sorted(os.listdir(out_plain)) == sorted(os.listdir(out_default)) and "dense_mesh.ply" not in os.listdir(out_plain)
    for name in os.listdir(out_plain):
        if os.path.isfile(out_plain / name):
            assert open(out_plain / name, "rb").read() == open(out_default / name, "rb").read(), name
    assert open(out_mesh / "dense_points.ply", "rb").read() == open(out_plain / "dense_points.ply", "rb").read()
    assert "mesh" not in text_plain.lower() and "Saved dense mesh" in text_mesh

    got = parse_mesh_ply(out_mesh / "dense_mesh.ply")
    nv, nf = len(got["vertices"]), len(got["faces"])
    print(f"dense_mesh.ply: {nv} vertices, {nf} triangles")
    assert nv > 0 and nf > 0 and got["faces"].min() >= 0 and got["faces"].max() < nv
    assert np.isfinite(got["vertices"]).all()
    ln = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1.0) <= 1e-6) | (ln == 0.0)) and (ln > 0).any()
    mesher = MapMesher()
    fused = fuse_chunks(rec.reconstructions, DEV, voxel_size=0.05, mesher=mesher)
    again = fused.mesh
    assert fused.mesh_error is None
    for k in ("vertices", "normals", "colors", "faces"):
        assert got[k].tobytes() == again[k].tobytes(), k

    # the online facade writes the same file from the same chunks; under a cleaner the mesh sees the kept voxels only
    from pi3_slam_amd.dense_map import MapCleaner
    from pi3_slam_amd.online import Pi3SLAMOnline
    slam = Pi3SLAMOnline.__new__(Pi3SLAMOnline)               # the export methods need the chunks and the cleaner only
    slam.chunk_reconstructions, slam.device, slam.dense_cleaner = rec.reconstructions, torch.device(DEV), None
    assert slam.save_dense_mesh(str(tmp_path / "online_mesh.ply")) == nf
    assert open(tmp_path / "online_mesh.ply", "rb").read() == open(out_mesh / "dense_mesh.ply", "rb").read()
    cleaner = MapCleaner(min_weight=2)
    fused = fuse_chunks(rec.reconstructions, DEV, voxel_size=0.05, cleaner=cleaner, mesher=mesher)
    cut = fused.mesh
    print(f"cleaned: {cleaner.last_stats['after_components']} of {cleaner.last_stats['voxels']} voxels kept, "
          f"{mesher.last_stats['sources']} sources, {len(cut['faces'])} triangles")
    assert fused.mesh_error is None and mesher.last_stats["sources"] <= cleaner.last_stats["after_components"]
    assert cut["faces"].size == 0 or cut["faces"].max() < len(cut["vertices"])
    capsys.readouterr()

    # chunks without normals: one notice, no file, nothing raised, the other outputs as ever
    out_bare = tmp_path / "r_bare"
    OfflineReconstructor(str(tmp_path / "off"), str(out_bare), device=DEV, bundle_adjust=False, dense_mesh=True).run()
    text_bare = capsys.readouterr().out
    assert text_bare.count("no dense mesh") == 1 and "Failed to save" not in text_bare
    assert "dense_mesh.ply" not in os.listdir(out_bare) and "dense_points.ply" in os.listdir(out_bare)
    slam.chunk_reconstructions = [torch.load(p, weights_only=False) for p in saved_off]
    assert slam.save_dense_mesh(str(tmp_path / "online_bare.ply")) is None and not os.path.exists(tmp_path / "online_bare.ply")
