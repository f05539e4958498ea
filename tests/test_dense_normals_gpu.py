"""Surface normals of the dense map on the GPU (csrc/voxel_normals.hip, dense_map.NormalAccumulator, render.MapRenderer)
against the numpy oracle tests/dense_normals_ref.py, byte for byte and twice the same bytes; then the option end to end
on the tiny engine configuration (56 x 70 frames): create, reconstruct, PLY and renders."""
import json
import os

import numpy as np
import pytest
import torch

import dense_map_ref as dm
import dense_normals_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu(built_lib):
    assert torch.cuda.is_available()
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)


def _same_rows(got, exp):
    assert got["keys"].view(np.uint64).tobytes() == np.asarray(exp["keys"], np.uint64).tobytes()
    assert got["normals"].dtype == np.float32 and got["normals"].tobytes() == exp["normals"].tobytes()
    assert got["normal_weights"].dtype == np.int32 and got["normal_weights"].tobytes() == exp["normal_weights"].tobytes()


def _surface(N, H, W, seed, holes):
    """A smooth random surface seen by N cameras: z = 2 + low-frequency waves, x / y from a pinhole with f = 3 W."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pts = np.empty((N, H, W, 3), np.float32)
    for f in range(N):
        a, b, c = rng.uniform(0.2, 0.6, 3)
        z = 2.0 + 0.3 * np.sin(a * x + f) * np.cos(b * y) + 0.05 * c * x
        pts[f] = np.stack([(x - W / 2) * z / (3.0 * W) + 0.1 * f, (y - H / 2) * z / (3.0 * W), z], -1)
    conf = rng.normal(1.5, 1.0, (N, H, W)).astype(np.float32)
    masks = np.ones((N, H, W), np.uint8)
    if holes:
        masks = (rng.random((N, H, W)) < 0.93).astype(np.uint8)
        flat = pts.reshape(-1, 3)
        idx = rng.choice(len(flat), 12, replace=False)
        flat[idx[0:3], 0] = np.nan
        flat[idx[3:6], 2] = np.inf
        flat[idx[6:9], 1] = -np.inf
        flat[idx[9:12], 0] = 3.0e5                  # |k| >= 2^20 at 2 cm
    else:
        conf[:] = 5.0
    return pts, conf, masks


def _stage1_dev(pts, conf, masks, thr, v):
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    fz = VoxelFuser(v, DEV)
    P, C, M = torch.from_numpy(pts).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(masks).to(DEV)
    fz.fuse_pixels(P, C, M, None, thr)
    acc = NormalAccumulator(fz)
    acc.clear()
    acc.add_pixels(P, C, M, thr)
    cloud, rows = fz.extract(), acc.extract()
    return cloud, rows, acc, fz, (P, C, M)


@pytest.mark.parametrize("shape,holes", [((1, 3, 3), False), ((2, 5, 67), False), ((3, 16, 24), True)])
def test_pixel_normals_match_the_oracle_byte_for_byte(shape, holes):
    """(a) + (c).  1x3x3: one contributing pixel.  2x5x67: rows (67) and frames (335) end inside a wave, so a border
    pixel's neighbouring lane holds another row's pixel.  3x16x24: mask holes, confidences below the threshold, NaN / inf
    points and |k| >= 2^20; the counters are compared too."""
    thr, v = 0.6, 0.02
    pts, conf, masks = _surface(*shape, seed=11 + shape[1], holes=holes)
    exp = ref.fuse_pixels_normals(pts, conf, masks, thr, v)
    cloud, rows, acc, fz, (P, C, M) = _stage1_dev(pts, conf, masks, thr, v)
    assert cloud["keys"].view(np.uint64).tobytes() == exp["keys"].tobytes()
    _same_rows(rows, exp)
    st = acc.last_stats
    got_stats = [st["contributions"], st["skipped"], st["degenerate"], st["lost"]]
    print(f"{shape}: stats {got_stats}, {st['rows']} voxels, {st['nonzero']} with a normal")
    assert got_stats == exp["stats"].tolist() and st["lost"] == 0
    assert st["rows"] == len(exp["keys"]) and st["nonzero"] == exp["nonzero"]
    if shape == (1, 3, 3):
        assert st["contributions"] == 1 and st["skipped"] == 8
    else:
        assert st["contributions"] > 50 and st["skipped"] > 0
    if holes:
        assert st["skipped"] > shape[0] * (2 * shape[1] + 2 * shape[2] - 4)      # more than the border pixels alone
    # twice the same bytes
    acc.clear()
    acc.add_pixels(P, C, M, thr)
    again = acc.extract()
    _same_rows(again, rows)


def test_normal_accumulator_refuses_a_reallocated_table():
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    pts, conf, masks = _surface(1, 8, 8, seed=3, holes=False)
    fz = VoxelFuser(0.02, DEV)
    P, C, M = torch.from_numpy(pts).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(masks).to(DEV)
    fz.fuse_pixels(P, C, M, None, 0.5)
    acc = NormalAccumulator(fz)
    acc.clear()
    acc.add_pixels(P, C, M, 0.5)
    fz.reserve(100000)                 # the table grows: the sums no longer lie beside its slots
    with pytest.raises(RuntimeError, match="reallocated"):
        acc.extract()


def _rotation(axis, deg):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.deg2rad(deg) * np.asarray(axis, np.float64) / np.linalg.norm(axis)).as_matrix()


def test_point_normals_of_two_clouds_match_the_oracle_byte_for_byte():
    """(b) + (c): two clouds, a 90 degree rotation and a general similarity of scale 1.7, overlapping voxels; one pair of
    opposite normals of equal weight that cancels to a zero normal with nweight > 0; then a MapCleaner(min_weight) mask:
    the rows equal the oracle's and their keys those of extract(keep)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapCleaner, NormalAccumulator, VoxelFuser, similarity_rotation
    v = 0.05
    rng = np.random.default_rng(5)
    G1 = np.eye(4)
    G1[:3, :3] = _rotation([0, 0, 1], 90.0)
    G1[:3, 3] = [0.3, -0.2, 0.1]
    G2 = np.eye(4)
    G2[:3, :3] = 1.7 * _rotation([1, 2, 3], 37.0)
    G2[:3, 3] = [-0.1, 0.4, 0.2]
    clouds = []
    for G in (G1, G2):
        n = 3000
        world = rng.uniform(-1.0, 1.0, (n, 3))                     # both clouds fill the same world box: shared voxels
        local = ((world - G[:3, 3]) @ np.linalg.inv(G[:3, :3]).T).astype(np.float32)
        nr = rng.normal(size=(n, 3))
        nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
        nw = rng.integers(0, 6, n).astype(np.int32)                # zeros included: rows without a normal
        nw[:6] = 2
        nr[nw == 0] = 0.0
        nr[:5] = 0.0                                               # zero normals with a weight: degenerate, counted
        nr[5] = np.nan
        w = np.maximum(nw, 1).astype(np.int32) + rng.integers(0, 3, n).astype(np.int32)
        cols = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        clouds.append(dict(points=local, normals=nr, normal_weights=nw, weights=w, colors=cols, G=G))
    # a voxel of its own with two opposite normals of equal weight (cloud 1's frame is a pure rotation: the rotated
    # components are exact negatives of one another)
    c = clouds[0]
    far = np.array([[5.01, 5.01, 5.01], [5.02, 5.02, 5.02]], np.float32)
    c["points"] = np.concatenate([c["points"], far])
    c["normals"] = np.concatenate([c["normals"], np.array([[0.6, 0.0, 0.8], [-0.6, 0.0, -0.8]], np.float32)])
    c["normal_weights"] = np.concatenate([c["normal_weights"], np.array([3, 3], np.int32)])
    c["weights"] = np.concatenate([c["weights"], np.array([3, 3], np.int32)])
    c["colors"] = np.concatenate([c["colors"], np.zeros((2, 3), np.uint8)])

    fz = VoxelFuser(v, DEV)
    fz.reserve(sum(len(c["points"]) for c in clouds))
    acc = NormalAccumulator(fz)
    acc.clear()
    parts, sets = [], []
    for c in clouds:
        pts = torch.from_numpy(c["points"]).to(DEV).contiguous().clone()
        ops.sim3_apply(torch.from_numpy(c["G"].reshape(16).copy()).to(DEV), pts, None)
        fz.fuse_points(pts, torch.from_numpy(c["colors"]).to(DEV), torch.from_numpy(c["weights"]).to(DEV))
        R = similarity_rotation(c["G"])
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
        acc.add_points(pts, torch.from_numpy(c["normals"]).to(DEV), torch.from_numpy(c["normal_weights"]).to(DEV),
                       torch.from_numpy(R.reshape(9).copy()).to(DEV))
        world = pts.cpu().numpy()
        parts.append(ref.point_normals(world, c["normals"], c["normal_weights"], R.reshape(9), dm.inv_voxel(v)))
        sets.append((world, c["colors"], c["weights"]))
    exp_cloud = dm.fuse_point_sets(sets, v)
    sums = ref.accumulate(parts)
    exp = ref.extract(exp_cloud["keys"], sums)
    cloud, rows = fz.extract(), acc.extract()
    assert cloud["keys"].view(np.uint64).tobytes() == exp_cloud["keys"].tobytes()
    _same_rows(rows, exp)
    st = acc.last_stats
    exp_stats = (parts[0]["stats"] + parts[1]["stats"]).tolist()
    assert [st["contributions"], st["skipped"], st["degenerate"], st["lost"]] == exp_stats
    assert st["degenerate"] == 12 and st["lost"] == 0
    multi = np.unique(np.concatenate([p["keys"] for p in parts]), return_counts=True)[1]
    assert (multi > 1).sum() > 100                              # voxels with several contributions
    # the cancelling pair
    world_far = sets[0][0][-2:]
    ok, kfar, _ = dm.quantise(world_far, dm.inv_voxel(v))
    assert ok.all() and kfar[0] == kfar[1]
    at = int(np.searchsorted(rows["keys"].view(np.uint64), kfar[0]))
    assert rows["keys"].view(np.uint64)[at] == kfar[0]
    assert rows["normal_weights"][at] == 6 and not rows["normals"][at].any()
    # cleaned
    cleaner = MapCleaner(min_weight=4)
    keep = cleaner.apply(fz)
    kept_cloud, kept_rows = fz.extract(keep), acc.extract(keep)
    sel = exp_cloud["weights"] >= 4
    assert 0 < sel.sum() < len(sel)
    assert kept_cloud["keys"].view(np.uint64).tobytes() == exp_cloud["keys"][sel].tobytes()
    _same_rows(kept_rows, ref.extract(exp_cloud["keys"][sel], sums))
    again = acc.extract(keep)
    _same_rows(again, kept_rows)


# The 512 points of the designed cloud (two workgroups of four waves), as runs of equal voxels: (voxel, first, last + 1).
#   A one point | C a weight-0 point at 13 and a NaN point at 16: three runs of one key | D .. E .. D the same key again,
#   not adjacent | F two opposite normals of weight 2 | H ends at lane 63 and goes on at lane 0 of the next wave: two
#   partial sums | J exactly one wave | L 130 points over the workgroup boundary at 256 and two wave boundaries |
#   N 65 points over the wave boundary at 384.
_RUNS = (("A", 0, 1), ("B", 1, 10), ("C", 10, 20), ("D", 20, 25), ("E", 25, 30), ("D", 30, 35), ("F", 35, 37),
         ("G", 37, 50), ("H", 50, 71), ("I", 71, 128), ("J", 128, 192), ("K", 192, 200), ("L", 200, 330),
         ("M", 330, 341), ("N", 341, 406), ("O", 406, 461), ("P", 461, 512))
# The summed weight per voxel, by hand: point i weighs 1 + i % 3 (F's two points 2 each), so three consecutive points
# weigh 6.  E.g. J = 128 .. 191: 21 triples and the point 128 (weight 3) = 129; C = 10 .. 19 without 13 and 16:
# (2+3+1) + (3+1) + (3+1+2) = 16; H = 50 .. 70: 7 triples = 42.
_RUN_WEIGHTS = {"A": 1, "B": 18, "C": 16, "D": 19, "E": 11, "F": 4, "G": 26, "H": 42, "I": 114, "J": 129, "K": 15,
                "L": 261, "M": 21, "N": 130, "O": 110, "P": 102}


def test_designed_runs_through_both_wave_merges():
    """fuse_points (7 summed words) and add_points (5) on one cloud whose order places every kind of run boundary (see
    _RUNS).  The points are voxel centres at a voxel size of 2^-5, colours depend on the voxel only and the normals are
    axis-aligned under the identity rotation: every sum is exact, so each voxel's weight is known by hand, and every
    output byte equals the oracles'."""
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    v = 0.03125
    names = sorted(_RUN_WEIGHTS)
    cell = {n: np.array([j - 7, 3 - 2 * j, 5 * j - 30], np.float64) for j, n in enumerate(names)}
    pts, cols = np.empty((512, 3), np.float32), np.empty((512, 3), np.uint8)
    w = (1 + np.arange(512) % 3).astype(np.int32)
    nr = np.eye(3, dtype=np.float32)[np.arange(512) % 3]
    at = 0
    for n, a, b in _RUNS:
        assert a == at and b > a
        at = b
        pts[a:b] = (cell[n] + 0.5) * v
        cols[a:b] = (10 * names.index(n), 20 + names.index(n), 255 - names.index(n))
    assert at == 512
    w[35:37] = 2
    nr[35], nr[36] = (1, 0, 0), (-1, 0, 0)
    w[13] = 0
    pts[16, 1] = np.nan
    eye9 = np.eye(3).reshape(9)

    exp_cloud = dm.fuse_points(pts, cols, w, v)
    part = ref.point_normals(pts, nr, w, eye9, dm.inv_voxel(v))
    exp = ref.extract(exp_cloud["keys"], ref.accumulate([part]))

    def run():
        fz = VoxelFuser(v, DEV)
        P, Wt = torch.from_numpy(pts).to(DEV), torch.from_numpy(w).to(DEV)
        fz.fuse_points(P, torch.from_numpy(cols).to(DEV), Wt)
        acc = NormalAccumulator(fz)
        acc.clear()
        acc.add_points(P, torch.from_numpy(nr).to(DEV), Wt, torch.from_numpy(eye9.copy()).to(DEV))
        return fz.extract(), acc.extract(), fz.last_stats, acc.last_stats

    cloud, rows, cst, st = run()
    assert len(cloud["keys"]) == len(names)
    for k in ("keys", "points", "colors", "weights"):
        assert cloud[k].dtype.itemsize == exp_cloud[k].dtype.itemsize and cloud[k].tobytes() == exp_cloud[k].tobytes(), k
    _same_rows(rows, exp)
    ok, keys, _ = dm.quantise(np.stack([(cell[n] + 0.5) * v for n in names]).astype(np.float32), dm.inv_voxel(v))
    assert ok.all()
    where = np.searchsorted(cloud["keys"].view(np.uint64), keys)
    assert (cloud["keys"].view(np.uint64)[where] == keys).all()
    got_w = dict(zip(names, cloud["weights"][where].tolist()))
    got_nw = dict(zip(names, rows["normal_weights"][where].tolist()))
    print(f"weights {got_w}, dropped {cst['dropped']}, normals {st}")
    assert got_w == _RUN_WEIGHTS and got_nw == _RUN_WEIGHTS
    assert not rows["normals"][where[names.index("F")]].any()           # the opposite pair cancels
    assert cst["dropped"] == 1 and cst["overflow"] == 0                 # the NaN point; the weight-0 point is no candidate
    assert (st["contributions"], st["skipped"], st["degenerate"], st["lost"]) == (510, 1, 0, 0)
    assert part["stats"].tolist() == [510, 1, 0, 0] and exp_cloud["dropped"] == 1
    cloud2, rows2, _, _ = run()
    for k in ("keys", "points", "colors", "weights"):
        assert cloud2[k].tobytes() == cloud[k].tobytes(), k
    _same_rows(rows2, rows)


def _pose_looking(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    P = np.eye(4)
    P[:3, :3] = np.stack([x, np.cross(z, x), z], 1)
    P[:3, 3] = eye
    return P


@pytest.mark.parametrize("M", [1, 3])
def test_render_shade_matches_the_oracle_byte_for_byte(M):
    """(d): V = 5000 voxels into M views of 16 x 24; empty pixels and voxels without a normal included."""
    import render_ref
    from pi3_slam_amd.render import MapRenderer, pack_cameras
    V, H, W = 5000, 16, 24
    rng = np.random.default_rng(21 + M)
    cloud = np.c_[rng.uniform(-1, 1, (V, 2)), rng.uniform(0.8, 3.0, V)].astype(np.float32)
    rgb = rng.integers(0, 256, (V, 3), dtype=np.uint8)
    nr = rng.normal(size=(V, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    nr[rng.random(V) < 0.2] = 0.0
    eyes = [(0, 0, 0), (1.5, 0.2, 0.5), (-1.0, -0.5, 0.2)][:M]
    poses = np.stack([_pose_looking(e, (0, 0, 2.0)) for e in eyes])
    cams = pack_cameras(poses, np.array([[14.0, 0.0, 11.5], [0.0, 14.0, 7.5], [0.0, 0.0, 1.0]]))
    r = MapRenderer(cloud, rgb, None, 0.02, DEV, normals=nr)
    got = r.render(cams, H, W)
    base = render_ref.render(cloud, rgb, None, cams, H, W, 0.02)
    assert got["index"].numpy().tobytes() == base["index"].tobytes()
    exp = ref.shade(base["index"], nr, cams)
    empty = int((base["index"] < 0).sum())
    bare = int(((base["index"] >= 0) & ~nr[np.maximum(base["index"], 0)].any(-1)).sum())
    print(f"M={M}: {exp['pixels']} shaded pixels, {empty} empty, {bare} on voxels without a normal")
    assert empty > 0 and bare > 0 and exp["pixels"] > 100
    assert got["normal"].dtype == torch.uint8 and tuple(got["normal"].shape) == (M, H, W, 3)
    assert got["normal"].numpy().tobytes() == exp["normal"].tobytes()
    assert got["shaded"].numpy().tobytes() == exp["shaded"].tobytes()
    assert r.last_stats["shaded"] == exp["pixels"]
    assert exp["shaded"].max() > 200 and (exp["shaded"][exp["normal"].any(-1)] == 0).any()     # lit and back-facing ones
    again = r.render(cams, H, W)
    assert again["normal"].numpy().tobytes() == exp["normal"].tobytes()
    assert again["shaded"].numpy().tobytes() == exp["shaded"].tobytes()
    # a renderer without normals returns what it always did
    plain = MapRenderer(cloud, rgb, None, 0.02, DEV).render(cams, H, W)
    assert set(plain) == {"depth", "color", "index"}


# ------------------------------------------------------------------------------------------------------ end to end
def _ply_header(path):
    data = open(path, "rb").read()
    return data[:data.index(b"end_header\n")].decode().split("\n")


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
    return [torch.load(p, weights_only=False) for p in saved]


def test_option_end_to_end_on_the_tiny_engine(tmp_path):
    """Two chunks of 56 x 70 frames with and without dense_normals: the clouds' points / colors / weights are
    byte-identical; normals are unit or exactly zero; reconstruct writes nx ny nz and the two new images per view from
    the chunks with normals, and the unchanged layout from the chunks without."""
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
    off = _create(tmp_path / "off", eng, items, False)
    on = _create(tmp_path / "on", eng, items, True)
    assert len(off) == len(on) == 2
    for a, b in zip(off, on):
        ca, cb = a["dense_cloud"], b["dense_cloud"]
        assert set(cb) - set(ca) == {"normals", "normal_weights"}
        for k in ("points", "colors", "weights"):
            assert ca[k].numpy().tobytes() == cb[k].numpy().tobytes(), k
        V = len(cb["points"])
        nr = cb["normals"].numpy()
        assert nr.dtype == np.float32 and nr.shape == (V, 3) and cb["normal_weights"].dtype == torch.int32
        norm = np.linalg.norm(nr.astype(np.float64), axis=1)
        zero = ~nr.any(1)
        print(f"chunk: {V} voxels, {int((~zero).sum())} with a normal, metrics "
              f"{b['_metrics'].get('dense_normal_pixels')} / {b['_metrics'].get('dense_normal_voxels')}")
        assert V > 0 and (~zero).sum() > 0
        assert np.all(np.abs(norm[~zero] - 1.0) <= 1e-6)
        assert b["_metrics"]["dense_normal_voxels"] == int((~zero).sum())
        assert b["_metrics"]["dense_normal_pixels"] == int(cb["normal_weights"].sum()) > 0
        assert "dense_normal_pixels" not in a["_metrics"]

    out_on, out_off = tmp_path / "r_on", tmp_path / "r_off"
    OfflineReconstructor(str(tmp_path / "on"), str(out_on), device=DEV, bundle_adjust=False, render_every=2,
                         render_overview=True).run()
    OfflineReconstructor(str(tmp_path / "off"), str(out_off), device=DEV, bundle_adjust=False, render_every=2,
                         render_overview=True).run()
    head_on, head_off = _ply_header(out_on / "dense_points.ply"), _ply_header(out_off / "dense_points.ply")
    assert head_off == ["ply", "format binary_little_endian 1.0", head_off[2], "property float x", "property float y",
                        "property float z", "property uchar red", "property uchar green", "property uchar blue", ""]
    assert head_on[:3] == head_off[:3]
    assert head_on[3:] == ["property float x", "property float y", "property float z", "property float nx",
                           "property float ny", "property float nz", "property uchar red", "property uchar green",
                           "property uchar blue", ""]
    # same voxels, same xyz / rgb bytes in both files
    n = int(head_on[2].split()[-1])
    body = lambda p: open(p, "rb").read().split(b"end_header\n", 1)[1]       # noqa: E731
    rec_on = np.frombuffer(body(out_on / "dense_points.ply"), dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    rec_off = np.frombuffer(body(out_off / "dense_points.ply"), dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(rec_on) == len(rec_off) == n > 0
    assert rec_on["xyz"].tobytes() == rec_off["xyz"].tobytes() and rec_on["rgb"].tobytes() == rec_off["rgb"].tobytes()
    ln = np.linalg.norm(rec_on["n"].astype(np.float64), axis=1)
    assert np.all((np.abs(ln - 1.0) <= 1e-6) | (ln == 0.0)) and (ln > 0).any()
    files_on, files_off = set(os.listdir(out_on / "renders")), set(os.listdir(out_off / "renders"))
    cams_on = json.load(open(out_on / "renders" / "cameras.json"))
    cams_off = json.load(open(out_off / "renders" / "cameras.json"))
    stems = [os.path.splitext(v["frame"])[0] for v in cams_off["views"]]
    assert len(stems) >= 2
    base = {"cameras.json", "overview.png"} | {f"{k}_{s}.png" for s in stems for k in ("depth", "color")}
    assert files_off == base
    assert files_on == base | {"overview_shaded.png"} | {f"{k}_{s}.png" for s in stems for k in ("normal", "shaded")}
    assert all(set(v) == {"frame", "pose", "fx", "fy", "cx", "cy", "H", "W", "depth", "color"} for v in cams_off["views"])
    assert "shaded" not in cams_off["overview"]
    assert all(v["normal"] == f"normal_{s}.png" and v["shaded"] == f"shaded_{s}.png"
               for v, s in zip(cams_on["views"], stems))
    assert cams_on["overview"]["shaded"] == "overview_shaded.png"
    for s in stems:                      # the depth and colour images are the same with and without normals
        for k in ("depth", "color"):
            assert open(out_on / "renders" / f"{k}_{s}.png", "rb").read() == open(out_off / "renders" / f"{k}_{s}.png", "rb").read()
    from PIL import Image
    sh = np.asarray(Image.open(out_on / "renders" / f"shaded_{stems[0]}.png"))
    nm = np.asarray(Image.open(out_on / "renders" / f"normal_{stems[0]}.png"))
    assert sh.shape == (56, 70) and sh.dtype == np.uint8 and nm.shape == (56, 70, 3)
