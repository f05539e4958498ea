"""Dense voxel map on the GPU (csrc/voxel.hip, pi3_slam_amd/dense_map.py) against the numpy oracle, bit for bit: the
kernels on synthetic and full-size chunks, the creator's dense_cloud, the 13-chunk chess room end to end, and the
online facade's save_dense_map."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")

import dense_map_ref as ref   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("keys", "points", "colors", "weights")


def _same(got, exp):
    assert len(got["keys"]) == len(exp["keys"]), (len(got["keys"]), len(exp["keys"]))
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if k == "keys":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes(), k


def _synthetic_maps(N, H, W, seed):
    """Surfaces at 1-6 m with noise, NaN / out-of-range holes, logits around the threshold, patchy masks."""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=torch.float32)[None, :, None]
    x = torch.arange(W, dtype=torch.float32)[None, None, :]
    n = torch.arange(N, dtype=torch.float32)[:, None, None]
    z = 1.0 + 5.0 * torch.rand(N, 1, 1, generator=g) + 0.3 * torch.sin(0.05 * x + 0.07 * y + n)
    pts = torch.stack([(x - W / 2) * z / 300.0 + 0.01 * n, (y - H / 2) * z / 300.0, z.expand(N, H, W)], -1)
    pts = pts + 1e-3 * torch.randn(pts.shape, generator=g)
    flat = pts.view(-1, 3)
    idx = torch.randint(0, flat.shape[0], (max(1, flat.shape[0] // 500),), generator=g)
    flat[idx[0::3], 0] = float("nan")
    flat[idx[1::3], 1] = 3.0e5                               # |k| >= 2^20 at 2 cm
    flat[idx[2::3], 2] = -float("inf")
    conf = (0.5 + 1.5 * torch.randn(N, H, W, 1, generator=g)).float()
    masks = (torch.rand(N, H, W, generator=g) < 0.9).to(torch.uint8)
    imgs = torch.rand(N, 3, H, W, generator=g)
    return pts.contiguous(), conf, masks, imgs


def _fuse_pixels_dev(pts, conf, masks, imgs, thr, v):
    from pi3_slam_amd.dense_map import VoxelFuser
    fz = VoxelFuser(v, DEV)
    fz.fuse_pixels(pts.to(DEV), conf.to(DEV), masks.to(DEV), imgs.to(DEV), thr)
    out = fz.extract()
    return out, fz


@pytest.mark.parametrize("shape", [(2, 16, 24), (10, 64, 80), (100, 308, 406)])
def test_fuse_pixels_matches_oracle_bit_for_bit(shape):
    pts, conf, masks, imgs = _synthetic_maps(*shape, seed=sum(shape))
    for v in (0.02, 0.005):
        got, fz = _fuse_pixels_dev(pts, conf, masks, imgs, 0.5, v)
        exp = ref.fuse_pixels(pts.numpy(), conf.numpy(), masks.numpy(), imgs.numpy(), 0.5, v)
        _same(got, exp)
        assert fz.last_stats["dropped"] == exp["dropped"] > 0
        assert fz.last_stats["overflow"] == 0
        again, _ = _fuse_pixels_dev(pts, conf, masks, imgs, 0.5, v)
        for k in KEYS:
            assert got[k].tobytes() == again[k].tobytes(), k


def test_fuse_pixels_full_chunk_of_the_scene_with_creator_masks():
    """A realistic chunk: the chess-room scene's dense maps at 100 x 308 x 406 with the creator's own masks."""
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16))
    eng = ss.SceneEngine(seq)
    imgs = seq.frames(1, DEV)
    out = eng(imgs)
    masks = OfflineChunkCreator._compute_masks(out)[0].to(torch.uint8).contiguous()
    pts, conf = out["points"][0].contiguous(), out["conf"][0].contiguous()
    assert 0.3 < float(masks.float().mean()) < 0.999
    got, fz = _fuse_pixels_dev(pts, conf, masks, imgs[0].contiguous(), 0.5, 0.02)
    exp = ref.fuse_pixels(pts.cpu().numpy(), conf.cpu().numpy(), masks.cpu().numpy(), imgs[0].cpu().numpy(), 0.5, 0.02)
    _same(got, exp)
    assert len(got["keys"]) > 10000


def test_worst_contention_all_points_in_one_voxel():
    from pi3_slam_amd.dense_map import VoxelFuser
    g = torch.Generator().manual_seed(5)
    n = 1 << 20
    p = (0.5 + 0.02 * torch.rand(n, 3, generator=g)).clamp(0.5, 0.5199).float()    # inside [0.50, 0.52) at v = 0.02
    c = torch.randint(0, 256, (n, 3), generator=g, dtype=torch.uint8)
    exp = ref.fuse_points(p.numpy(), c.numpy(), None, 0.02)
    assert len(exp["keys"]) <= 2
    fz = VoxelFuser(0.02, DEV)
    fz.fuse_points(p.to(DEV), c.to(DEV), None)
    got = fz.extract()
    _same(got, exp)
    assert int(got["weights"].sum()) == n
    # one-voxel pixel maps: every lane of every wave merges into one run
    N, H, W = 4, 64, 64
    pts = torch.full((N, H, W, 3), 0.123, dtype=torch.float32)
    got, _ = _fuse_pixels_dev(pts, torch.ones(N, H, W, 1), torch.ones(N, H, W, dtype=torch.uint8),
                              torch.full((N, 3, H, W), 0.5), 0.5, 0.02)
    assert len(got["keys"]) == 1 and int(got["weights"][0]) == N * H * W
    exp = ref.fuse_pixels(pts.numpy(), np.ones((N, H, W, 1), np.float32), np.ones((N, H, W), np.uint8),
                          np.full((N, 3, H, W), 0.5, np.float32), 0.5, 0.02)
    _same(got, exp)


def test_drops_are_counted_and_empty_input_gives_no_voxels():
    from pi3_slam_amd.dense_map import VoxelFuser
    p = torch.tensor([[1.0, 2.0, 3.0], [float("nan"), 0, 0], [0, float("inf"), 0], [1e5, 0, 0], [-1e5, 0, 0],
                      [0.0, 0.0, 0.0]], dtype=torch.float32)
    fz = VoxelFuser(0.05, DEV)
    fz.fuse_points(p.to(DEV), None, torch.ones(6, dtype=torch.int32, device=DEV))
    got = fz.extract()
    exp = ref.fuse_points(p.numpy(), None, None, 0.05)
    _same(got, exp)
    assert fz.last_stats["dropped"] == exp["dropped"] == 4 and len(got["keys"]) == 2
    # empty: nothing fused, or every pixel masked out
    fz = VoxelFuser(0.05, DEV)
    assert len(fz.extract()["keys"]) == 0
    pts, conf, masks, imgs = _synthetic_maps(2, 8, 8, 1)
    got, fz = _fuse_pixels_dev(pts, conf, torch.zeros_like(masks), imgs, 0.5, 0.05)
    assert len(got["keys"]) == 0 and fz.last_stats["dropped"] == 0
    fz.clear()
    fz.fuse_pixels(torch.zeros(0, 8, 8, 3, device=DEV), None, None, None, 0.5)
    assert len(fz.extract()["keys"]) == 0


def test_fuse_points_weighted_and_growth_beyond_first_capacity():
    """fuse_points with integer weights == the oracle; the second call brings 60x more unique voxels than the table
    was sized for, so the table grows (rehash of the first call's sums) and the result still equals the oracle."""
    from pi3_slam_amd.dense_map import VoxelFuser
    g = torch.Generator().manual_seed(11)
    p1 = (torch.randn(1000, 3, generator=g) * 0.05).float()
    p2 = (torch.rand(60000, 3, generator=g) * 4.0 - 2.0).float()
    c1 = torch.randint(0, 256, (1000, 3), generator=g, dtype=torch.uint8)
    c2 = torch.randint(0, 256, (60000, 3), generator=g, dtype=torch.uint8)
    w1 = torch.randint(-2, 5000, (1000,), generator=g, dtype=torch.int32)
    w2 = torch.randint(1, 1 << 20, (60000,), generator=g, dtype=torch.int32)
    fz = VoxelFuser(0.01, DEV)
    fz.fuse_points(p1.to(DEV), c1.to(DEV), w1.to(DEV))
    cap0 = fz.capacity
    first = fz.extract()
    _same(first, ref.fuse_points(p1.numpy(), c1.numpy(), w1.numpy(), 0.01))
    fz.fuse_points(p2.to(DEV), c2.to(DEV), w2.to(DEV))
    assert fz.capacity > cap0
    got = fz.extract()
    assert len(got["keys"]) > cap0
    _same(got, ref.fuse_point_sets([(p1.numpy(), c1.numpy(), w1.numpy()), (p2.numpy(), c2.numpy(), w2.numpy())], 0.01))


def _row_claim_case(n, seed, v=0.02):
    """n distinct voxels with colours, weights and normals on the device, and the oracles' rows by ascending key."""
    import dense_normals_ref as nref
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    rng = np.random.default_rng(seed)
    cells = np.unique(rng.integers(-40, 40, (3 * n, 3)), axis=0)
    cells = cells[rng.permutation(len(cells))[:n]]
    assert len(cells) == n
    pts = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * v).astype(np.float32)
    cols = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    w = rng.integers(1, 6, n).astype(np.int32)
    nr = rng.normal(size=(n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    eye9 = np.eye(3).reshape(9)
    exp = ref.fuse_points(pts, cols, w, v)
    assert len(exp["keys"]) == n
    exp.update(nref.extract(exp["keys"], nref.accumulate([nref.point_normals(pts, nr, w, eye9, ref.inv_voxel(v))])))
    fz = VoxelFuser(v, DEV)
    P, Wt = torch.from_numpy(pts).to(DEV), torch.from_numpy(w).to(DEV)
    fz.fuse_points(P, torch.from_numpy(cols).to(DEV), Wt)
    acc = NormalAccumulator(fz)
    acc.clear()
    acc.add_points(P, torch.from_numpy(nr).to(DEV), Wt, torch.from_numpy(eye9.copy()).to(DEV))
    return fz, acc, exp


def test_row_claim_in_a_table_smaller_than_one_workgroup():
    """Nine voxels in 32 slots: one workgroup of the extractions, most of its 256 x 16 slots past the capacity."""
    fz, acc, exp = _row_claim_case(9, seed=21)
    assert fz.capacity == 32
    _same(fz.extract(), exp)
    rows = acc.extract()
    assert rows["keys"].view(np.uint64).tobytes() == exp["keys"].tobytes()
    assert rows["normals"].tobytes() == exp["normals"].tobytes()
    assert rows["normal_weights"].tobytes() == exp["normal_weights"].tobytes()
    assert acc.last_stats["rows"] == 9 and acc.last_stats["nonzero"] == 9


def test_rows_that_do_not_fit_are_counted_and_not_written():
    """5000 voxels in 16384 slots (four workgroups of the extractions) into buffers of 1064 rows with max_out = 1000:
    1000 rows are stored, each the oracle's row of its key, the other 4000 are counted and rows 1000 .. 1063 keep their
    sentinel.  Then the same with a keep mask on every second occupied slot: 2500 rows, 1500 of them unstored."""
    from pi3_slam_amd import ops
    fz, acc, exp = _row_claim_case(5000, seed=22)
    assert fz.capacity == 16384
    occupied = torch.nonzero(fz.table.view(-1, 8)[:, 0] != -1).reshape(-1)
    assert occupied.numel() == 5000
    keep = torch.zeros(fz.capacity, dtype=torch.uint8, device=DEV)
    keep[occupied[::2]] = 1
    kept_keys = fz.table.view(-1, 8)[occupied[::2], 0].cpu().numpy().view(np.uint64)
    fills = {torch.int64: -2, torch.float32: -7.0, torch.uint8: 0xAB, torch.int32: -5}
    for mask, allowed, total in ((None, exp["keys"], 5000), (keep, kept_keys, 2500)):
        cloud = tuple(t.fill_(fills[t.dtype]) for t in ops.voxel_empty_outputs(1064, DEV))
        nrows = tuple(t.fill_(fills[t.dtype]) for t in ops.voxel_empty_normal_outputs(1064, DEV))
        stats, nstats = fz.stats.clone(), torch.zeros(4, dtype=torch.int64, device=DEV)
        ops.voxel_extract(fz.table, stats, fz.voxel_size, 1000, out=cloud, keep=mask)
        ops.voxel_extract_normals(fz.table, acc.nacc, nstats, 1000, out=nrows, keep=mask)
        stats, nstats = stats.tolist(), nstats.tolist()
        print(f"keep {mask is not None}: cloud stats {stats}, normal stats {nstats}")
        assert stats[2] == total and stats[3] == total - 1000 and stats[1] == 0
        assert nstats[0] == total and nstats[1] == total - 1000
        names = (("keys", "points", "colors", "weights"), ("keys", "normals", "normal_weights"))
        for bufs, cols_ in zip((cloud, nrows), names):
            host = [t.cpu().numpy() for t in bufs]
            keys = host[0][:1000].view(np.uint64)
            assert len(np.unique(keys)) == 1000 and np.isin(keys, allowed).all()
            at = np.searchsorted(exp["keys"], keys)
            assert (exp["keys"][at] == keys).all()
            for h, k in zip(host[1:], cols_[1:]):
                assert h.dtype == exp[k].dtype and h[:1000].tobytes() == exp[k][at].tobytes(), k
            for h, t in zip(host, bufs):
                assert (h[1000:] == np.asarray(fills[t.dtype], h.dtype)).all()
        assert nstats[2] == 1000                    # every voxel holds one unit normal: each stored row is non-zero


# ------------------------------------------------------------------------------------------------ creator / stage 2
def _creator(seq, out_dir, **kw):
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, keypoint_type=kw.pop("keypoint_type", "grid"),
                               max_num_keypoints=seq.max_kp, estimate_camera_params=True, num_loader_workers=0, **kw)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    return cr


def _items(seq, dev, chunks):
    for c in chunks:
        a, b = seq.chunks[c]
        yield {"frames": seq.frames(c, dev), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
               "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}


def test_creator_dense_cloud_matches_oracle_and_leaves_the_rest_unchanged(tmp_path):
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), n_frames=180)
    runs = {}
    for name, kw in (("off", {}), ("on", dict(dense_voxel_size=0.02, dense_conf_threshold=0.7)),
                     ("maps", dict(keypoint_type="none"))):
        cr = _creator(seq, str(tmp_path / name), **kw)
        runs[name] = [ch for _, ch in cr.process_chunks(_items(seq, cr.device, range(len(seq.chunks))))]
    assert len(runs["on"]) == len(seq.chunks) == 3          # [0, 100), [80, 180) and the overlap tail [160, 180)
    for c, (off, on, maps) in enumerate(zip(runs["off"], runs["on"], runs["maps"])):
        assert set(on) - set(off) == {"dense_cloud"} and "dense_cloud" not in off
        for k in off:
            if k in ("_metrics",):
                continue
            a, b = off[k], on[k]
            if isinstance(a, dict):
                assert set(a) == set(b) and all(torch.equal(a[x], b[x]) for x in a), k
            elif torch.is_tensor(a):
                assert torch.equal(a, b), k
            else:
                assert a == b, k
        imgs = seq.frames(c, "cpu")[0].numpy()
        exp = ref.fuse_pixels(maps["points"].numpy(), maps["conf"].numpy(), maps["masks"].numpy(), imgs, 0.7, 0.02)
        dc = on["dense_cloud"]
        assert dc["voxel_size"] == 0.02 and dc["conf_threshold"] == 0.7
        assert dc["points"].dtype == torch.float32 and dc["colors"].dtype == torch.uint8 and dc["weights"].dtype == torch.int32
        assert dc["points"].numpy().tobytes() == exp["points"].tobytes()
        assert dc["colors"].numpy().tobytes() == exp["colors"].tobytes()
        assert dc["weights"].numpy().tobytes() == exp["weights"].tobytes()
        assert on["_metrics"]["dense_voxels"] == len(exp["keys"]) > 1000


def _oracle_world(chunks, voxel):
    """ref.fuse_point_sets over every chunk cloud moved by its chunk's transform (the product's ops.sim3_apply, a kernel
    with tests of its own: the oracle checks the fusion)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import chunk_transform
    sets = []
    for d in chunks:
        cl = d.get("dense_cloud")
        if cl is None or int(cl["points"].shape[0]) == 0:
            continue
        pts = cl["points"].to(DEV, torch.float32).contiguous().clone()
        ops.sim3_apply(chunk_transform(d).reshape(16).to(DEV).contiguous(), pts, None)
        sets.append((pts.cpu().numpy(), cl["colors"].numpy(), cl["weights"].numpy()))
    return ref.fuse_point_sets(sets, voxel)


def _ply_bytes(points, colors, path):
    from pi3_slam_amd.export import write_ply
    write_ply(points, np.asarray(colors, np.uint8), path)
    return open(path, "rb").read()


def _read_ply_points(path):
    data = open(path, "rb").read()
    head = data.index(b"end_header\n") + len(b"end_header\n")
    rec = np.frombuffer(data[head:], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    return rec["xyz"].astype(np.float64)


def _surface_distance(P, seq):
    """Chunk 0's frame -> world; -> (world points, distance to the nearest wall, distance to the nearest surface)."""
    G0 = seq.gauge_matrix(0)
    Xw = P @ G0[:3, :3].T + G0[:3, 3]
    d_wall = np.min(np.concatenate([np.abs(Xw - seq.lo), np.abs(Xw - seq.hi)], 1), 1)
    d_sph = np.stack([np.abs(np.linalg.norm(Xw - c, axis=1) - r) for c, r in seq.spheres], 1)
    return Xw, d_wall, np.minimum(d_wall, d_sph.min(1))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_chess_room_end_to_end(tmp_path):
    import synth_sequence as ss
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_NONE))
    v = 0.02
    cr = _creator(seq, str(tmp_path), dense_voxel_size=v)
    saved, manifest, _ = cr.write_chunks(cr.process_chunks(_items(seq, cr.device, range(len(seq.chunks)))))
    cr.write_run_metadata(manifest)
    assert len(saved) == 13
    rec = OfflineReconstructor(str(tmp_path), str(tmp_path / "r1"), device=DEV, bundle_adjust=False)
    rec.run()
    ply = str(tmp_path / "r1" / "dense_points.ply")
    got = open(ply, "rb").read()
    exp = _oracle_world(rec.reconstructions, v)
    assert len(exp["keys"]) > 50000
    assert got == _ply_bytes(exp["points"], exp["colors"], str(tmp_path / "oracle.ply"))

    # geometry: chunk 0's frame -> world, distances to the room's walls and spheres
    Xw, d_wall, d = _surface_distance(_read_ply_points(ply), seq)
    P = Xw
    near = float(np.mean(d <= 1e-3))
    print(f"dense map: {len(P)} voxels, {100 * near:.2f} % within 1 mm of a surface, max {1e3 * d.max():.2f} mm")
    assert near >= 0.98
    assert d.max() <= v * np.sqrt(3.0) / 2 + 1e-3
    # sphere 0 carries low confidence: nothing of it may survive the filter (except where it touches a wall)
    c0, r0 = seq.spheres[0]
    on_s0 = np.abs(np.linalg.norm(Xw - c0, axis=1) - r0) <= 1e-2
    assert not np.any(on_s0 & (d_wall > 1e-3))

    # default settings (bundle adjustment on) write a map too.  The prior-constrained adjustment re-bases the chunks'
    # frames; each cloud must still follow its chunk's closed-form similarity ('_sim3_dense'), not the re-based identity
    rec2 = OfflineReconstructor(str(tmp_path), str(tmp_path / "r2"), device=DEV)
    rec2.run()
    assert sum(d.get("_sim3_dense") is not None for d in rec2.reconstructions) >= 6
    ply2 = str(tmp_path / "r2" / "dense_points.ply")
    exp2 = _oracle_world(rec2.reconstructions, v)
    assert open(ply2, "rb").read() == _ply_bytes(exp2["points"], exp2["colors"], str(tmp_path / "oracle2.ply"))
    # the adjusted trajectory itself moves the chunks by up to centimetres, hence the looser tolerance; the same clouds
    # placed by the re-based '_sim3_global' (the identity for every adjusted chunk) must fail it
    _, _, d2 = _surface_distance(_read_ply_points(ply2), seq)
    wrong = _oracle_world([{"dense_cloud": d["dense_cloud"], "_sim3_global": d.get("_sim3_global")}
                           for d in rec2.reconstructions], v)
    _, _, dw = _surface_distance(wrong["points"].astype(np.float64), seq)
    q = {t: (float(np.mean(d2 <= t)), float(np.mean(dw <= t))) for t in (5e-3, 2e-2, 5e-2)}
    print("dense map, bundle adjustment on: fraction within 5 mm / 2 cm / 5 cm of a surface (closed-form similarity, "
          "re-based identity): " + ", ".join(f"{a:.3f} / {b:.3f}" for a, b in q.values()))
    # measured: 0.56 within 5 mm with the closed-form similarity, 0.15 with the identity.  The rest of the adjusted map
    # is off because the per-chunk adjustment before the alignment moves a chunk's frame, which no similarity of the
    # cloud follows (limitation); this checks that every cloud at least follows its similarity
    assert q[5e-3][0] >= 0.5 and q[5e-3][1] <= 0.25 and q[5e-3][0] >= 2.5 * q[5e-3][1]
    OfflineReconstructor(str(tmp_path), str(tmp_path / "r3"), device=DEV, bundle_adjust=False).run()
    assert open(str(tmp_path / "r3" / "dense_points.ply"), "rb").read() == got

    # two ranks (gloo on this one card): the wave path (no bundle adjustment) and the sequential chain (bundle adjustment
    # on) gather the clouds and their transforms on rank 0; its map == the oracle over the chunk files' clouds
    import subprocess
    worker = os.path.join(os.path.dirname(__file__), "dense_dist_worker.py")
    env = dict(os.environ, PI3_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    clouds = [torch.load(f, map_location="cpu", weights_only=False)["dense_cloud"] for f in saved]
    for ba in ("0", "1"):
        out = tmp_path / f"dist{ba}"
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(tmp_path),
                            str(out), ba], env=env, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        tr = torch.load(out / "dense_transforms.pt", weights_only=False)
        assert len(tr["transforms"]) == 13 and (any(tr["rebased"]) == (ba == "1"))
        expd = _oracle_world([{"dense_cloud": c, "_sim3_global": G} for c, G in zip(clouds, tr["transforms"])], v)
        assert open(out / "dense_points.ply", "rb").read() == _ply_bytes(expd["points"], expd["colors"],
                                                                          str(tmp_path / f"oracle_dist{ba}.ply"))


def test_online_save_dense_map_matches_oracle(tmp_path):
    from PIL import Image

    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (232, 296, 3)).astype(np.float32)
    k = 9
    sm = np.cumsum(np.cumsum(base, 0), 1)
    sm = (sm[k:, k:] - sm[:-k, k:] - sm[k:, :-k] + sm[:-k, :-k]) / (k * k)
    paths = []
    for i in range(20):
        p = str(frames / f"frame_{i:05d}.png")
        Image.fromarray(np.clip(sm[i % 20: i % 20 + 192, (2 * i) % 20: (2 * i) % 20 + 256], 0, 255).astype(np.uint8)).save(p)
        paths.append(p)
    engine = Pi3Engine(Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5), DEV)
    with torch.no_grad():     # non-empty masks (the edit bench.py makes to plain recipe weights)
        w_, b_ = engine.w["point_head.proj.weight"], engine.w["point_head.proj.bias"]
        w_[392:588] = 0.05 * w_[392:393].clone()
        b_[392:588] = b_[392].clone()
        engine.w["conf_head.proj.bias"][:196] -= 2.2
    slam = Pi3SLAMOnline(model=engine, chunk_length=8, overlap=3, device=DEV, keypoint_type="grid", max_num_keypoints=100,
                         estimate_camera_params=True, hip_graph=True, output_dir=str(tmp_path / "online"),
                         bundle_adjust=False, conf_threshold=0.05, dense_voxel_size=0.05)
    slam.process_chunks(paths)
    chunks = slam.chunk_reconstructions
    assert all(c["dense_cloud"]["conf_threshold"] == 0.05 for c in chunks)
    out = str(tmp_path / "online" / "dense_points.ply")
    n = slam.save_dense_map(out)
    exp = _oracle_world(chunks, 0.05)
    print(f"online dense map: {n} voxels; per chunk {[c['_metrics'].get('dense_voxels') for c in chunks]} voxels, "
          f"{[c['_metrics'].get('dense_dropped') for c in chunks]} dropped, keypoint mask fraction "
          f"{[round(float(c['masks'].float().mean()), 3) for c in chunks]}")
    assert n == len(exp["keys"]) > 0
    assert open(out, "rb").read() == _ply_bytes(exp["points"], exp["colors"], str(tmp_path / "oracle.ply"))
