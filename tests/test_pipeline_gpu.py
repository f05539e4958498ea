"""GPU end-to-end plumbing (BASELINE.json configs[0] shape): 32 synthetic 256x192 PNG frames, chunk_length=32,
overlap=8 -> chunk files with the reference's layout -> OfflineReconstructor -> TUM trajectory.  Uses a narrow model
(recipe weights) so it runs in seconds; the frames are resized to 308x406 by the reference's target-size rule."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _write_frames(d, n=32, w=256, h=192):
    from PIL import Image
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (h + 40, w + 40, 3)).astype(np.float32)
    k = 9
    sm = np.cumsum(np.cumsum(base, 0), 1)           # box blur via integral image so the resize is non-trivial
    sm = (sm[k:, k:] - sm[:-k, k:] - sm[k:, :-k] + sm[:-k, :-k]) / (k * k)
    paths = []
    for i in range(n):
        crop = sm[i % 20: i % 20 + h, (2 * i) % 20: (2 * i) % 20 + w]
        p = os.path.join(d, f"frame_{i:05d}.png")
        Image.fromarray(np.clip(crop, 0, 255).astype(np.uint8)).save(p)
        paths.append(p)
    return paths


def test_process_and_save_then_reconstruct(tmp_path, built_lib):
    assert torch.cuda.is_available()
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.moge import MoGeEngine
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    paths = _write_frames(str(frames))
    out = tmp_path / "out"
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=str(out), chunk_length=32, overlap=8,
                               do_metric_depth=True, keypoint_type="grid", max_num_keypoints=200,
                               num_loader_workers=0, pin_memory=False)
    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    creator = OfflineChunkCreator(cfg, model=Pi3Engine(small, "cuda:0"),
                                  moge_model=MoGeEngine.from_pretrained("recipe", "cuda:0"))
    saved = creator.process_and_save(paths)
    assert creator.target_size == (308, 406)
    assert [os.path.basename(s) for s in saved] == ["chunk_000000.pt", "chunk_000001.pt"]   # (0,32) + tail (24,32)
    meta = json.load(open(out / "chunk_metadata.json"))
    assert meta == {"chunk_length": 32, "overlap": 8, "target_size": [308, 406]}
    man = json.load(open(out / "chunks_manifest.json"))
    assert [(m["start_idx"], m["end_idx"], m["num_frames"]) for m in man] == [(0, 32, 32), (24, 32, 8)]
    c0 = torch.load(saved[0], map_location="cpu", weights_only=False)
    assert c0["points"].shape == (32, 200, 3) and c0["points"].dtype == torch.float16
    assert c0["keypoints"].shape == (32, 200, 2) and c0["masks"].dtype == torch.bool
    assert c0["intrinsics"].shape == (32, 3, 3) and c0["chunk_index"] == 0 and c0["end_idx"] == 32
    assert torch.isfinite(c0["points"].float()).all() and torch.isfinite(c0["camera_poses"]).all()
    with pytest.raises(ValueError):
        creator.process_and_save([])                                             # offline_chunk_creator.py:263-264
    rec = OfflineReconstructor(str(out), str(tmp_path / "recon"), save_observations=True)
    assert (rec.chunk_length, rec.overlap) == (32, 8)
    rec.run()
    obs = torch.load(tmp_path / "recon" / "reconstructions" / "observations_000000.pt", weights_only=False)
    assert obs["uv"].shape == (obs["source_frame"].numel(), 2) and obs["source_frame"].numel() > 0
    assert (obs["uv"][:, 0] >= 0).all() and (obs["uv"][:, 0] < 406).all() and (obs["uv"][:, 1] < 308).all()
    assert (obs["target_frame"] != obs["source_frame"]).all()
    assert ((obs["target_frame"] < obs["source_frame"]) | (obs["target_frame"] - obs["source_frame"] <= 2)).all()
    lines = open(tmp_path / "recon" / "trajectory_tum.txt").read().strip().split("\n")
    assert len(lines) == 1 + 32                                                  # 40 poses, 8 duplicates dropped
    vals = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    assert np.isfinite(vals).all() and np.allclose(np.linalg.norm(vals[:, 4:8], axis=1), 1.0, atol=1e-5)


def test_device_resize_pipeline_is_identical_to_host_resize(tmp_path, built_lib):
    """§8f rank 2 wired into process_and_save: loader workers only decode, Resize + ToTensor run on the GPU.  The ingest
    is bit-identical to PIL + ToTensor, so every stored tensor of every chunk must equal the host-resize run."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    paths = _write_frames(str(frames))[:12]
    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine = Pi3Engine(small, "cuda:0")
    saved = {}
    for flag, workers in ((False, 0), (True, 2)):
        out = tmp_path / f"out_{int(flag)}"
        cfg = OfflineCreatorConfig(model_path="recipe", output_dir=str(out), chunk_length=8, overlap=2,
                                   do_metric_depth=False, keypoint_type="grid", max_num_keypoints=100,
                                   num_loader_workers=workers, pin_memory=False, device_resize=flag)
        saved[flag] = OfflineChunkCreator(cfg, model=engine, moge_model=None).process_and_save(paths)
    assert len(saved[False]) == len(saved[True]) == 2
    for a, b in zip(saved[False], saved[True]):
        ca = torch.load(a, map_location="cpu", weights_only=False)
        cb = torch.load(b, map_location="cpu", weights_only=False)
        for k in ("points", "local_points", "conf", "masks", "keypoints", "colors", "camera_poses", "intrinsics"):
            assert torch.equal(ca[k], cb[k]), k


def test_overlapped_stages_write_the_same_chunk_files(tmp_path, built_lib):
    """Pipelined execution (next chunk's upload + resize on the copy stream, MoGe beside the forward, packed D2H,
    writer thread) against the same run with overlap_stages=False (one chunk at a time): every stored tensor of every
    chunk file is bit-identical.  Reference for the overlap: slam/offline_chunk_creator.py:279-287."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.moge import MoGeEngine
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    paths = _write_frames(str(frames))[:26]
    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine, moge = Pi3Engine(small, "cuda:0"), MoGeEngine.from_pretrained("recipe", "cuda:0")
    saved = {}
    for flag in (False, True):
        out = tmp_path / f"out_{int(flag)}"
        cfg = OfflineCreatorConfig(model_path="recipe", output_dir=str(out), chunk_length=8, overlap=2,
                                   do_metric_depth=True, keypoint_type="grid", max_num_keypoints=100,
                                   num_loader_workers=2 if flag else 0, pin_memory=flag, device_resize=True,
                                   overlap_stages=flag)
        saved[flag] = OfflineChunkCreator(cfg, model=engine, moge_model=moge).process_and_save(paths)
    assert len(saved[False]) == len(saved[True]) == 5       # starts 0, 6, 12, 18, 24 (the last one: 2 frames)
    for a, b in zip(saved[False], saved[True]):
        ca = torch.load(a, map_location="cpu", weights_only=False)
        cb = torch.load(b, map_location="cpu", weights_only=False)
        assert set(ca) == set(cb)
        for k in ca:
            if torch.is_tensor(ca[k]) and k != "image_paths":
                assert ca[k].dtype == cb[k].dtype and torch.equal(ca[k], cb[k]), k
        for k in ca["camera_params"]:
            assert torch.equal(ca["camera_params"][k], cb["camera_params"][k]), k
        from pi3_slam_amd.export import view_name      # 1-tuples (collate) vs 1-lists (collate + pin): SURVEY §8b
        assert [view_name(p) for p in ca["image_paths"]] == [view_name(p) for p in cb["image_paths"]]
        assert ca["chunk_index"] == cb["chunk_index"]
        assert ca["_metrics"]["metric_scale"] == cb["_metrics"]["metric_scale"]


def test_graphed_moge_depth_belongs_to_its_own_chunk(built_lib):
    """hip_graph + MoGe + overlapped stages (Pi3SLAMOnline's default): the MoGe graph returns ONE static buffer and
    chunk k+1's replay is queued while chunk k's forward still runs, so chunk k must read a private copy.  A stand-in
    MoGe whose `infer_graphed` has exactly that static-buffer contract and whose depth encodes the chunk's first frame
    makes a mix-up visible as a wrong metric scale (offline_chunk_creator.py:184-192: the scale of a chunk comes from
    ITS first frame)."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config

    class StaticDepth:
        def __init__(self):
            self.static = None

        def infer(self, img):
            return {"depth": (1.0 + 4.0 * img.mean()).expand(img.shape[-2:]).contiguous()}

        def infer_graphed(self, img):
            if self.static is None:
                self.static = torch.empty(img.shape[-2:], device=img.device)
            self.static.copy_((1.0 + 4.0 * img.mean()).expand(img.shape[-2:]))
            return {"depth": self.static}

    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine = Pi3Engine(small, "cuda:0")
    g = torch.Generator().manual_seed(5)
    base = torch.rand(1, 6, 3, 56, 70, generator=g)
    items = [{"frames": (base * (0.15 + 0.2 * c)).clamp(0, 1), "paths": [[f"c{c}_{i}.png"] for i in range(6)],
              "meta": {"chunk_index": c}} for c in range(4)]                  # distinct first-frame brightness per chunk
    scales = {}
    for mode, graph, overlap in (("serial", False, False), ("graph_overlap", True, True)):
        cfg = OfflineCreatorConfig(model_path="recipe", output_dir="/tmp/pi3_t_graphmoge", chunk_length=6, overlap=2,
                                   do_metric_depth=True, keypoint_type="grid", max_num_keypoints=50,
                                   num_loader_workers=0, hip_graph=graph, overlap_stages=overlap)
        cr = OfflineChunkCreator(cfg, model=engine, moge_model=StaticDepth())
        cr.target_size = (56, 70)
        # recipe weights give an (almost) empty validity mask, hence no scale at all: take every pixel, so that the
        # median really is a function of the chunk's own depth map
        cr._compute_masks = lambda pi3: torch.ones(pi3["conf"].shape[:4], dtype=torch.bool, device=pi3["conf"].device)
        scales[mode] = [r["_metrics"]["metric_scale"] for _, r in cr.process_chunks(items)]
    assert all(s is not None for s in scales["serial"]), scales        # otherwise the test says nothing
    assert len(set(scales["serial"])) == 4, scales
    assert scales["graph_overlap"] == scales["serial"], scales


def test_metric_scale_fallback_is_reported(built_lib, capsys):
    """An unusable MoGe depth (no valid pixel under the mask) must not rescale the chunk and must say so: the reference
    would raise in torch.median of an empty tensor (offline_chunk_creator.py:121-127)."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config

    class NoDepth:
        def infer(self, img):
            return {"depth": torch.full(img.shape[-2:], float("inf"), device=img.device)}

    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine = Pi3Engine(small, "cuda:0")
    imgs = torch.rand(1, 3, 3, 56, 70, generator=torch.Generator().manual_seed(1))
    res = {}
    for name, moge in (("none", None), ("nodepth", NoDepth())):
        cfg = OfflineCreatorConfig(model_path="recipe", output_dir="/tmp/pi3_t_scale", do_metric_depth=moge is not None,
                                   keypoint_type="grid", max_num_keypoints=50, num_loader_workers=0)
        cr = OfflineChunkCreator(cfg, model=engine, moge_model=moge)
        cr.target_size = (56, 70)
        res[name] = cr._process_single_chunk(imgs, [[f"f{i}.png"] for i in range(3)])
    assert "metric scale not applied" in capsys.readouterr().out
    assert res["nodepth"]["_metrics"]["metric_scale"] is None and "metric_scale" not in res["none"]["_metrics"]
    for k in ("points", "local_points", "camera_poses"):
        assert torch.equal(res["none"][k], res["nodepth"][k]), k


def test_process_and_save_with_calibration_undistorts_on_device(tmp_path, built_lib):
    """BASELINE config 4 plumbing: --cam-dist-path (EuRoC calibration) -> frames are undistorted on the GPU before pi3;
    the frames handed to the model equal the oracle restatement of the reference's remap + ToTensor."""
    from PIL import Image
    from oracle import undistort_ref as U
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config
    cal_path = os.path.join(os.path.dirname(__file__), "golden", "calib_euroc_cam0_calib.json")
    rng = np.random.default_rng(9)
    frames = tmp_path / "frames"
    frames.mkdir()
    paths, raw = [], []
    for i in range(4):
        a = rng.integers(0, 256, (480, 752, 3), dtype=np.uint8)
        p = str(frames / f"{i:04d}.png")
        Image.fromarray(a).save(p)
        paths.append(p)
        raw.append(a)
    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine = Pi3Engine(small, "cuda:0")
    seen = []

    class Spy:
        def __call__(self, imgs):
            seen.append(imgs.detach().cpu().numpy())
            return engine.forward(imgs)

    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=str(tmp_path / "out"), chunk_length=4, overlap=1,
                               do_metric_depth=False, keypoint_type="grid", max_num_keypoints=50,
                               num_loader_workers=0, pin_memory=False, cam_dist_path=cal_path)
    creator = OfflineChunkCreator(cfg, model=Spy(), moge_model=None)
    assert creator.undistortion_maps is not None
    saved = creator.process_and_save(paths)
    assert len(saved) == 1 and seen[0].shape[:2] == (1, 4)
    import json
    ref = U.undistort_frames(np.stack(raw), json.load(open(cal_path)), creator.target_size)
    mism = (seen[0][0] != ref).mean()
    assert mism < 1e-3, mism          # maps may differ by 1 ulp -> a 1/32-pixel bucket flip on isolated pixels
    assert np.abs(seen[0][0] - ref).max() <= 8.0 / 255.0 + 1e-6


def test_two_rank_pipeline_matches_single_process(tmp_path, built_lib):
    """SURVEY §8e in the product path: under torch.distributed.run the creator shards chunks (c % world) and the
    reconstructor aligns wave by wave (boundary all-gather, own solve per rank, 136-byte all-gather, prefix product).
    Two gloo ranks on this box's GPU must write the chunk files of a single-process run bit for bit and the same
    trajectory (both paths solve on chunk-frame values and compose in fp64; the TUM file carries 6 decimals).  The same
    holds for the online sliding-window path with its chunk-parallel branch and in-order draining."""
    import subprocess
    import sys
    frames = tmp_path / "frames"
    frames.mkdir()
    _write_frames(str(frames))
    worker = os.path.join(os.path.dirname(__file__), "dist_pipeline_worker.py")
    env = dict(os.environ, PI3_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r1 = subprocess.run([sys.executable, worker, str(frames), str(tmp_path / "o1"), str(tmp_path / "r1")], env=env,
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                         "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(frames),
                         str(tmp_path / "o2"), str(tmp_path / "r2")], env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    f1 = sorted(os.listdir(tmp_path / "o1" / "chunks"))
    f2 = sorted(os.listdir(tmp_path / "o2" / "chunks"))
    assert f1 == f2 and len(f1) >= 5
    for name in f1:
        a = torch.load(tmp_path / "o1" / "chunks" / name, map_location="cpu", weights_only=False)
        b = torch.load(tmp_path / "o2" / "chunks" / name, map_location="cpu", weights_only=False)
        for k in ("points", "local_points", "conf", "masks", "keypoints", "colors", "camera_poses", "intrinsics"):
            assert torch.equal(a[k], b[k]), (name, k)
        assert a["chunk_index"] == b["chunk_index"] and a["start_idx"] == b["start_idx"]
    assert json.load(open(tmp_path / "o1" / "chunks_manifest.json")) == json.load(open(tmp_path / "o2" / "chunks_manifest.json"))
    assert json.load(open(tmp_path / "o1" / "chunk_metadata.json")) == json.load(open(tmp_path / "o2" / "chunk_metadata.json"))
    t1 = np.loadtxt(tmp_path / "r1" / "trajectory_tum.txt")
    t2 = np.loadtxt(tmp_path / "r2" / "trajectory_tum.txt")
    assert t1.shape == t2.shape and t1.shape[0] == 32
    scale = np.abs(t1[:, 1:4]).max() + 1e-9
    assert np.abs(t1[:, 1:4] - t2[:, 1:4]).max() / scale < 1e-4
    dq = np.minimum(np.abs(t1[:, 4:] - t2[:, 4:]).max(1), np.abs(t1[:, 4:] + t2[:, 4:]).max(1))
    assert dq.max() < 1e-4
    # online path: single process (sequential align) == two ranks (wave alignment + in-order drain on rank 0)
    o1 = np.loadtxt(tmp_path / "r1" / "online" / "traj.txt")
    o2 = np.loadtxt(tmp_path / "r2" / "online" / "traj.txt")
    assert o1.shape == o2.shape == (32, 8)
    assert np.abs(o1[:, 1:4] - o2[:, 1:4]).max() / (np.abs(o1[:, 1:4]).max() + 1e-9) < 1e-4
    assert np.abs(o1[:, 1:4] - t1[:, 1:4]).max() / scale < 1e-4      # and the online flow equals the offline one
    # online with bundle adjustment on: the two-rank run goes through the sequential refinement chain
    b1 = np.loadtxt(tmp_path / "r1" / "online_ba" / "traj.txt")
    b2 = np.loadtxt(tmp_path / "r2" / "online_ba" / "traj.txt")
    assert b1.shape == b2.shape == (32, 8) and np.array_equal(b1, b2), np.abs(b1 - b2).max()


def test_reconstruct_with_bundle_adjust_under_torchrun_equals_single_process(tmp_path, built_lib):
    """`reconstruct` under torch.distributed.run with bundle adjustment on (the default).  The reference's flow is
    strictly sequential (slam/offline_reconstructor.py:130-133: align chunk c to the already refined chunk c-1, then the
    prior-constrained BA of utils/reconstruction_alignment.py:107-171), so the chunk-parallel run takes the ranks in
    turn for that chain (reconstructor._run_chain: per-chunk BA in parallel, then alignment + prior BA in
    chunk order, the refined chunk handed to the next owner): all three stages run and the trajectory equals the
    single-process one (round 2 skipped the prior-constrained stage under torchrun and differed silently).  Five
    overlapping cuts of one synthetic scene, each in its own similarity frame; both recover the ground truth."""
    import subprocess
    import sys
    from ba_problem import make_problem
    N, K, W, H = 12, 40, 406, 308
    pb = make_problem(N=N, K=K, seed=2)
    poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    poses[:, :3, :3] = pb["R_gt"].transpose(0, 2, 1)
    poses[:, :3, 3] = pb["C_gt"]
    K3 = np.zeros((N, 3, 3), np.float32)
    K3[:, 0, 0], K3[:, 1, 1], K3[:, 0, 2], K3[:, 1, 2], K3[:, 2, 2] = pb["intr"][:, 0], pb["intr"][:, 1], pb["intr"][:, 2], pb["intr"][:, 3], 1
    idx = np.arange(N)
    full = dict(points=torch.from_numpy(pb["X_gt"].reshape(N, K, 3)).half(), camera_poses=torch.from_numpy(poses),
                intrinsics=torch.from_numpy(K3), keypoints=torch.from_numpy(pb["uv"][idx, idx]).half(),
                masks=torch.ones(N, K, 1, dtype=torch.bool), colors=torch.full((N, K, 3), 99.0).half())
    cdir = tmp_path / "chunks_root"
    os.makedirs(cdir / "chunks")
    cl, ov = 4, 2
    starts = list(range(0, N - ov, cl - ov))                    # 0, 2, 4, 6, 8 -> five chunks of four views
    for c, s0 in enumerate(starts):
        sl = slice(s0, s0 + cl)
        d = {k: v[sl].clone() for k, v in full.items()}
        # every chunk in its own frame: a similarity of the scene, as chunks of a real run are
        ang, sc, t = 0.2 * c, 1.0 + 0.05 * c, torch.tensor([0.3 * c, -0.1 * c, 0.05 * c])
        R = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
        d["points"] = (((d["points"].float() - t) @ R) / sc).half()
        P = d["camera_poses"].clone()
        P[:, :3, :3] = R.T @ P[:, :3, :3]
        P[:, :3, 3] = ((d["camera_poses"][:, :3, 3] - t) @ R) / sc
        d["camera_poses"] = P
        d.update(image_paths=[[f"img_{i:03d}.png"] for i in range(s0, s0 + cl)], original_width=W, original_height=H,
                 chunk_index=c)
        torch.save(d, cdir / "chunks" / f"chunk_{c:06d}.pt")
    json.dump({"chunk_length": cl, "overlap": ov, "target_size": [H, W]}, open(cdir / "chunk_metadata.json", "w"))
    worker = os.path.join(os.path.dirname(__file__), "dist_recon_worker.py")
    env = dict(os.environ, PI3_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r1 = subprocess.run([sys.executable, worker, str(cdir), str(tmp_path / "seq")], env=env, capture_output=True,
                        text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                         "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(cdir),
                         str(tmp_path / "par")], env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    s1, s2 = json.load(open(tmp_path / "seq" / "stages.json")), json.load(open(tmp_path / "par" / "stages.json"))
    assert s1["stages"] == s2["stages"] == ["per_chunk_bundle_adjust", "closed_form_sim3", "prior_constrained_bundle_adjust"]
    assert "sequential refinement chain" in r2.stdout
    assert all(s1["ba"]) and all(s2["ba"])
    t1 = np.loadtxt(tmp_path / "seq" / "trajectory_tum.txt")
    t2 = np.loadtxt(tmp_path / "par" / "trajectory_tum.txt")
    assert t1.shape == t2.shape == (N, 8)
    # both live in chunk 0's frame = the scene frame (chunk 0 was cut with the identity similarity)
    assert np.abs(t1[:, 1:4] - pb["C_gt"]).max() < 2e-2
    assert np.array_equal(t1, t2), np.abs(t1 - t2).max()          # the same arithmetic on the same data: 6-decimal text equal


@pytest.mark.parametrize("launcher", ["plain", "torchrun"])
def test_bench_two_ranks_rehearsal(tmp_path, built_lib, launcher):
    """`bench.py --gpus 2` both ways the driver may start it - as a PLAIN process (bench.py launches its own ranks before
    any GPU call and relays rank 0's line) and under torch.distributed.run - with gloo standing in for RCCL because both
    ranks share this box's one GPU: the N > 1 branch (one chunk per rank per step, boundary all-gather, own solve,
    136-byte all-gather, prefix product, max-over-ranks timing) runs end to end and prints ONE JSON line with the
    whole-job aggregate and the comm record (what torch.distributed saw)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PI3_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PI3_BENCH_LAUNCHER"):
        env.pop(k, None)
    bench = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"]
    if launcher == "plain":
        cmd = [sys.executable] + bench
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + bench
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["scaling"] == "weak" and rec["unit"] == "frames/s"
    assert rec["value"] > 0 and abs(rec["value"] - 2 * 100 * 2 / (rec["ms_per_step"] * 2 / 1e3)) < 1e-6 * rec["value"]
    assert rec["roofline"]["bound"] == "mfma" and 0 < rec["roofline"]["frac"] < 1
    assert "cpu_baseline" not in rec            # rank 0 at N = 1 only
    comm = rec["comm"]
    assert comm["backend"] == "gloo" and comm["world_size"] == 2
    assert comm["launcher"] == ("self" if launcher == "plain" else "torch.distributed.run")
    assert [x["rank"] for x in comm["ranks"]] == [0, 1] and len({x["pid"] for x in comm["ranks"]}) == 2
    assert all(x["device_name"] and x["device"].startswith("cuda:") for x in comm["ranks"])
    assert comm["allgather_bytes_per_wave"]["per_rank_boundary_block"] == (1 + 2 * 20 * 200 * 6 + 16) * 4
    assert len(comm["per_rank"]) == 2 and all(p["ms_per_step"] <= rec["ms_per_step"] * (1 + 1e-9) for p in comm["per_rank"])
    assert rec["n1_reference_ms_per_step"]["ms_per_step"] > 0


def test_bench_nccl_branch_with_a_forced_one_rank_group(built_lib):
    """bench.py's nccl (= RCCL) code path on the hardware that is available: PI3_DIST_FORCE=1 builds a ONE-rank RCCL group
    and takes the wave-alignment path (device-resident boundary blocks through dist.all_gather on nccl, the 136-byte
    record all-gather, max-over-ranks all_reduce, barrier) - the calls that otherwise run for the first time on the
    driver's 8-GPU node.  The line must carry the comm record with what RCCL reports."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PI3_DIST_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PI3_DIST_BACKEND", "PI3_BENCH_LAUNCHER"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--no-extras", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    comm = rec["comm"]
    assert rec["n_gpus"] == 1 and comm["backend"] == "nccl" and comm["world_size"] == 1
    assert comm["ranks"][0]["device"] == "cuda:0" and comm["ranks"][0]["device_name"]
    assert "rccl_version" in comm and "unavailable" not in str(comm["rccl_version"])
    assert comm["allgather_bytes_per_wave"]["boundary_blocks"] == (1 + 2 * 20 * 200 * 6 + 16) * 4
    assert rec["value"] > 30 and 0 < rec["roofline"]["frac"] < 1 and len(comm["per_rank"]) == 1


def test_bench_plain_run_dumps_the_last_step(tmp_path, built_lib):
    """The plain one-GPU bench: the headline keys, nothing of --full, and --dump-outputs writing the aligned chunk
    dictionary of the last timed step (float32 / float64, finite where the chunk file is)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PI3_DIST_BACKEND", "PI3_DIST_FORCE",
              "PI3_BENCH_LAUNCHER", "PI3_BENCH_STUB"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=600,
                       cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["unit"] == "frames/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["value"] == pytest.approx(100 * 2 / (rec["ms_per_step"] * 2e-3), rel=1e-6)
    assert not {"cpu_baseline", "extras", "second_metric", "comm"} & set(rec)
    files = {p.name[:-4]: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert {"points", "local_points", "conf", "keypoints", "colors", "masks", "camera_poses", "sim3_global"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["points"].shape[:2] == (100, 200) and files["sim3_global"].shape == (4, 4)
    assert np.isfinite(files["camera_poses"]).all() and np.isfinite(files["sim3_global"]).all()


def test_rccl_branch_with_a_one_rank_group(tmp_path, built_lib):
    """The nccl (= RCCL) branch of the chunk-parallel code on the hardware that is available: ONE rank on this box's GPU
    (two ranks cannot share a card under RCCL).  Device-resident boundary blocks, all-gathers of device tensors,
    process-group device binding (init_process_group(device_id=...)), 'cuda' -> cuda:LOCAL_RANK resolution: the wave
    alignment must reproduce the sequential run."""
    import subprocess
    import sys
    frames = tmp_path / "frames"
    frames.mkdir()
    _write_frames(str(frames))
    worker = os.path.join(os.path.dirname(__file__), "dist_pipeline_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "PI3_DIST_BACKEND", "PI3_DIST_FORCE"):
        env.pop(k, None)
    r1 = subprocess.run([sys.executable, worker, str(frames), str(tmp_path / "o1"), str(tmp_path / "r1")], env=env,
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    env2 = dict(env, PI3_DIST_BACKEND="nccl", PI3_DIST_FORCE="1")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                         "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(frames),
                         str(tmp_path / "o2"), str(tmp_path / "r2")], env=env2, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert "on 1 ranks" in r2.stdout                              # the distributed code path ran
    t1 = np.loadtxt(tmp_path / "r1" / "trajectory_tum.txt")
    t2 = np.loadtxt(tmp_path / "r2" / "trajectory_tum.txt")
    assert t1.shape == t2.shape == (32, 8)
    assert np.abs(t1[:, 1:] - t2[:, 1:]).max() < 1e-4


def test_cli_entry_points_full_model(tmp_path, built_lib):
    """python -m pi3_slam_amd.cli create / reconstruct with the reference's flags, full-size pi3
    (recipe weights) + recipe MoGe, undistortion off, 10 frames."""
    from pi3_slam_amd import cli
    frames = tmp_path / "frames"
    frames.mkdir()
    _write_frames(str(frames), n=10)
    out = tmp_path / "chunks_out"
    cli.main(["create", "--images", str(frames), "--output", str(out), "--chunk-length", "6", "--overlap", "2", "--model-path",
             "recipe", "--moge-model-path", "recipe", "--keypoints", "grid", "--max-kp", "64", "--num-workers", "0",
             "--skip-start", "1", "--device-resize", "--hip-graph"])
    man = json.load(open(out / "chunks_manifest.json"))
    assert [(m["start_idx"], m["end_idx"]) for m in man] == [(0, 6), (4, 9)]        # (8, 9) has < 2 frames: dropped
    cli.main(["reconstruct", "--chunks", str(out), "--output", str(tmp_path / "rec"), "--save-observations"])
    lines = open(tmp_path / "rec" / "trajectory_tum.txt").read().strip().split("\n")
    assert len(lines) == 1 + 9                                   # 10 frames, the first one skipped
    assert os.path.exists(tmp_path / "rec" / "final_points.ply")


def test_cli_online_entry_point_full_model(tmp_path, built_lib):
    """python -m pi3_slam_amd.cli online with the reference online script's flags (pi3_slam_online_modular.py:117-183):
    full-size pi3 with recipe weights, 14 frames in sliding windows of 6 / overlap 2, trajectory.ply + trajectory.tum
    under --output_path as the reference writes them."""
    from pi3_slam_amd import cli
    frames = tmp_path / "frames"
    frames.mkdir()
    _write_frames(str(frames), n=14)
    out = tmp_path / "result"
    cli.main(["online", "--image_dir", str(frames), "--output_path", str(out), "--chunk_length", "6", "--overlap", "2",
              "--model_path", "recipe", "--no_metric_depth", "--max_num_keypoints", "64", "--num_workers", "0",
              "--save_tum", "--tum_integer_timestamp", "--no_visualization", "--skip_end", "1", "--no_bundle_adjust"])
    tum = np.loadtxt(out / "trajectory.tum")
    assert tum.shape == (13, 8) and np.isfinite(tum).all()
    assert np.array_equal(tum[:, 0], np.round(tum[:, 0]))                        # integer time stamps
    assert os.path.getsize(out / "trajectory.ply") > 0


def test_online_sliding_window_matches_offline_two_stage(tmp_path, built_lib):
    """BASELINE config 5 plumbing: the online facade (stream -> chunks -> progressive alignment, hipGraph forward) must
    give the trajectory of the offline two-stage flow (same kernels, no disk round trip)."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    from pi3_slam_amd.weights import Pi3Config
    frames = tmp_path / "frames"
    frames.mkdir()
    paths = _write_frames(str(frames), n=20)
    small = Pi3Config(dim=128, enc_depth=1, dec_depth=2, head_depth=1, cam_dim=128, pos_grid=5)
    engine = Pi3Engine(small, "cuda:0")
    slam = Pi3SLAMOnline(model=engine, chunk_length=8, overlap=3, device="cuda:0", keypoint_type="grid",
                         max_num_keypoints=100, estimate_camera_params=True, hip_graph=True,
                         output_dir=str(tmp_path / "online"))
    res = slam.process_chunks(paths)
    assert slam.get_reconstruction_count() == len(res) == 4 and slam.get_statistics()["num_frames"] == 20
    slam.save_trajectory_tum(str(tmp_path / "online" / "traj.txt"), integer_timestamp=True)
    slam.save_final_result(str(tmp_path / "online" / "points.ply"))
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=str(tmp_path / "off"), chunk_length=8, overlap=3,
                               do_metric_depth=False, keypoint_type="grid", max_num_keypoints=100,
                               num_loader_workers=0, pin_memory=False)
    OfflineChunkCreator(cfg, model=engine, moge_model=None).process_and_save(paths)
    OfflineReconstructor(str(tmp_path / "off"), str(tmp_path / "off_rec")).run()
    t_on = np.loadtxt(tmp_path / "online" / "traj.txt")
    t_off = np.loadtxt(tmp_path / "off_rec" / "trajectory_tum.txt")
    assert t_on.shape == t_off.shape == (20, 8)
    # the offline flow stores chunks as fp16 / reloads them; the online one aligns the same tensors in memory
    assert np.abs(t_on - t_off).max() < 1e-4
    assert "pi3_forward" in slam.get_timing_statistics() and os.path.getsize(tmp_path / "online" / "points.ply") > 0


def test_consumer_side_alignment_does_not_wait_for_the_running_forward(built_lib):
    """Pipeline rule: no host<->device copy is ever queued behind a forward, so the consumer's Sim(3)
    alignment of chunk k-1 and the stage-in of chunk k+1 run BESIDE the forward of chunk k.  Before the rule held, the
    alignment's first upload returned only when the running forward ended (~60 % of a forward per chunk on average)
    and a stage-in took 80-180 ms instead of ~2 ms.  Full-size model so that a forward is long enough to tell."""
    import time
    from pi3_slam_amd.alignment import align_and_refine_reconstructions, create_view_graph_matches
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config
    dev = "cuda:0"
    engine = Pi3Engine(Pi3Config(), dev)
    n, ov = 60, 12
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir="/tmp/pi3_test_unused", chunk_length=n, overlap=ov, device=dev,
                               do_metric_depth=False, keypoint_type="grid", max_num_keypoints=200, device_resize=True)
    cr = OfflineChunkCreator(cfg, model=engine, moge_model=None)
    cr.target_size = (308, 406)
    frames = torch.randint(0, 256, (n, 384, 512, 3), dtype=torch.uint8).pin_memory()
    paths = [[f"f{i}.png"] for i in range(n)]
    matches = create_view_graph_matches(n, ov)
    side = torch.cuda.Stream(dev, priority=-1)
    items = ({"frames": frames, "kind": "u8", "paths": paths, "meta": {"chunk_index": i}} for i in range(7))
    prev, waits, forwards, stage = None, [], [], []
    for meta, chunk in cr.process_chunks(items):
        if prev is not None:
            t0 = time.perf_counter()
            with torch.cuda.stream(side):
                ok, _ = align_and_refine_reconstructions(prev, chunk, matches, device=dev)
            waits.append(time.perf_counter() - t0)
            assert ok
        forwards.append(chunk["_metrics"]["infer_s"])
        stage.append(chunk["_metrics"].get("stage_in_s", 0.0))
        prev = chunk
    fwd = float(np.median(forwards))
    assert fwd > 0.1                                   # the premise: a forward long enough to hide behind
    # steady state (the first two chunks include first-use allocations and table builds).  This is a STRUCTURAL check, not
    # a latency bound: when a copy is queued behind a forward EVERY alignment waits ~60 % of a forward and every stage-in
    # 40-90 %, so the median says whether the rule holds.  (Round 4's one-off 92 ms sample among 1-2 ms ones was found in
    # round 5 - an OpenMP region of a small ATen CPU operator under the box's CPU quota, pi3_slam_amd/hostmem.py - and is
    # gone: 0 of 198 alignments above 2.6 ms, gpurun_out/r5c/stall3.log.  The wall-clock figures - median, maximum, count
    # above 10 ms over the timed steps - are reported by bench.py under `stages_ms.align_host_wait_*` with their bound.)
    w, st = sorted(waits[2:]), sorted(stage[2:])
    assert w[len(w) // 2] < 0.25 * fwd, (waits, fwd)
    assert st[len(st) // 2] < 0.25 * fwd, (stage, fwd)


def test_online_stream_full_model_hipgraph_replay_equals_eager_launches(tmp_path, built_lib):
    """BASELINE configs[4] on one GPU at stream scale: 980 frames 512x384 -> 13 chunks of 100 frames
    at 308x406 (overlap 20, the last chunk 20 frames), the FULL model, MoGe metric scale and LM intrinsics on, through
    Pi3SLAMOnline.process_chunks (slam/online_reconstructor.py:761-920: loader, per-chunk forward, progressive alignment,
    in-order results) - once with the per-chunk forward replayed from one captured hipGraph, once with plain launches.
    The two runs must produce the same chunk tensors bit for bit and the same global similarities; results come out in
    chunk order; every new frame is accounted exactly once; after the start-up chunks no alignment keeps the host
    waiting (the alignment of chunk k-1 rides beside the forward of chunk k)."""
    from PIL import Image
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.moge import MoGeEngine
    from pi3_slam_amd.online import Pi3SLAMOnline
    from pi3_slam_amd.weights import Pi3Config
    dev = "cuda:0"
    n_frames, n_distinct, cl, ov = 980, 100, 100, 20
    fdir = tmp_path / "frames"
    fdir.mkdir()
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (384 + 64, 512 + 64, 3)).astype(np.uint8)
    files = []
    for i in range(n_frames):                      # 100 distinct images, the rest hard links (the stream's content repeats)
        p = str(fdir / f"frame_{i:05d}.png")
        if i < n_distinct:
            Image.fromarray(base[i % 64: i % 64 + 384, (3 * i) % 64: (3 * i) % 64 + 512]).save(p, compress_level=1)
        else:
            os.link(files[i % n_distinct], p)
        files.append(p)
    engine = Pi3Engine(Pi3Config(), dev)
    with torch.no_grad():      # non-empty masks, so that the metric scale is live (bench.py, fixture pi3_full_masks)
        w_, b_ = engine.w["point_head.proj.weight"], engine.w["point_head.proj.bias"]
        w_[392:588] = 0.05 * w_[392:393].clone()
        b_[392:588] = b_[392].clone()
        engine.w["conf_head.proj.bias"][:196] -= 2.2
    moge = MoGeEngine.from_pretrained("recipe", dev)
    runs = {}
    for mode, graph in (("hip_graph", True), ("eager", False)):
        slam = Pi3SLAMOnline(model=engine, chunk_length=cl, overlap=ov, device=dev, keypoint_type="grid",
                             max_num_keypoints=200, estimate_camera_params=True, do_metric_depth=True, moge_model=moge,
                             hip_graph=graph, output_dir=str(tmp_path / mode), bundle_adjust=False, num_loader_workers=4)
        res = slam.process_chunks(files)
        torch.cuda.synchronize()
        runs[mode] = (slam, res)
    (s_g, r_g), (s_e, r_e) = runs["hip_graph"], runs["eager"]
    assert len(r_g) == len(r_e) == 13
    for s in (s_g, s_e):
        assert s.get_statistics()["num_frames"] == n_frames          # every new frame once: 100 + 11 x 80 + 0 (tail = overlap only)
        assert s.get_reconstruction_count() == 13
    for k, (a, b) in enumerate(zip(r_g, r_e)):
        ca, cb = a["chunk"], b["chunk"]
        # in-order drain: chunk k shows frames [80 k, 80 k + 100)
        first = os.path.basename(ca["image_paths"][0] if isinstance(ca["image_paths"][0], str) else ca["image_paths"][0][0])
        assert first == f"frame_{80 * k:05d}.png", (k, first)
        assert ca["camera_poses"].shape[0] == (100 if k < 12 else 20)
        for key in ("keypoints", "colors", "conf", "masks", "local_points"):
            assert torch.equal(ca[key], cb[key]), (k, key)
        # points / poses sit in the global frame after the alignment: the chunk-frame originals and the similarity
        for key in ("points", "camera_poses"):
            assert torch.equal(ca["_chunk_frame"][key] if "_chunk_frame" in ca else ca[key],
                               cb["_chunk_frame"][key] if "_chunk_frame" in cb else cb[key]), (k, key)
            assert torch.equal(ca[key], cb[key]), (k, key, "global frame")
        assert np.array_equal(np.asarray(a["transformation"]), np.asarray(b["transformation"])), k
        assert ca["_metrics"].get("metric_scale") is not None and ca["_metrics"]["metric_scale"] == cb["_metrics"]["metric_scale"]
        assert torch.equal(ca["camera_params"]["fx"], cb["camera_params"]["fx"])
    assert all(i is not None for i in s_g.alignment_infos[1:])       # every alignment accepted
    # the consumer never waits for a running forward: after the two start-up chunks (first-use allocations, graph capture)
    # (bound: 10 ms; one sample may exceed it - a scheduling hiccup of the shared box, round 5 saw 0 of 198 above 2.6 ms -
    # but none may look like a wait for the running forward, which costs ~0.6 of its 0.38 s on EVERY chunk)
    al = sorted(s_g._timing["align_chunk"][2:])
    assert al[-2] < 0.010 and al[-1] < 0.050, al
    fwd = float(np.median(s_g._timing["pi3_forward"]))
    assert 0.2 < fwd < 1.0, fwd                                      # the premise: full-size forwards (~0.38 s)
