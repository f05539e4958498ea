"""A synthetic stand-in for the network on a REAL trajectory: evaluation tooling for the second BASELINE metric.

The reference's 7-Scenes number (README.md:73-85, scripts/eval_7scenes.sh:175: chess seq-01, chunk length 100, overlap
20, `evo_ape tum GT EST -as`) needs the released pi3 weights and the dataset's images; neither is on this filesystem.
What IS here is the ground-truth trajectory the reference ships (tests/golden/gt_7scenes_chess.txt, 1 000 cam->world
poses).  This module cuts that trajectory into the chunks the reference would cut (13 at 100 / 20) and produces, for
each chunk, what pi3 would emit if it were right up to a stated noise level: dense pointmaps of a fixed synthetic room
seen from the ground-truth cameras, each chunk in its own random similarity gauge.  Everything AFTER the network is
then the product: masks, LM intrinsics, grid keypoints, bilinear gather + fp16 pack, the chunk writer (stage 1) and the
overlap Sim(3) alignment, optional bundle adjustment and the TUM export (stage 2).  The APE of that trajectory against
the ground truth measures the part of the "within 1 mm of the reference" budget that this build owns - fp16 chunk
storage, fp32 Sim(3) solve, f64 prefix product over 13 chunks, fp32 export - not the network's accuracy.

Two routes to the same chunk-file layout:
  * `SceneEngine` + `write_chunks_product`: the scene takes the place of Pi3Engine inside the REAL OfflineChunkCreator
    (needs the GPU: every post-network step runs in csrc/post.hip);
  * `sparse_chunk` / `write_chunks_sparse`: numpy / torch-CPU only, the scene is ray-cast at the sub-pixel grid
    keypoints directly (no dense maps, no bilinear gather) - for the CPU suite (chunk-parallel == sequential
    composition on gloo).
Nothing here imports oracle/ or is part of the hot path."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

# Per-output deviation of the reference's own bf16-autocast forward from its fp32 forward at the headline size
# (tests/golden/pi3_full.npz, keys bf16err_*: local_points 0.28 % rms relative, camera_poses 0.49 %, rotation <= 1.64
# deg): the level at which two runs of the network on the same overlap frame (once per chunk) disagree.
NOISE_BF16 = dict(local_rel=0.0028, pose_trans_rel=0.0049, pose_rot_deg=0.3, frame_scale_rel=0.002)
NOISE_NONE = dict(local_rel=0.0, pose_trans_rel=0.0, pose_rot_deg=0.0, frame_scale_rel=0.0)


def load_tum_poses(path: str) -> np.ndarray:
    """`timestamp tx ty tz qx qy qz qw` rows -> (n, 4, 4) float64 cam->world."""
    from scipy.spatial.transform import Rotation
    a = np.loadtxt(path, comments="#").reshape(-1, 8)
    P = np.tile(np.eye(4), (len(a), 1, 1))
    P[:, :3, :3] = Rotation.from_quat(a[:, 4:8]).as_matrix()
    P[:, :3, 3] = a[:, 1:4]
    return P


def _rotvec_matrix(v: np.ndarray) -> np.ndarray:
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(v).as_matrix()


@dataclass
class SyntheticSequence:
    """The room, the cameras, the chunk list and the per-chunk gauges / noise draws (all seeded, host side)."""
    gt_path: str
    H: int = 308                    # 640x480 after calculate_target_size(..., 127 500)
    W: int = 406
    chunk_length: int = 100
    overlap: int = 20
    max_kp: int = 200
    seed: int = 20261006
    noise: Dict[str, float] = field(default_factory=lambda: dict(NOISE_BF16))
    n_frames: Optional[int] = None  # first n frames of the trajectory (None: all)
    margin_m: float = 1.2           # room walls this far outside the trajectory's bounding box: depths of 1-6 m

    def __post_init__(self):
        from pi3_slam_amd.image_io import chunk_indices
        P = load_tum_poses(self.gt_path)
        self.poses_gt = P[: self.n_frames] if self.n_frames else P
        self.n = len(self.poses_gt)
        self.chunks: List[Tuple[int, int]] = chunk_indices(self.n, self.chunk_length, self.overlap)
        # Kinect intrinsics of 7-Scenes (585 px at 640x480) at the network's frame size.  Principal point: the image
        # centre in the convention pi3 / MoGe pointmaps are trained in and the reference's focal estimator assumes
        # (utils/geometry_torch.py:39-51: pixel i sits at (2 i + 1 - W) / W of the half-width), i.e. pixel INDEX
        # (W - 1) / 2.  The chunk's intrinsics matrix says W // 2 (utils/camera_estimation.py:52-53) - the same point in
        # corner-based coordinates, half a pixel off in the index coordinates keypoints are stored in; that offset is the
        # reference's and stays in the data.  (A camera centred on index W // 2 instead makes the LM estimator trade
        # the half pixel for a shift of -0.046 and a focal 1 % low, and the bundle adjustment then drags the barely
        # triangulated tracks of a chunk's first views along their rays by metres: tools/dev_ape_ba_probe.py.)
        self.fx = self.fy = 585.0 * self.W / 640.0
        self.cx, self.cy = (self.W - 1) / 2.0, (self.H - 1) / 2.0
        c = self.poses_gt[:, :3, 3]
        self.lo, self.hi = c.min(0) - self.margin_m, c.max(0) + self.margin_m
        rng = np.random.default_rng(self.seed)
        # occluders: spheres between the trajectory and the walls (depth discontinuities -> depth_edge masks; sphere 0
        # is a low-confidence object -> conf masks)
        self.spheres = []
        for _ in range(8):
            ctr = self.lo + (self.hi - self.lo) * rng.random(3)
            r = 0.25 + 0.25 * rng.random()
            if np.linalg.norm(c - ctr, axis=1).min() > r + 0.6:      # no camera inside or right at a sphere
                self.spheres.append((ctr, r))
        self.median_depth = 0.5 * float(np.linalg.norm(self.hi - self.lo)) / np.sqrt(3.0)

    # ---------------------------------------------------------------- per-chunk draws
    def frame_name(self, i: int) -> str:
        return f"frame-{i:06d}.color.png"       # 7-Scenes file names: stage 2 de-duplicates views by name

    def chunk_draws(self, c: int) -> Dict[str, np.ndarray]:
        """Gauge (s, R, t: x_chunk = R^T (x_world - t) / s) and pose / scale noise of chunk c."""
        a, b = self.chunks[c]
        rng = np.random.default_rng([self.seed, 1000 + c])
        nz = self.noise
        N = b - a
        gauge_R = _rotvec_matrix(rng.standard_normal(3) * 1.2)
        gauge_s = float(np.exp(rng.uniform(np.log(0.7), np.log(1.4))))
        gauge_t = self.poses_gt[a, :3, 3] + 0.3 * rng.standard_normal(3)
        rot_noise = np.stack([_rotvec_matrix(v) for v in
                              rng.standard_normal((N, 3)) * np.deg2rad(nz["pose_rot_deg"])])
        trans_noise = rng.standard_normal((N, 3)) * nz["pose_trans_rel"] * self.median_depth
        frame_scale = 1.0 + nz["frame_scale_rel"] * rng.standard_normal(N)
        return dict(gauge_R=gauge_R, gauge_s=gauge_s, gauge_t=gauge_t, rot_noise=rot_noise, trans_noise=trans_noise,
                    frame_scale=frame_scale)

    def gauge_matrix(self, c: int) -> np.ndarray:
        """4x4 similarity chunk frame -> world (what a perfect alignment recovers up to chunk 0's gauge)."""
        d = self.chunk_draws(c)
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = d["gauge_s"] * d["gauge_R"], d["gauge_t"]
        return M

    # ---------------------------------------------------------------- geometry (torch, any device, float64)
    def _cast(self, o: torch.Tensor, d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Rays o (N,1,3) + t d (N,P,3), cameras inside the room -> (t of the first surface (N,P), hit sphere 0 (N,P))."""
        dev = d.device
        lo = torch.as_tensor(self.lo, dtype=torch.float64, device=dev)
        hi = torch.as_tensor(self.hi, dtype=torch.float64, device=dev)
        wall = torch.where(d > 0, hi - o, lo - o) / torch.where(d.abs() < 1e-12, torch.full_like(d, 1e-12), d)
        t = wall.min(dim=-1).values
        low_conf = torch.zeros_like(t, dtype=torch.bool)
        a = (d * d).sum(-1)
        for i, (ctr, r) in enumerate(self.spheres):
            oc = o - torch.as_tensor(ctr, dtype=torch.float64, device=dev)
            b = 2.0 * (d * oc).sum(-1)
            c0 = (oc * oc).sum(-1) - r * r
            disc = b * b - 4.0 * a * c0
            ts = (-b - torch.sqrt(disc.clamp_min(0.0))) / (2.0 * a)
            hit = (disc > 0) & (ts > 0.1) & (ts < t)
            t = torch.where(hit, ts, t)
            low_conf = torch.where(hit, torch.full_like(low_conf, i == 0), low_conf)
        return t, low_conf

    def maps(self, c: int, uv: torch.Tensor, device, frames: Optional[np.ndarray] = None) -> Dict[str, torch.Tensor]:
        """What the network would emit for chunk c at pixel positions uv ((P,2) shared by all frames or (N,P,2)):
        points / local_points (N,P,3), conf (N,P,1) logits, camera_poses (N,4,4), float32 on `device`, in the chunk's
        gauge.  points = camera_poses . local_points, as Pi3.forward forms them (pi3/models/pi3.py:205-207)."""
        a, b = self.chunks[c]
        ids = np.arange(a, b) if frames is None else np.asarray(frames)
        dr = self.chunk_draws(c)
        f64 = dict(dtype=torch.float64, device=device)
        Pw = torch.as_tensor(self.poses_gt[ids], **f64)
        R, o = Pw[:, :3, :3], Pw[:, :3, 3]
        uv = uv.to(**f64)
        if uv.ndim == 2:
            uv = uv[None].expand(len(ids), -1, -1)
        d_cam = torch.stack([(uv[..., 0] - self.cx) / self.fx, (uv[..., 1] - self.cy) / self.fy,
                             torch.ones_like(uv[..., 0])], dim=-1)                       # (N,P,3), z = 1
        d_w = torch.einsum("nij,npj->npi", R, d_cam)
        t, low_conf = self._cast(o[:, None, :], d_w)
        # the network's output: depth noise along the ray, a per-frame scale error, a noisy pose
        gen = torch.Generator(device=device).manual_seed(int(self.seed) * 1000003 + 7919 * c + 17)
        nz = self.noise
        z = t * torch.as_tensor(dr["frame_scale"][ids - a], **f64)[:, None]
        if nz["local_rel"] > 0:
            z = z * (1.0 + nz["local_rel"] * torch.randn(z.shape, generator=gen, **f64))
        local = z[..., None] * d_cam
        Rn = R @ torch.as_tensor(dr["rot_noise"][ids - a], **f64)
        on = o + torch.as_tensor(dr["trans_noise"][ids - a], **f64)
        # chunk gauge: x_chunk = Rg^T (x_world - tg) / sg
        Rg = torch.as_tensor(dr["gauge_R"], **f64)
        tg = torch.as_tensor(dr["gauge_t"], **f64)
        sg = dr["gauge_s"]
        local_c = local / sg
        Rc = Rg.T @ Rn
        oc = (on - tg) @ Rg / sg
        pose = torch.zeros(len(ids), 4, 4, **f64)
        pose[:, :3, :3], pose[:, :3, 3], pose[:, 3, 3] = Rc, oc, 1.0
        pose32 = pose.to(torch.float32)
        local32 = local_c.to(torch.float32)
        points32 = torch.einsum("nij,npj->npi", pose32[:, :3, :3], local32) + pose32[:, None, :3, 3]
        conf = 3.0 + 0.5 * torch.randn(z.shape, generator=gen, **f64) - 6.0 * low_conf.to(torch.float64)
        return dict(points=points32, local_points=local32, conf=conf.to(torch.float32)[..., None], camera_poses=pose32)

    def reference_cloud(self, frame_step: int = 1, pixel_stride: int = 1, device="cpu") -> torch.Tensor:
        """The room as the ground-truth cameras see it: the world-frame, noise-free hit point of every pixel_stride-th
        pixel (rows and columns) of every frame_step-th frame, ray-cast in f64, returned as f32 (P,3) on `device`.
        Hits on sphere 0 are left out: it is the low-confidence object, which a map's confidence filter removes on
        purpose.  The ground truth for scoring a dense map of this sequence (pi3_slam_amd/map_eval.py)."""
        f64 = dict(dtype=torch.float64, device=device)
        v, u = torch.meshgrid(torch.arange(0, self.H, int(pixel_stride), **f64),
                              torch.arange(0, self.W, int(pixel_stride), **f64), indexing="ij")
        d_cam = torch.stack([(u.reshape(-1) - self.cx) / self.fx, (v.reshape(-1) - self.cy) / self.fy,
                             torch.ones(u.numel(), **f64)], dim=-1)                      # (P,3), z = 1
        ids = np.arange(0, self.n, int(frame_step))
        out = []
        for a in range(0, len(ids), 16):
            Pw = torch.as_tensor(self.poses_gt[ids[a:a + 16]], **f64)
            R, o = Pw[:, :3, :3], Pw[:, :3, 3]
            d_w = torch.einsum("nij,pj->npi", R, d_cam)
            t, low_conf = self._cast(o[:, None, :], d_w)
            X = o[:, None, :] + t[..., None] * d_w
            out.append(X[~low_conf].to(torch.float32))
        return torch.cat(out, 0) if out else torch.zeros(0, 3, dtype=torch.float32, device=device)

    def intrinsics(self, n: int) -> torch.Tensor:
        """What a chunk file says about this camera: the true focal, the principal point as the reference writes it
        (utils/camera_estimation.py:52-53: W // 2, H // 2)."""
        K = torch.zeros(n, 3, 3, dtype=torch.float32)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = self.fx, self.fy, self.W // 2, self.H // 2, 1.0
        return K

    # ---------------------------------------------------------------- frames for the product's creator
    def frames(self, c: int, device) -> torch.Tensor:
        """(1, N, 3, H, W) fp32 in [0, 1]: a texture for the keypoint colours; pixel (0, 0) of channel 0 carries the
        frame number / 1024 (exact in fp32) so that SceneEngine knows which cameras a batch shows."""
        a, b = self.chunks[c]
        ids = torch.arange(a, b, device=device)
        y = torch.arange(self.H, device=device)[None, None, :, None]
        x = torch.arange(self.W, device=device)[None, None, None, :]
        ch = torch.arange(3, device=device)[None, :, None, None]
        tex = ((x * 7 + y * 13 + ch * 61 + ids[:, None, None, None] * 3) % 251).to(torch.float32) / 255.0
        tex[:, 0, 0, 0] = ids.to(torch.float32) / 1024.0
        return tex[None].contiguous()


class SceneEngine:
    """The scene behind Pi3Engine's call surface: engine(imgs) -> {points, local_points, conf, camera_poses} with the
    shapes and dtypes of Pi3.forward (pi3/models/pi3.py:173-216).  Goes where the model goes:
    OfflineChunkCreator(config, model=SceneEngine(seq))."""

    def __init__(self, seq: SyntheticSequence):
        self.seq = seq
        self.calls = 0

    def flops(self, B, N, H, W):
        return {"total": 0.0}

    def __call__(self, imgs: torch.Tensor, **_) -> Dict[str, torch.Tensor]:
        s = self.seq
        if imgs.ndim != 5 or tuple(imgs.shape[-2:]) != (s.H, s.W):
            raise ValueError(f"SceneEngine serves (1, N, 3, {s.H}, {s.W}) frames, got {tuple(imgs.shape)}")
        ids = (imgs[0, :, 0, 0, 0].to(torch.float64) * 1024.0).round().long().cpu().numpy()
        cl, ov = s.chunk_length, s.overlap
        c = int(ids[0]) // (cl - ov)
        a, b = s.chunks[c]
        if not np.array_equal(ids, np.arange(a, b)):
            raise ValueError(f"frames {ids[0]}..{ids[-1]} are not chunk {c} = [{a}, {b})")
        dev = imgs.device
        v, u = torch.meshgrid(torch.arange(s.H, device=dev), torch.arange(s.W, device=dev), indexing="ij")
        uv = torch.stack([u.reshape(-1), v.reshape(-1)], dim=-1)
        m = s.maps(c, uv, dev)
        N = b - a
        self.calls += 1
        return dict(points=m["points"].reshape(1, N, s.H, s.W, 3), local_points=m["local_points"].reshape(1, N, s.H, s.W, 3),
                    conf=m["conf"].reshape(1, N, s.H, s.W, 1), camera_poses=m["camera_poses"][None])


def write_chunks_product(seq: SyntheticSequence, out_dir: str, device: str = "cuda",
                         estimate_camera_params: bool = True) -> Dict:
    """Stage 1 with the scene in the network's place: the product's OfflineChunkCreator (masks, LM intrinsics, grid
    keypoints, gather + fp16 pack, writer thread, manifest + metadata) -> out_dir/chunks/chunk_%06d.pt."""
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=device, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=estimate_camera_params, num_loader_workers=0)
    cr = OfflineChunkCreator(cfg, model=SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)

    def items():
        for c, (a, b) in enumerate(seq.chunks):
            yield {"frames": seq.frames(c, cr.device), "kind": "float", "paths": [seq.frame_name(i) for i in range(a, b)],
                   "meta": {"chunk_index": c, "start_idx": a, "end_idx": b}}

    saved, manifest, _ = cr.write_chunks(cr.process_chunks(items()))
    cr.write_run_metadata(manifest)
    return {"files": saved, "manifest": manifest}


def sparse_chunk(seq: SyntheticSequence, c: int, extractor=None) -> Dict:
    """Chunk c in the chunk-file layout without the GPU: the scene ray-cast at the grid keypoints themselves."""
    from pi3_slam_amd.keypoints import GridKeypointExtractor
    a, b = seq.chunks[c]
    N = b - a
    ex = extractor or GridKeypointExtractor(max_num_keypoints=seq.max_kp, device="cpu", seed=0)
    ex.reseed(c)
    kp = ex.extract(torch.zeros(N, 3, seq.H, seq.W))["keypoints"]                      # (N, K, 2) f32
    m = seq.maps(c, kp, "cpu")
    K3 = seq.intrinsics(N)
    K = kp.shape[1]
    ones = torch.ones(1, N)
    return dict(points=m["points"].to(torch.float16), local_points=m["local_points"].to(torch.float16),
                conf=m["conf"].to(torch.float16), masks=torch.sigmoid(m["conf"]) > 0.1, keypoints=kp.to(torch.float16),
                colors=torch.zeros(N, K, 3, dtype=torch.float16), descriptors=torch.zeros(N, K, 128, dtype=torch.float16),
                scores=torch.ones(N, K, dtype=torch.float16), camera_poses=m["camera_poses"], intrinsics=K3,
                camera_params=dict(intrinsics=K3, fx=ones * seq.fx, fy=ones * seq.fy, cx=ones * (seq.W // 2), cy=ones * (seq.H // 2),
                                   focal=ones, shift=ones * 0.0),
                original_width=seq.W, original_height=seq.H, image_paths=[seq.frame_name(i) for i in range(a, b)],
                chunk_index=c, start_idx=a, end_idx=b)


def write_chunks_sparse(seq: SyntheticSequence, out_dir: str) -> List[str]:
    os.makedirs(os.path.join(out_dir, "chunks"), exist_ok=True)
    files = []
    for c in range(len(seq.chunks)):
        files.append(os.path.join(out_dir, "chunks", f"chunk_{c:06d}.pt"))
        torch.save(sparse_chunk(seq, c), files[-1])
    with open(os.path.join(out_dir, "chunk_metadata.json"), "w") as f:
        json.dump({"chunk_length": seq.chunk_length, "overlap": seq.overlap, "target_size": [seq.H, seq.W]}, f)
    return files
