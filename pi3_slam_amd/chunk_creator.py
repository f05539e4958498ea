"""OfflineChunkCreator: drop-in for slam/offline_chunk_creator.py — same config dataclass, same public and
underscore methods, same chunk_*.pt / chunks_manifest.json / chunk_metadata.json layout — with every arithmetic step
on the MI355X and the host kept off the critical path.

One chunk is three stages, and consecutive chunks overlap them (the reference overlaps only the loader,
offline_chunk_creator.py:279-287):

    stage-in   (copy stream)     pinned frames --H2D--> [device resize / undistortion] -> imgs (1,N,3,H,W) fp32
    launch     (compute stream)  Pi3Engine.forward -> masks -> metric scale (MoGe runs beside the forward on its own
                                 stream: it needs only frame 0) -> intrinsics (LM per frame) -> grid keypoints gather +
                                 fp16 pack -> ONE packed D2H into a pinned buffer
    finish     (host)            wait for the chunk's event, cut the pinned buffer into the result dict, hand it to the
                                 writer thread (torch.save)

While the GPU runs chunk k the host finishes chunk k-1 and the copy stream brings in chunk k+1.  The reference copies
the four dense maps (350 MB at N=100) to the host and samples them there (offline_chunk_creator.py:204-213, 228); here
only ~1 MB of per-keypoint values crosses PCIe.  Failure policy as in the reference: a model / keypoint / intrinsics /
save problem is reported and the run continues without that feature (offline_chunk_creator.py:77-79, 92-94, 199-201,
242-243, 330-331).
"""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, Iterable, Iterator, List, Optional, Tuple

import torch
from torch.utils.data import DataLoader

from . import ops
from .dense_map import ChunkCloudBuilder
from .engine import Pi3Engine
from .image_io import ChunkImageDataset, ThreadedChunkLoader, calculate_target_size, ingest_frames_device
from .hostmem import clone_host, full_host, zeros_host
from .keypoints import create_keypoint_extractor
from .undistortion import create_undistortion_maps
from .weights import Pi3Config


@dataclass
class OfflineCreatorConfig:
    """Fields and defaults of slam/offline_chunk_creator.py:36-50, then the knobs the reference hard-codes."""
    model_path: str
    output_dir: str
    chunk_length: int = 100
    overlap: int = 10
    device: str = "cuda"
    do_metric_depth: bool = True
    keypoint_type: str = "aliked"  # 'aliked' | 'grid' | 'none'
    max_num_keypoints: int = 512
    keypoint_detection_threshold: float = 0.005
    estimate_camera_params: bool = True
    num_loader_workers: int = 2
    pin_memory: bool = True
    cam_dist_path: Optional[str] = None
    # --- additions (the reference hard-codes "Ruicheng/moge-2-vits-normal" and an unseeded device randperm)
    moge_model_path: Optional[str] = None   # local MoGe-2 model.pt, or "recipe" for synthetic weights
    keypoint_seed: Optional[int] = 0
    device_resize: bool = False             # loader workers only decode; Resize + ToTensor run on the GPU (bit-identical)
    hip_graph: bool = False                 # replay the per-chunk pi3 forward as one captured hipGraph per chunk shape
    overlap_stages: bool = True             # False: stage-in, launch and finish of a chunk run back to back (A/B knob)
    reuse_overlap_encoder: bool = False     # a chunk whose first `overlap` paths are the previous chunk's last ones takes
                                            # their (frame-local) encoder output from that chunk: bit-identical results
    dense_voxel_size: Optional[float] = None  # set: every chunk also carries 'dense_cloud', its masked dense pointmap fused
                                              # into voxels of this edge length (dense_map.py; chunk frame)
    dense_conf_threshold: float = 0.5         # a pixel enters the dense cloud when sigmoid(conf) > this (and its mask)
    dense_min_views: Optional[int] = None     # set (with dense_voxel_size): a pixel must also agree in depth with this many
                                              # neighbouring frames of its chunk (dense_map.ConsistencyFilter)
    dense_view_radius: int = 3                # neighbours i +- s * dense_view_stride, s = 1..dense_view_radius
    dense_view_stride: int = 2
    dense_depth_tolerance: float = 0.03       # relative depth difference that still counts as the same surface
    dense_normals: bool = False               # with dense_voxel_size: the cloud also carries 'normals' / 'normal_weights',
                                              # a camera-facing surface normal per voxel (dense_map.NormalAccumulator)
    dense_depth_every: Optional[int] = None   # set (with dense_voxel_size): the chunk also carries 'dense_depth', the fp16
                                              # local z of every K-th frame's dense-map pixels, for stage 2's carving
                                              # (dense_map.MapCarver); needs the intrinsics estimate
    dense_depth_stride: int = 2               # those planes keep every S-th row and column (1, 2 or 4)


_UV_CACHE: Dict = {}


def _uv_tables(H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """normalized_view_plane_uv (utils/geometry_torch.py:39-51) as two 1-D fp32 tables (constants per image size, built
    once: a pageable H2D copy per chunk would stall the host behind the whole forward pass)."""
    key = (H, W, str(device))
    if key not in _UV_CACHE:
        _UV_CACHE[key] = _uv_tables_build(H, W, device)
    return _UV_CACHE[key]


def _uv_tables_build(H: int, W: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    ar = W / H
    sx = ar / (1 + ar ** 2) ** 0.5
    sy = 1 / (1 + ar ** 2) ** 0.5
    u = torch.linspace(-sx * (W - 1) / W, sx * (W - 1) / W, W, dtype=torch.float32)
    v = torch.linspace(-sy * (H - 1) / H, sy * (H - 1) / H, H, dtype=torch.float32)
    return u.to(device), v.to(device)


_Layout = List[Tuple[str, torch.dtype, tuple, int, int]]       # (key, dtype, shape, offset, nbytes) per packed tensor


def pack_results(out: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, _Layout]:
    """Every tensor of `out` as bytes in ONE uint8 buffer on their device, each at a 16-byte aligned offset ->
    (packed, layout in `out`'s order): one copy brings all of them to the host."""
    layout, parts, off = [], [], 0
    for k, t in out.items():
        b = t.contiguous().view(torch.uint8).reshape(-1)
        pad = (-b.numel()) % 16
        layout.append((k, t.dtype, tuple(t.shape), off, b.numel()))
        parts.append(b)
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8, device=b.device))
        off += b.numel() + pad
    return torch.cat(parts), layout


def unpack_results(host_bytes: torch.Tensor, layout: _Layout) -> Dict[str, torch.Tensor]:
    """The tensors of pack_results from a host copy of its buffer, each in storage of its own (memcpy, no ATen operator:
    hostmem.py)."""
    return {k: clone_host(host_bytes[off:off + nbytes]).view(dt).reshape(shape) for k, dt, shape, off, nbytes in layout}


@dataclass
class _Staged:
    """A chunk whose frames are on the device, or on their way there on the copy stream."""
    imgs: torch.Tensor                       # (1, N, 3, H, W) fp32
    ready: Optional[torch.cuda.Event]        # recorded on the copy stream after the last stage-in kernel; None = usable now
    paths: List
    meta: Dict = field(default_factory=dict)
    keep: tuple = ()                         # host tensors the asynchronous upload still reads


@dataclass
class _InFlight:
    """A chunk whose kernels are queued; `done` fires when `packed` (one device byte buffer with every small result
    tensor) is complete.  The copy to the host is issued by finish(), after that event: a D2H command queued behind the
    forward would sit at the head of the copy engine's queue for the whole forward and hold up every other device->host
    copy of the process (the alignment of the previous chunk waited 420 ms for its 33 doubles that way)."""
    packed: Optional[torch.Tensor]
    layout: _Layout
    done: torch.cuda.Event
    timing: Dict[str, torch.cuda.Event]
    host: Dict                               # values that never left the host (paths, zero descriptors, ...)
    dense: Optional[Dict[str, torch.Tensor]]  # device tensors of the no-keypoint fallback (copied in finish)
    meta: Dict
    t_launch: float = 0.0
    dense_job: Optional[object] = None       # the dense voxel cloud's host job (dense_map.ChunkCloudBuilder.queue)


class OfflineChunkCreator:
    """Per-chunk pi3 results (metric-scaled by MoGe, sampled at grid keypoints) written as chunk files."""

    def __init__(self, config: OfflineCreatorConfig, model: Optional[Pi3Engine] = None, moge_model=None):
        self.config = config
        self.chunks_dir = os.path.join(config.output_dir, "chunks")
        os.makedirs(self.chunks_dir, exist_ok=True)
        from .dist import ensure_process_group, resolve_device
        self.rank, self.world = ensure_process_group()          # (0, 1) unless launched under torch.distributed.run
        dev = resolve_device(config.device)
        if not dev.startswith("cuda"):
            raise RuntimeError("this build runs the hot path on an MI355X only; there is no CPU path (device='cuda')")
        self.device = torch.device(dev)
        torch.cuda.set_device(self.device)

        # pi3 weights: a local checkpoint directory / file (offline_chunk_creator.py:65) or "recipe" (synthetic)
        if model is not None:
            self.model = model
        elif config.model_path == "recipe":
            self.model = Pi3Engine(Pi3Config(), dev)
        else:
            self.model = Pi3Engine.from_pretrained(config.model_path, dev)

        self._tail_paths: Optional[List[str]] = None    # reuse_overlap_encoder: the files whose encoder output the engine holds
        self.reused_frames = 0

        # MoGe is optional equipment: without it chunks keep pi3's own scale (offline_chunk_creator.py:70-79)
        self.moge_model = moge_model
        if self.moge_model is None and config.do_metric_depth:
            self.moge_model = self._optional("MoGe metric depth", self._load_moge)
        self.keypoint_extractor = None
        if config.keypoint_type and config.keypoint_type.lower() != "none":
            self.keypoint_extractor = self._optional("keypoint extractor", lambda: create_keypoint_extractor(
                keypoint_type=config.keypoint_type, max_num_keypoints=config.max_num_keypoints,
                detection_threshold=config.keypoint_detection_threshold, device=dev, seed=config.keypoint_seed))
            if self.keypoint_extractor is not None:
                print(f"   Keypoint extractor: {config.keypoint_type}")
        # frame undistortion (offline_chunk_creator.py:98-112): maps are built and applied on the device
        self.undistortion_maps = None
        if config.cam_dist_path:
            if os.path.exists(config.cam_dist_path):
                self.undistortion_maps = self._optional(f"undistortion maps ({config.cam_dist_path})",
                                                        lambda: create_undistortion_maps(config.cam_dist_path, dev))
            else:
                print(f"⚠️  calibration file {config.cam_dist_path} does not exist: frames are used as they are")

        self.target_size: Optional[Tuple[int, int]] = None
        self._copy_stream = torch.cuda.Stream(self.device)
        self._moge_stream = torch.cuda.Stream(self.device)
        self._d2h_stream = torch.cuda.Stream(self.device)
        self._pinned_pool: Dict[int, List[torch.Tensor]] = {}
        self._last_forward_end: Optional[torch.cuda.Event] = None
        self.host_seconds: Dict[str, float] = {}     # of the last process_chunks: the pipeline thread's time per stage
        self.last_run: Dict = {}                     # of the last process_and_save
        # dense voxel map (opt-in): one device table, cleared and refilled per chunk on the compute stream
        self._dense = ChunkCloudBuilder.from_config(config, self.device)

    @staticmethod
    def _optional(what: str, make):
        """Build an optional component; report and carry on without it when that fails."""
        try:
            obj = make()
            if obj is None:
                print(f"⚠️  {what}: not available, continuing without it")
            return obj
        except Exception as e:  # noqa: BLE001
            print(f"⚠️  {what}: {e}; continuing without it")
            return None

    def _load_moge(self):
        from .moge import MoGeEngine
        if not self.config.moge_model_path:
            raise FileNotFoundError("no local MoGe-2 checkpoint configured (moge_model_path)")
        eng = MoGeEngine.from_pretrained(self.config.moge_model_path, str(self.device))
        print("   MoGe loaded for metric scaling")
        return eng

    # ------------------------------------------------------------------ device steps (the reference's method names)
    @staticmethod
    def _compute_masks(pi3_result: Dict[str, torch.Tensor]) -> torch.Tensor:
        """(B, N, H, W) bool — offline_chunk_creator.py:114-119."""
        conf, lp = pi3_result["conf"], pi3_result["local_points"]
        B, N, H, W = lp.shape[:4]
        m = ops.compute_masks(conf.reshape(B * N, H, W, 1).contiguous(), lp.reshape(B * N, H, W, 3).contiguous())
        return m.view(B, N, H, W).bool()

    @staticmethod
    def _ratio_median(moge_metric_depth: torch.Tensor, pi3_metric_depth: torch.Tensor,
                      mask: torch.Tensor) -> torch.Tensor:
        """Device tensor [median(moge/pi3 over the mask), number of masked pixels]."""
        assert pi3_metric_depth.stride(-1) in (1, 3)
        return ops.masked_ratio_median(moge_metric_depth.contiguous(), pi3_metric_depth, pi3_metric_depth.stride(-1),
                                       mask.contiguous(), moge_metric_depth.numel())

    @classmethod
    def _get_scale_factor_for_pi3(cls, moge_metric_depth: torch.Tensor, pi3_metric_depth: torch.Tensor,
                                  mask: torch.Tensor) -> torch.Tensor:
        """0-dim device tensor — offline_chunk_creator.py:121-127.  pi3_metric_depth may be a strided view of
        local_points[..., 2]."""
        return cls._ratio_median(moge_metric_depth, pi3_metric_depth, mask)[0]

    @staticmethod
    def _interpolate_world_points_for_keypoints(result_dense: Dict, keypoints: torch.Tensor) -> Dict[str, torch.Tensor]:
        """offline_chunk_creator.py:129-159 (+ the fp16 pack of :231-241), on the device."""
        dev = result_dense["points"].device
        images = result_dense.get("images")
        if not keypoints.is_cuda:     # through pinned memory: an asynchronous upload, the host does not wait for the GPU
            kp_host = keypoints.to(torch.float32).contiguous()
            keypoints = (kp_host.pin_memory() if torch.cuda.is_available() else kp_host).to(dev, non_blocking=True)
        return ops.gather_keypoints(result_dense["points"].contiguous(), result_dense["local_points"].contiguous(),
                                    result_dense["conf"].contiguous(), result_dense["masks"].contiguous(),
                                    images.contiguous() if images is not None else None,
                                    keypoints.to(dev, torch.float32).contiguous())

    def _estimate_camera_parameters(self, pi3_result: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """estimate_camera_parameters_single_chunk (utils/camera_estimation.py:101-132) on the device."""
        lp = pi3_result["local_points"][0].contiguous()
        conf = pi3_result["conf"][0].contiguous()
        H, W = lp.shape[1:3]
        uvx, uvy = _uv_tables(H, W, lp.device)
        r = ops.focal_shift(lp, conf, uvx, uvy)
        fxy = r["fxfycxcy"]
        return dict(intrinsics=r["intrinsics"], focal=r["focal"][None], shift=r["shift"][None], fx=fxy[:, 0][None],
                    fy=fxy[:, 1][None], cx=fxy[:, 2][None], cy=fxy[:, 3][None])

    def _queue_camera_parameters(self, pi3_result: Dict[str, torch.Tensor], out: Dict[str, torch.Tensor]) -> None:
        """Queue the intrinsics estimate into out['cam.*']; a failure is reported and the chunk goes on without."""
        try:
            for k, v in self._estimate_camera_parameters(pi3_result).items():
                out["cam." + k] = v
        except Exception as e:  # noqa: BLE001
            print(f"⚠️  Camera parameter estimation failed: {e}")

    # ------------------------------------------------------------------ stage-in
    def _stage_in(self, frames, paths: List, meta: Optional[Dict] = None, kind: str = "float") -> _Staged:
        """Queue the upload (and the device resize / undistortion when frames are decoded uint8) on the copy stream.
        kind: 'float' (1,N,3,H,W) fp32 in [0,1], CPU or device; 'u8' (N,H0,W0,3) uint8 -> device resize to
        target_size; 'u8_undist' -> remap through the undistortion maps."""
        meta = dict(meta or {})
        if frames.is_cuda and kind == "float":
            return _Staged(frames.to(self.device, torch.float32), None, paths, meta)
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._copy_stream):
            t_in = torch.cuda.Event(enable_timing=True)
            t_in.record(self._copy_stream)
            dev_in = frames.to(self.device, non_blocking=True)
            if kind == "u8":
                imgs = ingest_frames_device(dev_in, self.target_size)[None]
            elif kind == "u8_undist":
                imgs = self.undistortion_maps.undistort_frames_device(dev_in, self.target_size)[None]
            else:
                imgs = dev_in.to(torch.float32)
            ready = torch.cuda.Event(enable_timing=True)
            ready.record(self._copy_stream)
            meta["_stage_in"] = (t_in, ready)
        for t in (dev_in, imgs):
            t.record_stream(cur)          # allocated on the copy stream, consumed on the compute stream
            t.record_stream(self._moge_stream)
        return _Staged(imgs, ready, paths, meta, keep=(frames,))

    # ------------------------------------------------------------------ launch
    def _launch(self, st: _Staged, chunk_images_for_kp: Optional[torch.Tensor] = None) -> _InFlight:
        """Queue every kernel of one chunk and pack its small results; returns without waiting for the GPU."""
        cur = torch.cuda.current_stream(self.device)
        if st.ready is not None:
            cur.wait_event(st.ready)
        imgs = st.imgs
        assert imgs.ndim == 5, "Expected (B=1, N, C, H, W) tensor for chunk images"
        N = int(imgs.shape[1])
        ev = {k: torch.cuda.Event(enable_timing=True) for k in ("f0", "f1", "post")}

        moge_depth = self._queue_moge(st, cur)
        kp, kp_dev, kp_err = self._queue_keypoints(chunk_images_for_kp if chunk_images_for_kp is not None else imgs, cur)
        reuse = self._overlap_reuse(st.paths, N)
        ev["f0"].record(cur)
        pi3 = self._queue_forward(imgs, reuse)
        ev["f1"].record(cur)

        out: Dict[str, torch.Tensor] = {}       # the small device tensors of the packed copy
        masks = self._compute_masks(pi3)[0]
        if moge_depth is not None:
            self._queue_metric_scale(pi3, masks, moge_depth, cur, out)
        if self.config.estimate_camera_params:
            self._queue_camera_parameters(pi3, out)
        dense_job = self._queue_dense_cloud(pi3, masks, imgs, out) if self._dense is not None else None
        out["camera_poses"] = pi3["camera_poses"][0]
        host = self._queue_gather(pi3, masks, imgs, kp, kp_dev, kp_err, out) if self.keypoint_extractor is not None else {}
        dense = None if "points" in out else self._dense_fallback(pi3, masks)
        ev["post"].record(cur)

        packed, layout = pack_results(out)
        done = torch.cuda.Event()
        done.record(cur)
        return _InFlight(packed, layout, done, ev, host, dense, dict(st.meta, paths=st.paths, num_frames=N),
                         t_launch=time.time(), dense_job=dense_job)

    def _queue_moge(self, st: _Staged, cur: torch.cuda.Stream) -> Optional[torch.Tensor]:
        """MoGe needs only the first frame: it runs beside the pi3 forward instead of after it (400 small
        single-image kernels that would otherwise run on an idle GPU).  -> its depth map, or None without MoGe."""
        if self.moge_model is None:
            return None
        if st.ready is not None:
            self._moge_stream.wait_event(st.ready)
        else:
            self._moge_stream.wait_stream(cur)
        with torch.cuda.stream(self._moge_stream):
            graphed = (self.config.hip_graph and hasattr(self.moge_model, "infer_graphed")
                       and os.environ.get("PI3_MOGE_GRAPH", "1") != "0")
            if graphed:
                # the graph's output is ONE static buffer, and chunk k+1's replay is queued on this stream while
                # chunk k's forward still runs on the compute stream (this stream waits for the stage-in only):
                # without a private copy, chunk k's scale would be taken from chunk k+1's first frame.
                # record_stream does not protect graph-pool memory, a copy does.
                moge_depth = self.moge_model.infer_graphed(st.imgs[0, 0])["depth"].clone()
            else:
                moge_depth = self.moge_model.infer(st.imgs[0, 0])["depth"]
        moge_depth.record_stream(cur)
        return moge_depth

    def _queue_keypoints(self, images: torch.Tensor, cur: torch.cuda.Stream):
        """Keypoints depend on the frame size only: extracted now and uploaded on the copy stream (idle at this point).
        Queued on the compute stream the upload would wait behind the forward at the head of the H2D engine's queue
        and hold up every other upload of the process, e.g. the previous chunk's alignment beside this forward.
        -> (the extractor's dict, device keypoints, the exception that _queue_gather reports instead of gathering)."""
        if self.keypoint_extractor is None:
            return None, None, None
        try:
            kp = self.keypoint_extractor.extract(images)
            kp_dev = kp["keypoints"]
            if not kp_dev.is_cuda:
                kp_host = kp_dev.to(torch.float32).contiguous().pin_memory()
                with torch.cuda.stream(self._copy_stream):
                    kp_dev = kp_host.to(self.device, non_blocking=True)
                    kp_ready = torch.cuda.Event()
                    kp_ready.record(self._copy_stream)
                cur.wait_event(kp_ready)
                kp_dev.record_stream(cur)
            return kp, kp_dev, None
        except Exception as e:  # noqa: BLE001
            return None, None, e

    def _overlap_reuse(self, paths: Optional[List], N: int) -> Dict[str, int]:
        """Overlap reuse (opt-in): the SAME files at the head of this chunk as at the tail of the one launched before
        it.  -> the forward's keyword arguments, {} when nothing is reused or kept."""
        rh = kt = 0
        ov = int(self.config.overlap)
        if self.config.reuse_overlap_encoder and getattr(self.model, "supports_overlap_reuse", False) and 0 < ov < N \
                and paths is not None and len(paths) == N:
            names = [str(p) for p in paths]
            rh = ov if self._tail_paths == names[:ov] else 0
            kt, self._tail_paths = ov, names[-ov:]
        else:
            self._tail_paths = None
        self.reused_frames += rh
        return dict(reuse_head=rh, keep_tail=kt) if (rh or kt) else {}

    def _queue_forward(self, imgs: torch.Tensor, reuse: Dict[str, int]) -> Dict[str, torch.Tensor]:
        # the graph of a shape costs one eager run + one capture the first time: worth it for the nominal chunk shape, which
        # repeats, not for the ragged last chunk of a sequence (in a 4 000-frame stream its capture was 2.6 % of the run)
        if self.config.hip_graph and hasattr(self.model, "forward_graphed") \
                and int(imgs.shape[1]) == int(self.config.chunk_length):
            return self.model.forward_graphed(imgs, **reuse)     # static outputs: packed before the next replay
        return self.model(imgs, **reuse)

    def _queue_metric_scale(self, pi3: Dict[str, torch.Tensor], masks: torch.Tensor, moge_depth: torch.Tensor,
                            cur: torch.cuda.Stream, out: Dict[str, torch.Tensor]) -> None:
        """Rescale points, local points and poses in place by median(MoGe depth / pi3 depth) over frame 0's mask."""
        cur.wait_stream(self._moge_stream)
        med = self._ratio_median(moge_depth, pi3["local_points"][0, 0][..., 2], masks[0])
        ops.apply_scale(med[:1], pi3["local_points"], pi3["points"], pi3["camera_poses"])
        out["_scale"] = med                         # [median, masked pixel count]: checked on the host

    def _queue_dense_cloud(self, pi3: Dict[str, torch.Tensor], masks: torch.Tensor, imgs: torch.Tensor,
                           out: Dict[str, torch.Tensor]):
        """The metric points into the dense cloud, queued before the next graph replay can reuse the static outputs.
        Its consistency filter projects with the intrinsics that _queue_camera_parameters left in `out`; its depth
        keyframes are kept only when those exist."""
        fxy = None
        if (self._dense.filter is not None or self._dense.depth_every is not None) and "cam.fx" in out:
            fxy = torch.stack([out["cam." + k][0] for k in ("fx", "fy", "cx", "cy")], dim=1)
        return self._dense.queue(pi3["points"][0], pi3["local_points"][0], pi3["conf"][0], masks, imgs[0],
                                 pi3["camera_poses"][0], fxy, out)

    def _queue_gather(self, pi3: Dict[str, torch.Tensor], masks: torch.Tensor, imgs: torch.Tensor, kp: Optional[Dict],
                      kp_dev: Optional[torch.Tensor], kp_err: Optional[Exception], out: Dict[str, torch.Tensor]) -> Dict:
        """Sample the maps at the keypoints into `out`; -> the values that stay on the host (descriptors, scores).
        A failure, of the extraction before the forward or here, is reported and leaves `out` without keypoint results."""
        try:
            if kp_err is not None:
                raise kp_err
            g = self._interpolate_world_points_for_keypoints(
                dict(points=pi3["points"][0], local_points=pi3["local_points"][0], conf=pi3["conf"][0],
                     masks=masks, images=imgs[0]), kp_dev)
            for k in ("points", "local_points", "conf", "keypoints", "colors"):
                out[k] = g[k]
            out["masks"] = g["masks"].view(torch.uint8)
            if kp.get("constant"):     # all-zero descriptors, all-one scores (keypoint_extraction.py:150-151)
                # fresh calloc'ed zeros / a small filled array per chunk (callers own and may mutate their chunk)
                return {"descriptors": zeros_host(kp["descriptors"].shape, torch.float16),
                        "scores": full_host(kp["scores"].shape, 1.0, torch.float16)}
            return {"descriptors": kp["descriptors"].to(torch.float16), "scores": kp["scores"].to(torch.float16)}
        except Exception as e:  # noqa: BLE001
            print(f"⚠️  Keypoint extraction failed: {e}")
            for k in ("points", "local_points", "conf", "keypoints", "colors", "masks"):
                out.pop(k, None)
            return {}

    def _dense_fallback(self, pi3: Dict[str, torch.Tensor], masks: torch.Tensor) -> Dict[str, torch.Tensor]:
        """No keypoints: the dense maps are the result (offline_chunk_creator.py:204-209)."""
        dense = dict(points=pi3["points"][0], local_points=pi3["local_points"][0], conf=pi3["conf"][0], masks=masks)
        if self.config.hip_graph:     # static graph outputs: the next replay would overwrite them before finish() reads
            dense = {k: v.clone() for k, v in dense.items()}
        return dense

    # ------------------------------------------------------------------ finish
    def _finish(self, fl: _InFlight) -> Dict:
        """Wait for one chunk's results and build its chunk-file dictionary (host tensors)."""
        fl.done.synchronize()
        got = self._fetch_packed(fl)
        metrics = self._chunk_metrics(fl, got)
        result = self._chunk_result(fl, got, metrics)
        if fl.dense_job is not None:
            result["dense_cloud"] = self._dense.collect(fl.dense_job, got, metrics)
            depth = self._dense.collect_depth(fl.dense_job, got, metrics)
            if depth is not None:
                result["dense_depth"] = depth
            fl.dense_job = None
        return result

    def _pinned(self, nbytes: int) -> torch.Tensor:
        pool = self._pinned_pool.setdefault(nbytes, [])
        return pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

    def _fetch_packed(self, fl: _InFlight) -> Dict[str, torch.Tensor]:
        """The packed copy (see _InFlight for why it is issued here, after `done`) -> host tensors by key."""
        pinned = self._pinned(fl.packed.numel())
        with torch.cuda.stream(self._d2h_stream):      # nothing else is ever queued on this stream
            pinned.copy_(fl.packed, non_blocking=True)
        self._d2h_stream.synchronize()
        fl.packed = None
        got = unpack_results(pinned, fl.layout)
        self._pinned_pool.setdefault(pinned.numel(), []).append(pinned)
        return got

    def _chunk_metrics(self, fl: _InFlight, got: Dict[str, torch.Tensor]) -> Dict:
        """The chunk's '_metrics' from its timing events and the scale kernel's [median, count]."""
        N = fl.meta["num_frames"]
        infer_s = max(1e-6, fl.timing["f0"].elapsed_time(fl.timing["f1"]) / 1e3)
        post_s = fl.timing["f1"].elapsed_time(fl.timing["post"]) / 1e3
        fps = N / infer_s if N > 0 else 0.0
        print(f"   ⏱️ Inference: {infer_s:.3f}s for {N} frames  ->  {fps:.2f} FPS")
        metrics = {"infer_s": float(infer_s), "num_frames": int(N), "fps": float(fps), "post_s": float(post_s)}
        if self._last_forward_end is not None:      # device idle between consecutive forwards (pipelined runs)
            try:
                metrics["gap_before_forward_s"] = self._last_forward_end.elapsed_time(fl.timing["f0"]) / 1e3
            except RuntimeError:
                pass
        self._last_forward_end = fl.timing["f1"]
        if "_stage_in" in fl.meta:     # H2D + device resize / undistortion on the copy stream
            a, b = fl.meta.pop("_stage_in")
            metrics["stage_in_s"] = a.elapsed_time(b) / 1e3
        if "_scale" in got:
            med, cnt = float(got["_scale"][0]), int(got["_scale"][1])
            ok = cnt > 0 and med > 0.0 and med != float("inf") and med == med
            metrics["metric_scale"] = med if ok else None
            if not ok:   # the reference would raise on an empty mask (torch.median of nothing); say so, keep pi3's scale
                print(f"⚠️  metric scale not applied: median {med} over {cnt} masked pixels of frame 0")
        return metrics

    def _chunk_result(self, fl: _InFlight, got: Dict[str, torch.Tensor], metrics: Dict) -> Dict:
        result: Dict = {"camera_poses": got["camera_poses"], "image_paths": fl.meta["paths"], "_metrics": metrics}
        cam = {k[4:]: v for k, v in got.items() if k.startswith("cam.")}
        if cam:
            result["camera_params"] = cam
        if self.target_size is not None:
            result["original_width"] = self.target_size[1]
            result["original_height"] = self.target_size[0]
        if fl.dense is None:
            for k in ("points", "local_points", "conf", "keypoints", "colors"):
                result[k] = got[k]
            result["masks"] = got["masks"].bool()
            result["descriptors"] = fl.host["descriptors"]
            result["scores"] = fl.host["scores"]
        else:
            with torch.cuda.stream(self._d2h_stream):   # not behind the next chunk's forward on the compute stream
                for k, v in fl.dense.items():
                    result[k] = v.cpu()
        if cam:
            result["intrinsics"] = cam.get("intrinsics")
        return result

    # ------------------------------------------------------------------ one chunk, start to end (reference surface)
    def _process_single_chunk(self, chunk_images: torch.Tensor, chunk_paths: List[str]) -> Dict:
        """pi3, optional MoGe scaling, intrinsics, keypoints and the gather for one chunk
        (offline_chunk_creator.py:161-256).  chunk_images: (1, N, 3, H, W) fp32 in [0, 1], CPU or device."""
        assert chunk_images.ndim == 5, "Expected (B=1, N, C, H, W) tensor for chunk images"
        return self._finish(self._launch(self._stage_in(chunk_images, chunk_paths), chunk_images))

    # ------------------------------------------------------------------ a stream of chunks, stages overlapped
    def process_chunks(self, items: Iterable[Dict]) -> Iterator[Tuple[Dict, Dict]]:
        """items: dicts with 'frames' (+ 'kind', see _stage_in), 'paths' and free-form 'meta'.  Yields (meta, result) in
        order.  With overlap_stages the upload of chunk k+1 and the host work of chunk k-1 hide behind the kernels of
        chunk k; results are identical either way."""
        it = iter(items)

        def stage_next() -> Optional[_Staged]:
            item = next(it, None)
            if item is None:
                return None
            meta = dict(item.get("meta") or {})
            if self.keypoint_extractor is not None and hasattr(self.keypoint_extractor, "reseed") \
                    and "chunk_index" in meta:
                meta["_reseed"] = meta["chunk_index"]
            return self._stage_in(item["frames"], item["paths"], meta, item.get("kind", "float"))

        overlap = self.config.overlap_stages
        host = self.host_seconds = {"wait_for_frames": 0.0, "launch": 0.0, "finish": 0.0}

        def clocked(key, fn, *a):
            t0 = time.perf_counter()
            r = fn(*a)
            host[key] += time.perf_counter() - t0
            return r

        staged = clocked("wait_for_frames", stage_next)
        prev: Optional[_InFlight] = None
        while staged is not None:
            if "_reseed" in staged.meta:      # the random grid subset of chunk c must not depend on the sharding
                self.keypoint_extractor.reseed(staged.meta.pop("_reseed"))
            fl = clocked("launch", self._launch, staged)
            staged = clocked("wait_for_frames", stage_next)   # its upload runs on the copy stream beside the kernels above
            if not overlap:
                yield fl.meta, clocked("finish", self._finish, fl)
                continue
            if prev is not None:
                yield prev.meta, clocked("finish", self._finish, prev)
            prev = fl
        if prev is not None:
            yield prev.meta, clocked("finish", self._finish, prev)

    def process_and_save(self, image_paths: List[str]) -> List[str]:
        """offline_chunk_creator.py:258-371: cut the sequence into chunks, run them, write chunk files + manifest +
        metadata.  Chunk c is created by rank c % world under torch.distributed.run."""
        if not image_paths:
            raise ValueError("image_paths is empty")
        cfg = self.config
        self.target_size = calculate_target_size(image_paths[0], pixel_limit=255000 // 2)
        print(f"Target size: {self.target_size}")
        undist = self.undistortion_maps
        u8 = cfg.device_resize or undist is not None
        dataset = ChunkImageDataset(image_paths, cfg.chunk_length, cfg.overlap, self.target_size, decode_only=u8)
        mine = list(range(self.rank, len(dataset), self.world))
        nw = cfg.num_loader_workers
        if nw > 0:    # decode threads in this process, two chunks ahead, into pinned staging buffers
            loader = ThreadedChunkLoader(dataset, mine, threads=max(nw, 4), depth=2, pin=cfg.pin_memory)
        else:         # in-line loading (tests, tiny runs)
            shard = dataset if self.world == 1 else torch.utils.data.Subset(dataset, mine)
            loader = DataLoader(shard, batch_size=1, shuffle=False, num_workers=0, pin_memory=cfg.pin_memory)
        print(f"🔄 Processing {len(mine)} of {len(dataset)} chunks (rank {self.rank}/{self.world})...")

        t_first = [None]

        def items():
            for local_idx, batch in enumerate(loader):
                if t_first[0] is None:
                    t_first[0] = time.time()      # loader workers are up and the first chunk is decoded
                c = mine[local_idx]
                meta = {"chunk_index": c, "start_idx": int(batch["start_idx"].item()),
                        "end_idx": int(batch["end_idx"].item())}
                print(f"📦 Chunk {c + 1}/{len(dataset)}: frames {meta['start_idx'] + 1}-{meta['end_idx']}")
                if u8:
                    yield {"frames": batch["chunk_u8"][0], "kind": "u8_undist" if undist is not None else "u8",
                           "paths": batch["chunk_paths"][0], "meta": meta}
                else:
                    yield {"frames": batch["chunk"], "kind": "float", "paths": batch["chunk_paths"][0], "meta": meta}

        t_all = time.time()
        saved, manifest, stats = self.write_chunks(self.process_chunks(items()))
        wall = max(1e-6, time.time() - t_all)

        total_t, total_n = sum(s[0] for s in stats), sum(s[1] for s in stats)
        if total_t > 0:
            print(f"\n⏱️ Overall inference: {total_n} frames in {total_t:.3f}s  ->  {total_n / total_t:.2f} FPS (weighted); "
                  f"end to end incl. loader and writer: {total_n / wall:.2f} FPS")
            full = sorted(s[2] for s in stats if s[1] == cfg.chunk_length)
            if full:
                print(f"   Steady-state FPS (full {cfg.chunk_length}-frame chunks, median): {full[len(full) // 2]:.2f} FPS")
        hs = self.host_seconds
        print("   host time: " + ", ".join(f"{k} {v:.2f} s" for k, v in hs.items()) + f" of {wall:.2f} s wall")
        self.last_run = {"frames": total_n, "wall_s": wall, "infer_s": total_t, "host_seconds": dict(hs),
                         "wall_after_first_chunk_decoded_s": max(1e-6, time.time() - (t_first[0] or t_all))}

        self.write_run_metadata(manifest)
        print(f"✅ Completed. Saved {len(saved)} chunks to {self.chunks_dir}")
        return saved

    def write_chunks(self, stream: Iterable[Tuple[Dict, Dict]]) -> Tuple[List[str], List[Dict], List[Tuple[float, int, float]]]:
        """The chunk writer of process_and_save (offline_chunk_creator.py:300-334): every (meta, result) of `stream`
        (process_chunks) becomes chunks/chunk_%06d.pt through one writer thread, so torch.save of chunk k runs beside the
        kernels of chunk k+1.  -> (saved paths, manifest entries, (infer_s, num_frames, fps) per chunk).  meta needs
        chunk_index, start_idx, end_idx and paths."""
        saved: List[str] = []
        manifest: List[Dict] = []
        stats: List[Tuple[float, int, float]] = []
        writer = ThreadPoolExecutor(max_workers=1, thread_name_prefix="chunk-writer")
        pending = []

        def write(result: Dict, path: str) -> Optional[str]:
            try:
                torch.save(result, path)
                return None
            except Exception as e:  # noqa: BLE001
                return str(e)

        for meta, result in stream:
            m = result["_metrics"]
            stats.append((m["infer_s"], m["num_frames"], m["fps"]))
            name = f"chunk_{meta['chunk_index']:06d}.pt"
            result.update(chunk_index=meta["chunk_index"], start_idx=meta["start_idx"], end_idx=meta["end_idx"])
            entry = {"chunk_index": meta["chunk_index"], "file": name, "start_idx": meta["start_idx"],
                     "end_idx": meta["end_idx"], "num_frames": len(meta["paths"]), "image_paths": meta["paths"]}
            pending.append((writer.submit(write, result, os.path.join(self.chunks_dir, name)), entry))
        for fut, entry in pending:
            err = fut.result()
            path = os.path.join(self.chunks_dir, entry["file"])
            if err is None:
                saved.append(path)
                manifest.append(entry)
                print(f"   💾 Saved: {path}")
            else:
                print(f"❌ Failed to save chunk {entry['chunk_index']}: {err}")
        writer.shutdown()
        return saved, manifest, stats

    def write_run_metadata(self, manifest: List[Dict]) -> None:
        """chunks_manifest.json + chunk_metadata.json (offline_chunk_creator.py:336-369); under torch.distributed.run
        rank 0 writes the manifest of all ranks' chunks and no rank returns before the files are on disk."""
        cfg = self.config
        if self.world > 1:
            from .dist import gather_objects
            parts = gather_objects(manifest)
            if self.rank != 0:
                torch.distributed.barrier()
                return
            manifest = sorted((e for part in parts for e in part), key=lambda e: e["chunk_index"])
        self._write_json("chunks_manifest.json", manifest)
        self._write_json("chunk_metadata.json", {
            "chunk_length": int(cfg.chunk_length), "overlap": int(cfg.overlap),
            "target_size": list(self.target_size) if self.target_size is not None else None})
        if self.world > 1:
            torch.distributed.barrier()     # metadata is on disk before any rank starts stage 2

    def _write_json(self, name: str, obj) -> None:
        try:
            with open(os.path.join(self.config.output_dir, name), "w") as f:
                json.dump(obj, f, indent=2)
        except Exception as e:  # noqa: BLE001
            print(f"⚠️  Failed to write {name}: {e}")
