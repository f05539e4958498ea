"""OfflineReconstructor: mirror of slam/offline_reconstructor.py (same constructor, run(), input layout
<chunk_dir>/chunks/chunk_*.pt + chunk_metadata.json, outputs final_points.ply / final_camera_poses.ply /
trajectory_tum.txt) for the part of stage 2 that is on the hot path: progressive overlap Sim(3) alignment of the
chunks (offline_reconstructor.py:93-133 -> utils/reconstruction_alignment.py:74-105).

What the reference additionally does through pytheia/Ceres — per-chunk bundle adjustment
(utils/chunk_reconstruction.py:192-219) and the prior-constrained BA after each alignment
(reconstruction_alignment.py:107-171) — is third-party C++ outside this path and is not done here, so
trajectories equal the reference's only up to those refinements.
"""
from __future__ import annotations

import glob
import json
import os
import struct
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .alignment import align_and_refine_reconstructions, create_view_graph_matches


def _view_name(p) -> str:
    """image_paths entries are str, 1-lists or 1-tuples depending on the DataLoader collate/pin path."""
    while isinstance(p, (list, tuple)):
        p = p[0] if p else "frame"
    return os.path.basename(str(p))


def write_ply(points: np.ndarray, colors: np.ndarray, path: str) -> None:
    """Binary little-endian PLY with float xyz + uchar rgb (the layout pi3/utils/basic.py:377-460 writes).  Float colours
    in [0, 1] are scaled by 255; uint8 colours are written as they are."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    if np.asarray(colors).dtype == np.uint8:
        rgb = np.asarray(colors).reshape(-1, 3)
    else:
        colors = np.asarray(colors, np.float32).reshape(-1, 3)
        if colors.size and colors.max() <= 1.0:
            colors = colors * 255.0
        rgb = np.clip(colors, 0, 255).astype(np.uint8)
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(points)}\nproperty float x\n"
                 "property float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                 "property uchar blue\nend_header\n").encode())
        rec = np.empty(len(points), dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
        rec["xyz"], rec["rgb"] = points, rgb
        f.write(rec.tobytes())


class OfflineReconstructor:
    def __init__(self, chunk_dir: str, output_dir: str, chunk_length: Optional[int] = None,
                 overlap: Optional[int] = None, max_observations_per_track: int = 5, save_per_chunk: bool = False,
                 use_inverse_depth: bool = False, device: str = "cuda", save_observations: bool = False,
                 bundle_adjust: bool = True, ba_sanity_gate: bool = True, align_estimated_tracks_only: bool = False,
                 render_every: Optional[int] = None, render_overview: bool = False, render_min_weight: int = 1,
                 render_splat_scale: float = 1.0):
        self.chunk_dir, self.output_dir = chunk_dir, output_dir
        # render_every / render_overview: after dense_points.ply, depth + colour images of the dense map from every N-th
        # view of the trajectory and a top-down overview, under <output>/renders (pi3_slam_amd/render.py); off by default
        if render_every is not None and int(render_every) <= 0:
            raise ValueError(f"render_every must be a positive number of views, got {render_every!r}")
        self.render_every = int(render_every) if render_every is not None else None
        self.render_overview = bool(render_overview)
        self.render_min_weight, self.render_splat_scale = int(render_min_weight), float(render_splat_scale)
        loaded_cl = loaded_ov = None
        try:  # offline_reconstructor.py:32-46
            meta_path = os.path.join(self.chunk_dir, "chunk_metadata.json")
            if os.path.exists(meta_path):
                with open(meta_path) as f:
                    meta = json.load(f)
                loaded_cl = int(meta.get("chunk_length")) if meta.get("chunk_length") is not None else None
                loaded_ov = int(meta.get("overlap")) if meta.get("overlap") is not None else None
        except Exception:  # noqa: BLE001
            pass
        self.chunk_length = int(chunk_length) if chunk_length is not None else (loaded_cl or 100)
        self.overlap = int(overlap) if overlap is not None else (loaded_ov or 10)
        self.max_observations_per_track = max_observations_per_track
        self.save_per_chunk = save_per_chunk
        # the reference's --use-inverse-depth: both adjustments run with one inverse depth per track
        # (utils/chunk_reconstruction.py:187-204, utils/reconstruction_alignment.py:147-152; pi3_bundle_adjust_inverse_depth)
        self.use_inverse_depth = bool(use_inverse_depth)
        from .dist import resolve_device
        self.device = resolve_device(device)     # 'cuda' -> this rank's card (the one the process group is bound to)
        if torch.cuda.is_available():
            torch.cuda.set_device(self.device)   # every kernel wrapper launches on the current device's stream
        # bundle_adjust: the reference's two refinement stages (per chunk: utils/chunk_reconstruction.py:188-219; after each
        # alignment with pose priors: utils/reconstruction_alignment.py:107-171) on the device (csrc/ba.hip, parity
        # unpinned); False = closed-form Sim(3) chain only
        self.bundle_adjust = bool(bundle_adjust)
        # ba_sanity_gate: keep the input when an adjustment "succeeds" on contradictory geometry (bundle_adjust.sanity_gate;
        # not in the reference, which applies whatever Ceres returns) - False for reference-parity runs.  Rejections are
        # counted in refinement_summary and printed at the end of run().
        self.ba_sanity_gate = bool(ba_sanity_gate)
        self.align_estimated_tracks_only = bool(align_estimated_tracks_only)
        self.ba_infos: List[Dict] = []
        self.refinement_summary: Dict[str, Dict[str, int]] = {}
        # save_observations: also write, per chunk, the track observations the reference builds for its bundle adjuster
        # (ChunkPTRecon.create_recon_from_chunk, utils/chunk_reconstruction.py:162-185) as observations_%06d.pt
        self.save_observations = save_observations
        os.makedirs(self.output_dir, exist_ok=True)
        self.recon_dir = os.path.join(self.output_dir, "reconstructions")
        os.makedirs(self.recon_dir, exist_ok=True)
        self.reconstructions: List[Dict] = []   # chunk dicts, transformed in place into the global frame
        self.alignment_infos: List[Optional[Dict]] = []

    def _load_chunks(self) -> List[str]:
        files = sorted(glob.glob(os.path.join(self.chunk_dir, "chunks", "chunk_*.pt")))
        if not files:
            raise FileNotFoundError(f"No chunk_*.pt files found in {self.chunk_dir}")
        return files

    def _align_last_two(self) -> Optional[Dict]:
        if len(self.reconstructions) < 2:
            return None
        matches = create_view_graph_matches(self.chunk_length, self.overlap)
        ok, info = align_and_refine_reconstructions(self.reconstructions[-2], self.reconstructions[-1], matches,
                                                    use_inverse_depth=self.use_inverse_depth, device=self.device,
                                                    bundle_adjust=self._ba_args(self.reconstructions[-1]),
                                                    skip_unestimated=self.align_estimated_tracks_only)
        if not ok:
            print(f"   ❌ Alignment failed for chunk {len(self.reconstructions) - 1}")
            return None
        return info

    def _ba_args(self, data: Dict) -> Optional[Dict]:
        if not self.bundle_adjust or data.get("keypoints") is None:
            return None
        # offline_reconstructor.py:66-67: 1920x1080 when a chunk file does not carry its size
        return {"width": int(data.get("original_width", 1920)), "height": int(data.get("original_height", 1080)),
                "max_observations_per_track": self.max_observations_per_track,
                "settings": {"sanity_gate": self.ba_sanity_gate, "inverse_depth": self.use_inverse_depth}}

    def _summarise_refinement(self) -> None:
        """Which adjustments ran, were applied, or were kept out by the sanity gate - `refinement_stages` alone lists a
        stage even when every one of its adjustments was rejected."""
        if not self.bundle_adjust:
            return
        from .bundle_adjust import ba_summary
        self.refinement_summary = {
            "per_chunk_bundle_adjust": ba_summary(self.ba_infos),
            "prior_constrained_bundle_adjust": ba_summary([(a or {}).get("bundle_adjustment") for a in self.alignment_infos])}
        for stage, c in self.refinement_summary.items():
            print(f"   {stage}: {c['applied']} of {c['ran']} applied"
                  + (f", {c['rejected_by_sanity_gate']} rejected by the sanity gate" if c["rejected_by_sanity_gate"] else "")
                  + (f", {c['failed']} failed" if c["failed"] else ""))

    def _bundle_adjust_new_chunk(self, data: Dict, idx: int) -> None:
        """The refinement inside ChunkPTRecon.create_recon_from_chunk (chunk_reconstruction.py:188-219)."""
        args = self._ba_args(data)
        if args is None:
            return
        try:
            from .bundle_adjust import PER_CHUNK, bundle_adjust_chunk
            info = bundle_adjust_chunk(data, args["width"], args["height"], args["max_observations_per_track"],
                                       self.device, dict(PER_CHUNK, **args["settings"]))
            self.ba_infos.append(info)
            if info.get("success"):
                print(f"   Removed {info['removed_tracks']} tracks after initial bundle adjustment "
                      f"(cost {info['initial_cost']:.4f} -> {info['final_cost']:.4f}, {info['iterations']} iterations)")
        except Exception as e:  # noqa: BLE001 - degrade, do not crash
            print(f"   ⚠️  Bundle adjustment of chunk {idx} failed: {e}")

    def run(self) -> None:
        from .dist import ensure_process_group
        rank, world = ensure_process_group()
        import torch.distributed as _dist
        if world > 1 or (_dist.is_available() and _dist.is_initialized()):
            self._run_distributed(rank, world)
            return
        chunk_files = self._load_chunks()
        self.refinement_stages = (["per_chunk_bundle_adjust", "closed_form_sim3", "prior_constrained_bundle_adjust"]
                                  if self.bundle_adjust else ["closed_form_sim3"])
        print(f"🔄 Reconstructing {len(chunk_files)} chunks from {self.chunk_dir}")
        for idx, path in enumerate(chunk_files):
            print(f"\n📦 Loading {os.path.basename(path)} ({idx + 1}/{len(chunk_files)})")
            data: Dict = torch.load(path, map_location="cpu", weights_only=False)
            t0 = time.time()
            self._bundle_adjust_new_chunk(data, idx)
            self.reconstructions.append(data)
            if idx > 0:
                print("   🔗 Aligning with previous reconstruction...")
                self.alignment_infos.append(self._align_last_two())
            # the cached observation arrays (~18 MB of device memory per chunk) are released by the chunk's last
            # adjustment; chunk 0 has none after this point and a chunk whose alignment failed never reaches it
            data.pop("_observations", None)
            dt = max(1e-6, time.time() - t0)
            n = int(data["camera_poses"].shape[0])
            print(f"   ⏱️ Reconstruction: {dt:.3f}s for {n} frames  ->  {n / dt:.2f} FPS")
            if self.save_per_chunk:
                self._save_chunk(data, idx)
            if self.save_observations:
                self._save_observations(data, idx)
        if not self.reconstructions:
            return
        self._summarise_refinement()
        self._write_outputs()

    def _write_outputs(self) -> None:
        try:
            pts, cols = self._extract_points_colors()
            if pts.size > 0:
                write_ply(pts, cols if cols.size else np.ones_like(pts), os.path.join(self.output_dir, "final_points.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save final PLY: {e}")
        try:
            pos, _, _ = self._extract_camera_positions()
            if pos:
                cam = np.asarray(pos, np.float32)
                write_ply(cam, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (len(cam), 1)),
                          os.path.join(self.output_dir, "final_camera_poses.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save camera trajectory PLY: {e}")
        try:
            self._save_trajectory_tum(os.path.join(self.output_dir, "trajectory_tum.txt"), integer_timestamp=True)
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save TUM trajectory: {e}")
        try:
            self._write_dense_map(os.path.join(self.output_dir, "dense_points.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"❌ Failed to save the dense map: {e}")
        if getattr(self, "render_every", None) is not None or getattr(self, "render_overview", False):
            try:
                self._write_renders(os.path.join(self.output_dir, "renders"), self.render_every, self.render_overview,
                                    self.render_min_weight, self.render_splat_scale)
            except Exception as e:  # noqa: BLE001
                print(f"❌ Failed to save the renders of the dense map: {e}")

    def _write_dense_map(self, path: str) -> Optional[int]:
        """dense_points.ply from the chunks' dense clouds (chunks created with a dense voxel size); nothing when no chunk
        carries one.  The voxel size is chunk 0's: the world frame is chunk 0's frame."""
        with_cloud = [d for d in self.reconstructions if d.get("dense_cloud") is not None]
        if not with_cloud:
            return None
        from .dense_map import fuse_chunk_clouds, write_dense_ply
        voxel = float(with_cloud[0]["dense_cloud"]["voxel_size"])
        pts, cols, w = fuse_chunk_clouds(self.reconstructions, voxel, getattr(self, "device", "cuda"))
        self._dense_map = (pts, cols, w, voxel)      # _write_renders draws the same arrays
        write_dense_ply(pts, cols, path)
        print(f"✅ Saved dense map with {len(pts)} voxels ({voxel} m) to: {path}")
        return len(pts)

    def _render_views(self) -> List[Dict]:
        """The de-duplicated trajectory (first occurrence of a view name wins, as in the TUM export) with what a render
        needs: name, cam->world pose, the chunk's intrinsics moved to index coordinates, image size."""
        views, seen = [], set()
        for d in self.reconstructions:
            poses = d["camera_poses"].double().numpy()
            paths = d.get("image_paths") or [f"frame_{i}" for i in range(len(poses))]
            K = d.get("intrinsics")
            for i, P in enumerate(poses):
                name = _view_name(paths[i]) if i < len(paths) else f"view_{i}"
                if name in seen:
                    continue
                seen.add(name)
                view = {"name": name, "pose": P, "K": None, "H": d.get("original_height"), "W": d.get("original_width")}
                if K is not None and view["H"] is not None and view["W"] is not None:
                    Ki = torch.as_tensor(K).double().reshape(-1, 3, 3)[min(i, len(K) - 1)].numpy().copy()
                    # the chunk says W // 2: the image centre in corner-based coordinates; pixel i has its centre at
                    # i + 0.5 there and at i in the index coordinates the renderer (and the keypoints) use
                    Ki[0, 2] -= 0.5
                    Ki[1, 2] -= 0.5
                    view["K"], view["H"], view["W"] = Ki, int(view["H"]), int(view["W"])
                views.append(view)
        return views

    def _write_renders(self, out_dir: str, every: Optional[int], overview: bool, min_weight: int = 1,
                       splat_scale: float = 1.0) -> Optional[int]:
        """<out_dir>/depth_<frame>.png (16 bit, millimetres, 0 = empty) and color_<frame>.png of the dense map for every
        `every`-th view of the de-duplicated trajectory, overview.png (a top-down orthographic view with the trajectory
        in red) and cameras.json.  Without dense clouds in the chunks: one line, no directory."""
        if not any(d.get("dense_cloud") is not None for d in self.reconstructions):
            print("   ℹ️  No dense clouds in the chunks (create them with a dense voxel size): no renders")
            return None
        from .render import DEPTH_PNG_SCALE, MapRenderer, pack_cameras, render_overview, write_color_png, write_depth_png
        device = getattr(self, "device", "cuda")
        if getattr(self, "_dense_map", None) is None:
            from .dense_map import fuse_chunk_clouds
            voxel = float(next(d for d in self.reconstructions if d.get("dense_cloud") is not None)["dense_cloud"]["voxel_size"])
            self._dense_map = fuse_chunk_clouds(self.reconstructions, voxel, device) + (voxel,)
        pts, cols, w, voxel = self._dense_map
        views = self._render_views()
        chosen = [v for v in views[:: int(every)] if v["K"] is not None] if every else []
        if every and not chosen:
            print("   ℹ️  The chunks carry no intrinsics / image size: no per-view renders")
        os.makedirs(out_dir, exist_ok=True)
        t0, t_png = time.time(), 0.0
        record = {"depth_scale": DEPTH_PNG_SCALE, "voxel_size": voxel, "min_weight": int(min_weight),
                  "splat_scale": float(splat_scale), "near": 0.05, "views": [], "overview": None}
        renderer = MapRenderer(pts, cols, w, voxel, device) if chosen else None
        for size in sorted({(v["H"], v["W"]) for v in chosen}):
            group = [v for v in chosen if (v["H"], v["W"]) == size]
            cams = pack_cameras(np.stack([v["pose"] for v in group]), np.stack([v["K"] for v in group]))
            out = renderer.render(cams, size[0], size[1], min_weight=min_weight, splat_scale=splat_scale, near=0.05)
            for j, v in enumerate(group):
                stem = os.path.splitext(v["name"])[0]
                v["depth"], v["color"] = f"depth_{stem}.png", f"color_{stem}.png"
                t1 = time.time()
                write_depth_png(out["depth"][j], os.path.join(out_dir, v["depth"]))
                write_color_png(out["color"][j], os.path.join(out_dir, v["color"]))
                t_png += time.time() - t1
        for v in chosen:
            K = v["K"]
            record["views"].append({"frame": v["name"], "pose": [[float(x) for x in row] for row in v["pose"]],
                                    "fx": float(K[0, 0]), "fy": float(K[1, 1]), "cx": float(K[0, 2]), "cy": float(K[1, 2]),
                                    "H": v["H"], "W": v["W"], "depth": v["depth"], "color": v["color"]})
        if overview and views:
            sized = next((v for v in views if v["K"] is not None), None)
            H, W = (sized["H"], sized["W"]) if sized else (480, 640)
            ov = render_overview(pts, cols, w, voxel, np.stack([v["pose"] for v in views]), H, W, min_weight=min_weight,
                                 splat_scale=splat_scale, device=device)
            t1 = time.time()
            write_color_png(ov["color"], os.path.join(out_dir, "overview.png"))
            t_png += time.time() - t1
            record["overview"] = {"color": "overview.png", "ortho": True, "near": ov["near"], "H": H, "W": W,
                                  "pose": [[float(x) for x in row] for row in ov["pose"]],
                                  "fx": float(ov["K"][0, 0]), "fy": float(ov["K"][1, 1]), "cx": float(ov["K"][0, 2]),
                                  "cy": float(ov["K"][1, 2])}
        with open(os.path.join(out_dir, "cameras.json"), "w") as f:
            json.dump(record, f, indent=1)
        print(f"✅ Saved {len(chosen)} depth / colour renders" + (" and the overview" if record["overview"] else "")
              + f" of the dense map to: {out_dir} ({time.time() - t0:.2f}s, {t_png:.2f}s of it PNG encoding)")
        self.render_seconds = {"total": time.time() - t0, "png": t_png}
        return len(chosen)

    def _keep_keys(self) -> Tuple[str, ...]:
        """What rank 0 collects of every chunk; a render also needs the intrinsics and the image size."""
        keep = ("points", "colors", "keypoints", "masks", "camera_poses", "image_paths", "chunk_order", "alignment_ok",
                "dense_cloud", "_sim3_global", "_sim3_dense")
        if self.render_every is not None or self.render_overview:
            keep += ("intrinsics", "original_width", "original_height")
        return keep

    def _run_distributed(self, rank: int, world: int, solve=None) -> None:
        """Chunk-parallel alignment: chunk c lives on rank c % world.  Per wave of `world` chunks:
          1. a 2-int all-gather of (K, n_frames) sizes the blocks;
          2. ONE all-gather of the boundary blocks (overlap keypoints / points / validity + last pose, ~50 KB per rank;
             the blocks stay on the device under nccl = RCCL over xGMI);
          3. rank r solves only its own T_{c-1<-c}; a 136-byte all-gather distributes the [accepted, T] records;
          4. every rank forms G_c = G_{c-1} . T_c by the prefix product (dist.align_wave) and applies G_c to its chunk.
        Rank 0 collects the transformed chunks for the trajectory / point-cloud files.
        This wave form serves bundle_adjust=False and equals the sequential run: both solve on chunk-frame fp16 values
        and compose (alignment.align_and_refine_reconstructions).  With bundle_adjust=True the refinement after each
        alignment (reconstruction_alignment.py:107-171) needs the REFINED predecessor - a strictly sequential chain
        (offline_reconstructor.py:130-133) - so run() goes through _run_distributed_chain instead, which reproduces the
        single-process trajectory exactly; self.refinement_stages says which stages ran.
        `solve` (tests): replaces the device solver, see dist.default_solver."""
        import torch.distributed as dist

        from .alignment import transform_chunk
        from .dist import WaveAligner, gather_objects
        if self.bundle_adjust and solve is None:
            return self._run_distributed_chain(rank, world)
        files = self._load_chunks()
        n_chunks = len(files)
        aligner = WaveAligner(rank, world, self.overlap, self.chunk_length, self.device, solve)
        print(f"🔄 Reconstructing {n_chunks} chunks from {self.chunk_dir} on {world} ranks (rank {rank})")
        self.refinement_stages = (["per_chunk_bundle_adjust"] if self.bundle_adjust else []) + ["closed_form_sim3"]
        mine: List[Dict] = []
        for w0 in range(0, n_chunks, world):
            c = w0 + rank
            data = torch.load(files[c], map_location="cpu", weights_only=False) if c < n_chunks else None
            if data is not None:    # the per-chunk refinement is independent per chunk; the prior-constrained one after
                self._bundle_adjust_new_chunk(data, c)   # each alignment needs the refined predecessor: sequential only
                data.pop("_observations", None)          # no later adjustment will read them (device memory)
            Gs, oks = aligner.step(data, w0, n_chunks)
            for r, ok in enumerate(oks):
                if not ok and rank == 0:
                    print(f"   ❌ Alignment failed for chunk {w0 + r}: it stays in its own frame")
            if data is not None:
                transform_chunk(data, Gs[rank], device=self.device, absolute=True)
                data["chunk_order"] = c
                data["alignment_ok"] = bool(oks[rank])
                mine.append(data)
                if self.save_per_chunk:
                    self._save_chunk(data, c)
                if self.save_observations:
                    self._save_observations(data, c)
        keep = self._keep_keys()
        parts = gather_objects([{k: d[k] for k in keep if k in d} for d in mine])
        if rank == 0:
            self.reconstructions = sorted((d for part in parts for d in part), key=lambda d: d["chunk_order"])
            self._write_outputs()
        dist.barrier()

    def _run_distributed_chain(self, rank: int, world: int) -> None:
        """Bundle adjustment on, several ranks: the SAME arithmetic as the single-process run, chunk c on rank
        c % world.  The per-chunk adjustment of a rank's chunks is independent and runs up front; alignment + the
        prior-constrained adjustment need the refined predecessor, so the ranks take turns in chunk order and the refined
        chunk travels to the next owner (dist.chain_step).  Identical trajectories to `run()` without torchrun (tested)."""
        import torch.distributed as dist

        from .dist import chain_payload, chain_step, gather_objects
        files = self._load_chunks()
        n_chunks = len(files)
        self.refinement_stages = ["per_chunk_bundle_adjust", "closed_form_sim3", "prior_constrained_bundle_adjust"]
        print(f"🔄 Reconstructing {n_chunks} chunks from {self.chunk_dir} on {world} ranks (rank {rank}), sequential "
              f"refinement chain (bundle adjustment on)")
        keep = self._keep_keys()
        own: Dict[int, Dict] = {}
        done: List[Dict] = []

        def prepare(c: int) -> None:
            # load + the independent per-chunk adjustment of this rank's chunk c.  Done ONE chunk ahead of the chain (the
            # first before the chain starts, the next right after this rank's turn, while the other ranks take theirs):
            # a chunk carries ~18 MB of device-resident observation arrays between its two adjustments, so preparing
            # every chunk up front grew HBM and host memory linearly with the chunks per rank
            if c < n_chunks:
                data = torch.load(files[c], map_location="cpu", weights_only=False)
                self._bundle_adjust_new_chunk(data, c)
                own[c] = data

        prepare(rank)
        matches = create_view_graph_matches(self.chunk_length, self.overlap)
        prev: Optional[Dict] = None
        for c in range(n_chunks):
            owner = c % world
            payload = None
            if rank == owner:
                data = own.pop(c)
                ok = True
                if c > 0:
                    ok, info = align_and_refine_reconstructions(prev, data, matches, device=self.device,
                                                                use_inverse_depth=self.use_inverse_depth,
                                                                bundle_adjust=self._ba_args(data),
                                                                skip_unestimated=self.align_estimated_tracks_only)
                    self.alignment_infos.append(info if ok else None)
                    if not ok:
                        print(f"   ❌ Alignment failed for chunk {c}")
                data.pop("_observations", None)      # chunk 0 / a failed alignment: no later adjustment releases them
                data["chunk_order"], data["alignment_ok"] = c, bool(ok)
                payload = chain_payload(data)
                if self.save_per_chunk:
                    self._save_chunk(data, c)
                if self.save_observations:
                    self._save_observations(data, c)
                done.append({k: data[k] for k in keep if k in data})
            prev = chain_step(payload, owner)
            if rank == owner:
                prepare(c + world)
        self._summarise_refinement()
        parts = gather_objects(done)
        if rank == 0:
            self.reconstructions = sorted((d for part in parts for d in part), key=lambda d: d["chunk_order"])
            self._write_outputs()
        dist.barrier()

    def _save_observations(self, data: Dict, idx: int) -> None:
        try:
            from .observations import project_chunk_observations
            if "intrinsics" not in data or data["intrinsics"] is None:
                return
            chunk = {"points": data["points"].to(self.device), "camera_poses": data["camera_poses"].to(self.device),
                     "intrinsics": data["intrinsics"].to(self.device)}
            obs = project_chunk_observations(chunk, int(data["original_width"]), int(data["original_height"]),
                                             self.max_observations_per_track)
            torch.save({k: v.cpu() for k, v in obs.items()}, os.path.join(self.recon_dir, f"observations_{idx:06d}.pt"))
        except Exception as e:  # noqa: BLE001
            print(f"   ❌ Failed to save observations {idx}: {e}")

    def _save_chunk(self, data: Dict, idx: int) -> None:
        try:
            m = data["masks"].reshape(-1).numpy() if "masks" in data else slice(None)
            write_ply(data["points"].float().reshape(-1, 3).numpy()[m],
                      np.full((int(np.sum(m)) if not isinstance(m, slice) else data["points"].numel() // 3, 3), 255.0),
                      os.path.join(self.recon_dir, f"chunk_{idx:06d}.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"   ❌ Failed to save recon {idx}: {e}")

    def _extract_points_colors(self) -> Tuple[np.ndarray, np.ndarray]:
        """offline_reconstructor.py:170-193: every track of every chunk (no de-duplication)."""
        pts, cols = [], []
        for d in self.reconstructions:
            if "keypoints" not in d:
                continue
            pts.append(d["points"].float().reshape(-1, 3).numpy())
            if "colors" in d and d["colors"] is not None:
                cols.append(d["colors"].float().reshape(-1, 3).numpy())
        if not pts:
            return np.array([]), np.array([])
        P = np.concatenate(pts, 0)
        C = np.concatenate(cols, 0) if cols else np.array([])
        if C.size > 0 and C.max() > 1.0:
            C = C / 255.0
        return P.astype(np.float32), C.astype(np.float32)

    def _extract_camera_positions(self):
        positions, orientations, names = [], [], []
        for d in self.reconstructions:
            poses = d["camera_poses"].float().numpy()
            paths = d.get("image_paths") or [f"frame_{i}" for i in range(len(poses))]
            for i, P in enumerate(poses):
                positions.append(P[:3, 3].astype(np.float32))
                orientations.append(P[:3, :3].astype(np.float32))
                names.append(_view_name(paths[i]) if i < len(paths) else f"view_{i}")
        return positions, orientations, names

    def _build_full_camera_trajectory(self):
        """First occurrence of each view name wins (offline_reconstructor.py:218-229)."""
        positions, orientations, names = self._extract_camera_positions()
        seen, traj, rots = set(), [], []
        for name, pos, R in zip(names, positions, orientations):
            if name in seen:
                continue
            seen.add(name)
            traj.append(pos)
            rots.append(R)
        return traj, rots

    def _save_trajectory_tum(self, save_path: str, integer_timestamp: bool = True) -> None:
        """TUM format of offline_reconstructor.py:231-255 ("{i} {x:.6f} ... {qw:.6f}")."""
        from scipy.spatial.transform import Rotation
        traj, rots = self._build_full_camera_trajectory()
        if not traj:
            print("No camera trajectory available to save from reconstructions")
            return
        os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
        with open(save_path, "w") as f:
            f.write("# timestamp tx ty tz qx qy qz qw\n")
            for i, (pos, R) in enumerate(zip(traj, rots)):
                x, y, z = pos
                qx, qy, qz, qw = Rotation.from_matrix(R.astype(np.float64)).as_quat()
                ts = f"{i}" if integer_timestamp else f"{float(i):.9f}"
                f.write(f"{ts} {x:.6f} {y:.6f} {z:.6f} {qx:.6f} {qy:.6f} {qz:.6f} {qw:.6f}\n")
        print(f"✅ Saved trajectory with {len(traj)} poses to: {save_path}")
