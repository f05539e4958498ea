"""OfflineReconstructor: the stage-2 driver, a mirror of slam/offline_reconstructor.py (same constructor, run(), input
layout <chunk_dir>/chunks/chunk_*.pt + chunk_metadata.json).  Per chunk: load, the per-chunk bundle adjustment
(utils/chunk_reconstruction.py:188-219 -> bundle_adjust.py, csrc/ba.hip), the closed-form Sim(3) alignment to the
predecessor over the overlap views and the prior-constrained adjustment after it (offline_reconstructor.py:93-133 ->
utils/reconstruction_alignment.py:74-171 -> alignment.py, csrc/sim3.hip).  bundle_adjust=False leaves the closed form.

Two loops share the per-chunk steps (_load_chunk, _align, _finish_chunk, _collect_and_write):
  _run_chain   chunk after chunk, each aligned to its refined predecessor: the single-process run, and under torchrun
               with bundle adjustment on, where the ranks take turns and the refined chunk travels on (dist.chain_step);
  _run_waves   under torchrun without the prior-constrained adjustment: `world` chunks at a time (dist.WaveAligner).
Rank 0 ends up with the chunks in the global frame and writes the output files (export.write_outputs)."""
from __future__ import annotations

import glob
import json
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import export
from .alignment import align_and_refine_reconstructions, create_view_graph_matches, transform_chunk
from .dist import (COLLECT_KEYS, WaveAligner, chain_payload, chain_step, ensure_process_group, gather_objects,
                   resolve_device)


class OfflineReconstructor:
    def __init__(self, chunk_dir: str, output_dir: str, chunk_length: Optional[int] = None,
                 overlap: Optional[int] = None, max_observations_per_track: int = 5, save_per_chunk: bool = False,
                 use_inverse_depth: bool = False, device: str = "cuda", save_observations: bool = False,
                 bundle_adjust: bool = True, ba_sanity_gate: bool = True, align_estimated_tracks_only: bool = False,
                 render_every: Optional[int] = None, render_overview: bool = False, render_min_weight: int = 1,
                 render_splat_scale: float = 1.0, dense_min_weight: Optional[int] = None,
                 dense_min_support: Optional[int] = None, dense_support_radius: int = 1,
                 dense_min_component: Optional[int] = None, dense_mesh: bool = False,
                 dense_carve_min_conflicts: Optional[int] = None, dense_carve_tolerance: float = 0.03,
                 loop_closure: bool = False, loop_min_gap: int = 2, loop_min_overlap: float = 0.3,
                 loop_max_edges: int = 3, loop_max_dist: float = 0.1, loop_max_rms: float = 0.03,
                 loop_min_pair_fraction: float = 0.2, loop_cell: float = 0.16,
                 occupancy_cell: Optional[float] = None, occupancy_min_free_views: int = 2,
                 occupancy_tolerance: float = 0.03, occupancy_clearance: Optional[float] = None,
                 occupancy_unknown_obstacle: bool = False, occupancy_max_cells: int = 1 << 27,
                 map_follow_poses: bool = False, map_follow_tolerance: float = 0.03):
        self.chunk_dir, self.output_dir = chunk_dir, output_dir
        # loop_closure: before the outputs are written, chunks that see the same surface are found by the co-occupancy
        # of their dense clouds, measured against each other by ICP and reconciled with the chain in a Sim(3) pose graph
        # (loop_closure.close_loops; the chunks must carry dense clouds).  Off by default: nothing is imported or run.
        # The loop_* defaults are starting points, not measured optima
        self.loop_closure = bool(loop_closure)
        self.loop_options = dict(loop_min_gap=int(loop_min_gap), loop_min_overlap=float(loop_min_overlap),
                                 loop_max_edges=int(loop_max_edges), loop_max_dist=float(loop_max_dist),
                                 loop_max_rms=float(loop_max_rms), loop_min_pair_fraction=float(loop_min_pair_fraction),
                                 loop_cell=float(loop_cell))
        self.loop_closure_info: Optional[Dict] = None
        # dense_mesh: after dense_points.ply also dense_mesh.ply, a triangle mesh of the same fused (and cleaned) table
        # (dense_map.MapMesher); the chunks must carry normals (created with dense_normals)
        self.dense_mesh = bool(dense_mesh)
        # dense_min_weight / dense_min_support / dense_min_component: filters on the fused dense map before it is written
        # and rendered (dense_map.MapCleaner); all off by default, and then no cleaner exists
        from .dense_map import MapCarver, MapCleaner
        self.dense_cleaner = MapCleaner.from_options(dense_min_weight, dense_min_support, dense_support_radius,
                                                     dense_min_component)
        # dense_carve_min_conflicts: before those filters, drop the voxels of the fused map that this many depth keyframes
        # (chunks created with dense_depth_every) looked through (dense_map.MapCarver); off by default: no carver.  The
        # keyframes sit where the chunks' similarities put them: use it with bundle_adjust=False or map_follow_poses
        self.dense_carver = MapCarver.from_options(dense_carve_min_conflicts, dense_carve_tolerance)
        # occupancy_cell: also occupancy.npz, the occupied / free / unknown grid of cells of this size around the dense
        # map, voted on by the same depth keyframes, and with occupancy_clearance (metres) its clearance field
        # (dense_map.MapOccupancy); off by default: no stage.  The same caveat: bundle_adjust=False or map_follow_poses.
        # The defaults are starting points, not measured optima
        from .dense_map import MapOccupancy
        self.dense_occupancy = MapOccupancy.from_options(occupancy_cell, occupancy_min_free_views, occupancy_tolerance,
                                                         occupancy_clearance, occupancy_unknown_obstacle,
                                                         occupancy_max_cells)
        # map_follow_poses: the dense map follows the final poses view by view (dense_map.MapFollower): every chunk keeps
        # the camera_poses of its file as '_poses_created', and a cloud point moves with the depth keyframes (chunks
        # created with dense_depth_every) that saw it; chunks without keyframes keep their similarity.  Off by
        # default: no follower, and nothing is kept
        from .dense_map import MapFollower
        self.dense_follower = MapFollower.from_options(map_follow_poses, map_follow_tolerance)
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

    def _ba_args(self, data: Dict) -> Optional[Dict]:
        if not self.bundle_adjust:
            return None
        from .bundle_adjust import chunk_ba_args
        return chunk_ba_args(data, self.max_observations_per_track, sanity_gate=self.ba_sanity_gate,
                             inverse_depth=self.use_inverse_depth)

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

    # ------------------------------------------------------------------ the per-chunk steps every loop calls
    def _load_chunk(self, files: List[str], idx: int, announce: bool = False) -> Tuple[Optional[Dict], float]:
        """Chunk `idx` from its file, after the refinement inside ChunkPTRecon.create_recon_from_chunk
        (chunk_reconstruction.py:188-219), and when its processing began; (None, 0.0) past the last chunk."""
        if idx >= len(files):
            return None, 0.0
        if announce:
            print(f"\n📦 Loading {os.path.basename(files[idx])} ({idx + 1}/{len(files)})")
        data: Dict = torch.load(files[idx], map_location="cpu", weights_only=False)
        t0 = time.time()
        if self.dense_follower is not None:     # the frame the chunk's dense cloud and depth keyframes stay in
            data["_poses_created"] = data["camera_poses"].clone()
        args = self._ba_args(data)
        if args is not None:
            try:
                from .bundle_adjust import bundle_adjust_new_chunk
                info = bundle_adjust_new_chunk(data, args, self.device)
                self.ba_infos.append(info)
                if info.get("success"):
                    print(f"   Removed {info['removed_tracks']} tracks after initial bundle adjustment "
                          f"(cost {info['initial_cost']:.4f} -> {info['final_cost']:.4f}, {info['iterations']} iterations)")
            except Exception as e:  # noqa: BLE001 - degrade, do not crash
                print(f"   ⚠️  Bundle adjustment of chunk {idx} failed: {e}")
        return data, t0

    def _align(self, prev: Dict, data: Dict, idx: int) -> bool:
        """Chunk `idx` into its (refined) predecessor's frame; `prev` is that chunk or its dist.chain_payload."""
        ok, info = align_and_refine_reconstructions(prev, data, create_view_graph_matches(self.chunk_length, self.overlap),
                                                    use_inverse_depth=self.use_inverse_depth, device=self.device,
                                                    bundle_adjust=self._ba_args(data),
                                                    skip_unestimated=self.align_estimated_tracks_only)
        self.alignment_infos.append(info if ok else None)
        if not ok:
            print(f"   ❌ Alignment failed for chunk {idx}")
        return ok

    def _finish_chunk(self, data: Dict, idx: int, ok: bool, collect: bool, t0: Optional[float] = None) -> Dict:
        """Bookkeeping and per-chunk files of a chunk that has reached the global frame -> what is kept of it: all of it,
        or (`collect`: it travels to rank 0) dist.COLLECT_KEYS.  `t0`: print the single-process timing line."""
        # the cached observation arrays (~18 MB of device memory per chunk) are released by the chunk's last
        # adjustment; chunk 0 has none after this point and a chunk whose alignment failed never reaches it
        data.pop("_observations", None)
        data["chunk_order"], data["alignment_ok"] = idx, bool(ok)
        if t0 is not None:
            dt = max(1e-6, time.time() - t0)
            n = int(data["camera_poses"].shape[0])
            print(f"   ⏱️ Reconstruction: {dt:.3f}s for {n} frames  ->  {n / dt:.2f} FPS")
        if self.save_per_chunk:
            self._save_chunk(data, idx)
        if self.save_observations:
            self._save_observations(data, idx)
        return {k: data[k] for k in COLLECT_KEYS if k in data} if collect else data

    def _collect_and_write(self, done: List[Dict], rank: int, grouped: bool) -> None:
        """This rank's finished chunks -> rank 0, which writes the output files."""
        if grouped:
            parts = gather_objects(done)
            done = sorted((d for part in parts or [] for d in part), key=lambda d: d["chunk_order"])
        if rank == 0:
            self.reconstructions = done
            if self.loop_closure:
                from .loop_closure import close_loops
                self.loop_closure_info = close_loops(done, self.device, **self.loop_options)
                if self.loop_closure_info["skipped"] != "fewer_than_three_participants":
                    with open(os.path.join(self.output_dir, "loop_closure.json"), "w") as f:
                        json.dump(self.loop_closure_info, f, indent=1, default=float)
            seconds = export.write_outputs(done, self.output_dir, self.device, self.render_every, self.render_overview,
                                           self.render_min_weight, self.render_splat_scale, self.dense_cleaner,
                                           self.dense_mesh, dense_occupancy=self.dense_occupancy,
                                           dense_carver=self.dense_carver,
                                           dense_follower=self.dense_follower)
            if seconds is not None:
                self.render_seconds = seconds
        if grouped:
            dist.barrier()

    # ------------------------------------------------------------------ the two loops
    def run(self) -> None:
        rank, world = ensure_process_group()
        grouped = world > 1 or (dist.is_available() and dist.is_initialized())
        if grouped and not self.bundle_adjust:
            self._run_waves(rank, world)
        else:
            self._run_chain(rank, world, grouped)

    def _run_chain(self, rank: int, world: int, grouped: bool) -> None:
        """Chunk after chunk, each aligned to its predecessor AFTER that one's refinement (offline_reconstructor.py:
        130-133).  Without a process group this is the whole single-process run.  With one (bundle adjustment on): the
        SAME arithmetic, chunk c on rank c % world; the ranks take turns in chunk order and the refined chunk travels to
        the next owner (dist.chain_step).  Identical trajectories either way (tested)."""
        files = self._load_chunks()
        self.refinement_stages = (["per_chunk_bundle_adjust", "closed_form_sim3", "prior_constrained_bundle_adjust"]
                                  if self.bundle_adjust else ["closed_form_sim3"])
        print(f"🔄 Reconstructing {len(files)} chunks from {self.chunk_dir}"
              + (f" on {world} ranks (rank {rank}), sequential refinement chain (bundle adjustment on)" if grouped else ""))
        # ranks load + adjust their own chunks ONE chunk ahead of the chain (the first before the chain starts, the next
        # right after this rank's turn, while the other ranks take theirs): a chunk carries ~18 MB of device-resident
        # observation arrays between its two adjustments, so preparing every chunk up front grew HBM and host memory
        # linearly with the chunks per rank
        ahead = self._load_chunk(files, rank) if grouped else None
        prev: Optional[Dict] = None
        done: List[Dict] = []
        for c in range(len(files)):
            owner, mine = c % world, None
            if rank == owner:
                mine, t0 = ahead if grouped else self._load_chunk(files, c, announce=True)
                if c > 0 and not grouped:
                    print("   🔗 Aligning with previous reconstruction...")
                ok = c == 0 or self._align(prev, mine, c)
                done.append(self._finish_chunk(mine, c, ok, grouped, None if grouped else t0))
            prev = chain_step(chain_payload(mine), owner) if grouped else mine
            if grouped and rank == owner:
                ahead = self._load_chunk(files, c + world)
        self._summarise_refinement()
        self._collect_and_write(done, rank, grouped)

    def _run_waves(self, rank: int, world: int, solve=None) -> None:
        """Chunk-parallel alignment: chunk c lives on rank c % world.  Per wave of `world` chunks:
          1. a 2-int all-gather of (K, n_frames) sizes the blocks;
          2. ONE all-gather of the boundary blocks (overlap keypoints / points / validity + last pose, ~50 KB per rank;
             the blocks stay on the device under nccl = RCCL over xGMI);
          3. rank r solves only its own T_{c-1<-c}; a 136-byte all-gather distributes the [accepted, T] records;
          4. every rank forms G_c = G_{c-1} . T_c by the prefix product (dist.align_wave) and applies G_c to its chunk.
        This wave form serves bundle_adjust=False and equals the sequential run: both solve on chunk-frame fp16 values
        and compose (alignment.align_and_refine_reconstructions).  With bundle_adjust=True the refinement after each
        alignment (reconstruction_alignment.py:107-171) needs the REFINED predecessor - a strictly sequential chain
        (offline_reconstructor.py:130-133) - so run() goes through _run_chain instead; self.refinement_stages says
        which stages ran.  `solve` (tests): replaces the device solver, see dist.default_solver."""
        files = self._load_chunks()
        n_chunks = len(files)
        aligner = WaveAligner(rank, world, self.overlap, self.chunk_length, self.device, solve)
        print(f"🔄 Reconstructing {n_chunks} chunks from {self.chunk_dir} on {world} ranks (rank {rank})")
        self.refinement_stages = (["per_chunk_bundle_adjust"] if self.bundle_adjust else []) + ["closed_form_sim3"]
        done: List[Dict] = []
        for w0 in range(0, n_chunks, world):
            # the per-chunk refinement is independent per chunk; the prior-constrained one after each alignment needs
            # the refined predecessor: sequential only
            data, _ = self._load_chunk(files, w0 + rank)
            Gs, oks = aligner.step(data, w0, n_chunks)
            for r, ok in enumerate(oks):
                if not ok and rank == 0:
                    print(f"   ❌ Alignment failed for chunk {w0 + r}: it stays in its own frame")
            if data is not None:
                transform_chunk(data, Gs[rank], device=self.device, absolute=True)
                done.append(self._finish_chunk(data, w0 + rank, oks[rank], True))
        self._collect_and_write(done, rank, True)

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
            export.write_ply(data["points"].float().reshape(-1, 3).numpy()[m],
                             np.full((int(np.sum(m)) if not isinstance(m, slice) else data["points"].numel() // 3, 3), 255.0),
                             os.path.join(self.recon_dir, f"chunk_{idx:06d}.ply"))
        except Exception as e:  # noqa: BLE001
            print(f"   ❌ Failed to save recon {idx}: {e}")
