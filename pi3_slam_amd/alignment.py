"""Overlap-based Sim(3) chunk alignment: mirror of utils/reconstruction_alignment.py (create_view_graph_matches :16-37,
align_and_refine_reconstructions :40-198, steps 1-3 + the transform), operating on chunk-file dictionaries instead of
pytheia Reconstructions.  The bundle adjustment of steps 4-5 (:107-171) lives in bundle_adjust.py (SURVEY.md §8f rank
3); the returned info dict keeps the reference's keys.
All arithmetic runs in csrc/sim3.hip."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .hostmem import pinned_copy


def create_view_graph_matches(chunk_size: int, overlap_size: int) -> List[Tuple[int, int]]:
    """(ref_view_idx, qry_view_idx) pairs of the overlapping region — utils/reconstruction_alignment.py:16-37."""
    return [(chunk_size - overlap_size + i, i) for i in range(overlap_size)]


def _chunk_frame(chunk: Dict) -> Dict:
    """The chunk's data in ITS OWN frame: what the chunk file holds.  transform_chunk() stashes it on the first
    transform, so a chunk that already sits in the global frame can still be aligned on its original (fp16, chunk-frame)
    values; see align_and_refine_reconstructions."""
    return chunk.get("_chunk_frame") or chunk


def upload(t: torch.Tensor, device, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Host tensor -> device through a pinned staging buffer and an asynchronous copy on the current stream.  A copy
    from pageable memory is a synchronous call that was measured to return only when the forward running beside it on
    the compute stream had finished (the first such copy of every alignment: 250 ms of host wait per chunk, 15 ms of idle
    device before the next launch); the pinned form returns at once.  torch's host allocator keeps the staging block
    alive until the copy has run."""
    if t.device.type != "cpu" or torch.device(device).type == "cpu":
        return t.to(device) if dtype is None else t.to(device, dtype)
    # No ATen CPU operator on this path (round 5).  A dtype conversion or copy_ of >= 32 768 elements and every advanced
    # index open an OpenMP parallel region; on a box whose CPU share is a cgroup quota (16 of the host's cores) the
    # region's threads - torch sizes its pool by the HOST's core count - were seen to stall the caller for 85-110 ms,
    # one alignment in 25 (tools/dev_host_stall.py: 6 of 148 alignments, every one inside `t.to(float32)` of a
    # (60, 200, 3) tensor or `t[idx]`; gpurun_out/r5c/stall2.log).  So: a plain memcpy into the pinned staging block,
    # the asynchronous copy, and the conversion on the device (exact for the widening conversions used here).
    if not t.is_pinned():
        t = pinned_copy(t)
    out = t.to(device, non_blocking=True)
    return out if dtype is None or out.dtype == dtype else out.to(dtype)


def fresh_upload(t: torch.Tensor, device, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """A contiguous copy of `t` on `device` that a kernel may overwrite: upload(), cloned when that handed back the
    source's own memory (a tensor that already sits on `device` in `dtype`)."""
    out = upload(t, device, dtype).contiguous()
    return out.clone() if out.data_ptr() == t.data_ptr() else out


def _overlap_block(chunk: Dict[str, torch.Tensor], frames: List[int], device) -> Dict[str, torch.Tensor]:
    src = _chunk_frame(chunk)
    out = {}
    n = int(chunk["keypoints"].shape[0])
    frames = [f % n for f in frames]     # [-20 .. -1] is a run that ends AT the last view: t[-20:0] would be empty
    consecutive = all(b == a + 1 for a, b in zip(frames, frames[1:]))      # the overlap views of a chunk pair always are
    for k in ("points", "keypoints", "masks"):
        t = src[k] if k == "points" else chunk[k]
        if consecutive:          # a slice of the leading axis: contiguous memory, no index operator on the host
            out[k] = upload(t[frames[0]: frames[0] + len(frames)], device).contiguous()
        elif t.device.type == "cpu":       # a ragged view graph: gather on the device
            out[k] = upload(t, device)[torch.tensor(frames, dtype=torch.long, device=device)].contiguous()
        else:
            out[k] = t[torch.tensor(frames, dtype=torch.long, device=t.device)].contiguous()
    return out


def keypoint_weights(chunk: Dict, frames: List[int]) -> torch.Tensor:
    """w = mask * sigmoid(conf) at the keypoints of the given views, float32 [len(frames), K] on the host (SURVEY.md §7
    step 7).  conf is stored as logits (offline_chunk_creator.py:233), masks as bool (:234)."""
    idx = torch.tensor(frames, dtype=torch.long)
    conf = chunk["conf"][idx.to(chunk["conf"].device)].to(torch.float32).cpu().reshape(len(frames), -1)
    mask = chunk["masks"][idx.to(chunk["masks"].device)].cpu().reshape(len(frames), -1)
    return (torch.sigmoid(conf) * mask.to(torch.float32)).contiguous()


def _and_estimated(w: Optional[torch.Tensor], chunk: Dict, frames: List[int], device) -> Optional[torch.Tensor]:
    """Fold chunk['track_estimated'] (set by a bundle adjustment's SetOutlierTracksToUnestimated) into the pair
    validity / weights of the given views; chunks that were never adjusted have none and pass through."""
    est = chunk.get("track_estimated")
    if est is None:
        return w
    frames = [f % int(est.shape[0]) for f in frames]
    if all(b == a + 1 for a, b in zip(frames, frames[1:])):
        e = upload(est[frames[0]: frames[0] + len(frames)], device)
    else:
        e = upload(est, device)[torch.tensor(frames, dtype=torch.long, device=device)]
    e = e.reshape(len(frames), -1)
    if w is None:
        return e.to(torch.uint8).contiguous()
    return (w * e.to(w.dtype)).contiguous()


def estimate_sim3(chunk_ref: Dict, chunk_qry: Dict, view_graph_matches: List[Tuple[int, int]], device="cuda:0",
                  use_masks: bool = False, use_filter: bool = True, weights: Optional[str] = None,
                  skip_unestimated: bool = False) -> torch.Tensor:
    """Relative similarity qry -> ref from the overlap views (steps 1-3), BOTH chunks taken in their own (chunk-file)
    frames.  Returns the f64 device vector of pi3_sim3_umeyama: s, R(9), t(3), M(16), n_used, n_common, median, rms.
    The reference passes all common points unweighted (reconstruction_alignment.py:97) - the default here.
    use_masks=True lets only pairs take part whose keypoints are valid in both chunks' masks; weights='conf' is the
    weighted Umeyama with w = mask * sigmoid(conf) per keypoint (pi3_sim3_umeyama_weighted)."""
    if weights not in (None, "conf"):
        raise ValueError(f"weights={weights!r}: None or 'conf'")
    n_ref = int(chunk_ref["points"].shape[0])
    n_qry = int(chunk_qry["points"].shape[0])
    pairs = [(r, q) for (r, q) in view_graph_matches if r < n_ref and q < n_qry]
    if not pairs:
        raise ValueError("no overlapping views between the two chunks")
    ref = _overlap_block(chunk_ref, [r for r, _ in pairs], device)
    qry = _overlap_block(chunk_qry, [q for _, q in pairs], device)
    idx = ops.sim3_match_keypoints(ref["keypoints"].to(torch.float16), qry["keypoints"].to(torch.float16))
    # "last camera" of the reference reconstruction = its last view (reconstruction_alignment.py:79)
    last_pose = upload(_chunk_frame(chunk_ref)["camera_poses"][n_ref - 1], device, torch.float32).contiguous()
    w_ref = ref["masks"].reshape(len(pairs), -1).to(torch.uint8).contiguous() if use_masks else None
    w_qry = qry["masks"].reshape(len(pairs), -1).to(torch.uint8).contiguous() if use_masks else None
    # chunk-file points are fp16 and go in as they are; bundle-adjusted chunks carry refined fp32 points
    dt = torch.float16 if ref["points"].dtype == torch.float16 and qry["points"].dtype == torch.float16 else torch.float32
    if weights == "conf":
        w_ref = upload(keypoint_weights(chunk_ref, [r for r, _ in pairs]), device).contiguous()
        w_qry = upload(keypoint_weights(chunk_qry, [q for _, q in pairs]), device).contiguous()
    if skip_unestimated:
        w_ref = _and_estimated(w_ref, chunk_ref, [r for r, _ in pairs], device)
        w_qry = _and_estimated(w_qry, chunk_qry, [q for _, q in pairs], device)
    return ops.sim3_umeyama(ref["points"].to(dt), qry["points"].to(dt), idx, last_pose, w_ref, w_qry, use_filter)


def sim3_accepted(out33_cpu: torch.Tensor) -> bool:
    """The one acceptance rule of a closed-form solve, shared by the sequential and the chunk-parallel path:
    at least 3 pairs survived and every number of the similarity is finite."""
    return int(out33_cpu[29].item()) >= 3 and bool(torch.isfinite(out33_cpu[:29]).all())


def global_transform(chunk: Dict) -> torch.Tensor:
    """4x4 f64 similarity chunk frame -> global frame accumulated on this chunk (identity if never transformed)."""
    G = chunk.get("_sim3_global")
    return torch.eye(4, dtype=torch.float64) if G is None else G


def transform_chunk(chunk: Dict, M4: torch.Tensor, device="cuda:0", absolute: bool = False) -> None:
    """TransformReconstruction4 (reconstruction_alignment.py:105) on a chunk dict, in place: world points and
    cam->world poses.

    The reference holds a reconstruction in Eigen doubles and applies every Sim(3) in double
    (utils/chunk_reconstruction.py:130, reconstruction_alignment.py:105).  Here the chunk file's fp16 points are kept
    untouched under chunk['_chunk_frame']; the accumulated similarity lives in chunk['_sim3_global'] (f64) and
    chunk['points'] / ['camera_poses'] are always (accumulated similarity) x (original values), stored as fp32:
    nothing is ever re-quantised to fp16 in the global frame (ulp 1.6 cm at 16-32 m) and repeated transforms do not
    stack rounding.  absolute=True replaces the accumulated similarity by M4 instead of composing M4 with it."""
    if "_chunk_frame" not in chunk:
        chunk["_chunk_frame"] = {"points": chunk["points"], "camera_poses": chunk["camera_poses"]}
    M4 = upload(M4.detach(), device, torch.float64).reshape(4, 4).contiguous()
    if absolute or "_sim3_global" not in chunk:
        G = M4
    else:   # M4 . G_old, on the device like every other 4x4 product of the path (pi3_sim3_compose_prefix)
        G = ops.sim3_compose_prefix(torch.stack([M4.reshape(16), upload(chunk["_sim3_global"], device).reshape(16)])
                                    .contiguous())[1].reshape(4, 4)
    src = chunk["_chunk_frame"]
    pts = fresh_upload(src["points"], device, torch.float32)      # fresh fp32 copies of the originals
    poses = fresh_upload(src["camera_poses"], device, torch.float32)
    ops.sim3_apply(G.contiguous(), pts, poses)
    chunk["_sim3_global"] = G.cpu()
    chunk["points"] = pts.to(src["points"].device)
    chunk["camera_poses"] = poses.to(src["camera_poses"].device)


def apply_world_correction(chunk: Dict, D: torch.Tensor, device="cuda:0") -> None:
    """A correction D (4x4 f64 similarity, world -> world) on a finished chunk, in place: what loop closure applies.
    chunk['points'] and ['camera_poses'] move by D from their CURRENT world values (as fp32); '_sim3_global', and
    '_sim3_dense' when present, become D times what they were (pi3_sim3_compose_prefix), so the dense cloud follows
    through dense_map.chunk_transform.  '_poses_created', '_chunk_frame' and the dense cloud's rows stay as they are.
    Not transform_chunk: that rebuilds the world values from '_chunk_frame', and a chunk that was collected from another
    rank carries '_sim3_global' but no '_chunk_frame' - its world values would get the accumulated similarity twice."""
    D = upload(torch.as_tensor(D).detach().to(torch.float64).reshape(4, 4).contiguous(), device, torch.float64).contiguous()
    pts = fresh_upload(chunk["points"], device, torch.float32)
    poses = fresh_upload(chunk["camera_poses"], device, torch.float32)
    ops.sim3_apply(D, pts, poses)
    chunk["points"] = pts.to(chunk["points"].device)
    chunk["camera_poses"] = poses.to(chunk["camera_poses"].device)
    for key in ("_sim3_global", "_sim3_dense"):
        G = chunk.get(key)
        if G is None and key == "_sim3_dense":
            continue
        if G is None:            # a chunk that was never transformed sits at the identity
            chunk[key] = D.cpu().clone()
            continue
        G = upload(torch.as_tensor(G, dtype=torch.float64).reshape(16), device, torch.float64)
        chunk[key] = ops.sim3_compose_prefix(torch.stack([D.reshape(16), G]).contiguous())[1].reshape(4, 4).cpu()


def align_and_refine_reconstructions(chunk_ref: Dict, chunk_qry: Dict, view_graph_matches: List[Tuple[int, int]],
                                     use_inverse_depth: bool = False, device="cuda:0",
                                     use_masks: bool = False, bundle_adjust: Optional[Dict] = None,
                                     weights: Optional[str] = None, skip_unestimated: bool = False) -> Tuple[bool, Dict]:
    """Same contract as the reference (returns (False, {"error": ...}) instead of raising): chunk_qry is transformed
    in place into chunk_ref's frame.

    chunk_ref may already sit in the global frame (progressive alignment).  The relative similarity T (qry chunk frame
    -> ref chunk frame) is solved on both chunks' ORIGINAL fp16 values and composed with the reference's accumulated
    similarity, G_qry = G_ref . T.  For the closed-form step this equals aligning to the transformed reference (the
    match, the strict near-half filter and the Umeyama optimum are similarity-equivariant; tested), it is what the
    chunk-parallel path does, and it never feeds re-rounded global-frame points into the next solve."""
    print("🔄 Starting reconstruction alignment (closed-form Sim(3) over the overlap views)...")
    try:
        out = estimate_sim3(chunk_ref, chunk_qry, view_graph_matches, device, use_masks, weights=weights,
                            skip_unestimated=skip_unestimated)
        o = out.cpu()
        n_used = int(o[29].item())
        if not sim3_accepted(o):
            print("❌ Sim3 alignment failed")
            return False, {"error": "sim3_failed", "num_common_tracks": n_used}
        G = ops.sim3_compose_prefix(torch.stack([upload(global_transform(chunk_ref).reshape(16), device),
                                                 out[13:29]]).contiguous())[1].reshape(4, 4)
        transform_chunk(chunk_qry, G, device, absolute=True)
        info = {"success": True, "num_common_tracks": n_used,
                "sim3_summary": {"success": True, "alignment_error": float(o[32].item()), "scale": float(o[0].item()),
                                 "matrix": o[13:29].reshape(4, 4).clone(), "global_matrix": G.cpu().clone()},
                "priors_set": 0, "bundle_adjustment": None}
        if bundle_adjust is not None:
            # steps 4-5 (reconstruction_alignment.py:107-171): pose priors on the overlap views from the reference
            # chunk, 50 LM iterations with Huber 3.0, outlier tracks; the refined values become the chunk's new frame
            from .bundle_adjust import AFTER_ALIGNMENT, bundle_adjust_chunk, overlap_priors
            priors = overlap_priors(chunk_ref, view_graph_matches)
            settings = dict(AFTER_ALIGNMENT, **bundle_adjust.get("settings", {}))
            if use_inverse_depth:      # reconstruction_alignment.py:147-149
                settings["inverse_depth"] = True
            ba = bundle_adjust_chunk(chunk_qry, bundle_adjust["width"], bundle_adjust["height"],
                                     bundle_adjust.get("max_observations_per_track", 5), device, settings, priors,
                                     release_observations=True)     # a chunk's last adjustment: free ~18 MB of HBM
            info["priors_set"] = len(priors)
            info["bundle_adjustment"] = ba
            if ba.get("success"):
                print(f"   Bundle adjustment completed: Success=True, Final cost={ba['final_cost']:.6f}; "
                      f"removed {ba['removed_tracks']} tracks")
                chunk_qry["_chunk_frame"] = {"points": chunk_qry["points"], "camera_poses": chunk_qry["camera_poses"]}
                chunk_qry["_sim3_dense"] = chunk_qry["_sim3_global"]     # the dense cloud keeps the closed-form similarity
                chunk_qry["_sim3_global"] = torch.eye(4, dtype=torch.float64)
            else:    # rejected by the sanity gate or failed numerically: the chunk keeps its closed-form alignment
                     # (points / poses untouched, frame bookkeeping unchanged); the caller sees it in the info dict
                print(f"   ⚠️  prior-constrained bundle adjustment NOT applied "
                      f"({ba.get('rejected') or ba.get('reason') or 'numerical failure'}); closed-form alignment kept")
        return True, info
    except Exception as e:  # noqa: BLE001 - the reference swallows and reports (reconstruction_alignment.py:194-198)
        print(f"❌ Complete reconstruction alignment failed: {e}")
        return False, {"error": "exception", "message": str(e)}
