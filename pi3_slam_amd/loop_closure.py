"""Loop closure of stage 2 (opt-in): the chunks that see the same surface are found on the geometry, measured against
each other by ICP and reconciled with the chain in a Sim(3) pose graph.

  candidates  every chunk's dense cloud moved to the world by its similarity (dense_map.chunk_transform); ONE
              pi3_chunk_cooccupancy call (csrc/chunk_overlap.hip) counts, for every pair of chunks, the cells of edge
              `loop_cell` both occupy: overlap(i, j) = counts[i][j] / min(counts[i][i], counts[j][j]);
  edges       map_eval.icp_refine of cloud j on cloud i from the chain's own relative similarity, its steps truncated to
              the directions the surfaces hold (ICP_TRUNCATE below); accepted when the ICP
              ended converged or at its iteration limit, paired loop_min_pair_fraction of the smaller cloud, its rms is
              within loop_max_rms and it moved the cloud by no more than loop_max_dist (rms) from the chain's placement;
  weights     pair_information: the ICP normal matrix A of the edge at its measurement, O = A / sigma^2 with
              sigma^2 = max(r2 / pairs, (1e-3 x the rms radius of cloud i)^2): an edge is weighted down by its own misfit,
              and an exact fit does not get infinite weight.  A loop edge's A is the point-to-plane one its ICP solved:
              it says nothing where the surfaces hold nothing.  Sequential edges carry the chain's result as their
              measurement (their residual starts at zero); that came from keypoints, which hold all seven parameters,
              so their A is the point-to-point one (full rank), weighted by the point-to-point misfit of the clouds;
  solve       pi3_pose_graph_sim3 (csrc/pose_graph.hip), the first participant fixed;
  apply       alignment.apply_world_correction moves every chunk by D_c = W'_c W_c^-1.

A chunk takes part when it has a non-empty dense cloud and its alignment succeeded.  Sequential edges join consecutive
participants (so the graph stays connected when a chunk in between takes no part); a chunk that takes no part is moved
with the nearest earlier participant.  DESIGN.md 7e has the method and what was measured."""
from __future__ import annotations

import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import map_eval, ops
from .alignment import apply_world_correction
from .dense_map import chunk_transform

DEFAULTS = dict(loop_min_gap=2, loop_min_overlap=0.3, loop_max_edges=3, loop_max_dist=0.1, loop_max_rms=0.03,
                loop_min_pair_fraction=0.2, loop_cell=0.16)
SOLVER_ITERATIONS = 50
SIGMA_FLOOR = 1e-3          # of the rms radius of the reference cloud
# The ICP of a loop edge steps only along directions that the surfaces hold at least this fraction as firmly as the
# best-held one (map_eval.icp_refine(truncate=...)).  Measured on the chess room: the unit-diagonal normal
# matrix of a chunk pair has five or six eigenvalues of 0.1 .. 1 and one or two of 6e-6 .. 2e-4 times the largest (the
# scaling about the point where the walls and the floor meet, a slide along a lone edge); 1e-3 lies in the gap.
ICP_TRUNCATE = 1e-3
# A correction smaller than the solver's own stopping tolerance (max |step| < 1e-9, csrc/pose_graph.hip) is below what the
# solve resolves, and far below the fp32 values it would be applied to: such a chunk is left exactly as it is.
MIN_CORRECTION = 1e-9


def similarity_scale(M: np.ndarray) -> float:
    return float(np.cbrt(np.linalg.det(M[:3, :3])))


def _centroid(points: torch.Tensor) -> np.ndarray:
    ok = torch.isfinite(points).all(1)
    return points[ok].double().mean(0).cpu().numpy() if bool(ok.any()) else np.zeros(3)


def _rms_displacement(points: torch.Tensor, A, B, device) -> float:
    """The rms distance between A p and B p over the finite rows of a cloud (f32 (n,3) on the device; A, B 4x4)."""
    out = []
    for M in (A, B):
        moved = points.clone()
        if int(moved.shape[0]):
            ops.sim3_apply(torch.from_numpy(np.ascontiguousarray(M, np.float64)).to(device).contiguous(), moved, None)
        out.append(moved.double())
    d2 = ((out[0] - out[1]) ** 2).sum(1)
    d2 = d2[torch.isfinite(d2)]
    return float(d2.mean().sqrt()) if int(d2.numel()) else float("inf")


def pair_information(cloud_j: Dict, cloud_i: Dict, Z, *, max_dist: float, device="cuda",
                     index: Optional[map_eval.CloudIndex] = None) -> Dict:
    """The normal matrix of the ICP between cloud j, moved by Z (chunk j's frame -> chunk i's), and cloud i, at Z: one
    ops.sim3_apply, one CloudIndex.nearest_into and one ops.cloud_pair_equations in the mode the clouds allow (point to
    plane on cloud i's normals, else on cloud j's rotated ones, else point to point).  Nothing is solved.
    clouds: {'points': (n,3), 'normals': (n,3) or absent}.  -> A (7,7), pairs, r2, centre (the f64 centroid of cloud i),
    radius (the rms distance of cloud i from it)."""
    dev = torch.device(device)
    pi = map_eval._device_points(cloud_i["points"], dev)
    moved = map_eval._device_points(cloud_j["points"], dev).clone()
    Z = np.asarray(Z, np.float64).reshape(4, 4)
    m = int(moved.shape[0])
    if m:
        ops.sim3_apply(torch.from_numpy(Z).to(dev).contiguous(), moved, None)
    if index is None:
        index = map_eval.CloudIndex(pi, max_dist, dev)
    centre = _centroid(pi)
    ok = torch.isfinite(pi).all(1)
    radius = float(((pi[ok].double() - torch.from_numpy(centre).to(dev)) ** 2).sum(1).mean().sqrt()) if bool(ok.any()) else 0.0
    normals, normals_of, Rn = None, 0, None
    if cloud_i.get("normals") is not None:
        normals, normals_of = map_eval._device_normals(cloud_i["normals"], int(pi.shape[0]), dev), 1
    elif cloud_j.get("normals") is not None:
        normals, normals_of, Rn = map_eval._device_normals(cloud_j["normals"], m, dev), 2, map_eval._rotation_of(Z)
    d2 = torch.empty(m, dtype=torch.float64, device=dev)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    nn_counters = torch.zeros(4, dtype=torch.int64, device=dev)
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    partials = torch.empty((ops.cloud_icp_partial_rows(m), ops.CLOUD_ICP_DOUBLES), dtype=torch.float64, device=dev)
    out = torch.zeros(ops.CLOUD_ICP_DOUBLES, dtype=torch.float64, device=dev)
    index.nearest_into(moved, d2, idx, nn_counters)
    ops.cloud_pair_equations(moved, index.points, idx, d2, index.max_dist, centre, normals, normals_of, Rn, partials, out,
                             counters)
    A, _, r2, _ = map_eval.unpack_equations(out.cpu().numpy())
    return {"A": A, "pairs": int(counters[0]), "r2": r2, "centre": centre, "radius": radius}


def edge_information(pi: Dict) -> Optional[np.ndarray]:
    """O = A / sigma^2 of a pair_information result, sigma^2 = max(r2 / pairs, (SIGMA_FLOOR x the rms radius of cloud
    i)^2); None below map_eval.ICP_MIN_PAIRS pairs."""
    if pi["pairs"] < map_eval.ICP_MIN_PAIRS:
        return None
    sigma2 = max(pi["r2"] / pi["pairs"], (SIGMA_FLOOR * pi["radius"]) ** 2)
    return pi["A"] / sigma2 if sigma2 > 0.0 and np.isfinite(pi["A"]).all() else None


def select_candidates(counts: np.ndarray, min_gap: int, min_overlap: float, max_edges: int) -> List[Dict]:
    """counts (n,n) of the participants in chunk order -> every pair with j - i >= min_gap and overlap >= min_overlap,
    sorted by (-overlap, i, j), 'taken' greedily while neither chunk has max_edges loop edges yet."""
    n = len(counts)
    found = []
    for i in range(n):
        for j in range(i + int(min_gap), n):
            low = min(int(counts[i][i]), int(counts[j][j]))
            ov = int(counts[i][j]) / low if low else 0.0
            if ov >= float(min_overlap):
                found.append({"i": i, "j": j, "overlap": ov, "shared_cells": int(counts[i][j])})
    found.sort(key=lambda c: (-c["overlap"], c["i"], c["j"]))
    used = [0] * n
    for c in found:
        c["taken"] = used[c["i"]] < max_edges and used[c["j"]] < max_edges
        if c["taken"]:
            used[c["i"]] += 1
            used[c["j"]] += 1
        else:
            c["outcome"] = "chunk_has_max_edges"
    return found


def cooccupancy(worlds: List[torch.Tensor], cell: float, device) -> Dict:
    """worlds: every participant's cloud in the world frame -> counts (n,n) and the kernel's counters."""
    dev = torch.device(device)
    pts = torch.cat(worlds).contiguous()
    sizes = [int(w.shape[0]) for w in worlds]
    offsets = torch.tensor(np.r_[0, np.cumsum(sizes)], dtype=torch.int64, device=dev)
    n = len(worlds)
    table = torch.empty(ops.voxel_capacity(int(pts.shape[0])) * 8, dtype=torch.int64, device=dev)
    counts = torch.empty((n, n), dtype=torch.int64, device=dev)
    counters = torch.empty(4, dtype=torch.int64, device=dev)
    inv_cell = float(np.float32(1.0 / float(cell)))
    ops.chunk_cooccupancy(pts, offsets, inv_cell, table, counts, counters)
    return {"counts": counts.cpu().numpy(), "counters": dict(zip(ops.CHUNK_OVERLAP_COUNTERS, (int(v) for v in counters.tolist())))}


def _decompose(D: np.ndarray, about: np.ndarray) -> Dict:
    """A correction in figures: how far it moves the point `about` (the cloud's world centroid), its angle, its scale."""
    s = similarity_scale(D)
    R = D[:3, :3] / s
    angle = float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))
    return {"translation": float(np.linalg.norm(D[:3, :3] @ about + D[:3, 3] - about)), "rotation_deg": angle, "scale": s}


def close_loops(chunks: List[Dict], device="cuda", **options) -> Dict:
    """Runs on the finished chunks of stage 2 (in place) -> info: the options, the participants, the co-occupancy
    counters, every candidate with its overlap and outcome, every accepted edge with Z, pairs and rms, the solver's out,
    and per chunk the correction's translation, rotation (deg) and scale.  info['applied'] says whether any chunk
    moved; info['skipped'] why nothing was tried."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"close_loops: unknown options {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    dev = torch.device(device)
    t0 = time.time()
    info: Dict = {"options": dict(opt), "participants": [], "candidates": [], "edges": [], "applied": False, "skipped": None}
    part = [c for c, ch in enumerate(chunks)
            if ch.get("dense_cloud") is not None and int(ch["dense_cloud"]["points"].shape[0]) > 0 and ch.get("alignment_ok", True)]
    info["participants"] = part
    if len(part) < 3:
        info["skipped"] = "fewer_than_three_participants"
        print(f"   ℹ️  Loop closure: {len(part)} of {len(chunks)} chunks carry a dense cloud and an alignment; nothing to do")
        return info
    n = len(part)
    W = [chunk_transform(chunks[c]).numpy().astype(np.float64) for c in part]
    clouds, worlds = [], []
    for k, c in enumerate(part):
        cl = chunks[c]["dense_cloud"]
        pts = map_eval._device_points(torch.as_tensor(cl["points"]), dev)
        clouds.append({"points": pts, "normals": None if cl.get("normals") is None
                       else map_eval._device_normals(torch.as_tensor(cl["normals"]), int(pts.shape[0]), dev)})
        world = pts.clone()
        ops.sim3_apply(torch.from_numpy(W[k]).to(dev).contiguous(), world, None)
        worlds.append(world)
    co = cooccupancy(worlds, opt["loop_cell"], dev)
    info["cooccupancy_counters"] = co["counters"]
    info["candidates"] = select_candidates(co["counts"], opt["loop_min_gap"], opt["loop_min_overlap"], opt["loop_max_edges"])
    scales = [similarity_scale(M) for M in W]

    def pair(i, j):
        """Clouds i and j as the pair uses them: point to plane when both carry normals, else the points alone."""
        plane = clouds[i]["normals"] is not None and clouds[j]["normals"] is not None
        return plane, (clouds[i] if plane else {"points": clouds[i]["points"]}), \
            (clouds[j] if plane else {"points": clouds[j]["points"]})

    # ---- measure the candidates
    graph = []       # (i, j, Z, information, centre)
    for cand in info["candidates"]:
        if not cand["taken"]:
            continue
        i, j = cand["i"], cand["j"]
        cand["chunks"] = [part[i], part[j]]
        md = float(opt["loop_max_dist"]) / scales[i]
        init = np.linalg.inv(W[i]) @ W[j]
        plane, ci, cj = pair(i, j)
        icp = map_eval.icp_refine(cj["points"], ci["points"], mode="plane" if plane else "point",
                                  ref_normals=ci.get("normals"), with_scale=True, max_dist=md, init=init, device=dev,
                                  truncate=ICP_TRUNCATE)
        last = icp["history"][-1] if icp["history"] else {"pairs": 0, "rms": None}
        smaller = min(int(clouds[i]["points"].shape[0]), int(clouds[j]["points"].shape[0]))
        rms = None if last["rms"] is None else last["rms"] * scales[i]
        cand.update(status=icp["status"], iterations=icp["iterations"], pairs=last["pairs"], rms=rms)
        if icp["status"] not in ("converged", "max_iterations"):
            cand["outcome"] = "icp_" + icp["status"]
        elif last["pairs"] < float(opt["loop_min_pair_fraction"]) * smaller:
            cand["outcome"] = "too_few_pairs"
        elif rms is None or not rms <= float(opt["loop_max_rms"]):
            cand["outcome"] = "rms_above_limit"
        elif not _rms_displacement(cj["points"], init, icp["transform"], dev) * scales[i] <= float(opt["loop_max_dist"]):
            # a drift beyond the search radius is not what this closes: an ICP that walked farther than that from the
            # chain's own placement slid along what the surfaces leave free, whatever its rms says
            cand["outcome"] = "moved_beyond_max_dist"
        else:
            Z = icp["transform"]
            pinfo = pair_information(cj, ci, Z, max_dist=md, device=dev)
            O = edge_information(pinfo)
            if O is None:
                cand["outcome"] = "no_information"
                continue
            cand["outcome"] = "accepted"
            graph.append((i, j, Z, O, pinfo["centre"]))
            info["edges"].append({"chunks": [part[i], part[j]], "Z": Z.tolist(), "pairs": last["pairs"], "rms": rms,
                                  "overlap": cand["overlap"]})
            print(f"   🔁 Loop edge {part[i]} <- {part[j]}: overlap {cand['overlap']:.2f}, {last['pairs']} pairs, "
                  f"rms {rms:.4f}")
    n_loop = len(graph)
    if n_loop == 0:
        info["seconds"] = time.time() - t0
        print(f"   ℹ️  Loop closure: {len(info['candidates'])} candidates, no loop edge accepted; the chain stays as it is")
        return info

    # ---- the chain's own edges between consecutive participants
    seq, missing = [], []
    for k in range(1, n):
        Z = np.linalg.inv(W[k - 1]) @ W[k]
        md = float(opt["loop_max_dist"]) / scales[k - 1]
        # point to point (the clouds without their normals): the chain's measurement holds every direction, and a
        # point-to-plane A would leave the graph soft exactly where the loop edges are silent
        pinfo = pair_information({"points": clouds[k]["points"]}, {"points": clouds[k - 1]["points"]}, Z, max_dist=md,
                                 device=dev)
        O = edge_information(pinfo)
        seq.append([k - 1, k, Z, O, pinfo["centre"]])
        if O is None:
            missing.append(len(seq) - 1)
    have = [e[3] for e in seq if e[3] is not None]
    if not have:
        info["skipped"] = "no_sequential_information"
        info["seconds"] = time.time() - t0
        print("   ℹ️  Loop closure: no sequential edge has an information matrix; skipped")
        return info
    weakest = min(have, key=lambda O: float(np.trace(O)))
    for q in missing:
        seq[q][3] = weakest
    info["sequential_edges_without_pairs"] = len(missing)
    graph = [tuple(e) for e in seq] + graph

    # ---- solve
    E = len(graph)
    nodes = torch.from_numpy(np.stack(W)).to(dev).contiguous()
    centres = np.stack([W[k][:3, :3] @ _centroid(clouds[k]["points"]) + W[k][:3, 3] for k in range(n)])
    tri = np.triu_indices(7)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    out = ops.pose_graph_sim3(nodes, torch.from_numpy(centres).to(dev).contiguous(),
                              torch.tensor([[e[0], e[1]] for e in graph], dtype=torch.int32, device=dev).contiguous(),
                              torch.from_numpy(np.stack([e[2] for e in graph])).to(dev).contiguous(),
                              torch.from_numpy(np.stack([e[4] for e in graph])).to(dev).contiguous(),
                              torch.from_numpy(np.stack([e[3][tri] for e in graph])).to(dev).contiguous(),
                              torch.from_numpy(fixed).to(dev), SOLVER_ITERATIONS).cpu().numpy()
    solver = dict(zip(ops.POSE_GRAPH_OUT, (float(v) for v in out[:6])))
    solver["status"] = ops.POSE_GRAPH_STATUS[int(out[5])]
    info["solver"] = solver
    W_new = nodes.cpu().numpy()

    # ---- apply: D_c = W'_c W_c^-1; the fixed node and everything before it stay exactly where they are
    D_of = {part[0]: (None, centres[0])}
    for k in range(1, n):
        D = W_new[k] @ np.linalg.inv(W[k]) if solver["status"] != "factorisation_failed" else None
        if D is not None:
            d = _decompose(D, centres[k])
            if max(d["translation"], np.radians(d["rotation_deg"]), abs(np.log(d["scale"]))) < MIN_CORRECTION:
                D = None
        D_of[part[k]] = (D, centres[k])
    current, about = None, None
    info["corrections"] = []
    for c, chunk in enumerate(chunks):
        if c in D_of:
            current, about = D_of[c]
        if c < part[0] or current is None:
            info["corrections"].append({"chunk": c, "translation": 0.0, "rotation_deg": 0.0, "scale": 1.0})
            continue
        apply_world_correction(chunk, torch.from_numpy(current), dev)
        info["corrections"].append(dict(_decompose(current, about), chunk=c))
        info["applied"] = True
    info["seconds"] = time.time() - t0
    worst = max(info["corrections"], key=lambda d: d["translation"])
    print(f"   🔁 Loop closure: {len(info['candidates'])} candidates, {n_loop} loop edges + {n - 1} sequential; cost "
          f"{solver['initial_cost']:.6g} -> {solver['final_cost']:.6g} in {int(solver['iterations'])} iterations "
          f"({solver['status']}); largest correction {worst['translation']:.4f} at chunk {worst['chunk']}; "
          f"{info['seconds']:.2f} s")
    return info
