"""Cost of the dense voxel map (pi3_slam_amd/dense_map.py, csrc/voxel.hip) at the bench workload.

  1. the kernels of one 100 x 308 x 406 chunk (the chess-room scene's maps with the creator's masks, 2 cm voxels):
     clear / fuse_pixels / extract, HIP events, median of 20 after 3 warm-up runs;
  2. creator frames/s with the dense map on and off: two OfflineChunkCreators on the same recipe engine (bench.py's
     mask edit, device resize of 512x384 uint8 frames, grid keypoints), alternated in one process, 4 chunks per leg after
     one warm-up chunk per creator, 3 rounds (dense confidence threshold 0.05: see --conf-threshold).

  3. --consistency: the multi-view depth consistency filter (csrc/dense_filter.hip) with its defaults on the same
     100 x 308 x 406 chunk (the scene's true intrinsics), HIP events, median of 20 after 3 warm-up runs, with the bytes
     it must move (pass A: mask 1 + conf 4 + points 12 + local z 4 read, zplane 4 written; pass B: zplane 4 read, mask 1
     written, and per candidate its point 12 and one 4-byte gather per neighbour in range) and the rate that gives
     against the 8 TB/s HBM figure of profiles/ - a lower bound of the traffic: local z sits at a 12-byte stride, so
     whole lines of local_points are fetched (about 12 B per pixel, not 4), and a gather fetches a line, not 4 bytes; and the creator leg a third time with the filter on.

  4. --clean: the map-cleaning filters (csrc/voxel_clean.hip, dense_map.MapCleaner) on the table of leg 1 and on a
     synthetic map of about 1 M voxels (the six faces of a 410-voxel box and 1 % floaters inside it), HIP events, median
     of 20 after 3 warm-up runs: the support kernel at radius 1 and 2 (min_support 4: it probes), the labelling in total
     (label init, the host's sweep loop with its reads of the `changed` words, sizes, the component filter) with its
     sweep count, and the masked extract; with the counted bytes of the support kernel (26 or 124 probes of a 64-byte
     slot per eligible voxel, the first slot of each probe chain only) and the rate they give.

  5. --normals: the surface normals (csrc/voxel_normals.hip): fuse_pixel_normals and extract_normals beside fuse_pixels
     and extract in the same run of leg 1 (the zeroing of the 32-byte-per-slot side array as well), with the counters;
     and a creator leg with dense_normals on.

  6. --mesh: the surface mesh (csrc/voxel_mesh.hip, dense_map.MapMesher) on the table of leg 1 with its pixel normals
     and on the synthetic box map of leg 4 (outward normals on the faces, none on the floaters), HIP events, median of
     20 after 3 warm-up runs: the cell insert (with the clearing of the cell table), the vertex kernel and the
     extraction at the cell-table size MapMesher grows to, beside voxel_support at radius 1 on the same table; with the
     counters, the cell table's bytes and, for the vertex kernel, the counted bytes (27 probes of a 64-byte slot per
     cell, the first slot of each chain only, 32 B of normal sums per source found, the 8-byte key read and the 32-byte
     vertex written per slot) and the rate they give.

  7. --carve: the carving with depth keyframes (csrc/voxel_carve.hip, dense_map.MapCarver) on the table of leg 1 with
     the planes of 500 views (the chunk's own 50 keyframes at K = 2, S = 2 and the scene's true intrinsics, ten times
     over) and on the synthetic box map of leg 4 with 500 cameras inside the box that each see a constant-depth plane,
     HIP events, median of 20 after 3 warm-up runs, beside voxel_support at radius 1 in the same run; the depth-plane
     kernel (csrc/dense_filter.hip) on the chunk; and a creator leg with dense_depth_every = 2.

Prints one JSON line.  Usage: python tools/dense_fusion_timing.py [--voxel 0.02] [--rounds 3] [--chunks 4] [--consistency] [--clean] [--normals] [--mesh] [--carve]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CL, OV, SRC_H, SRC_W, H, W, KP = 100, 20, 384, 512, 308, 406, 200


def synthetic_frames_u8(n: int, h: int, w: int, seed: int) -> torch.Tensor:
    """bench.py's frames: smooth low-frequency structure + noise, uint8 [n, h, w, 3], pinned."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h)[None, :, None, None]
    xx = torch.linspace(0, 1, w)[None, None, :, None]
    ph = torch.rand(n, 1, 1, 3, generator=g) * 6.28
    img = 0.5 + 0.25 * torch.sin(7 * xx + 3 * yy + ph) * torch.cos(5 * yy - ph) + 0.1 * torch.rand(n, h, w, 3, generator=g)
    return (img.clamp(0, 1) * 255).to(torch.uint8).contiguous().pin_memory()


def clean_times(fz, reps: int = 20):
    """The cleaning stages on a filled VoxelFuser (min_support 4, min_component 50; starting points, not optima)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapCleaner
    cl = MapCleaner(min_support=4, min_component=50)
    dev, cap = fz.device, fz.capacity
    keep = torch.empty(cap, dtype=torch.uint8, device=dev)
    counters = torch.zeros(8, dtype=torch.int64, device=dev)
    size = torch.empty(cap, dtype=torch.int32, device=dev)
    t = {"support_r1_ms": [], "support_r2_ms": [], "labelling_ms": [], "extract_kept_ms": []}
    sweeps = 0
    for i in range(3 + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        ops.voxel_support(fz.table, 1, 2, 4, keep, None, counters)
        e[1].record()
        ops.voxel_support(fz.table, 1, 1, 4, keep, None, counters)
        e[2].record()
        label, sweeps = cl.label_components(fz, keep, int(counters[2].item()))
        ops.voxel_component_sizes(fz.table, label, size)
        ops.voxel_component_filter(fz.table, label, size, cl.min_component, keep, counters)
        e[3].record()
        fz.extract_async(keep)
        e[4].record()
        torch.cuda.synchronize()
        if i >= 3:
            for k, (a, b) in zip(("support_r2_ms", "support_r1_ms", "labelling_ms", "extract_kept_ms"), zip(e, e[1:])):
                t[k].append(a.elapsed_time(b))
    c = dict(zip(ops.VOXEL_CLEAN_COUNTERS, (int(x) for x in counters.tolist())))
    res = {k: float(np.median(v)) for k, v in t.items()} | {k + "_minmax": [float(np.min(v)), float(np.max(v))]
                                                           for k, v in t.items()}
    for r, cells in ((1, 26), (2, 124)):
        b = c["eligible"] * cells * 64 + cap * 16
        res[f"support_r{r}_bytes"] = b
        res[f"support_r{r}_TBps"] = b / (res[f"support_r{r}_ms"] * 1e-3) / 1e12
    return res | {"sweeps": sweeps, "table_slots": cap, "side_bytes_per_slot": 1 + 8 + 4, **c}


def mesh_times(fz, nacc, reps: int = 20):
    """The mesh kernels on a filled VoxelFuser with its normal sums, at the cell-table size MapMesher settles on."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapMesher
    mesher = MapMesher()
    mesher.apply(fz, nacc)
    st = dict(mesher.last_stats)
    dev, cap, ccap = fz.device, fz.capacity, st["cell_capacity"]
    cells = torch.empty(ccap, dtype=torch.int64, device=dev)
    verts = torch.empty(ccap, ops.VOXEL_MESH_VERT_WORDS, dtype=torch.int32, device=dev)
    stats = torch.zeros(12, dtype=torch.int64, device=dev)
    keep = torch.empty(cap, dtype=torch.uint8, device=dev)
    counters = torch.zeros(8, dtype=torch.int64, device=dev)
    t = {"cell_insert_ms": [], "vertices_ms": [], "extract_ms": [], "support_r1_ms": []}
    for i in range(3 + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        ops.voxel_mesh_cells(fz.table, nacc, None, cells, stats)
        e[1].record()
        ops.voxel_mesh_vertices(fz.table, nacc, None, cells, verts, fz.voxel_size, stats)
        e[2].record()
        ops.voxel_mesh_extract(cells, verts, st["vertices"], st["quads"], stats)
        e[3].record()
        ops.voxel_support(fz.table, 1, 1, 4, keep, None, counters)
        e[4].record()
        torch.cuda.synchronize()
        if i >= 3:
            for k, (a, b) in zip(t, zip(e, e[1:])):
                t[k].append(a.elapsed_time(b))
    res = {k: float(np.median(v)) for k, v in t.items()} | {k + "_minmax": [float(np.min(v)), float(np.max(v))]
                                                           for k, v in t.items()}
    c = dict(zip(ops.VOXEL_CLEAN_COUNTERS, (int(x) for x in counters.tolist())))
    vb = st["cells"] * 27 * 64 + st["sources"] * 27 * 32 + ccap * (8 + 32)
    sb = c["eligible"] * 26 * 64 + cap * 16
    return res | st | {"table_slots": cap, "voxels": c["voxels"], "vertices_bytes": vb,
                       "vertices_TBps": vb / (res["vertices_ms"] * 1e-3) / 1e12, "support_r1_bytes": sb,
                       "support_r1_TBps": sb / (res["support_r1_ms"] * 1e-3) / 1e12}


def carve_times(fz, views: np.ndarray, planes: torch.Tensor, stride: int, reps: int = 20):
    """pi3_voxel_carve on a filled VoxelFuser (min_conflicts 3, MapCarver's tolerance and margin) beside voxel_support at
    radius 1; views f64 (M,20) on the host, planes fp16 (M,H',W') on the device."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapCarver
    dev, cap = fz.device, fz.capacity
    v = torch.from_numpy(views).to(dev).contiguous()
    carved = torch.empty(cap, dtype=torch.uint8, device=dev)
    keep = torch.empty(cap, dtype=torch.uint8, device=dev)
    cc = torch.zeros(4, dtype=torch.int64, device=dev)
    counters = torch.zeros(8, dtype=torch.int64, device=dev)
    t = {"carve_ms": [], "support_r1_ms": []}
    for i in range(3 + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        ops.voxel_carve(fz.table, fz.voxel_size, v, planes, stride, 0.03, MapCarver.MARGIN_VOXELS * fz.voxel_size, 3, carved,
                        None, None, cc)
        e[1].record()
        ops.voxel_support(fz.table, 1, 1, 4, keep, None, counters)
        e[2].record()
        torch.cuda.synchronize()
        if i >= 3:
            for k, (a, b) in zip(t, zip(e, e[1:])):
                t[k].append(a.elapsed_time(b))
    res = {k: float(np.median(x)) for k, x in t.items()} | {k + "_minmax": [float(np.min(x)), float(np.max(x))]
                                                           for k, x in t.items()}
    st = dict(zip(ops.VOXEL_CARVE_COUNTERS, (int(x) for x in cc.tolist())))
    return res | st | {"views": int(len(views)), "plane_shape": list(planes.shape[1:]), "pixel_stride": stride,
                       "plane_stack_bytes": int(planes.numel()) * 2, "table_slots": cap,
                       "ns_per_voxel_and_view": 1e6 * res["carve_ms"] / max(1, st["voxels"] * len(views))}


def box_views(voxel: float, dev: str, side: int = 410, M: int = 500, Hp: int = 154, Wp: int = 203, seed: int = 1):
    """M cameras inside the synthetic box, looking around its vertical axis, each with a constant-depth plane (a
    quarter of the box's side): timing input only."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.render import pack_cameras
    rng = np.random.default_rng(seed)
    half = 0.5 * side * voxel
    poses = np.tile(np.eye(4), (M, 1, 1))
    yaw = rng.uniform(0, 2 * np.pi, M)
    poses[:, 0, 0], poses[:, 0, 2], poses[:, 2, 0], poses[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    poses[:, :3, 3] = rng.uniform(-0.5 * half, 0.5 * half, (M, 3))
    K = np.array([[0.9 * 2 * Wp, 0, Wp - 0.5], [0, 0.9 * 2 * Wp, Hp - 0.5], [0, 0, 1.0]])
    views = pack_cameras(poses, K)
    views[:, ops.CARVE_DEPTH_SCALE_AT] = 1.0
    planes = torch.full((M, Hp, Wp), 0.5 * half, dtype=torch.float16, device=dev)
    return views, planes


def synthetic_box_map(voxel: float, dev: str, side: int = 410, seed: int = 0, normals: bool = False):
    """About 1 M voxels: the six faces of a box of `side` voxels, one point per voxel, and 1 % floaters inside.
    normals: -> (the fuser, its NormalAccumulator) with the faces' outward normals; the floaters carry none."""
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    g = torch.Generator().manual_seed(seed)
    a = torch.arange(side)
    u, v = (x.reshape(-1) for x in torch.meshgrid(a, a, indexing="ij"))
    faces = []
    for axis in range(3):
        for w in (0, side - 1):
            f = [u, v]
            f.insert(axis, torch.full_like(u, w))
            faces.append(torch.stack(f, 1))
    idx = torch.cat(faces + [torch.randint(1, side - 1, (6 * side * side // 100, 3), generator=g)]) - side // 2
    pts = ((idx.double() + 0.5) * voxel).float().to(dev).contiguous()
    fz = VoxelFuser(voxel, dev)
    fz.fuse_points(pts, None, None)
    if not normals:
        return fz
    n = side * side
    nrm = torch.zeros(len(idx), 3)
    for j in range(6):
        nrm[j * n:(j + 1) * n, j // 2] = -1.0 if j % 2 == 0 else 1.0
    nw = torch.zeros(len(idx), dtype=torch.int32)
    nw[:6 * n] = 1
    acc = NormalAccumulator(fz)
    acc.clear()
    acc.add_points(pts, nrm.to(dev).contiguous(), nw.to(dev).contiguous(),
                   torch.eye(3, dtype=torch.float64, device=dev).reshape(9).contiguous())
    return fz, acc


def kernel_times(voxel: float, dev: str, reps: int = 20, clean: bool = False, normals: bool = False,
                 mesh: bool = False, carve: bool = False):
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator
    from pi3_slam_amd.dense_map import NormalAccumulator, VoxelFuser
    seq = ss.SyntheticSequence(os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt"), noise=dict(ss.NOISE_BF16))
    imgs = seq.frames(1, dev)
    out = ss.SceneEngine(seq)(imgs)
    masks = OfflineChunkCreator._compute_masks(out)[0].contiguous()
    pts, conf, im = out["points"][0].contiguous(), out["conf"][0].contiguous(), imgs[0].contiguous()
    fz = VoxelFuser(voxel, dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    t = {"clear_ms": [], "fuse_pixels_ms": [], "extract_ms": []}
    if normals:
        t.update(normals_clear_ms=[], fuse_pixel_normals_ms=[], extract_normals_ms=[])
    acc = NormalAccumulator(fz) if normals else None
    for i in range(3 + reps):
        e = [ev() for _ in range(7 if normals else 4)]
        e[0].record()
        fz.clear()
        e[1].record()
        fz.fuse_pixels(pts, conf, masks, im, 0.5)
        e[2].record()
        fz.extract_async()
        e[3].record()
        if normals:
            acc.clear()
            e[4].record()
            acc.add_pixels(pts, conf, masks, 0.5)
            e[5].record()
            acc.extract_async()
            e[6].record()
        torch.cuda.synchronize()
        if i >= 3:
            for k, (a, b) in zip(t, zip(e, e[1:])):
                t[k].append(a.elapsed_time(b))
    res = fz.extract()
    out = {k: float(np.median(v)) for k, v in t.items()} | {
        "voxels": len(res["keys"]), "pixels": int(pts.numel() // 3), "masked_in": int(masks.sum()),
        "table_slots": fz.capacity, "table_bytes": fz.capacity * 64}
    if normals:
        acc.extract()
        out["normals"] = dict(acc.last_stats, nacc_bytes=fz.capacity * 32,
                              minmax_ms={k: [float(np.min(v)), float(np.max(v))] for k, v in t.items()})
    if clean:
        out["clean"] = clean_times(fz, reps)
    if mesh:
        if acc is None:
            acc = NormalAccumulator(fz)
            acc.clear()
            acc.add_pixels(pts, conf, masks, 0.5)
        out["mesh"] = mesh_times(fz, acc.nacc, reps)
    if carve:
        from pi3_slam_amd import ops
        from pi3_slam_amd.dense_map import conf_logit_threshold
        from pi3_slam_amd.render import pack_cameras
        lp = ss.SceneEngine(seq)(imgs)["local_points"][0].contiguous()
        m8 = masks.view(torch.uint8)
        ms = []
        for i in range(3 + reps):
            a, b = ev(), ev()
            a.record()
            planes, count = ops.dense_depth_planes(pts, lp, conf, m8, conf_logit_threshold(0.5), 2, 2)
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(a.elapsed_time(b))
        K = np.array([[seq.fx, 0, seq.cx], [0, seq.fy, seq.cy], [0, 0, 1.0]])
        views = pack_cameras(ss.SceneEngine(seq)(imgs)["camera_poses"][0, ::2].double().cpu().numpy(), K)
        views[:, ops.CARVE_DEPTH_SCALE_AT] = 1.0
        out["carve"] = carve_times(fz, np.tile(views, (10, 1)), planes.repeat(10, 1, 1).contiguous(), 2, reps)
        out["carve"].update(depth_planes_ms=float(np.median(ms)), depth_planes_minmax=[float(np.min(ms)), float(np.max(ms))],
                            depth_plane_samples=int(count), depth_plane_bytes_per_chunk=int(planes.numel()) * 2)
    return out


def consistency_times(dev: str, reps: int = 20):
    """pi3_dense_consistency at the bench chunk with ConsistencyFilter's defaults."""
    import synth_sequence as ss
    from pi3_slam_amd import ops
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator
    from pi3_slam_amd.dense_map import ConsistencyFilter, conf_logit_threshold
    seq = ss.SyntheticSequence(os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt"), noise=dict(ss.NOISE_BF16))
    out = ss.SceneEngine(seq)(seq.frames(1, dev))
    masks = OfflineChunkCreator._compute_masks(out)[0].contiguous().view(torch.uint8)
    pts, lp, conf = (out[k][0].contiguous() for k in ("points", "local_points", "conf"))
    poses = out["camera_poses"][0].contiguous()
    N = int(pts.shape[0])
    K = torch.tensor([seq.fx, seq.fy, seq.cx, seq.cy], dtype=torch.float32, device=dev).repeat(N, 1).contiguous()
    f = ConsistencyFilter()
    thr = conf_logit_threshold(0.5)
    ms = []
    for i in range(3 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        mask, _, stats = ops.dense_consistency(pts, lp, conf, masks, poses, K, thr, f.radius, f.stride, f.min_views, f.rel_tol)
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
    cand, kept = (int(x) for x in stats.tolist())
    n = int(mask.numel())
    # neighbours in range per frame (the gathers that are issued at most: a projection outside the image issues none)
    nb = sum(0 <= i + sg * s * f.stride < N for i in range(N) for s in range(1, f.radius + 1) for sg in (-1, 1)) / N
    bytes_moved = n * (1 + 4 + 12 + 4 + 4) + n * (4 + 1) + cand * (12 + 4 * nb)
    t = float(np.median(ms))
    return {"consistency_ms": t, "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "pixels": n, "candidates": cand,
            "kept": kept, "neighbours_in_range_per_pixel": nb, "bytes": int(bytes_moved),
            "achieved_TBps": bytes_moved / (t * 1e-3) / 1e12, "settings": f.settings()}


def creator_fps(voxel: float, dev: str, rounds: int, chunks: int, conf_threshold: float, consistency: bool = False,
                normals: bool = False, depth: bool = False):
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config
    engine = Pi3Engine(Pi3Config(), dev)
    with torch.no_grad():      # bench.py's edit of the plain recipe weights: non-empty masks
        w_, b_ = engine.w["point_head.proj.weight"], engine.w["point_head.proj.bias"]
        w_[392:588] = 0.05 * w_[392:393].clone()
        b_[392:588] = b_[392].clone()
        engine.w["conf_head.proj.bias"][:196] -= 2.2
    frames = synthetic_frames_u8(CL, SRC_H, SRC_W, 1234)
    tmp = tempfile.mkdtemp(prefix="dense_timing_")
    creators = {}
    legs = (("off", None, None), ("on", voxel, None)) + ((("filtered", voxel, 2),) if consistency else ()) \
        + ((("normals", voxel, None),) if normals else ()) + ((("depth", voxel, None),) if depth else ())
    for name, vs, mv in legs:
        cc = OfflineCreatorConfig(model_path="recipe", output_dir=os.path.join(tmp, name), chunk_length=CL, overlap=OV,
                                  device=dev, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=KP,
                                  num_loader_workers=0, device_resize=True, dense_voxel_size=vs,
                                  dense_conf_threshold=conf_threshold, dense_min_views=mv,
                                  dense_normals=name == "normals", dense_depth_every=2 if name == "depth" else None)
        cr = OfflineChunkCreator(cc, model=engine)
        cr.target_size = (H, W)
        creators[name] = cr
    paths = [[f"frame_{i:06d}.png"] for i in range(CL)]

    def leg(cr, n):
        items = ({"frames": frames, "kind": "u8", "paths": paths, "meta": {"chunk_index": i}} for i in range(n))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        voxels = [ch.get("dense_cloud", {}).get("points", torch.zeros(0, 3)).shape[0] for _, ch in cr.process_chunks(items)]
        torch.cuda.synchronize()
        return n * CL / (time.perf_counter() - t0), voxels, {k: v / n for k, v in cr.host_seconds.items()}

    for cr in creators.values():
        leg(cr, 1)                                            # warm-up: first-use allocations, the 2 GiB table
    fps = {name: [] for name in creators}
    host = {name: [] for name in creators}
    voxels = []
    for _ in range(rounds):
        for name in creators:
            f, v, hs = leg(creators[name], chunks)
            fps[name].append(f)
            host[name].append(hs)
            if name == "on":
                voxels = v
    off, on = float(np.median(fps["off"])), float(np.median(fps["on"]))
    # host seconds per chunk of the creator's pipeline thread (OfflineChunkCreator.host_seconds): launch = queueing one
    # chunk's kernels, finish = waiting for its results and building its dict (with the map on: the dense cloud's
    # copy + key sort, which runs on a thread of its own from the end of the chunk's extraction)
    host_ms = {name: {k: 1e3 * float(np.median([h[k] for h in host[name]])) for k in host[name][0]} for name in host}
    res = {"fps_off": fps["off"], "fps_on": fps["on"], "median_fps_off": off, "median_fps_on": on,
           "cost_pct": 100.0 * (off - on) / off, "voxels_per_chunk": voxels[:1], "host_ms_per_chunk": host_ms}
    if consistency:
        flt = float(np.median(fps["filtered"]))
        res.update(fps_filtered=fps["filtered"], median_fps_filtered=flt, filter_cost_pct=100.0 * (on - flt) / on)
    if normals:
        nrm = float(np.median(fps["normals"]))
        res.update(fps_normals=fps["normals"], median_fps_normals=nrm, normals_cost_pct=100.0 * (on - nrm) / on)
    if depth:
        dep = float(np.median(fps["depth"]))
        res.update(fps_depth=fps["depth"], median_fps_depth=dep, depth_cost_pct=100.0 * (on - dep) / on)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--conf-threshold", type=float, default=0.05,
                    help="creator leg: the edited recipe weights put few pixels above sigmoid 0.5; 0.05 lets the "
                         "creator's masked pixels through, so the fusion does real work")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--consistency", action="store_true", help="also time the multi-view consistency filter (kernel and "
                                                               "a creator leg with it on)")
    ap.add_argument("--clean", action="store_true", help="also time the map-cleaning filters on the chunk's table and on "
                                                         "a synthetic map of about 1 M voxels")
    ap.add_argument("--normals", action="store_true", help="also time the surface-normal kernels beside fuse_pixels and "
                                                           "extract, and a creator leg with dense_normals on")
    ap.add_argument("--mesh", action="store_true", help="also time the surface-mesh kernels on the chunk's table and on "
                                                        "a synthetic map of about 1 M voxels")
    ap.add_argument("--carve", action="store_true", help="also time the carve kernel with the planes of 500 views on the "
                                                         "chunk's table and on a synthetic map of about 1 M voxels, the "
                                                         "depth-plane kernel, and a creator leg with depth keyframes on")
    a = ap.parse_args()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    out = {"voxel_size": a.voxel, "kernels": kernel_times(a.voxel, dev, clean=a.clean, normals=a.normals, mesh=a.mesh,
                                                        carve=a.carve)}
    if a.mesh:
        fz, acc = synthetic_box_map(a.voxel, dev, normals=True)
        out["mesh_synthetic"] = mesh_times(fz, acc.nacc)
    if a.clean:
        out["clean_synthetic"] = clean_times(synthetic_box_map(a.voxel, dev))
    if a.carve:
        out["carve_synthetic"] = carve_times(synthetic_box_map(a.voxel, dev), *box_views(a.voxel, dev), 2)
    if a.consistency:
        out["consistency"] = consistency_times(dev)
    if not a.kernels_only:
        out["creator"] = creator_fps(a.voxel, dev, a.rounds, a.chunks, a.conf_threshold, a.consistency, a.normals, a.carve)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
