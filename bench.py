"""Headline benchmark of the hot path (BASELINE.json): frames/s end-to-end for chunk creation + overlap alignment at
chunk_length=100, overlap=20, 512x384 input (-> 308x406 by the reference's calculate_target_size rule).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
N > 1 runs one rank per GPU over RCCL either way: under `python -m torch.distributed.run --nproc-per-node N bench.py
--gpus N ...` (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), or started as a plain process, in which
case this file launches its own N ranks BEFORE anything touches the GPU (launch_ranks below) and relays rank 0's line.

One "step" = one chunk of 100 synthetic frames through the PRODUCT path (OfflineChunkCreator.process_chunks), starting
from the decoded uint8 frames in pinned host memory, as SURVEY.md §8(d) defines the metric:
    H2D of the frames -> device resize + ToTensor (pi3_ingest_frames) -> pi3 forward -> masks -> MoGe metric scale ->
    per-frame intrinsics (LM) -> grid keypoints (K=200) gather + fp16 pack -> packed D2H -> chunk dict on the host ->
    closed-form Sim(3) overlap alignment against the previous chunk and its application
(N > 1: one chunk per rank per step, then the wave alignment: RCCL all-gather of the boundary blocks, each rank's own
solve, a 136-byte all-gather of the transforms, prefix composition, application).  The stages of consecutive chunks
overlap exactly as in production (copy stream / compute stream / host), so the K timed steps include one pipeline fill.
Prints ONE JSON line on rank 0: the headline, per-stage milliseconds and the roofline figures read from HIP events of
the timed steps.  A plain run does nothing else: set-up, warm-up, the K timed steps, the outputs (--dump-outputs) and
the line.  --full adds what takes runs of its own (N = 1): the all-online-max step, the 378x504 and K=400 variants, the
from-disk rate of process_and_save() and the other extras, the APE proxy, the second metric and the CPU baseline of the
whole path (--no-extras / --no-cpu-baseline leave parts of it out).
--dump-outputs DIR: after the timed steps, rank 0 writes the chunk dictionary its last timed step handed back (after the
alignment) as DIR/<key>.npy, float32 (float64 for the accumulated similarity): the inputs are seeded, so two builds can
be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CL, OV, SRC_H, SRC_W, H, W, KP = 100, 20, 384, 512, 308, 406, 200
PEAK_BF16_DENSE_TFLOPS = 2500.0   # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0             # HBM3E (MI355X_MICROARCH.md)
# HBM-side bytes of ONE global-attention launch, from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this
# kernel (profiles/r06_attention_pmc.csv = r05d, tools/gpu_profile_r06.sh + tools/pmc_summary.py): FETCH_SIZE 714 428 KB (x2: gfx950
# reports half of a wide coalesced read stream) + WRITE_SIZE 128 600 KB (= the output, nothing through scratch) = 1.595 GB.
# (Rounds 1-4, the compiler-scheduled kernel: 643 121 / 128 601 KB = 1.449 GB; the eight-wave asm-loop kernel: 660 282 /
# 164 891 KB.)  PMC counters cannot be read from inside this process, so the JSON cites the committed profile; algorithmic
# bytes are 527 MB (q, k, v read once + o written), L2 hit rate ~95 %.
ATTN_TRAFFIC_BYTES = (2 * 714427.5 + 128600.0) * 1024.0
ATTN_TRAFFIC_SOURCE = "profiles/r06_attention_pmc.csv (unchanged since profiles/r05d_attention_pmc.csv)"


# the REAL reference (sdpa_kernel context not entered) timed once in the build container (8 Xeon
# cores, fp32 eager) with tools/cpu_reference_timing.py; profiles/r03_cpu_reference.json.  /root/reference does not exist
# on the GPU box, so the live cpu_baseline below is the oracle port on that box's host cores; these two figures are the
# reference's own and are quoted beside it.
# N = 1 figure of this bench on one MI355X (the newest driver record BENCH_rNN.json; round 4: 406.85 ms per step, 245.8
# frames/s; cards of the pool differ by +-4 %), quoted in the N > 1 line so weak scaling can be read against it
def _n1_reference() -> dict:
    """The newest committed driver record of the N = 1 run (BENCH_rNN.json at the repo root); the constant below is the
    fall-back when none travels with the tree."""
    import glob
    import re
    best = None
    for path in glob.glob(os.path.join(ROOT, "BENCH_r*.json")):
        m = re.search(r"BENCH_r(\d+)\.json$", path)
        try:
            rec = json.load(open(path)).get("parsed") or {}
            if m and rec.get("n_gpus") == 1 and rec.get("ms_per_step") and (best is None or int(m.group(1)) > best[0]):
                best = (int(m.group(1)), rec, os.path.basename(path))
        except Exception:
            continue
    if best is None:
        return {"ms_per_step": 406.85, "frames_per_s": 245.8, "source": "BENCH_r04.json (driver run, 1 x MI355X)"}
    return {"ms_per_step": float(best[1]["ms_per_step"]), "frames_per_s": float(best[1]["value"]),
            "source": f"{best[2]} (driver run, 1 x MI355X)"}


N1_REFERENCE = _n1_reference()
REFERENCE_CPU = {"source": "profiles/r03_cpu_reference.json", "cores": 8,
                 "frames_32": {"wall_s": 176.33, "frames_per_s": 0.1815},
                 "frames_100": {"wall_s": 993.05, "frames_per_s": 0.1007}}


def synthetic_frames_u8(n: int, h: int, w: int, seed: int) -> torch.Tensor:
    """n smooth synthetic frames (low-frequency structure + noise), uint8 [n, h, w, 3], pinned."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, h)[None, :, None, None]
    xx = torch.linspace(0, 1, w)[None, None, :, None]
    ph = torch.rand(n, 1, 1, 3, generator=g) * 6.28
    img = 0.5 + 0.25 * torch.sin(7 * xx + 3 * yy + ph) * torch.cos(5 * yy - ph) + 0.1 * torch.rand(n, h, w, 3, generator=g)
    out = (img.clamp(0, 1) * 255).to(torch.uint8).contiguous()
    return out.pin_memory() if torch.cuda.is_available() else out


def cpu_baseline(engine_cfg, n_frames: int):
    """The oracle (CPU restatement of the reference) timed on this box's host cores over the WHOLE path on a bounded
    sample: pi3 forward (fp32, flash SDPA as BASELINE.md §3.2), masks, MoGe metric scale (oracle forward + focal/shift),
    per-frame intrinsics (scipy LM), grid keypoints + gather + colours, and the numpy closed-form Sim(3) on a 20 x 200
    overlap block.  Per-chunk stages (MoGe, alignment) are charged pro rata (n_frames / 100) so the figure is the rate of
    a 100-frame chunk with the forward measured at n_frames (its global attention is quadratic in the frame count, so
    the true 100-frame CPU rate is lower still)."""
    import numpy as np
    from oracle import moge_ref, pi3_ref, post_ref
    from pi3_slam_amd.moge import SYNTHETIC_CONFIG, moge_param_shapes, moge_recipe_params
    from pi3_slam_amd import ops
    from pi3_slam_amd.recipe import fnv1a64
    from pi3_slam_amd.weights import param_shapes, recipe_fill_device
    sd = {name: recipe_fill_device(name, shape, "cuda:0").cpu() for name, shape in param_shapes(engine_cfg).items()}
    msd = {}
    for name, shape in moge_param_shapes(SYNTHETIC_CONFIG).items():     # same recipe as the device engine
        off, sc = moge_recipe_params(name, shape)
        t = torch.empty(shape, device="cuda:0", dtype=torch.float32)
        ops.recipe_fill(t, fnv1a64("moge." + name), off, sc)
        msd[name] = t.cpu()
    from pi3_slam_amd.weights import IMAGE_MEAN, IMAGE_STD
    msd["encoder.image_mean"] = torch.tensor(IMAGE_MEAN).view(1, 3, 1, 1)
    msd["encoder.image_std"] = torch.tensor(IMAGE_STD).view(1, 3, 1, 1)
    threads = min(torch.get_num_threads(), len(os.sched_getaffinity(0)), 16)  # the GPU box grants 16 cores per GPU
    torch.set_num_threads(threads)
    imgs = torch.rand(1, n_frames, 3, H, W, generator=torch.Generator().manual_seed(0))
    pi3_ref.SDPA_FLASH = True
    t = {}
    t0 = time.perf_counter()
    out = pi3_ref.pi3_forward(sd, imgs, engine_cfg)
    t["forward"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lp, conf, pts = out["local_points"][0], out["conf"][0], out["points"][0]
    masks = post_ref.compute_masks(conf, lp)
    t["masks"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    md = moge_ref.moge_infer(msd, SYNTHETIC_CONFIG, imgs[0, 0], 9)["depth"]
    m0 = masks[0] & torch.isfinite(md)
    if m0.any():
        post_ref.scale_factor(md, lp[0][..., 2], m0)
    t["moge"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    post_ref.estimate_camera_parameters(lp, conf)
    t["intrinsics"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    kp = post_ref.grid_keypoints(n_frames, H, W, KP, torch.Generator().manual_seed(0))
    post_ref.interpolate_at_keypoints(pts, lp, conf, masks, kp, H, W)
    post_ref.keypoint_colors(imgs[0], kp)
    t["gather"] = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    world = rng.standard_normal((OV, KP, 3)) + np.array([0, 0, 4.0])
    kp16 = (rng.random((OV, KP, 2)) * 300).astype(np.float16)
    t0 = time.perf_counter()
    post_ref.align_chunks(world.astype(np.float16), (world * 0.8 + 0.1).astype(np.float16), kp16, kp16,
                          np.eye(4, dtype=np.float32), True)
    t["align"] = time.perf_counter() - t0
    per_frames = t["forward"] + t["masks"] + t["intrinsics"] + t["gather"]
    per_chunk = t["moge"] + t["align"]
    total = per_frames + per_chunk * n_frames / CL
    return {"reference_in_build_container": REFERENCE_CPU,
            "value": n_frames / total, "unit": "frames/s", "cores": threads, "kind": "port",
            "like_for_like": "value (this box's host cores, the oracle port over the whole path, measured now) is the figure to "
                             "set beside the GPU number of the same run; reference_in_build_container is the REAL "
                             "reference's own code, measured once on the build container's 8 cores - same workload, "
                             "different host, quoted for scale",
            "sample": f"oracle whole path on {n_frames} frames {H}x{W}, fp32 torch CPU with flash SDPA, {threads} threads: "
                      + ", ".join(f"{k} {v:.2f} s" for k, v in t.items())
                      + f"; per-chunk stages (moge, align) charged x {n_frames}/{CL}; the global attention is quadratic "
                        f"in the frame count, so the 100-frame CPU rate is lower still (BASELINE.md)"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)     # 10 x 0.4 s: the pipeline's fill + drain (~14 ms) is 0.35 % of the region
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--cpu-frames", type=int, default=32,
                    help="frames of the CPU baseline sample of --full (32 = BASELINE configs[0], ~80 s on 16 host threads; 8: ~30 s)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the all-online-max step and the 378x504 / K=400 / from-disk extras")
    ap.add_argument("--no-moge", action="store_true", help="diagnostic only: leave the MoGe metric scale out (the line then says "
                    "moge_metric_scale_in_timed_region: false and is not the headline workload)")
    ap.add_argument("--launch-check", action="store_true",
                    help="rendezvous only: every rank joins the process group, one all-gather, rank 0 prints the comm "
                         "record; no chunk is processed (with PI3_DIST_BACKEND=gloo it needs no GPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also the measurements that take runs of their own (N = 1): all-online-max "
                         "step, extras, APE proxy, second metric, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's chunk dictionary as DIR/<key>.npy (float32 / float64)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir: str, chunk: dict, extra: dict = None) -> dict:
    """The arrays of one chunk dictionary (nested dicts flattened to 'a.b', masks as 0 / 1) as out_dir/<name>.npy, float32
    (float64 where the product holds float64).  An array that would take the total past DUMP_BUDGET_BYTES is replaced by
    a fixed, seeded sample of its flattened elements (the same indices on every run)."""
    import numpy as np
    arrays = {}

    def walk(prefix, obj):
        if isinstance(obj, dict):
            for k, v in obj.items():
                if not str(k).startswith("_metrics"):
                    walk(f"{prefix}.{str(k).lstrip('_')}" if prefix else str(k).lstrip("_"), v)
        elif isinstance(obj, torch.Tensor):
            t = obj.detach().cpu()
            arrays[prefix] = t.double().numpy() if t.dtype == torch.float64 else t.float().numpy()
        elif isinstance(obj, np.ndarray) and obj.dtype.kind in "biuf":
            arrays[prefix] = obj.astype(np.float64 if obj.dtype == np.float64 else np.float32)

    walk("", chunk)
    walk("", extra or {})
    os.makedirs(out_dir, exist_ok=True)
    left, written = DUMP_BUDGET_BYTES, {}
    for i, name in enumerate(sorted(arrays, key=lambda n: arrays[n].nbytes)):
        a = np.ascontiguousarray(arrays[name])
        share = left // (len(arrays) - i)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=max(1, share // a.itemsize), replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes
        written[name] = list(a.shape)
    return written


def launch_ranks(n: int, argv) -> int:
    """`python bench.py --gpus N` started as a PLAIN process: start the N ranks as child processes (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set, one rank per GPU) and relay rank 0's JSON line.  The parent
    never initialises the GPU - it imports torch, nothing more (no HIP call, no torch.cuda.is_available()) - and never
    replaces itself (no exec): it waits for its children and returns non-zero if any of them failed, stopping the others
    (by their exact PIDs) as soon as one does, so a crashed rank cannot leave the rest blocked in a collective."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE",
                                                              "GROUP_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base.update(WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), PI3_BENCH_LAUNCHER="self")
    procs = []
    for r in range(n):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    import threading
    out0 = []
    reader = threading.Thread(target=lambda: out0.extend(procs[0].stdout), daemon=True)   # drain rank 0's pipe as it fills
    reader.start()
    failed = 0
    live = set(range(n))
    while live and not failed:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is not None:
                live.discard(r)
                if rc != 0:
                    failed = rc
                    print(f"[bench launcher] rank {r} exited with code {rc}; stopping the other ranks", file=sys.stderr)
        time.sleep(0.05)
    for r in sorted(live):                   # only reached with ranks alive when one failed
        procs[r].terminate()
    for r in sorted(live):
        try:
            procs[r].wait(timeout=20)
        except subprocess.TimeoutExpired:
            procs[r].kill()
            procs[r].wait()
    reader.join(timeout=10)
    for ln in out0:
        if ln.startswith("{"):
            sys.stdout.write(ln if ln.endswith("\n") else ln + "\n")
    sys.stdout.flush()
    return failed


def comm_record(backend: str, world: int, dev, boundary_bytes=None):
    """Evidence that the collective library saw `world` ranks: what torch.distributed itself reports, every rank's
    device (gathered THROUGH the process group), and the bytes the alignment moves per wave."""
    import torch.distributed as dist
    mine = {"rank": dist.get_rank(), "pid": os.getpid(), "local_rank": int(os.environ.get("LOCAL_RANK", "0")),
            "device": str(dev), "device_name": torch.cuda.get_device_name(dev) if dev is not None else "cpu (launch check)"}
    ranks = [None] * world
    dist.all_gather_object(ranks, mine)
    rec = {"backend": dist.get_backend(), "requested_backend": backend, "world_size": dist.get_world_size(),
           "launcher": os.environ.get("PI3_BENCH_LAUNCHER", "torch.distributed.run"), "ranks": ranks,
           "collective_library": "RCCL (torch.distributed backend 'nccl' on ROCm) over xGMI" if backend == "nccl"
                                 else "gloo over TCP loopback: a rehearsal of the N > 1 logic, not a scaling measurement"}
    if backend == "nccl":
        try:
            rec["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:  # noqa: BLE001
            rec["rccl_version"] = f"unavailable ({e})"
    if boundary_bytes is not None:
        rec["allgather_bytes_per_wave"] = {"boundary_blocks": boundary_bytes * world, "sim3_records": 17 * 8 * world,
                                           "per_rank_boundary_block": boundary_bytes}
    return rec


def launch_check(args) -> None:
    """--launch-check: the rendezvous and nothing else (tests the plain-process launcher without a GPU under gloo)."""
    import torch.distributed as dist
    backend = os.environ.get("PI3_DIST_BACKEND", "nccl")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dev = None
    if backend == "nccl":
        dev = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)
    t = torch.full((1,), float(dist.get_rank()), device=dev if dev is not None else "cpu")
    got = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    assert [int(g.item()) for g in got] == list(range(world))
    rec = comm_record(backend, world, dev)
    if dist.get_rank() == 0:
        _REAL_STDOUT.write(json.dumps({"launch_check": True, "n_gpus": world, "comm": rec}) + "\n")
        _REAL_STDOUT.flush()
    dist.destroy_process_group()


def main(args) -> None:
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and args.gpus == 1 and "RANK" in os.environ:
        # started under torch.distributed.run without --gpus: the launcher's WORLD_SIZE is the rank count
        if rank == 0:
            print(f"[bench] --gpus left at its default under a launcher with WORLD_SIZE={world}: using {world}",
                  file=sys.stderr)
        args.gpus = world
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start bench.py as a plain process (it launches its own "
                         f"ranks) or under torch.distributed.run with --nproc-per-node {args.gpus}")
    if args.launch_check:
        return launch_check(args)
    ndev = torch.cuda.device_count()
    backend = os.environ.get("PI3_DIST_BACKEND", "nccl")   # "gloo" only to rehearse the N > 1 logic on a 1-GPU box
    # PI3_BENCH_STUB=1 (tests only, gloo only): every GPU object replaced by tests/bench_stub.py so that THIS function's
    # N > 1 control flow runs on a box without a GPU; the line then says "stub": true and is not a measurement
    stub = os.environ.get("PI3_BENCH_STUB") == "1"
    if stub and backend != "gloo":
        raise SystemExit("PI3_BENCH_STUB=1 is a CPU rehearsal of the control flow: it needs PI3_DIST_BACKEND=gloo")
    dev = None if stub else torch.device(f"cuda:{local_rank % max(1, ndev) if backend == 'gloo' else local_rank}")
    if not stub:
        torch.cuda.set_device(dev)
    # PI3_DIST_FORCE=1: build the process group and take the wave-alignment path even with ONE rank - a 1-rank RCCL group
    # is the only way to run the nccl branch of this file (device-resident boundary blocks, all-gathers, comm record) on
    # a one-GPU box; the line then carries `comm` like an N > 1 line (tests/test_pipeline_gpu.py)
    grouped = world > 1 or os.environ.get("PI3_DIST_FORCE") == "1"
    if grouped:
        import torch.distributed as dist
        if world == 1:
            import socket
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)   # RCCL over xGMI
        else:
            dist.init_process_group(backend)
        # build the communicator now (untimed set-up, like weight initialisation): the first collective of a process
        # group pays the RCCL ring / xGMI topology discovery, which must not land in a timed step when --warmup is 0
        _w = torch.zeros(1, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(_w)
        dist.all_gather([torch.empty_like(_w) for _ in range(world)], _w)
    comm_dev = dev if backend == "nccl" else "cpu"

    from pi3_slam_amd import ops
    from pi3_slam_amd.alignment import align_and_refine_reconstructions, create_view_graph_matches, transform_chunk
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    from pi3_slam_amd.dist import (align_wave, allgather_boundaries, default_solver, pack_boundary, unpack_boundary)
    from pi3_slam_amd.engine import Pi3Engine
    from pi3_slam_amd.weights import Pi3Config

    cfg = Pi3Config()
    moge = None
    if stub:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bench_stub
        engine = bench_stub.StubEngine()
    else:
        engine = Pi3Engine(cfg, str(dev))
        try:
            from pi3_slam_amd.moge import MoGeEngine
            if not args.no_moge:
                moge = MoGeEngine.from_pretrained("recipe", str(dev))
        except Exception as e:  # noqa: BLE001
            if rank == 0:
                print(f"[bench] MoGe engine unavailable ({e}); metric scaling is NOT in the timed region", file=sys.stderr)

    if not stub and os.environ.get("PI3_BENCH_PLAIN_RECIPE") != "1":
        # Plain recipe weights make EVERY pixel a depth edge (z = exp(random) differs by ~50 % between neighbours): masks
        # empty, the MoGe ratio median NaN, the rescale a no-op - the post-processing kernels would run on degenerate
        # data.  The same edit as oracle/gen_golden_full.mask_overrides (fixture pi3_full_masks): z constant inside a
        # patch and a few per cent apart between patches, confidence logits straddling the sigmoid > 0.1 threshold.
        # Shapes, kernels and launch counts are unchanged (the edit touches 197 rows of two fp32 head matrices).
        with torch.no_grad():
            w_, b_ = engine.w["point_head.proj.weight"], engine.w["point_head.proj.bias"]
            w_[392:588] = 0.05 * w_[392:393].clone()
            b_[392:588] = b_[392].clone()
            engine.w["conf_head.proj.bias"][:196] -= 2.2

    def make_creator(kp: int, out_dir: str = "/tmp/pi3_bench_out", workers: int = 0):
        cc = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=CL, overlap=OV,
                                  device=str(dev), do_metric_depth=moge is not None, keypoint_type="grid",
                                  max_num_keypoints=kp, num_loader_workers=workers, device_resize=True)
        return OfflineChunkCreator(cc, model=engine, moge_model=moge)

    import contextlib
    if stub:
        creator = bench_stub.StubCreator(CL, OV, KP, rank, world)
        frames_u8 = None
        solve = bench_stub.stub_solver(OV, CL)
        on_align_stream = contextlib.nullcontext
        compose = None                                       # align_wave's own f64 prefix product
        apply_global = bench_stub.transform_chunk_cpu
    else:
        creator = make_creator(KP)
        frames_u8 = synthetic_frames_u8(CL, SRC_H, SRC_W, 1234 + rank)        # decoded frames, pinned host memory
        align_stream = torch.cuda.Stream(dev, priority=-1)   # the tiny alignment kernels slot in beside the next chunk's forward
        solve = default_solver(OV, dev, CL)
        on_align_stream = lambda: torch.cuda.stream(align_stream)   # noqa: E731
        compose = lambda T: ops.sim3_compose_prefix(T.to(dev))      # noqa: E731
        apply_global = lambda ch, G: transform_chunk(ch, G, device=str(dev), absolute=True)   # noqa: E731
    creator.target_size = (H, W)
    paths = [[f"frame_{i:06d}.png"] for i in range(CL)]
    matches = create_view_graph_matches(CL, OV)
    attn_events = []
    kernel_events = {}          # {kernel name: [(start, end)]} of three sampled blocks per step (engine.forward)
    last_wave = {"Gs": []}      # the global transforms of the most recent wave (the stub run prints them to be checked)
    last_out = {}               # the chunk dictionary of the most recent step, aligned (--dump-outputs)

    class _EventedModel:   # HIP events on the launch stream around the dominant kernel (global attention)
        def __init__(self, eng, events, kevents=None):
            self.eng, self.events, self.kevents = eng, events, kevents

        def __call__(self, imgs):
            return self.eng.forward(imgs, global_attn_events=self.events, kernel_events=self.kevents)

    def run(cr, src, n_steps: int, timed: bool, kind: str = "u8"):
        """n_steps chunks through the pipelined product path + alignment; returns the per-chunk _metrics."""
        state = {"prev": None, "G_last": torch.eye(4, dtype=torch.float64), "prev_tail": None, "wave": 0}
        # the warm-up goes through the same (plain-launch, evented) forward as the timed steps: warmed up through the
        # hipGraph replay instead, the first timed step paid for the plain path's first-use allocations (20-85 ms, i.e. up
        # to 4 % of a 5-step measurement)
        if not stub:
            # (PI3_BENCH_NO_KERNEL_EVENTS=1: the headline without the ~40 sampled per-kernel event pairs per step, to price them)
            kev = None if os.environ.get("PI3_BENCH_NO_KERNEL_EVENTS") == "1" else (kernel_events if timed else {})
            cr.model = _EventedModel(engine, attn_events if timed else [], kev)
        items = ({"frames": src, "kind": kind, "paths": paths, "meta": {"chunk_index": i}} for i in range(n_steps))
        stats = []
        for meta, chunk in cr.process_chunks(items):
            t0 = time.perf_counter()
            with on_align_stream():
                if not grouped:
                    if state["prev"] is not None:
                        ok, _ = align_and_refine_reconstructions(state["prev"], chunk, matches, device=str(dev))
                        assert ok
                    state["prev"] = chunk
                else:
                    kk = int(chunk["keypoints"].shape[1])
                    blocks = [unpack_boundary(b, OV, kk, n_frames=CL)
                              for b in allgather_boundaries(pack_boundary(chunk, OV, kk, device=comm_dev), comm_dev)]
                    w0 = state["wave"] * world
                    Gs, _ = align_wave(rank, world, w0, w0 + world, blocks, state["prev_tail"], state["G_last"], solve,
                                       comm_dev, compose)
                    apply_global(chunk, Gs[rank])
                    last_wave["Gs"] = Gs
                    state["G_last"], state["prev_tail"], state["wave"] = Gs[-1], blocks[-1], state["wave"] + 1
            m = dict(chunk["_metrics"])
            m["align_host_s"] = time.perf_counter() - t0
            stats.append(m)
            last_out["chunk"] = chunk
        if not stub:
            cr.model = engine
        return stats

    quiet = contextlib.redirect_stdout(open(os.devnull, "w")) if rank != 0 else contextlib.nullcontext()

    def sync_all():
        if not stub:
            torch.cuda.synchronize(dev)
        if grouped:
            import torch.distributed as dist
            dist.barrier()
            if not stub:
                torch.cuda.synchronize(dev)

    # which softmax loop the attention waves' results come from in the timed steps (the bounded-score
    # loop is what the headline runs on; softmax_paths() says when it is kept): a device
    # counter block registered for the timed region (one no-return atomic per wave), read after it
    path_counters = torch.zeros(2, 2, 32, device=dev, dtype=torch.int32)
    with quiet:
        if args.warmup > 0:
            run(creator, frames_u8, args.warmup, False)
        sync_all()
        if not stub:
            ops.attention_path_counters(path_counters)
        t0 = time.perf_counter()
        stats = run(creator, frames_u8, args.steps, True)
        sync_all()
        dt = time.perf_counter() - t0
        if not stub:
            ops.attention_path_counters(None)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_out["chunk"],
                     {"wave_global_transforms": torch.stack(last_wave["Gs"])} if last_wave["Gs"] else None)
    n_headline_events = len(attn_events)
    headline_kernel_events = {k: list(v) for k, v in kernel_events.items()}
    online_max = None
    if world == 1 and not grouped and args.full and not args.no_extras:
        # the same step with every wave on the online-max loop (knob attn_nomax = 0): the worst case for real weights.
        # (--no-extras skips it: the rocprofv3 kernel-trace of the bench command must average the headline launches only,
        # the two loops being one kernel instance)
        from pi3_slam_amd import lib as _lib
        k_steps = max(3, min(5, args.steps))
        with quiet:
            nomax_before = _lib.get_knob("attn_nomax")     # PI3_ATTN_NOMAX of an A/B run stays in force for the later legs
            _lib.set_knob("attn_nomax", 0)
            try:
                run(creator, frames_u8, 2, False)
                sync_all()
                t1 = time.perf_counter()
                run(creator, frames_u8, k_steps, True)
                sync_all()
                dt1 = time.perf_counter() - t1
            finally:
                _lib.restore_knob("attn_nomax", nomax_before)   # unset = the default: optimistic bounded-score loop (attn64.hip)
        ev = attn_events[n_headline_events:]
        ms1 = sum(a.elapsed_time(b) for a, b in ev) / max(1, len(ev))
        online_max = {"steps": k_steps, "ms_per_step": dt1 / k_steps * 1e3, "frames_per_s": CL * k_steps / dt1,
                      "global_attention_launch_ms": ms1, "launches_timed": len(ev)}
        del attn_events[n_headline_events:]
    comm = None
    if grouped:
        import torch.distributed as dist
        from pi3_slam_amd.dist import boundary_numel
        own_dt = dt
        tt = torch.tensor([dt], device=comm_dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        comm = comm_record(backend, world, dev, boundary_numel(OV, KP) * 4)
        per_rank = [None] * world
        dist.all_gather_object(per_rank, {
            "rank": rank, "ms_per_step": own_dt / args.steps * 1e3,
            "pi3_forward_ms": 1e3 * sum(s.get("infer_s", 0.0) for s in stats) / max(1, len(stats)),
            "align_host_wait_ms": 1e3 * sum(s.get("align_host_s", 0.0) for s in stats) / max(1, len(stats))})
        comm["per_rank"] = per_rank

    if rank == 0 and os.environ.get("PI3_BENCH_STEPLOG"):      # per-step stage times on stderr (diagnostic)
        for i, st in enumerate(stats):
            print(f"[bench step {i}] " + " ".join(f"{k}={1e3 * st[k]:.2f}ms" for k in ("stage_in_s", "infer_s", "post_s", "align_host_s")
                                                   if k in st), file=sys.stderr)
    if rank == 0:
        T = (H // 14) * (W // 14) + cfg.n_dec_reg
        S = CL * T
        attn_flops = 4.0 * cfg.heads * float(S) * float(S) * 64.0          # one global-attention launch
        attn_ms = sum(a.elapsed_time(b) for a, b in attn_events) / max(1, len(attn_events))
        achieved = attn_flops / (attn_ms * 1e-3) / 1e12 if attn_ms > 0 else 0.0
        fl = engine.flops(1, CL, H, W)
        mean = lambda k: 1e3 * sum(s.get(k, 0.0) for s in stats) / max(1, len(stats))   # noqa: E731
        line = {
            "metric": "frames/sec end-to-end (chunk create+align), 512x384 cl=100 ov=20",
            "value": world * CL * args.steps / dt,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "dtype_note": "pi3 computes in bf16 (the reference's autocast dtype); the MoGe forward inside the timed region "
                          "computes in IEEE half on f16 MFMA (the reference's own use_fp16 autocast)",
            "data": "synthetic",
            "config": {"workload": "configs[1]-shaped synthetic chunk: 100 frames 512x384 uint8 in pinned host memory -> "
                                   "308x406 (calculate_target_size), cl=100 ov=20, grid keypoints K=200, recipe weights",
                       "chunks_per_step_per_gpu": 1, "parallelism": f"chunk-parallel x{world}",
                       "timed_from": "pinned host uint8 frames (H2D + device resize inside the timed region)",
                       "moge_metric_scale_in_timed_region": moge is not None,
                       "metric_scale_usable_chunks": sum(1 for s in stats if s.get("metric_scale") is not None),
                       "metric_scale_note": "MoGe forward, masked ratio median and the rescale kernels run in every chunk; the "
                                            "recipe's point / confidence heads are edited as in fixture pi3_full_masks so that "
                                            "masks are not empty (plain recipe weights make every pixel a depth edge: "
                                            "PI3_BENCH_PLAIN_RECIPE=1 restores that, the median is then NaN and the rescale "
                                            "applies 1.0)",
                       "algorithmic_tflop_per_chunk": fl["total"] / 1e12},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_BF16_DENSE_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_BF16_DENSE_TFLOPS, "traffic": ATTN_TRAFFIC_BYTES,
                         "traffic_source": ATTN_TRAFFIC_SOURCE,
                         "kernel": "attn_fwd64b_kernel (global attention, S=64300, 16 heads, d=64; hand-placed main loop, one wave per SIMD x 128 rows, round 5)",
                         "launch_ms": attn_ms, "launches_timed": len(attn_events),
                         "end_to_end_tflops": fl["total"] * args.steps / dt / 1e12,
                         "softmax_paths": softmax_paths(path_counters, online_max, attn_flops),
                         "kernels": kernel_table(headline_kernel_events, S, cfg, CL, T, attn_ms, len(attn_events))},
            "stages_ms": {"stage_in_h2d_resize": mean("stage_in_s"), "pi3_forward": mean("infer_s"),
                          "post_masks_scale_intrinsics_gather": mean("post_s"), "align_host_wait": mean("align_host_s"),
                          # the consumer-side wall-clock gate (moved here from the correctness suite):
                          # the alignment of chunk k-1 runs beside the forward of chunk k and must not wait for it
                          "align_host_wait_median": 1e3 * sorted(s.get("align_host_s", 0.0) for s in stats)[len(stats) // 2],
                          "align_host_wait_max": 1e3 * max(s.get("align_host_s", 0.0) for s in stats),
                          "align_host_wait_over_10ms": sum(1 for s in stats if s.get("align_host_s", 0.0) > 0.010),
                          "align_host_wait_bound": "median < 5 ms and no sample > 10 ms (0 of 198 in gpurun_out/r5c/stall3.log; "
                                                   "a violated rule shows as ~0.6 x pi3_forward on every chunk)",
                          "note": "GPU-event times per chunk (copy stream / compute stream); stages of consecutive chunks "
                                  "overlap, so they do not add up to ms_per_step"},
        }
        if stub:     # a control-flow rehearsal: say so, and carry nothing that reads like a measurement of the GPU path
            line.update(stub=True, data="STUB: no GPU work (tests/bench_stub.py on gloo); control-flow rehearsal only",
                        vs_baseline=None)
            line.pop("roofline")
            line["stub_check"] = {"global_transforms_last_wave": [g.reshape(-1).tolist() for g in last_wave["Gs"]]}
        if comm is not None:
            line["comm"] = comm
            # what ONE GPU takes for the same step, to cross-check this N-rank line against the N = 1 line: the committed
            # N = 1 record and, live, every rank's own wall time per step and forward time by GPU events (comm.per_rank)
            line["n1_reference_ms_per_step"] = N1_REFERENCE
        if args.full:
            line["second_metric"] = second_metric(dev) if world == 1 else {
                "metric": "7-Scenes APE", "value": None, "note": "reported by the N = 1 run"}
        proxy = None
        if world == 1 and args.full and not args.no_extras and not stub:
            with contextlib.redirect_stdout(sys.stderr):
                line["extras"] = extras(engine, moge, make_creator, run, dev)
                proxy = ape_proxy_product(dev)
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(cfg, args.cpu_frames)
            if proxy is not None and "dir" in proxy:      # the CPU side of the proxy: the fp64 oracle over the same 13 files
                with contextlib.redirect_stdout(sys.stderr):
                    line["cpu_baseline"]["stage2_chess_proxy"] = ape_proxy_oracle(proxy["dir"])
                    for scene, o in proxy.get("other_scenes", {}).items():
                        o["ape_oracle_m"] = ape_proxy_oracle(o["dir"], scene)["ape_oracle_m"]
        if proxy is not None:
            line["second_metric"]["proxy"] = ape_proxy_summary(proxy, (line.get("cpu_baseline") or {}).get("stage2_chess_proxy"))
            shutil.rmtree(proxy.pop("dir", ""), ignore_errors=True)
        _REAL_STDOUT.write(json.dumps(line) + "\n")
        _REAL_STDOUT.flush()
    if grouped:
        import torch.distributed as dist
        dist.destroy_process_group()


# HBM-side bytes per launch of the block GEMMs (FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 --pmc passes over
# tools/dev_gemm.py at M = 64 300: profiles/r06_gemm256_pmc.csv, summary and algorithmic bytes in profiles/r06_gemm_summary.md)
GEMM_TRAFFIC_BYTES = {"qkv_fused_qk_epilogue": 1.146e9, "qkv_k2max_epilogue": 1.146e9, "qkv_plain": 1.145e9, "proj": 0.683e9,
                      "fc1_gelu": 1.426e9, "fc2": 1.361e9}
GEMM_ALGORITHMIC_BYTES = {"qkv_fused_qk_epilogue": 0.533e9, "qkv_k2max_epilogue": 0.533e9, "qkv_plain": 0.533e9,
                          "proj": 0.660e9, "fc1_gelu": 0.666e9, "fc2": 1.061e9}


def kernel_table(events: dict, S: int, cfg, n_frames: int, T: int, global_attn_ms: float, n_global: int) -> list:
    """The other kernels of the step under the driver's clock: HIP-event time per launch, measured
    in the timed steps on three sampled blocks per step (one encoder block, one frame-wise and one global decoder block;
    every block of the chunk runs the same shapes), against the roofline that bounds each: dense bf16 MFMA peak for the
    GEMMs and the attention (algorithmic FLOPs: 2 M N K; 4 heads B S^2 64), HBM for LayerNorm (fp32 row in, bf16 row out)."""
    D, Hh = cfg.dim, cfg.heads
    flops = {"qkv_fused_qk_epilogue": 2.0 * S * 3 * D * D, "qkv_k2max_epilogue": 2.0 * S * 3 * D * D,
             "qkv_plain": 2.0 * S * 3 * D * D, "proj": 2.0 * S * D * D, "fc1_gelu": 2.0 * S * 4 * D * D,
             "fc2": 2.0 * S * 4 * D * D, "attention_frame": 4.0 * Hh * n_frames * float(T) * float(T) * 64.0,
             "attention_global": 4.0 * Hh * float(S) * float(S) * 64.0}
    what = {"qkv_fused_qk_epilogue": "decoder qkv projection, q/k LayerNorm(64) + RoPE-2D + max|k|^2 in the epilogue (gemm256_kernel<QK>)",
            "qkv_k2max_epilogue": "encoder qkv projection, softmax scale + max|k|^2 in the epilogue (gemm256_kernel<QK>)",
            "qkv_plain": "qkv projection (gemm256_kernel)", "proj": "attention output projection + LayerScale + residual, fp32 out",
            "fc1_gelu": "MLP fc1 + GELU, bf16 out", "fc2": "MLP fc2 + LayerScale + residual, fp32 out",
            "attention_frame": f"frame-wise attention, {n_frames} sequences of {T} tokens (attn_fwd64_kernel<4>)",
            "attention_global": "global attention (attn_fwd64b_kernel)", "layernorm": "LayerNorm, fp32 rows in, bf16 rows out"}
    rows = [{"name": "attention_global", "what": what["attention_global"], "bound": "mfma", "launch_ms": global_attn_ms,
             "launches_timed": n_global, "achieved": flops["attention_global"] / (global_attn_ms * 1e-3) / 1e12 if global_attn_ms > 0 else 0.0,
             "peak": PEAK_BF16_DENSE_TFLOPS, "unit": "TFLOP/s"}]
    for name in ("qkv_fused_qk_epilogue", "qkv_k2max_epilogue", "qkv_plain", "proj", "fc1_gelu", "fc2", "attention_frame", "layernorm"):
        ev = events.get(name) or []
        if not ev:
            continue
        ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
        if name == "layernorm":
            gbs = S * D * (4 + 2) / (ms * 1e-3) / 1e9
            rows.append({"name": name, "what": what[name], "bound": "hbm", "launch_ms": ms, "launches_timed": len(ev),
                         "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s"})
        else:
            rows.append({"name": name, "what": what[name], "bound": "mfma", "launch_ms": ms, "launches_timed": len(ev),
                         "achieved": flops[name] / (ms * 1e-3) / 1e12, "peak": PEAK_BF16_DENSE_TFLOPS, "unit": "TFLOP/s"})
    for r in rows:
        r["frac"] = r["achieved"] / r["peak"]
        if r["name"] in GEMM_TRAFFIC_BYTES:       # PMC counters cannot be read from inside this process: the committed profile
            r["traffic"] = GEMM_TRAFFIC_BYTES[r["name"]]
            r["algorithmic_bytes"] = GEMM_ALGORITHMIC_BYTES[r["name"]]
            r["traffic_source"] = "profiles/r06_gemm256_pmc.csv"
        elif r["name"] == "attention_global":
            r["traffic"], r["traffic_source"] = ATTN_TRAFFIC_BYTES, ATTN_TRAFFIC_SOURCE
    return rows


def softmax_paths(counters: torch.Tensor, online_max, attn_flops: float) -> dict:
    """What the headline's attention speed depends on: the share of waves of the timed steps whose result came from the
    bounded-score loop (no running max) against the online-max loop, for the global (eight-wave workgroups) and the
    frame-wise (four-wave) launches, and the same step with EVERY wave forced onto the online-max loop (knob attn_nomax = 0).
    Since round 5 the bounded-score loop is taken optimistically (knob attn_nomax = 2, the default): a workgroup runs it
    unconditionally and keeps the result iff every row's sum lies in [2^-60, 2^120] and its outputs are finite; a workgroup
    that fails re-runs on the online-max loop in a follow-up launch and is counted there (twice its time).  The a-priori
    form of rounds 3-4 (knob 1: |q| max|k| <= 90 for every row of a wave, a Cauchy-Schwarz bound that one large key breaks)
    gives the same counts on recipe weights."""
    w = counters.sum(-1).cpu().tolist()
    out = {"loop_selection": "knob attn_nomax = 2: bounded-score loop kept by the a-priori bound |q| max|k| <= 90 where it holds, "
                             "elsewhere by the test 2^-60 <= row sum <= 2^120 and finite outputs, rejected workgroups re-run on "
                             "the online-max loop in a follow-up launch (attn64.hip a64_reject); online_max_waves counts those"}
    for name, (fast, slow) in (("global_attention", w[0]), ("frame_attention", w[1])):
        out[name] = {"bounded_score_waves": int(fast), "online_max_waves": int(slow),
                     "fraction_bounded": (fast / (fast + slow)) if fast + slow else None}
    if online_max is not None:
        ms = online_max["global_attention_launch_ms"]
        out["all_online_max"] = dict(online_max, roofline_frac=attn_flops / (ms * 1e-3) / 1e12 / PEAK_BF16_DENSE_TFLOPS,
                                     note="knob attn_nomax = 0 (PI3_ATTN_NOMAX=0): every attention wave of the step on "
                                          "the online-max loop - the bound of what real weights can cost")
    return out


def second_metric(dev):
    """BASELINE.json's second metric, 7-Scenes APE (README.md:73-85: chess seq-01 0.032 m): runs when the released
    weights and the dataset are on the box - PI3_WEIGHTS = directory with the pi3 checkpoint (model.safetensors),
    PI3_MOGE_WEIGHTS = MoGe-2 model.pt (optional), PI3_SEVEN_SCENES = dataset root holding <scene>/seq-01/color/ - through
    the product's two offline stages with the flags of scripts/eval_7scenes.sh (chunk length / overlap of the README
    table: 100 / 20) and tools/eval_ape.py (= evo_ape tum ... -as).  Otherwise it says what is missing."""
    need = {"PI3_WEIGHTS": os.environ.get("PI3_WEIGHTS"), "PI3_SEVEN_SCENES": os.environ.get("PI3_SEVEN_SCENES")}
    base = {"metric": "7-Scenes APE (chess seq-01, Sim(3)-aligned translation RMSE, m)", "value": None,
            "reference_published": 0.032, "evaluator": "tools/eval_ape.py (restates evo_ape tum REF EST -as)"}
    missing = [k for k, v in need.items() if not v]
    if missing:
        return dict(base, note="not measurable offline: set " + " and ".join(missing) + " (released pi3 checkpoint directory, "
                               "7-Scenes root; PI3_MOGE_WEIGHTS for the metric scale) and this entry reports the APE; the "
                               "evaluator itself is tested on the reference's ground-truth file (tests/test_eval_ape.py)")
    try:
        import glob
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import eval_ape
        from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
        from pi3_slam_amd.reconstructor import OfflineReconstructor
        scene = os.environ.get("PI3_SCENE", "chess")
        frames = sorted(glob.glob(os.path.join(need["PI3_SEVEN_SCENES"], scene, "seq-01", "color", "*.png"))) or \
            sorted(glob.glob(os.path.join(need["PI3_SEVEN_SCENES"], scene, "seq-01", "*.color.png")))
        gt = os.path.join(ROOT, "tests", "golden", f"gt_7scenes_{scene}.txt")
        if not frames or not os.path.exists(gt):
            return dict(base, note=f"no frames under {need['PI3_SEVEN_SCENES']}/{scene}/seq-01 or no ground truth {gt}")
        out = tempfile.mkdtemp(prefix="pi3_ape_")
        moge_path = os.environ.get("PI3_MOGE_WEIGHTS")
        cfg = OfflineCreatorConfig(model_path=need["PI3_WEIGHTS"], output_dir=out, chunk_length=CL, overlap=OV,
                                   device=str(dev), do_metric_depth=bool(moge_path), moge_model_path=moge_path,
                                   keypoint_type="grid", max_num_keypoints=400, estimate_camera_params=True,
                                   num_loader_workers=4, device_resize=True)
        t0 = time.perf_counter()
        OfflineChunkCreator(cfg).process_and_save(frames)
        t1 = time.perf_counter()
        OfflineReconstructor(out, os.path.join(out, "reconstruction"), device=str(dev), max_observations_per_track=10).run()
        t2 = time.perf_counter()
        res = eval_ape.ape(gt, os.path.join(out, "reconstruction", "trajectory_tum.txt"))
        shutil.rmtree(out, ignore_errors=True)
        return dict(base, value=res["rmse"], unit="m", scene=scene, frames=len(frames), pose_pairs=res["pairs"],
                    scale_correction=res["scale"], mean=res["mean"], median=res["median"], max=res["max"],
                    create_s=t1 - t0, reconstruct_s=t2 - t1, metric_depth=bool(moge_path),
                    within_1mm_of_reference=abs(res["rmse"] - 0.032) <= 1e-3)
    except Exception as e:  # noqa: BLE001 - the headline line must not die on the optional metric
        return dict(base, note=f"failed: {type(e).__name__}: {e}")


def ape_proxy_product(dev) -> dict:
    """The part of the 7-Scenes APE budget this build owns, measured without weights or images:
    tools/synth_sequence.py puts a synthetic room seen from the reference-held ground-truth cameras of chess seq-01 in
    the network's place; the REAL chunk creator turns it into the 13 chunk files (masks, LM intrinsics, keypoint gather +
    fp16 pack, writer), the REAL OfflineReconstructor aligns them (closed form; then with both bundle adjustments) and
    tools/eval_ape.py scores the trajectory.  The fp64 oracle runs over the same files in the cpu_baseline leg."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import eval_ape
        import synth_sequence as ss
        from pi3_slam_amd.reconstructor import OfflineReconstructor
        gt = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")
        seq = ss.SyntheticSequence(gt, chunk_length=CL, overlap=OV, max_kp=KP)
        tmp = tempfile.mkdtemp(prefix="pi3_ape_proxy_")
        t0 = time.perf_counter()
        ss.write_chunks_product(seq, tmp, str(dev))
        t1 = time.perf_counter()
        OfflineReconstructor(tmp, os.path.join(tmp, "closed"), device=str(dev), bundle_adjust=False).run()
        t2 = time.perf_counter()
        OfflineReconstructor(tmp, os.path.join(tmp, "ba"), device=str(dev), bundle_adjust=True,
                             max_observations_per_track=10).run()
        t3 = time.perf_counter()
        closed = eval_ape.ape(gt, os.path.join(tmp, "closed", "trajectory_tum.txt"))
        ba = eval_ape.ape(gt, os.path.join(tmp, "ba", "trajectory_tum.txt"))
        # BASELINE configs[2]: the other six sequences whose ground truth the reference ships (closed form only)
        others = {}
        for i, scene in enumerate(("fire", "heads", "office", "pumpkin", "redkitchen", "stairs")):
            g2 = os.path.join(ROOT, "tests", "golden", f"gt_7scenes_{scene}.txt")
            if not os.path.exists(g2):
                continue
            d2 = os.path.join(tmp, "scene_" + scene)
            s2 = ss.SyntheticSequence(g2, chunk_length=CL, overlap=OV, max_kp=KP, seed=8 + i)
            ss.write_chunks_product(s2, d2, str(dev))
            OfflineReconstructor(d2, os.path.join(d2, "closed"), device=str(dev), bundle_adjust=False).run()
            others[scene] = {"dir": d2, "ape_hip_m": eval_ape.ape(g2, os.path.join(d2, "closed", "trajectory_tum.txt"))["rmse"],
                             "frames": s2.n, "chunks": len(s2.chunks)}
        return {"dir": tmp, "ape_hip_m": closed["rmse"], "ape_hip_with_bundle_adjust_m": ba["rmse"], "pose_pairs": closed["pairs"],
                "chunks": len(seq.chunks), "noise": seq.noise, "stage1_post_network_s": t1 - t0,
                "stage2_closed_form_s": t2 - t1, "stage2_with_bundle_adjust_s": t3 - t2, "other_scenes": others}
    except Exception as e:  # noqa: BLE001 - the headline line must not die on the optional metric
        return {"note": f"failed: {type(e).__name__}: {e}"}


def ape_proxy_oracle(chunk_dir: str, scene: str = "chess") -> dict:
    """cpu_baseline leg: stage 2 of the same chunk files on the host in float64, the reference's literal order of
    operations (oracle.post_ref.reconstruct_sequence: slam/offline_reconstructor.py:110-133 +
    utils/reconstruction_alignment.py:74-105, closed form only), timed and scored."""
    import glob
    from oracle import post_ref
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_ape
    chunks = [torch.load(p, map_location="cpu", weights_only=False)
              for p in sorted(glob.glob(os.path.join(chunk_dir, "chunks", "chunk_*.pt")))]
    t0 = time.perf_counter()
    res = post_ref.reconstruct_sequence(chunks, CL, OV, "progressive")
    dt = time.perf_counter() - t0
    tum = os.path.join(chunk_dir, "oracle_tum.txt")
    post_ref.write_tum(tum, res["positions"], res["rotations"])
    a = eval_ape.ape(os.path.join(ROOT, "tests", "golden", f"gt_7scenes_{scene}.txt"), tum)
    return {"ape_oracle_m": a["rmse"], "seconds": dt, "cores": 1, "kind": "port", "chunks": len(chunks),
            "alignments_accepted": int(sum(res["ok"][1:]))}


def ape_proxy_summary(proxy: dict, oracle) -> dict:
    out = {"label": "PROXY, not the 7-Scenes metric: synthetic room on the reference-held chess seq-01 ground-truth trajectory "
                    "(1 000 frames, 13 chunks at 100 / 20, K = 200), network noise at the reference's own bf16-vs-fp32 level, "
                    "each chunk in a random similarity gauge; everything after the network is the product.  It bounds what "
                    "fp16 chunk storage, the Sim(3) solve, the f64 prefix product and the fp32 export contribute to the "
                    "'within 1 mm of the reference' budget (tests/test_ape_proxy_gpu.py gates delta_mm < 1)"}
    out.update({k: v for k, v in proxy.items() if k not in ("dir", "other_scenes")})
    scenes = {}
    for scene, o in (proxy.get("other_scenes") or {}).items():
        scenes[scene] = {k: v for k, v in o.items() if k != "dir"}
        if "ape_oracle_m" in o:
            scenes[scene]["delta_mm"] = abs(o["ape_hip_m"] - o["ape_oracle_m"]) * 1e3
    if scenes:
        out["seven_scenes"] = dict(scenes, chess={"ape_hip_m": proxy.get("ape_hip_m"), "frames": proxy.get("pose_pairs"),
                                                  "chunks": proxy.get("chunks")})
        vals = [v["ape_hip_m"] for v in out["seven_scenes"].values() if v.get("ape_hip_m") is not None]
        out["seven_scenes_mean_ape_hip_m"] = sum(vals) / len(vals)
        deltas = [v["delta_mm"] for v in scenes.values() if "delta_mm" in v]
        if deltas:
            out["seven_scenes_max_delta_mm"] = max(deltas)
    if oracle and "ape_hip_m" in proxy:
        out["ape_oracle_m"] = oracle["ape_oracle_m"]
        out["delta_mm"] = abs(proxy["ape_hip_m"] - oracle["ape_oracle_m"]) * 1e3
        out["oracle_seconds_1_core"] = oracle["seconds"]
    return out


def synthetic_ba_problem(N: int, K: int, seed: int, noise_px: float, perturb: float, W: int = 406, H: int = 308):
    """A geometrically consistent chunk for the bundle adjustment (recipe weights give none): cameras on an arc, every
    track a keypoint pixel of its own frame lifted along its ray, observed - as the reference adds observations,
    utils/chunk_reconstruction.py:161-185 - by every earlier frame and the next two when it projects inside the image.
    Returns start values perturbed from the truth (f64 numpy) and uv / valid in the dense [source][target][keypoint] layout."""
    import numpy as np
    rng = np.random.default_rng(seed)

    def rot(axis, ang):
        a = np.asarray(axis, float) / np.linalg.norm(axis)
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx

    R = np.stack([rot([0, 1, 0], 0.012 * t) @ rot([1, 0, 0], 0.004 * t) for t in range(N)])
    C = np.stack([[0.05 * t, 0.004 * t, 0.01 * t] for t in range(N)]).astype(float)
    intr = np.tile(np.array([[320.0, 330.0, W / 2.0, H / 2.0]]), (N, 1))
    px = np.stack([rng.uniform(20, W - 20, (N, K)), rng.uniform(20, H - 20, (N, K))], -1)
    d = rng.uniform(3.0, 7.0, (N, K))
    ray = np.stack([(px[..., 0] - intr[:, None, 2]) / intr[:, None, 0], (px[..., 1] - intr[:, None, 3]) / intr[:, None, 1],
                    np.ones((N, K))], -1)
    X = C[:, None, :] + np.einsum("skj,sji->ski", ray * d[..., None], R)          # world = C + R^T (ray d)
    P = np.einsum("tij,stkj->stki", R, X[:, None, :, :] - C[None, :, None, :])    # [s][t][k] camera coordinates
    z = P[..., 2]
    u = intr[None, :, None, 0] * P[..., 0] / np.where(z > 0.1, z, 1.0) + intr[None, :, None, 2]
    v = intr[None, :, None, 1] * P[..., 1] / np.where(z > 0.1, z, 1.0) + intr[None, :, None, 3]
    s_idx, t_idx = np.arange(N)[:, None, None], np.arange(N)[None, :, None]
    valid = (t_idx <= s_idx + 2) & (z > 0.1) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    uv = (np.stack([u, v], -1) + noise_px * rng.standard_normal((N, N, K, 2))) * valid[..., None]
    R0 = np.stack([rot(rng.standard_normal(3), perturb * 0.004 * rng.standard_normal()) @ R[t] for t in range(N)])
    C0 = C + perturb * 0.01 * rng.standard_normal(C.shape)
    X0 = X.reshape(N * K, 3) + perturb * 0.02 * rng.standard_normal((N * K, 3))
    return dict(R=R0, C=C0, X=X0, intr=intr, uv=uv.astype(np.float32), valid=valid.astype(np.uint8))


def extras(engine, moge, make_creator, run, dev):
    """Variants BASELINE.md §3 names, each a short run outside the headline number."""
    out = {}

    def timed(cr, src, n, kind):
        # a fresh creator pays first-use allocations (pinned pools, keypoint tables, graph-free workspaces of a new
        # shape) over its first TWO passes: round 2 timed 3 steps after one warm-up and read 481 ms where the steady
        # state is 413 ms.  Two untimed passes of two chunks each, then n timed steps.
        run(cr, src, 2, False, kind)
        run(cr, src, 2, False, kind)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run(cr, src, n, False, kind)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n

    # K = 400 grid keypoints (spacing 16, 432 -> 400)
    cr = make_creator(400)
    cr.target_size = (H, W)
    s = timed(cr, synthetic_frames_u8(CL, SRC_H, SRC_W, 77), 6, "u8")
    out["k400"] = {"frames_per_s": CL / s, "ms_per_step": s * 1e3}
    # direct 378x504 tensors ("nominal 512x384 pixel count", 912.8 TFLOP per chunk): resident fp32 frames
    cr = make_creator(KP)
    cr.target_size = (378, 504)
    big = torch.rand(1, CL, 3, 378, 504, device=dev)
    s = timed(cr, big, 4, "float")
    out["direct_378x504"] = {"frames_per_s": CL / s, "ms_per_step": s * 1e3,
                             "algorithmic_tflop_per_chunk": engine.flops(1, CL, 378, 504)["total"] / 1e12}
    del big
    # from disk: PNG files -> loader workers (decode only) -> the same pipeline -> chunk files written by the writer thread
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="pi3_bench_disk_")
    try:
        n_distinct, n_files = 100, 660                       # 8 full chunks (stride 80) + a 20-frame tail
        fr = synthetic_frames_u8(n_distinct, SRC_H, SRC_W, 5).numpy()
        os.makedirs(os.path.join(tmp, "frames"))
        files = []
        for i in range(n_files):                              # 100 distinct images, the rest are hard links to them
            p = os.path.join(tmp, "frames", f"frame_{i:05d}.png")
            if i < n_distinct:
                Image.fromarray(fr[i]).save(p, compress_level=1)
            else:
                os.link(files[i % n_distinct], p)
            files.append(p)
        cr = make_creator(KP, os.path.join(tmp, "out"), workers=min(8, max(2, len(os.sched_getaffinity(0)) // 2)))
        cr.process_and_save(files[:120])                      # tables, graphs of both chunk shapes: untimed
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        saved = cr.process_and_save(files)
        dt = time.perf_counter() - t0
        nfr, steady = cr.last_run["frames"], cr.last_run["wall_after_first_chunk_decoded_s"]
        out["from_disk_process_and_save"] = {
            "frames_per_s": nfr / steady, "frames_per_s_incl_loader_start": nfr / dt, "frames": nfr, "chunks": len(saved),
            "wall_s": dt, "wall_after_first_chunk_decoded_s": steady, "loader_workers": cr.config.num_loader_workers,
            "note": "660 PNG files 512x384 (100 distinct), decoded by the loader workers, device resize, chunk files written "
                    "by the writer thread.  frames_per_s counts from the moment the first decoded chunk leaves the loader "
                    "(worker processes forked and first 100 PNGs decoded), frames_per_s_incl_loader_start from the call"}
        # stage 2 of the offline flow (reconstruct_offline.py -> OfflineReconstructor.run, the reference's "Reconstruction
        # FPS", slam/offline_reconstructor.py:114-125) over the chunk files just written: load, Sim(3) chain, TUM / PLY
        from pi3_slam_amd.reconstructor import OfflineReconstructor
        stage2 = {}
        for tag, ba in (("closed_form_only", False), ("with_bundle_adjust", True)):
            rec = OfflineReconstructor(os.path.join(tmp, "out"), os.path.join(tmp, "rec_" + tag), device=str(dev),
                                       bundle_adjust=ba)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            rec.run()
            torch.cuda.synchronize(dev)
            dt2 = time.perf_counter() - t0
            stage2[tag] = {"frames_per_s": nfr / dt2, "wall_s": dt2, "chunks": len(saved)}
        out["reconstruct_stage2"] = dict(stage2, note=(
            "OfflineReconstructor.run over the 9 chunk files of from_disk_process_and_save (torch.load, alignment of every "
            "chunk to its predecessor, trajectory_tum.txt + ply files).  with_bundle_adjust adds the per-chunk (10 LM "
            "iterations) and prior-constrained (50) device bundle adjustment on recipe-weight geometry, i.e. its cost "
            "on data it cannot improve"))
        # configs[4] on one GPU: a 4 000-frame 512x384 stream through the online sliding-window class (chunk-parallel
        # over ranks when a process group exists; here one rank), hipGraph-captured per-chunk forward, in-order results
        from pi3_slam_amd.online import Pi3SLAMOnline
        n_stream = 4000
        sdir = os.path.join(tmp, "stream")
        os.makedirs(sdir)
        stream_files = []
        for i in range(n_stream):
            q = os.path.join(sdir, f"frame_{i:05d}.png")
            os.link(files[i % n_distinct], q)
            stream_files.append(q)
        workers = min(8, max(2, len(os.sched_getaffinity(0)) // 2))
        online = {}
        for mode, graph in (("hip_graph", True), ("eager", False), ("hip_graph_reuse_overlap", True)):
            slam = Pi3SLAMOnline(model=engine, chunk_length=CL, overlap=OV, device=str(dev), keypoint_type="grid",
                                 max_num_keypoints=KP, do_metric_depth=moge is not None, moge_model=moge, hip_graph=graph,
                                 output_dir=os.path.join(tmp, "online_" + mode), bundle_adjust=False,
                                 num_loader_workers=workers, reuse_overlap_encoder=mode.endswith("reuse_overlap"))
            slam.process_chunks(stream_files[:260])           # graph capture of the chunk shape: untimed
            torch.cuda.synchronize(dev)
            before = slam.get_statistics()["num_frames"]
            t0 = time.perf_counter()
            res = slam.process_chunks(stream_files)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            st = slam.get_timing_statistics()
            online[mode] = {
                "frames_per_s": n_stream / dt, "chunk_frames_per_s": sum(r["chunk"]["_metrics"]["num_frames"] for r in res) / dt,
                "chunks": len(res), "wall_s": dt, "new_frames_accounted": slam.get_statistics()["num_frames"] - before,
                "pi3_forward_ms_mean": 1e3 * st.get("pi3_forward", {}).get("mean_s", float("nan")),
                "consume_ms_max": 1e3 * st.get("consume_chunk", {}).get("max_s", float("nan")),
                "encoder_frames_reused": slam._creator.reused_frames}
            del slam
        out["online_stream_4k"] = dict(
            online["hip_graph"], hip_graph=True, bundle_adjust=False, input_frames=n_stream,
            eager_launches=online["eager"], reuse_overlap_encoder=online["hip_graph_reuse_overlap"],
            note="Pi3SLAMOnline.process_chunks on 4000 PNG files (100 distinct), cl=100 ov=20 -> 50 chunks; decode threads, "
                 "device resize, hipGraph replay of the forward (eager_launches: the same run with plain launches; "
                 "reuse_overlap_encoder: the opt-in switch that takes the 20 overlap frames' encoder output from the previous "
                 "chunk - same bits, less work, so it is reported here and never in the headline), "
                 "Sim(3) alignment of every chunk to its predecessor, results drained in order.  frames_per_s counts input "
                 "frames (every chunk re-processes its 20 overlap frames: chunk_frames_per_s).  Bundle adjustment is off: "
                 "recipe weights give no consistent geometry")
        # configs[3] shape: EuRoC 752x480 frames, the reference's own cam0 calibration (undistortion on the device),
        # -> 280x448, --estimate-intrinsics, grid K = 200
        calib = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "calib_euroc_cam0_calib.json")
        if os.path.exists(calib):
            edir = os.path.join(tmp, "euroc")
            os.makedirs(edir)
            efr = synthetic_frames_u8(50, 480, 752, 6).numpy()
            efiles = []
            for i in range(340):                              # 4 full chunks (stride 80) + a 20-frame tail
                q = os.path.join(edir, f"{1403636579763555584 + i * 50000000}.png")
                if i < 50:
                    Image.fromarray(efr[i]).save(q, compress_level=1)
                else:
                    os.link(efiles[i % 50], q)
                efiles.append(q)
            from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
            cc = OfflineCreatorConfig(model_path="recipe", output_dir=os.path.join(tmp, "euroc_out"), chunk_length=CL,
                                      overlap=OV, device=str(dev), do_metric_depth=moge is not None, keypoint_type="grid",
                                      max_num_keypoints=KP, estimate_camera_params=True, cam_dist_path=calib,
                                      num_loader_workers=min(8, max(2, len(os.sched_getaffinity(0)) // 2)),
                                      device_resize=True)
            ecr = OfflineChunkCreator(cc, model=engine, moge_model=moge)
            ecr.process_and_save(efiles[:120])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            saved = ecr.process_and_save(efiles)
            dt = time.perf_counter() - t0
            out["euroc_752x480_undistort_intrinsics"] = {
                "frames_per_s": ecr.last_run["frames"] / ecr.last_run["wall_after_first_chunk_decoded_s"],
                "frames_per_s_incl_loader_start": ecr.last_run["frames"] / dt, "frames": ecr.last_run["frames"],
                "chunks": len(saved), "target_size": list(ecr.target_size),
                "undistortion_on_device": ecr.undistortion_maps is not None,
                "note": "340 PNG files 752x480 (50 distinct) + calib_euroc_cam0_calib.json: decode threads, device "
                        "undistortion + resize to 280x448 (S = 64 500), forward, masks, scale, LM intrinsics, K = 200 gather, "
                        "chunk files written"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # the per-chunk bundle adjustment (10 LM iterations, Huber 2.0) at the chunk size of the headline
    import numpy as np
    from pi3_slam_amd import ops
    pb = synthetic_ba_problem(CL, KP, seed=3, noise_px=0.5, perturb=1.0)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    uv_d, valid_d, intr_d = to(pb["uv"]), to(pb["valid"]), to(pb["intr"])
    times, summary = [], None
    for rep in range(3):
        pts = to(pb["X"])
        rc = to(np.concatenate([pb["R"].reshape(CL, 9), pb["C"]], 1))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        summary = ops.bundle_adjust(pts, rc, intr_d, uv_d, valid_d, 2.0, 10).cpu().numpy()
        times.append(time.perf_counter() - t0)
    forms = {}
    for form, kw in (("homogeneous_points_reference_default", dict(homogeneous=True)), ("inverse_depth", dict(inverse_depth=True))):
        tf, sf = [], None
        for rep in range(2):
            pts = to(pb["X"])
            rc = to(np.concatenate([pb["R"].reshape(CL, 9), pb["C"]], 1))
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            sf = ops.bundle_adjust(pts, rc, intr_d, uv_d, valid_d, 2.0, 10, **kw).cpu().numpy()
            tf.append(time.perf_counter() - t0)
        forms[form] = {"ms_total": 1e3 * min(tf), "lm_iterations": int(sf[5]), "accepted_steps": int(sf[6]),
                       "ms_per_lm_iteration": 1e3 * min(tf) / max(1, int(sf[5])), "final_cost": float(sf[0])}
    out["bundle_adjust_chunk"] = {
        "point_parametrization": "euclidean (pi3_bundle_adjust); other_forms: the reference's default and --use-inverse-depth",
        "other_forms": forms,
        "ms_total": 1e3 * min(times), "lm_iterations": int(summary[5]), "accepted_steps": int(summary[6]),
        "ms_per_lm_iteration": 1e3 * min(times) / max(1, int(summary[5])),
        "initial_cost": float(summary[8]), "final_cost": float(summary[0]), "cameras": CL, "tracks": CL * KP,
        "observations": int(pb["valid"].sum()),
        "note": "pi3_bundle_adjust on a synthetic consistent chunk (0.5 px noise, perturbed start), the reference's "
                "observation pattern (every earlier frame + the next two), per-chunk settings of "
                "utils/chunk_reconstruction.py:188-219; not part of the headline (recipe weights give no geometry to refine)"}
    return out


if __name__ == "__main__":
    _args = parse_args()
    if _args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher.  Nothing above has touched the GPU (module imports only).
        _argv = sys.argv[1:]
        if _args.dump_outputs:        # the ranks run in the repository root: hand them the directory as an absolute path
            _argv += ["--dump-outputs", os.path.abspath(_args.dump_outputs)]
        sys.exit(launch_ranks(_args.gpus, _argv))
    # stdout carries exactly ONE line, the JSON record of rank 0; the pipeline's progress prints (per-chunk inference
    # FPS etc., on every rank) go to stderr
    _REAL_STDOUT = sys.stdout
    sys.stdout = sys.stderr
    try:
        main(_args)
    finally:
        sys.stdout = _REAL_STDOUT
