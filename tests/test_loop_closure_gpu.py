"""Loop closure on the GPU: the co-occupancy kernel (csrc/chunk_overlap.hip) byte for byte and the pose-graph solver
(csrc/pose_graph.hip) step for step against the numpy oracle (tests/loop_closure_ref.py), then close_loops end to end
on exact chunks of the chess room, on the same chunks with an injected drift, and on inputs it has nothing to do for."""
import copy
import os
import shutil
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import loop_closure_ref as ref                    # noqa: E402
import test_dense_consistency_gpu as cons_gpu     # noqa: E402  (the creator's work items)
import test_dense_follow_gpu as follow_gpu        # noqa: E402  (_reconstruct, _tree, the chess ground truth)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. co-occupancy
INV_CELL = 4.0                   # cells of 0.25
SHARED = (0.125, -0.125, 0.625)  # the centre of the cell every chunk gets a point in


def _overlap_case(P, C, seed=0):
    """P points for C chunks (offsets with empty chunks among them).  Uniform in [-2, 2]^3, negative coordinates
    included; every 5th on a cell face (a multiple of 0.25 on one axis), every 7th beside its predecessor (several points
    of one chunk in one cell), every 11th NaN or inf, every 13th at or beyond 2^20 cells; the first point of every
    non-empty chunk in the shared cell."""
    rng = np.random.default_rng([seed, P, C])
    cuts = np.sort(rng.integers(0, P + 1, C - 1)) if C > 1 else np.zeros(0, np.int64)
    offsets = np.r_[0, cuts, P].astype(np.int64)
    X = rng.uniform(-2.0, 2.0, (P, 3))
    rows = np.arange(P)
    face = rows % 5 == 1
    X[face, rng.integers(0, 3, int(face.sum()))] = rng.integers(-8, 9, int(face.sum())) * 0.25
    near = np.flatnonzero((rows % 7 == 2) & (rows > 0))
    X[near] = X[near - 1] + rng.uniform(-0.01, 0.01, (len(near), 3))
    X = X.astype(np.float32)
    bad = np.flatnonzero(rows % 11 == 5)
    X[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(bad))
    far = np.flatnonzero(rows % 13 == 7)
    X[far, rng.integers(0, 3, len(far))] = rng.choice(np.array([2.0 ** 18, -2.0 ** 18 - 0.1, 3e30], np.float32), len(far))
    for c in range(C):
        if offsets[c + 1] > offsets[c]:
            X[offsets[c]] = np.asarray(SHARED, np.float32) + rng.uniform(-0.1, 0.1, 3).astype(np.float32)
    return X, offsets


def _overlap_device(X, offsets):
    from pi3_slam_amd import ops
    P, C = len(X), len(offsets) - 1
    table = torch.full((ops.voxel_capacity(P) * 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    counts = torch.full((C, C), -3, dtype=torch.int64, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    ops.chunk_cooccupancy(_dev(X).reshape(P, 3), _dev(offsets), INV_CELL, table, counts, counters)
    return counts.cpu().numpy().view(np.uint64), counters.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("P", [0, 1, 257, 5000])
@pytest.mark.parametrize("C", [1, 2, 65, 448])
def test_cooccupancy_matches_the_oracle_byte_for_byte(C, P):
    X, offsets = _overlap_case(P, C)
    exp_counts, exp_counters = ref.cooccupancy(X, offsets, INV_CELL)
    if P == 5000:        # the inputs do what the docstring says, on the oracle, before the device is asked
        assert exp_counters[0] > P // 13 and exp_counters[3] == np.count_nonzero(np.diff(offsets))
        assert exp_counters[1] < P - exp_counters[0]                           # cells hold several points
        if C == 448:
            assert offsets[-1] > offsets[-2] and exp_counts[447, 447] > 0      # the last bit of the last word is in use
        if C >= 65:
            assert np.count_nonzero(exp_counts[64:, :64]) > 0                  # pairs across the mask words
    got_counts, got_counters = _overlap_device(X, offsets)
    assert got_counts.shape == exp_counts.shape and got_counts.tobytes() == exp_counts.tobytes(), (C, P)
    assert got_counters.tobytes() == exp_counters.tobytes(), (got_counters, exp_counters)
    again_counts, again_counters = _overlap_device(X, offsets)
    assert again_counts.tobytes() == got_counts.tobytes() and again_counters.tobytes() == got_counters.tobytes()
    print(f"C={C} P={P}: counters {got_counters.tolist()}, pairs {int(np.count_nonzero(np.triu(got_counts, 1)))}")


def test_cooccupancy_argument_errors_leave_the_outputs_alone():
    from pi3_slam_amd import lib as L
    lib = L.load()
    X, offsets = _overlap_case(257, 2)
    pts, off = _dev(X), _dev(offsets)
    table = torch.zeros(1024 * 8, dtype=torch.int64, device=DEV)
    counts = torch.full((2, 2), -3, dtype=torch.int64, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)

    def call(P=257, C=2, inv=INV_CELL, cap=1024):
        return lib.pi3_chunk_cooccupancy(pts.data_ptr(), P, off.data_ptr(), C, inv, table.data_ptr(), cap, counts.data_ptr(),
                                         counters.data_ptr(), L.stream_ptr())

    for kw in (dict(C=449), dict(cap=1000), dict(cap=512), dict(P=-1), dict(inv=0.0), dict(inv=float("nan"))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert counts.tolist() == [[-3, -3], [-3, -3]] and counters.tolist() == [11] * 4
    assert call() == 0
    torch.cuda.synchronize()
    exp_counts, exp_counters = ref.cooccupancy(X, offsets, INV_CELL)
    assert counts.cpu().numpy().view(np.uint64).tobytes() == exp_counts.tobytes()
    assert counters.cpu().numpy().view(np.uint64).tobytes() == exp_counters.tobytes()


# ------------------------------------------------------------------------------------------------ 2. the pose graph
def _spd(rng, scale):
    J = rng.normal(size=(40, 7)) * np.array([1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    return (J.T @ J) * scale


def _plane_information(rng):
    """Point to plane against ONE plane: j = (x x n, x.n, n) for points x of the plane about a centre on it; the sum of
    j j^T has rank 3 (a turn about an axis in the plane, the scale's share along n, the shift along n)."""
    n = np.array([0.0, 0.0, 1.0])
    x = np.c_[rng.uniform(-1, 1, (60, 2)), np.zeros(60)]
    j = np.c_[np.cross(x, n), x @ n, np.tile(n, (60, 1))]
    O = j.T @ j
    assert np.linalg.matrix_rank(O) == 3
    return O * 50.0


def _graph(C, seed, extra=(), fixed=(0,), isolated=(), plane_edge=None, duplicate=()):
    """C nodes along a noisy loop; sequential edges between consecutive connected nodes, `extra` loop edges, each
    measurement the true relative similarity times a small error; the nodes start on the chain of the sequential
    measurements (their residuals start at zero), so the loop edges are what the solver has to reconcile."""
    rng = np.random.default_rng([seed, C])
    truth = []
    for k in range(C):
        a = 2.0 * np.pi * k / max(C, 8)
        x = np.r_[rng.normal(size=3) * 0.3, rng.normal() * 0.05, 2.0 * np.cos(a), 2.0 * np.sin(a), 0.1 * rng.normal()]
        truth.append(ref.sim3_increment(x, np.zeros(3)))
    linked = [k for k in range(C) if k not in isolated]
    edges = [(a, b) for a, b in zip(linked, linked[1:])] + list(extra)
    edges += [edges[q] for q in duplicate]
    Z, info, ecentres = [], [], []
    for e, (i, j) in enumerate(edges):
        err = ref.sim3_increment(rng.normal(size=7) * np.r_[[0.004] * 3, 0.002, [0.01] * 3], rng.normal(size=3))
        Z.append(ref.sim_inv(truth[i]) @ truth[j] @ err)
        info.append(_plane_information(rng) if e == plane_edge else _spd(rng, rng.uniform(50.0, 400.0)))
        ecentres.append(rng.normal(size=3) * 0.5)
    nodes = list(truth)
    for e, (i, j) in enumerate(edges[:len(linked) - 1]):          # the chain: W_j = W_i Z
        nodes[j] = nodes[i] @ Z[e]
    for k in isolated:
        nodes[k] = truth[k]
    centres = np.stack([M[:3, 3] + rng.normal(size=3) * 0.2 for M in nodes])
    fx = np.zeros(C, np.uint8)
    fx[list(fixed)] = 1
    return dict(nodes=np.stack(nodes), centres=centres, edges=np.array(edges, np.int32).reshape(-1, 2), Z=np.stack(Z),
                ecentres=np.stack(ecentres), info=np.stack([ref.info_upper(O) for O in info]), fixed=fx)


GRAPHS = {
    "two_nodes_duplicate_edge": dict(C=2, seed=1, duplicate=(0,)),
    "three_nodes_fixed_middle": dict(C=3, seed=2, extra=((0, 2),), fixed=(1,)),
    "ten_nodes_isolated_plane_duplicates": dict(C=10, seed=3, extra=((0, 8), (2, 7), (1, 5)), isolated=(9,), plane_edge=10,
                                                duplicate=(3, 9)),
    "sixty_five_nodes": dict(C=65, seed=4, extra=((0, 64), (3, 40), (10, 30), (20, 60), (5, 50), (33, 34))),
}


def _solve_device(g, iters):
    from pi3_slam_amd import ops
    nodes = _dev(g["nodes"]).clone()
    out = ops.pose_graph_sim3(nodes, _dev(g["centres"]), _dev(g["edges"]), _dev(g["Z"]), _dev(g["ecentres"]), _dev(g["info"]),
                              _dev(g["fixed"]), iters)
    return nodes.cpu().numpy(), out.cpu().numpy()


@pytest.fixture(scope="module")
def oracle_runs():
    """The oracle's answers, computed once per graph: after one iteration and at convergence."""
    runs = {}
    for name, kw in GRAPHS.items():
        g = _graph(**kw)
        runs[name] = (g, {it: ref.pose_graph(g["nodes"], g["centres"], g["edges"], g["Z"], g["ecentres"], g["info"],
                                             g["fixed"], it) for it in (0, 1, 50)})
    return runs


@pytest.mark.parametrize("name", list(GRAPHS))
def test_pose_graph_matches_the_oracle(oracle_runs, name):
    """Tolerances as tests/test_ba_gpu.py holds the f64 bundle adjuster to: cost 1e-9 relative, the node matrices 1e-7
    after one step and 1e-6 at convergence; iterations and accepted steps equal."""
    g, exp = oracle_runs[name]
    C = len(g["nodes"])
    for it, tol in ((0, 0.0), (1, 1e-7), (50, 1e-6)):
        W, o = exp[it]
        nodes, out = _solve_device(g, it)
        print(f"{name} max_iterations={it}: device out {out[:6].tolist()}, oracle {o}, "
              f"max |W - oracle| {np.abs(nodes - W).max():.3g}")
        assert out[6:].tolist() == [0.0] * 10
        assert int(out[2]) == o["iterations"] and int(out[3]) == o["accepted_steps"] and int(out[5]) == o["status"]
        assert abs(out[1] - o["initial_cost"]) <= 1e-9 * o["initial_cost"]
        assert abs(out[0] - o["final_cost"]) <= 1e-9 * o["final_cost"]
        assert abs(out[4] - o["lambda"]) <= 1e-12 * o["lambda"]
        assert np.abs(nodes - W).max() <= tol
        if it == 0:      # the identity: the input's bits
            assert nodes.tobytes() == g["nodes"].tobytes() and o["status"] == 1 and out[0] == out[1]
        fixed_or_alone = [k for k in range(C) if g["fixed"][k] or not np.any(g["edges"] == k)]
        assert fixed_or_alone and all(nodes[k].tobytes() == g["nodes"][k].tobytes() for k in fixed_or_alone)
        again, out2 = _solve_device(g, it)
        assert again.tobytes() == nodes.tobytes() and out2.tobytes() == out.tobytes()
    W, o = exp[50]
    assert o["status"] == 0 and o["accepted_steps"] >= 2 and o["final_cost"] < 0.9 * o["initial_cost"]


def test_pose_graph_leaves_out_an_edge_that_names_no_node():
    g = _graph(**GRAPHS["three_nodes_fixed_middle"])
    base, out = _solve_device(g, 50)
    more = dict(g)
    more["edges"] = np.r_[g["edges"], np.array([[0, 3], [-1, 1], [2, 2]], np.int32)]
    for k in ("Z", "ecentres", "info"):
        more[k] = np.r_[g[k], g[k][:3]]
    nodes, out2 = _solve_device(more, 50)
    assert nodes.tobytes() == base.tobytes() and out2.tobytes() == out.tobytes()


# ------------------------------------------------------------------------------------------------ 2b. the truncated ICP step
def _corner(n, seed):
    """Three mutually perpendicular 2 x 2 patches that meet in the point (0.3, -0.2, 0.5), n points each with 0.3 mm of
    noise along the normal, and their normals."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for a in range(3):
        p = np.zeros((n, 3))
        p[:, (a + 1) % 3], p[:, (a + 2) % 3] = rng.uniform(0.0, 2.0, n), rng.uniform(0.0, 2.0, n)
        p[:, a] = rng.normal(size=n) * 0.0003
        pts.append(p)
        nrm.append(np.tile(np.eye(3)[a], (n, 1)))
    return (np.concatenate(pts) + np.array([0.3, -0.2, 0.5])).astype(np.float32), np.concatenate(nrm).astype(np.float32)


def test_icp_truncate_holds_what_three_planes_leave_free():
    """Two samplings of one corner, already in place.  A scaling about the corner maps every plane onto itself, so point
    to plane with scale has one direction the surfaces do not hold (its eigenvalue: 3e-6 of the largest, on the numpy
    restatement of this case): the plain solve steps along it on the noise, the truncated one (1e-3) solves the other
    six and stays.  Bound: the transform within 1e-3 of the identity in the chart, three times the points' noise."""
    from pi3_slam_amd import map_eval
    ref_pts, ref_nrm = _corner(1500, 1)
    est_pts, _ = _corner(1200, 2)
    centre = ref_pts.astype(np.float64).mean(0)
    kw = dict(mode="plane", ref_normals=ref_nrm, with_scale=True, max_dist=0.1, device=DEV)
    plain = map_eval.icp_refine(est_pts, ref_pts, **kw)
    held = map_eval.icp_refine(est_pts, ref_pts, truncate=1e-3, **kw)
    x_plain, x_held = ref.chart(plain["transform"], centre), ref.chart(held["transform"], centre)
    print(f"plain: {plain['status']} after {plain['iterations']}, first step {plain['history'][0]['step']}, chart "
          f"{np.round(x_plain, 4).tolist()}; truncated: {held['status']} after {held['iterations']}, kept "
          f"{[h['kept'] for h in held['history']]}, chart {np.round(x_held, 5).tolist()}")
    assert all("kept" not in h for h in plain["history"])
    assert plain["history"][0]["step"] > 0.1 or np.abs(x_plain).max() > 0.01        # the walk this is about
    assert held["status"] == "converged" and all(h["kept"] == 6 for h in held["history"])
    assert np.abs(x_held).max() <= 1e-3


# ------------------------------------------------------------------------------------------------ 3. end to end
VOXEL = 0.02
SCENE = dict(n_frames=120, chunk_length=20, overlap=5, H=154, W=203)


def _create(seq, out_dir):
    """test_dense_follow_gpu._create with dense normals and without depth keyframes."""
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, max_num_keypoints=seq.max_kp, num_loader_workers=0,
                               keypoint_type="grid", estimate_camera_params=True, dense_voxel_size=VOXEL,
                               dense_normals=True)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    done = list(cr.process_chunks(cons_gpu._items(seq, cr.device, tuple(range(len(seq.chunks))))))
    _, manifest, _ = cr.write_chunks(iter(done))
    cr.write_run_metadata(manifest)


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    import synth_sequence as ss
    tmp = tmp_path_factory.mktemp("loops")
    seq = ss.SyntheticSequence(follow_gpu.GT, noise=dict(ss.NOISE_NONE), **SCENE)
    _create(seq, str(tmp / "chunks"))
    runs = {"unasked": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "unasked"), bundle_adjust=False),
            "off": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "off"), bundle_adjust=False, loop_closure=False,
                                           loop_max_dist=0.15, loop_cell=0.2),
            "on": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "on"), bundle_adjust=False, loop_closure=True)}
    return seq, tmp, runs


def _centroids(chunks):
    """The world place of every chunk's cloud centroid (f64), through dense_map.chunk_transform."""
    from pi3_slam_amd.dense_map import chunk_transform
    out = []
    for c in chunks:
        g = c["dense_cloud"]["points"].double().mean(0).numpy()
        M = chunk_transform(c).numpy()
        out.append(M[:3, :3] @ g + M[:3, 3])
    return np.stack(out)


def test_flag_off_is_byte_identical_to_not_asking(room):
    seq, tmp, runs = room
    off, unasked = follow_gpu._tree(tmp / "off"), follow_gpu._tree(tmp / "unasked")
    assert len(seq.chunks) == 8 and len(runs["off"].reconstructions) == 8
    assert set(off) == set(unasked) and "dense_points.ply" in off and "trajectory_tum.txt" in off
    assert all(off[k] == unasked[k] for k in off) and "loop_closure.json" not in off
    assert runs["off"].loop_closure_info is None and runs["unasked"].loop_closure_info is None


def test_loop_closure_on_exact_chunks_finds_edges_and_moves_nothing(room):
    """Exact geometry: a correction above half a voxel is a defect.  Measured on an MI355X: 21 candidates,
    9 measured, 9 accepted (rms 0.0003 - 0.0007), the solve converges in 5 iterations, the centroids move by at most
    0.00026 against the bound 0.01."""
    import json
    seq, tmp, runs = room
    info = runs["on"].loop_closure_info
    assert json.load(open(tmp / "on" / "loop_closure.json"))["participants"] == info["participants"] == list(range(8))
    accepted = [c for c in info["candidates"] if c.get("outcome") == "accepted"]
    moved = np.linalg.norm(_centroids(runs["on"].reconstructions) - _centroids(runs["off"].reconstructions), axis=1)
    print(f"exact chunks: {len(info['candidates'])} candidates, {len(accepted)} accepted, solver {info.get('solver')}, "
          f"counters {info['cooccupancy_counters']}; centroid moves {np.round(moved, 6).tolist()} (max {moved.max():.3g}); "
          f"{info['seconds']:.2f} s")
    for c in info["candidates"]:
        print("  ", {k: c[k] for k in ("i", "j", "overlap", "taken", "outcome", "pairs", "rms") if k in c})
    assert len(accepted) >= 1 and len(info["edges"]) == len(accepted)
    assert moved.max() <= 0.5 * VOXEL
    on = follow_gpu._tree(tmp / "on")
    assert set(on) == set(follow_gpu._tree(tmp / "off")) | {"loop_closure.json"}


def test_loop_closure_takes_out_an_injected_drift(room):
    """Chunk c of the finished (exact) chunks is moved by delta^c, delta = 0.2 degrees about a fixed axis, scale 1.002,
    4 mm; close_loops(loop_max_dist=0.15) has to bring the clouds' centroids back: rms over chunks 2..7 at most half of
    the drifted input's, and no chunk farther off than it started.
    Measured on an MI355X: 10 loop edges, 5 iterations; centroid errors before 0.0081 ... 0.0655 (rms over
    chunks 2..7 0.04366), after 0.0081 ... 0.0223 (rms 0.01544, bound 0.02183); chunk 1, which no accepted edge ties to
    chunk 0, keeps its 0.0081."""
    from pi3_slam_amd.alignment import apply_world_correction
    from pi3_slam_amd.loop_closure import close_loops
    seq, tmp, runs = room
    chunks = copy.deepcopy(runs["off"].reconstructions)
    home = _centroids(chunks)
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    delta = ref.sim3_increment(np.r_[axis * np.radians(0.2), np.log(1.002), np.array([0.004, 0.0, 0.0])], np.zeros(3))
    for c, chunk in enumerate(chunks):
        if c:
            apply_world_correction(chunk, torch.from_numpy(np.linalg.matrix_power(delta, c)), DEV)
    before = np.linalg.norm(_centroids(chunks) - home, axis=1)
    info = close_loops(chunks, DEV, loop_max_dist=0.15)
    after = np.linalg.norm(_centroids(chunks) - home, axis=1)
    rms = lambda d: float(np.sqrt(np.mean(d[2:8] ** 2)))          # noqa: E731
    print(f"injected drift: before {np.round(before, 5).tolist()} (rms 2..7 {rms(before):.5f}), after "
          f"{np.round(after, 5).tolist()} (rms {rms(after):.5f}); {len(info['edges'])} loop edges, solver {info.get('solver')}")
    for c in info["candidates"]:
        print("  ", {k: c[k] for k in ("i", "j", "overlap", "taken", "outcome", "pairs", "rms") if k in c})
    assert before[1:].min() > 0.0 and info["applied"]
    assert rms(after) <= 0.5 * rms(before)
    assert np.all(after <= before + 1e-12)


def _strip_clouds(src, dst, keep):
    """The chunk files of `src` with the dense cloud left only in the chunks listed in `keep`."""
    os.makedirs(os.path.join(dst, "chunks"))
    for c, name in enumerate(sorted(n for n in os.listdir(os.path.join(src, "chunks")) if n.endswith(".pt"))):
        data = torch.load(os.path.join(src, "chunks", name), map_location="cpu", weights_only=False)
        if c not in keep:
            data.pop("dense_cloud", None)
        torch.save(data, os.path.join(dst, "chunks", name))
    for name in os.listdir(src):
        if os.path.isfile(os.path.join(src, name)):
            shutil.copy(os.path.join(src, name), os.path.join(dst, name))


@pytest.mark.parametrize("keep", [(), (1, 5)], ids=["no_clouds", "two_participants"])
def test_nothing_to_do_is_said_once_and_changes_nothing(room, capsys, keep):
    seq, tmp, runs = room
    src = str(tmp / f"chunks_{len(keep)}")
    _strip_clouds(str(tmp / "chunks"), src, keep)
    capsys.readouterr()
    on = follow_gpu._reconstruct(src, str(tmp / f"on_{len(keep)}"), bundle_adjust=False, loop_closure=True)
    said = capsys.readouterr().out
    follow_gpu._reconstruct(src, str(tmp / f"off_{len(keep)}"), bundle_adjust=False)
    a, b = follow_gpu._tree(tmp / f"on_{len(keep)}"), follow_gpu._tree(tmp / f"off_{len(keep)}")
    assert said.count("Loop closure:") == 1 and "nothing to do" in said
    assert on.loop_closure_info["skipped"] == "fewer_than_three_participants"
    assert on.loop_closure_info["participants"] == list(keep)
    assert set(a) == set(b) and all(a[k] == b[k] for k in a) and "trajectory_tum.txt" in a
