"""Loop closure without a GPU: the numpy oracle (tests/loop_closure_ref.py) against closed forms - the chart and its
analytic Jacobians, the Levenberg-Marquardt on a ring whose answer is known, the co-occupancy count on a hand-countable
case - the argument checks of the two entry points (nothing launches), the candidate selection, and
alignment.apply_world_correction on a collected chunk."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loop_closure_ref as ref
from conftest import ROOT


def _rand_sim(rng, angle=0.5, shift=1.0, scale=0.2):
    return ref.sim3_increment(np.r_[rng.normal(size=3) * angle, rng.normal() * scale, rng.normal(size=3) * shift],
                              rng.normal(size=3))


# ------------------------------------------------------------------------------------------------ chart, Jacobians
def test_chart_inverts_sim3_increment():
    from pi3_slam_amd import map_eval
    rng = np.random.default_rng(0)
    c = rng.normal(size=3)
    assert np.array_equal(ref.chart(map_eval.sim3_increment(np.zeros(7), c), c), np.zeros(7))
    worst = 0.0
    for k in range(200):
        w = rng.normal(size=3)
        w *= (3.0 if k < 20 else rng.uniform(0.0, 3.0)) / np.linalg.norm(w)        # |w| up to 3 rad, twenty at 3
        x = np.r_[w, rng.uniform(-0.5, 0.5), rng.normal(size=3)]
        c = rng.normal(size=3) * 2.0
        D = map_eval.sim3_increment(x, c)
        assert np.array_equal(D, ref.sim3_increment(x, c))
        worst = max(worst, float(np.abs(ref.chart(D, c) - x).max()))
    print(f"chart(sim3_increment(x, c), c) - x: worst {worst:.3g}")
    assert worst <= 1e-12


def test_analytic_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(20):
        Wi, Wj = _rand_sim(rng), _rand_sim(rng)
        # a measurement near the nodes' relative pose (small residual) and, every fourth, far from it (a large one)
        noise = ref.sim3_increment(rng.normal(size=7) * (0.5 if k % 4 == 3 else 0.02), rng.normal(size=3))
        Z = noise @ ref.sim_inv(Wi) @ Wj
        c, gi, gj = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        r, Ji, Jj = ref.edge_jacobians(Wi, Wj, Z, c, gi, gj)
        assert np.array_equal(r, ref.edge_residual(Wi, Wj, Z, c))
        h = 1e-6
        for J, side in ((Ji, 0), (Jj, 1)):
            num = np.zeros((7, 7))
            for p in range(7):
                res = []
                for sgn in (1.0, -1.0):
                    d = np.zeros(7)
                    d[p] = sgn * h
                    A = ref.sim3_increment(d, gi) @ Wi if side == 0 else Wi
                    B = ref.sim3_increment(d, gj) @ Wj if side == 1 else Wj
                    res.append(ref.edge_residual(A, B, Z, c))
                num[:, p] = (res[0] - res[1]) / (2.0 * h)
            worst = max(worst, float(np.abs(J - num).max() / np.abs(num).max()))
    print(f"analytic vs central differences: worst relative difference {worst:.3g}")
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------ the oracle solver
def _translation(t):
    M = np.eye(4)
    M[:3, 3] = t
    return M


def test_ring_spreads_the_discrepancy_evenly():
    """n + 1 nodes on a line; n sequential edges (k, k + 1) of equal information whose measurements carry the same
    translational bias b (Z = the true step + b), one exact closing edge (0, n) of the same information.  Going round,
    the measurements disagree by n b; with pure translations and equal weights the least-squares answer gives every
    one of the n + 1 edges the residual n b / (n + 1) (up to sign).  A node that turns or scales moves its neighbours'
    relative translations through the lever arm of the step (0.55), so the closed form is exact only while rotation and
    scale stay out of the trade: their information is 1e10 against 1 for the translation, which leaves them below
    |r| |step| / 1e10 ~ 1e-12 and their effect on the translations below that times the lever."""
    n = 6
    step, b = np.array([0.5, 0.1, -0.2]), np.array([0.01, -0.02, 0.015])
    truth = [_translation(k * step) for k in range(n + 1)]
    nodes = np.stack([_translation(k * (step + b)) for k in range(n + 1)])       # the chain as its edges measured it
    edges = [(k, k + 1) for k in range(n)] + [(0, n)]
    Z = np.stack([_translation(step + b)] * n + [_translation(n * step)])
    O = np.diag([1e10, 1e10, 1e10, 1e10, 1.0, 1.0, 1.0])
    info = np.stack([ref.info_upper(O)] * (n + 1))
    ecentres = np.zeros((n + 1, 3))
    centres = nodes[:, :3, 3].copy()
    fixed = np.zeros(n + 1, np.uint8)
    fixed[0] = 1
    W, out = ref.pose_graph(nodes, centres, edges, Z, ecentres, info, fixed, 50)
    assert out["status"] == 0 and out["accepted_steps"] >= 1 and out["final_cost"] < out["initial_cost"]
    want = n * b / (n + 1)
    res = np.stack([ref.edge_residual(W[i], W[j], Z[e], ecentres[e]) for e, (i, j) in enumerate(edges)])
    assert np.abs(res[:, :4]).max() <= 1e-10
    assert np.abs(res[:n, 4:] + want).max() <= 1e-10 and np.abs(res[n, 4:] - want).max() <= 1e-10
    # node k sits at k (step + b) - k n b / (n + 1) = k step + k b / (n + 1)
    for k in range(n + 1):
        assert np.abs(W[k] - _translation(k * step + k * b / (n + 1))).max() <= 1e-10
    assert np.array_equal(W[0], truth[0])
    # zero iterations: the identity
    W0, out0 = ref.pose_graph(nodes, centres, edges, Z, ecentres, info, fixed, 0)
    assert np.array_equal(W0, nodes) and out0["status"] == 1 and out0["iterations"] == 0
    assert out0["final_cost"] == out0["initial_cost"] == out["initial_cost"]


def test_cooccupancy_oracle_on_a_hand_countable_case():
    """Cells of edge 0.5.  Chunk 0: three points in cell (0,0,0), one in (1,0,0); chunk 1: one in (0,0,0), one in
    (-1,-1,-1), a NaN row; chunk 2: one in (1,0,0), one on the face x = 1.0 (cell (2,0,0)), one beyond 2^20 cells."""
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.4], [0.49, 0.0, 0.0], [0.5, 0.1, 0.1],
                    [0.3, 0.3, 0.3], [-0.1, -0.2, -0.3], [np.nan, 0.0, 0.0],
                    [0.7, 0.2, 0.2], [1.0, 0.0, 0.0], [2.0 ** 20, 0.0, 0.0]], np.float32)
    counts, counters = ref.cooccupancy(pts, [0, 4, 7, 10], 2.0)
    assert counts.dtype == np.uint64 and counters.dtype == np.uint64
    assert counts.tolist() == [[2, 1, 1], [1, 2, 0], [1, 0, 2]]
    assert counters.tolist() == [2, 4, 0, 2]            # dropped, cells, no slot, the most chunks in one cell
    # rows outside the offsets belong to no chunk
    counts, counters = ref.cooccupancy(pts, [1, 4, 7, 9], 2.0)
    assert counts.tolist() == [[2, 1, 1], [1, 2, 0], [1, 0, 2]] and counters.tolist() == [3, 4, 0, 2]
    empty, zero = ref.cooccupancy(np.zeros((0, 3), np.float32), [0, 0, 0], 2.0)
    assert empty.tolist() == [[0, 0], [0, 0]] and zero.tolist() == [0] * 4


def test_candidate_selection_is_greedy_by_overlap():
    from pi3_slam_amd.loop_closure import select_candidates
    counts = np.array([[100, 90, 60, 50, 40],
                       [90, 100, 80, 30, 70],
                       [60, 80, 50, 45, 10],
                       [50, 30, 45, 100, 90],
                       [40, 70, 10, 90, 200]])
    got = select_candidates(counts, 2, 0.3, 1)
    # overlaps: (0,2) 60/50, (2,4) 10/50 out, (0,3) .5, (0,4) .4, (1,3) .3, (1,4) .7
    assert [(c["i"], c["j"]) for c in got] == [(0, 2), (1, 4), (0, 3), (0, 4), (1, 3)]
    assert [c["taken"] for c in got] == [True, True, False, False, False]
    assert all(c.get("outcome") == "chunk_has_max_edges" for c in got if not c["taken"])
    assert [(c["i"], c["j"]) for c in select_candidates(counts, 3, 0.45, 3)] == [(1, 4), (0, 3)]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_bound_and_built(built_lib):
    from pi3_slam_amd import lib, ops
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    dll = ctypes.CDLL(built_lib)
    for name in ("pi3_chunk_cooccupancy", "pi3_pose_graph_sim3", "pi3_pose_graph_workspace"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and name in lib.SIGNATURES and hasattr(dll, name), name
    mk = open(os.path.join(ROOT, "pi3_slam_amd", "csrc", "Makefile")).read()
    srcs = mk.split("SRCS =")[1].split("\n")[0]
    assert "chunk_overlap.hip" in srcs and "pose_graph.hip" in srcs
    assert lib.load(require_gpu=False).pi3_abi_version() == 7
    # the workspace is the sum of the solver's arrays: state, two copies of the nodes, the flags, 210 doubles and a cost
    # per edge, the matrix, the right-hand side and the step
    for C, E in ((1, 0), (3, 2), (65, 200), (448, 1500)):
        n = 7 * C
        assert ops.pose_graph_workspace(C, E) == 16 + 16 * C + 16 * C + C + 210 * E + E + n * n + n + n, (C, E)


def test_argument_errors_return_a_code_and_launch_nothing(built_lib):
    """As test_abi does for pi3_gemm: no GPU is needed, because nothing may reach one."""
    from pi3_slam_amd import lib
    dll = lib.load(require_gpu=False)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def co(P=4, C=2, inv=2.0, cap=8, points=p, offsets=p, table=p, counts=p, counters=p):
        return dll.pi3_chunk_cooccupancy(points, P, offsets, C, inv, table, cap, counts, counters, None)

    for kw in (dict(points=None, offsets=None, table=None, counts=None, counters=None), dict(C=449), dict(cap=12),
               dict(cap=4), dict(P=-1), dict(C=-1), dict(inv=0.0), dict(inv=float("nan")), dict(inv=float("inf")),
               dict(points=None), dict(offsets=None), dict(table=None), dict(counts=None), dict(counters=None)):
        assert co(**kw) == -1, kw
        assert b"pi3_chunk_cooccupancy" in dll.pi3_last_error()

    def pg(C=2, E=1, iters=5, ws=1 << 20, nodes=p, centres=p, edges=p, Z=p, ec=p, info=p, fixed=p, work=p, out=p):
        return dll.pi3_pose_graph_sim3(nodes, centres, C, edges, Z, ec, info, E, fixed, iters, work, ws, out, None)

    for kw in (dict(nodes=None, centres=None, edges=None, Z=None, ec=None, info=None, fixed=None, work=None, out=None),
               dict(E=-1), dict(C=0), dict(C=449), dict(iters=-1), dict(nodes=None), dict(centres=None), dict(edges=None),
               dict(Z=None), dict(ec=None), dict(info=None), dict(fixed=None), dict(work=None), dict(out=None)):
        assert pg(**kw) == -1, kw
        assert b"pi3_pose_graph_sim3" in dll.pi3_last_error()
    assert pg(ws=10) == -3 and b"doubles of workspace" in dll.pi3_last_error()
    n = ctypes.c_long(-7)
    for C, E, out in ((0, 0, n), (449, 0, n), (2, -1, n), (2, 1, None)):
        assert dll.pi3_pose_graph_workspace(C, E, None if out is None else ctypes.byref(out)) == -1
        assert b"pi3_pose_graph_workspace" in dll.pi3_last_error()
    assert n.value == -7 and not any(buf)                # nothing was written anywhere
    assert dll.pi3_pose_graph_workspace(2, 1, ctypes.byref(n)) == 0 and n.value > 0


# ------------------------------------------------------------------------------------------------ the correction
def _np_sim3_apply(M4, pts, poses):
    M = M4.reshape(4, 4).double()
    s = torch.linalg.det(M[:3, :3]).abs() ** (1.0 / 3.0)
    if pts is not None:
        pts.copy_((pts.double().reshape(-1, 3) @ M[:3, :3].T + M[:3, 3]).reshape(pts.shape).to(pts.dtype))
    if poses is not None:
        P = poses.double().reshape(-1, 4, 4)
        out = P.clone()
        out[:, :3, :3] = (M[:3, :3] / s) @ P[:, :3, :3]
        out[:, :3, 3] = P[:, :3, 3] @ M[:3, :3].T + M[:3, 3]
        poses.copy_(out.reshape(poses.shape).to(poses.dtype))


def _np_compose_prefix(T):
    G = T.clone().reshape(-1, 4, 4)
    for k in range(1, len(G)):
        G[k] = G[k - 1] @ G[k]
    return G.reshape(T.shape)


def test_apply_world_correction_composes_once_on_a_collected_chunk(monkeypatch):
    """A chunk as rank 0 receives it (dist.COLLECT_KEYS): world points and poses, '_sim3_global', no '_chunk_frame'."""
    from pi3_slam_amd import alignment, ops
    monkeypatch.setattr(ops, "sim3_apply", _np_sim3_apply)
    monkeypatch.setattr(ops, "sim3_compose_prefix", _np_compose_prefix)
    rng = np.random.default_rng(5)
    G = torch.from_numpy(_rand_sim(rng))
    D = torch.from_numpy(ref.sim3_increment(np.r_[0.01, -0.02, 0.015, 0.002, 0.004, -0.003, 0.001], np.zeros(3)))
    own = torch.from_numpy(rng.normal(size=(2, 5, 3)))
    own_poses = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    own_poses[:, :3, 3] = torch.from_numpy(rng.normal(size=(2, 3)))
    world, world_poses = own.clone(), own_poses.clone()
    _np_sim3_apply(G, world, world_poses)
    created = torch.from_numpy(rng.normal(size=(2, 4, 4))).float()
    cloud = {"points": torch.from_numpy(rng.normal(size=(7, 3))).float()}
    chunk = {"points": world.float(), "camera_poses": world_poses.float(), "_sim3_global": G.clone(),
             "_poses_created": created.clone(), "dense_cloud": {"points": cloud["points"].clone()}}
    before = {k: chunk[k].clone() for k in ("points", "camera_poses")}
    alignment.apply_world_correction(chunk, D, "cpu")
    want, want_poses = before["points"].clone(), before["camera_poses"].clone()
    _np_sim3_apply(D, want, want_poses)
    assert torch.equal(chunk["points"], want) and torch.equal(chunk["camera_poses"], want_poses)
    assert chunk["points"].dtype == torch.float32 and not torch.equal(chunk["points"], before["points"])
    assert torch.allclose(chunk["_sim3_global"], D @ G, rtol=0, atol=1e-14) and "_sim3_dense" not in chunk
    # once, not twice: the world values are D (G own), not D G (G own)
    once = own.clone()
    _np_sim3_apply(D @ G, once, None)
    twice = world.clone()
    _np_sim3_apply(D @ G, twice, None)
    assert float((chunk["points"].double() - once).abs().max()) <= 1e-5
    assert float((chunk["points"].double() - twice).abs().max()) > 1e-2
    assert "_chunk_frame" not in chunk and torch.equal(chunk["_poses_created"], created)
    assert torch.equal(chunk["dense_cloud"]["points"], cloud["points"])
    # a bundle-adjusted chunk: the identity as '_sim3_global', the closed form kept as '_sim3_dense'; both are composed
    chunk2 = {"points": world.float(), "camera_poses": world_poses.float(), "_sim3_global": torch.eye(4, dtype=torch.float64),
              "_sim3_dense": G.clone()}
    alignment.apply_world_correction(chunk2, D, "cpu")
    assert torch.allclose(chunk2["_sim3_global"], D, rtol=0, atol=1e-15)
    assert torch.allclose(chunk2["_sim3_dense"], D @ G, rtol=0, atol=1e-14)


def test_the_flag_is_off_by_default_and_reaches_the_cli():
    import inspect
    from pi3_slam_amd import cli, loop_closure
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    sig = inspect.signature(OfflineReconstructor.__init__).parameters
    assert sig["loop_closure"].default is False
    for k, v in loop_closure.DEFAULTS.items():
        assert sig[k].default == v, k
    a = cli.build_parser().parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert a.loop_closure is False and all(getattr(a, k) == v for k, v in loop_closure.DEFAULTS.items())
    a = cli.build_parser().parse_args(["reconstruct", "--chunks", "c", "--output", "o", "--loop-closure", "--loop-min-gap", "4",
                                       "--loop-cell", "0.25"])
    assert a.loop_closure is True and a.loop_min_gap == 4 and a.loop_cell == 0.25
    with pytest.raises(TypeError, match="unknown options"):
        loop_closure.close_loops([], "cpu", loop_bogus=1)
