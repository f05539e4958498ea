"""The dense map following bundle-adjusted poses on the GPU: the follow kernel (csrc/cloud_follow.hip) byte for byte
against the numpy oracle (tests/dense_follow_ref.py), a planted two-view case, fuse_chunks(follower=...) on hand-made
chunks, and creator -> reconstruct on the chess-room sequence with and without bundle adjustment."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dense_carve_ref as cref          # noqa: E402
import dense_follow_ref as ref          # noqa: E402
import dense_map_ref as mref            # noqa: E402
import dense_normals_ref as nref        # noqa: E402
import test_dense_carve as carve_cpu    # noqa: E402  (the floater scene and the gauged chunks)
import test_dense_consistency_gpu as cons_gpu          # noqa: E402  (the creator's work items, today's oracle map)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 0.03
HP, WP = 12, 16


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _rot(v):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(v, np.float64)).as_matrix()


def _follow_device(points, normals, views, moves, planes, stride, rel_tol, margin, in_place):
    """The kernel on sentinel-filled outputs -> the oracle's dict."""
    from pi3_slam_amd import ops
    P = len(points)
    pts, nrm = _dev(points), _dev(normals)
    out_p = pts if in_place else torch.full((P, 3), 7.0, dtype=torch.float32, device=DEV)
    out_n = None if nrm is None else (nrm if in_place else torch.full((P, 3), 7.0, dtype=torch.float32, device=DEV))
    level = torch.full((P,), 9, dtype=torch.uint8, device=DEV)
    support = torch.full((P,), -5, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    ops.cloud_follow_views(pts, nrm, _dev(views), _dev(moves), _dev(planes), stride, rel_tol, margin, out_p, out_n,
                           level, support, counters)
    if not in_place:            # the inputs are read only
        assert pts.cpu().numpy().tobytes() == points.tobytes()
        assert nrm is None or nrm.cpu().numpy().tobytes() == normals.tobytes()
    return dict(points=out_p.cpu().numpy(), normals=None if out_n is None else out_n.cpu().numpy(),
                level=level.cpu().numpy(), support=support.cpu().numpy(), counters=counters.cpu().numpy())


def _same_bytes(got, exp, what):
    for k in ("points", "normals", "level", "support", "counters"):
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


# ------------------------------------------------------------------------------------------------ 1. byte for byte
Z = 4.0                         # the surface: the plane z = 4 of the cloud's frame (exact in fp16 and as a divisor)
INF_AT = (3, 5)                 # the (row, column) of view 0's plane that holds fp16 inf
CATEGORIES = 10


def _follow_scene(P, M, S, seed=0, shift=0):
    """M cameras in front of the plane z = 4, view 0 the identity with dyadic intrinsics (its projections are exact),
    planes 12 x 16 at stride S with holes, one inf and a unit per view; P points in ten categories by (row + shift) % 10:
    0-2 on the surface, 3 in front of it, 4 behind every camera, 5 not finite, 6 on view 0's last column and row, 7 on
    half-integer pixels of view 0, 8 on view 0's inf sample, 9 beside every image."""
    rng = np.random.default_rng([seed, P, M, S])
    K = np.array([16.0 * S, 16.0 * S, 8.0 * S, 6.0 * S])
    poses = np.tile(np.eye(4), (M, 1, 1))
    for m in range(1, M):
        poses[m, :3, :3] = _rot(rng.normal(size=3) * 0.05)
        poses[m, :3, 3] = rng.normal(size=3) * 0.2
    unit = np.r_[1.0, rng.uniform(0.5, 2.0, M - 1)]
    views = cref.pack_views(poses, np.tile(K, (M, 1)), 1.0)
    views[:, ref.SCALE_AT] = unit
    pv, pu = np.meshgrid(np.arange(HP), np.arange(WP), indexing="ij")
    rays = np.stack([(S * pu - K[2]) / K[0], (S * pv - K[3]) / K[1], np.ones_like(pu, np.float64)], -1)
    planes = np.zeros((M, HP, WP), np.float16)
    for m in range(M):
        dz = rays @ poses[m, :3, :3].T[:, 2]
        planes[m] = ((Z - poses[m, 2, 3]) / dz / unit[m]).astype(np.float16)
    assert np.all(planes[0] == np.float16(Z))
    planes[rng.random(planes.shape) < 0.1] = 0.0
    planes[0, HP - 1, WP - 1] = Z                # the last sample of view 0 is no hole
    planes[0][INF_AT] = np.inf
    moves = np.zeros((M, 3, 4))
    for m in range(M):
        moves[m, :, :3] = rng.uniform(0.8, 1.3) * _rot(rng.normal(size=3) * 0.3)
        moves[m, :, 3] = rng.normal(size=3)
    X = np.zeros((P, 3))
    cat = (np.arange(P) + shift) % CATEGORIES
    n = lambda c: int((cat == c).sum())         # noqa: E731
    on = cat <= 2
    X[on] = np.c_[rng.uniform(-0.9, 0.9, on.sum()), rng.uniform(-0.6, 0.6, on.sum()), Z + rng.normal(size=on.sum()) * 0.01]
    X[cat == 3] = np.c_[rng.uniform(-0.4, 0.4, (n(3), 2)), np.full(n(3), 2.5)]
    X[cat == 4] = np.c_[rng.uniform(-0.4, 0.4, (n(4), 2)), np.full(n(4), -3.0)]
    X[cat == 5] = rng.normal(size=(n(5), 3))
    X[cat == 6] = [(WP - 1 - 8) / 16 * Z, (HP - 1 - 6) / 16 * Z, Z]
    ku, kv = rng.integers(0, WP - 1, n(7)), rng.integers(0, HP - 1, n(7))
    X[cat == 7] = np.c_[(ku + 0.5 - 8) / 16 * Z, (kv + 0.5 - 6) / 16 * Z, np.full(n(7), Z)]
    X[cat == 8] = [(INF_AT[1] - 8) / 16 * Z, (INF_AT[0] - 6) / 16 * Z, Z]
    X[cat == 9] = np.c_[np.full(n(9), 50.0), rng.uniform(-0.4, 0.4, n(9)), np.full(n(9), Z)]
    X = X.astype(np.float32)
    bad = np.flatnonzero(cat == 5)
    X[bad, rng.integers(0, 3, len(bad))] = np.where(rng.random(len(bad)) < 0.5, np.nan, np.inf).astype(np.float32)
    N = rng.normal(size=(P, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    N[np.arange(P) % 7 == 3] = 0.0               # zero normals, in every category as P grows
    if P == 1 and shift % 2:
        N[:] = 0.0
    return dict(points=X, normals=N, views=views, moves=moves.reshape(M, 12), planes=planes, cat=cat)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("M", [1, 3, 7])
@pytest.mark.parametrize("P", [1, 255, 257, 1000])
def test_follow_matches_oracle_byte_for_byte(P, M, S):
    margin = 0.02
    shifts = range(CATEGORIES) if P == 1 else (0,)        # one point: one launch per category
    scenes = [_follow_scene(P, M, S, shift=k) for k in shifts]
    exps = [{wn: ref.follow(s["points"], s["normals"] if wn else None, s["views"], s["moves"], s["planes"], S, REL_TOL,
                            margin) for wn in (False, True)} for s in scenes]
    # the inputs exercise every level, the dropped case and the edge inputs: on the oracle, before the device is asked
    levels = np.concatenate([e[True]["level"] for e in exps])
    cats = np.concatenate([s["cat"] for s in scenes])
    assert set(levels.tolist()) == {0, 1, 2, 3}
    assert sum(int(e[True]["counters"][0]) for e in exps) == int((cats == 5).sum()) > 0
    assert np.all(levels[cats == 6] == 1)                 # the last column and row are inside
    assert np.all(levels[cats == 5] == 0) and np.all(levels[cats == 4] == 3) and np.all(levels[cats == 9] == 3)
    assert np.all(levels[cats == 3] == 2) and np.all(levels[cats == 7] >= 1)
    if M == 1:
        assert np.all(levels[cats == 8] == 2)             # the only view has inf there: seen, not agreed
        assert set(levels[cats == 7].tolist()) <= {1, 2}
    for e in exps:
        assert np.array_equal(e[True]["level"], e[False]["level"]) and np.array_equal(e[True]["support"], e[False]["support"])
    zero = np.concatenate([(s["normals"] == 0).all(1) for s in scenes])
    out_n = np.concatenate([e[True]["normals"] for e in exps])
    assert zero.any() and not out_n[zero & (levels > 0)].any()
    for s, e in zip(scenes, exps):
        for wn in (False, True):
            for in_place in (False, True):
                got = _follow_device(s["points"], s["normals"] if wn else None, s["views"], s["moves"], s["planes"], S,
                                     REL_TOL, margin, in_place)
                _same_bytes(got, e[wn], (P, M, S, wn, in_place))
    print(f"P={P} M={M} S={S}: counters {[e[True]['counters'].tolist() for e in exps][:2]}")


def test_follow_without_points_zeroes_the_counters():
    from pi3_slam_amd import ops
    s = _follow_scene(1, 3, 2)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    empty = torch.zeros(0, 3, dtype=torch.float32, device=DEV)
    ops.cloud_follow_views(empty, None, _dev(s["views"]), _dev(s["moves"]), _dev(s["planes"]), 2, REL_TOL, 0.02, empty, None,
                           None, None, counters)
    assert counters.tolist() == [0, 0, 0, 0]


def test_follow_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    s = _follow_scene(257, 3, 2)
    pts, v, mv, pl = _dev(s["points"]), _dev(s["views"]), _dev(s["moves"]), _dev(s["planes"])
    out = torch.full((257, 3), 7.0, dtype=torch.float32, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)

    def call(M=3, Hp=HP, Wp=WP, stride=2, tol=0.03, margin=0.02, normals=None, out_n=None, **null):
        a = dict(points=pts.data_ptr(), views=v.data_ptr(), moves=mv.data_ptr(), planes=pl.data_ptr(), out=out.data_ptr(),
                 counters=counters.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_cloud_follow_views(a["points"], normals, 257, a["views"], a["moves"], M, a["planes"], Hp, Wp, stride,
                                          tol, margin, a["out"], out_n, None, None, a["counters"], L.stream_ptr())

    inf, nan = float("inf"), float("nan")
    for kw in [dict(M=0), dict(M=-2), dict(Hp=0), dict(Wp=-3), dict(stride=0), dict(stride=3), dict(stride=8), dict(tol=0.0),
               dict(tol=-1.0), dict(tol=inf), dict(tol=nan), dict(margin=-1e-9), dict(margin=inf), dict(margin=nan),
               dict(points=1), dict(views=1), dict(moves=1), dict(planes=1), dict(out=1), dict(counters=1),
               dict(normals=pts.data_ptr()), dict(out_n=out.data_ptr())]:
        assert call(**kw) == -1, kw
        assert b"pi3_cloud_follow_views" in lib.pi3_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and counters.tolist() == [11] * 4
    assert call() == 0
    torch.cuda.synchronize()
    assert sum(counters.tolist()) == 257 and not bool((out == 7.0).all(1).any())


# ------------------------------------------------------------------------------------------------ 2. planted exactness
def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def test_two_patches_follow_their_own_views_exactly():
    """Two cameras at (-2, 0, 0) and (2, 0, 0) look along +z at the plane z = 4; with fx = 16 S each sees 4 units of it,
    x in [-4, 0] and [0, 4]: the patch x in [-3, -1] is in the first image only, x in [1, 3] in the second only.  Both
    moves take the plane z = 4 onto the target plane n . x = d, but with different motions inside it: a point must
    follow its own view's move alone.  Any ONE 4x4 (the chunk's similarity is one) leaves the patches off their places
    by centimetres: the best-fit similarity of the whole cloud (ops.sim3_umeyama) is the witness."""
    from pi3_slam_amd import ops
    S = 2
    K = np.array([16.0 * S, 16.0 * S, 8.0 * S, 6.0 * S])
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[0, 0, 3], poses[1, 0, 3] = -2.0, 2.0
    views = cref.pack_views(poses, np.tile(K, (2, 1)), 1.0)
    planes = np.full((2, HP, WP), Z, np.float16)
    rng = np.random.default_rng(3)
    n = 300
    X = np.concatenate([np.c_[rng.uniform(-3, -1, n), rng.uniform(-1, 1, n), np.full(n, Z)],
                        np.c_[rng.uniform(1, 3, n), rng.uniform(-1, 1, n), np.full(n, Z)]]).astype(np.float32)
    own = np.r_[np.zeros(n, int), np.ones(n, int)]
    T0 = np.eye(4)                                           # the plane z = 4 -> the target plane
    T0[:3, :3], T0[:3, 3] = _rot([0.4, -0.3, 0.2]), [0.5, -1.0, 2.0]
    normal = T0[:3, 2]
    d = float(normal @ (T0[:3, :3] @ [0, 0, Z] + T0[:3, 3]))
    moves = []
    for ang, shift in ((0.05, [0.10, -0.05, 0.0]), (-0.04, [-0.08, 0.12, 0.0])):       # motions inside the plane z = 4
        A = np.eye(4)
        A[:3, :3], A[:3, 3] = _rot([0.0, 0.0, ang]), shift
        moves.append((T0 @ A)[:3])
    moves = np.stack(moves).reshape(2, 12)
    exp = ref.follow(X, None, views, moves, planes, S, REL_TOL, 0.01)
    assert np.all(exp["level"] == 1) and np.all(exp["support"] == 1)      # each patch is in its own view's image only
    got = _follow_device(X, None, views, moves, planes, S, REL_TOL, 0.01, in_place=False)
    _same_bytes(got, exp, "planted")
    D = moves.reshape(2, 3, 4)[own]
    want = (np.einsum("pij,pj->pi", D[:, :, :3], X.astype(np.float64)) + D[:, :, 3]).astype(np.float32)
    err = np.abs(got["points"].astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= _ulp32(want))                       # (w Y) / w need not be Y in f64: one fp32 ulp
    off_plane = np.abs(got["points"].astype(np.float64) @ normal - d)
    print(f"planted: max |out - fp32(D X)| {err.max():.3g}, max distance to the target plane {off_plane.max():.3g}")
    assert off_plane.max() <= 1e-5                           # fp32 storage at metres
    # one similarity for the whole cloud, the best there is: it misses the places by far more than either bound
    idx = torch.arange(2 * n, dtype=torch.int32, device=DEV).reshape(1, -1)
    sim = ops.sim3_umeyama(_dev(want).reshape(1, -1, 3), _dev(X).reshape(1, -1, 3), idx,
                           torch.eye(4, dtype=torch.float32, device=DEV), use_filter=False).cpu().numpy()
    G = sim[13:29].reshape(4, 4)
    one = X.astype(np.float64) @ G[:3, :3].T + G[:3, 3]
    miss = np.linalg.norm(one - want, axis=1)
    print(f"planted: the best single similarity misses by up to {miss.max():.3g} (median {np.median(miss):.3g})")
    assert not np.all(np.abs(one - want) <= _ulp32(want)) and np.median(miss) > 1e-2


# ------------------------------------------------------------------------------------------------ 3. fuse_chunks
def _followed_chunk(s, m, S, Kf, gauge, seed, with_planes=True):
    """carve_cpu._gauged_chunk with a cloud (the scene's map, taken into the chunk's frame), the created poses, and
    final poses that an adjustment moved view by view (a few milliradians, a centimetre)."""
    chunk = carve_cpu._gauged_chunk(s, S, Kf, gauge, with_planes=with_planes)
    G = np.eye(4) if chunk["_sim3_global"] is None else chunk["_sim3_global"].numpy()
    F = np.linalg.inv(G)
    final = chunk["camera_poses"].numpy().astype(np.float64)
    created = F[None] @ final
    created[:, :3, :3] /= np.cbrt(np.linalg.det(created[:, :3, :3]))[:, None, None]
    rng = np.random.default_rng(seed)
    for i in range(len(final)):
        dP = np.eye(4)
        dP[:3, :3], dP[:3, 3] = _rot(rng.normal(size=3) * 0.004), rng.normal(size=3) * 0.01
        final[i] = final[i] @ dP
    chunk["camera_poses"] = torch.from_numpy(final.astype(np.float32))
    chunk["_poses_created"] = torch.from_numpy(created.astype(np.float32))
    pts = (m["points"].astype(np.float64) @ F[:3, :3].T + F[:3, 3]).astype(np.float32)
    V = len(pts)
    nr = rng.normal(size=(V, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
    nr[::11] = 0.0
    chunk["dense_cloud"] = {"points": torch.from_numpy(pts), "colors": torch.from_numpy(rng.integers(0, 256, (V, 3)).astype(np.uint8)),
                            "weights": torch.from_numpy(rng.integers(1, 5, V).astype(np.int32)),
                            "normals": torch.from_numpy(nr), "normal_weights": torch.from_numpy(rng.integers(0, 4, V).astype(np.int32)),
                            "voxel_size": gauge * 0.04, "conf_threshold": 0.5}
    return chunk


def _np_chunk(chunk):
    def conv(v):
        if torch.is_tensor(v):
            return v.numpy()
        return {k: conv(x) for k, x in v.items()} if isinstance(v, dict) else v
    return {k: conv(v) for k, v in chunk.items()}


def _oracle_followed_map(chunks, voxel, rel_tol=REL_TOL, normals=True):
    """fuse_chunks(follower=...) restated: every cloud moved by the follow oracle (by the device's sim3_apply where the
    chunk cannot be followed, as today's oracle map does), fused by dense_map_ref; the normals by dense_normals_ref."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import chunk_transform, similarity_rotation
    sets, parts, levels = [], [], np.zeros(4, np.int64)
    inv_v = mref.inv_voxel(voxel)
    for d in chunks:
        cl = d.get("dense_cloud")
        if cl is None or int(cl["points"].shape[0]) == 0:
            continue
        moved = ref.follow_chunk(_np_chunk(d), rel_tol)
        if moved is not None:
            world, wn, rot9 = moved["points"], moved["normals"], np.eye(3).reshape(9)
            levels += moved["counters"]
        else:
            pts = cl["points"].to(DEV, torch.float32).contiguous().clone()
            ops.sim3_apply(chunk_transform(d).reshape(16).to(DEV).contiguous(), pts, None)
            world = pts.cpu().numpy()
            wn = cl["normals"].numpy() if normals and cl.get("normals") is not None else None
            rot9 = similarity_rotation(chunk_transform(d)).reshape(9)
        sets.append((world, cl["colors"].numpy(), cl["weights"].numpy()))
        if normals and wn is not None:
            parts.append(nref.point_normals(world, wn, cl["normal_weights"].numpy(), rot9, inv_v))
    out = mref.fuse_point_sets(sets, voxel)
    if normals and parts:
        out["normals"] = nref.extract(out["keys"], nref.accumulate(parts))["normals"]
    out["levels"] = levels
    return out


def test_fuse_chunks_with_a_follower_matches_the_oracle(capsys):
    from pi3_slam_amd.dense_map import MapFollower, fuse_chunks
    from pi3_slam_amd.online import Pi3SLAMOnline
    N, H, W, voxel, S, Kf = carve_cpu.CONFIGS[3]
    s, m, dist = carve_cpu.floater_scene(N, H, W, voxel)
    chunks = [_followed_chunk(s, m, S, Kf, 1.0, 1), _followed_chunk(s, m, S, Kf, 1.7, 2), {"camera_poses": torch.eye(4)[None]}]
    follower = MapFollower()
    capsys.readouterr()
    dense = fuse_chunks(chunks, DEV, voxel_size=voxel, follower=follower)
    said = capsys.readouterr().out
    exp = _oracle_followed_map(chunks, voxel)
    V = len(m["points"])
    assert exp["levels"].sum() == 2 * V and exp["levels"][1] > V         # most points follow views that saw them
    assert follower.last_stats == dict(chunks_followed=2, chunks_fallen_back=0, points=2 * V, dropped=int(exp["levels"][0]),
                                       level1=int(exp["levels"][1]), level2=int(exp["levels"][2]),
                                       level3=int(exp["levels"][3]))
    assert "keep their chunk's similarity" not in said and said.count("Dense map follows the poses") == 1
    for k in ("points", "colors", "weights", "normals"):
        assert getattr(dense, k).tobytes() == np.asarray(exp[k]).tobytes(), k
    assert dense.normals.any()
    # the view-by-view adjustment is in the map: the same chunks without a follower give another one
    plain = fuse_chunks(chunks, DEV, voxel_size=voxel)
    today = cons_gpu._oracle_world(chunks, voxel)
    assert plain.points.tobytes() == today["points"].tobytes() != dense.points.tobytes()
    assert plain.colors.tobytes() == np.asarray(today["colors"], np.uint8).tobytes()
    none = fuse_chunks(chunks, DEV, voxel_size=voxel, follower=None)
    stripped = fuse_chunks([{k: v for k, v in c.items() if k != "_poses_created"} for c in chunks], DEV, voxel_size=voxel)
    for k in ("points", "colors", "weights", "normals"):
        assert getattr(none, k).tobytes() == getattr(plain, k).tobytes() == getattr(stripped, k).tobytes(), k
    # a chunk without depth keyframes keeps its similarity: one notice, the oracle's bytes
    mixed = [chunks[0], _followed_chunk(s, m, S, Kf, 1.7, 2, with_planes=False)]
    capsys.readouterr()
    dense2 = fuse_chunks(mixed, DEV, voxel_size=voxel, follower=follower)
    said = capsys.readouterr().out
    assert said.count("1 of 2 dense clouds") == 1 and said.count("keep their chunk's similarity") == 1
    assert (follower.last_stats["chunks_followed"], follower.last_stats["chunks_fallen_back"]) == (1, 1)
    assert follower.last_stats["points"] == V
    exp2 = _oracle_followed_map(mixed, voxel)
    for k in ("points", "colors", "weights", "normals"):
        assert getattr(dense2, k).tobytes() == np.asarray(exp2[k]).tobytes(), k
    # the online facade hands its follower to the same fusion
    slam = Pi3SLAMOnline.__new__(Pi3SLAMOnline)
    slam.chunk_reconstructions, slam.device, slam.dense_cleaner = chunks, torch.device(DEV), None
    slam.dense_follower = MapFollower()
    assert slam._fused_map().points.tobytes() == dense.points.tobytes()


# ------------------------------------------------------------------------------------------------ 4, 5. end to end
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")
VOXEL, EVERY = 0.02, 2
SCENE = dict(n_frames=70, chunk_length=40, overlap=10, H=154, W=203)
RESIDUAL_STEP = 4               # keyframe_residuals runs on every 4th voxel of a map: a median does not need them all


def _surface_distance(P, seq):
    """Chunk 0's frame -> world; -> (world points, distance to the nearest wall, distance to the nearest surface)."""
    G0 = seq.gauge_matrix(0)
    Xw = P @ G0[:3, :3].T + G0[:3, 3]
    d_wall = np.min(np.concatenate([np.abs(Xw - seq.lo), np.abs(Xw - seq.hi)], 1), 1)
    d_sph = np.stack([np.abs(np.linalg.norm(Xw - c, axis=1) - r) for c, r in seq.spheres], 1)
    return Xw, d_wall, np.minimum(d_wall, d_sph.min(1))


def _create(seq, out_dir):
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, max_num_keypoints=seq.max_kp, num_loader_workers=0,
                               keypoint_type="grid", estimate_camera_params=True, dense_voxel_size=VOXEL,
                               dense_depth_every=EVERY)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    done = list(cr.process_chunks(cons_gpu._items(seq, cr.device, tuple(range(len(seq.chunks))))))
    _, manifest, _ = cr.write_chunks(iter(done))
    cr.write_run_metadata(manifest)


def _reconstruct(chunk_dir, out_dir, **kw):
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    rec = OfflineReconstructor(chunk_dir=chunk_dir, output_dir=out_dir, **kw)
    rec.run()
    return rec


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _ply_bytes(tmp, name, world):
    from pi3_slam_amd.export import write_ply
    path = os.path.join(str(tmp), name)
    write_ply(world["points"], np.asarray(world["colors"], np.uint8), path)
    return open(path, "rb").read()


def _median_residual(points, chunks):
    zc, zo = ref.keyframe_residuals(points[::RESIDUAL_STEP], [_np_chunk(c) for c in chunks])
    r = np.abs(zc - zo)
    near = r <= 0.1 * zo
    return float(np.median(r[near])), int(near.sum())


def test_without_bundle_adjustment_the_follower_changes_nothing_that_matters(tmp_path):
    """Closed-form chain only: every final pose is its chunk's similarity times its created pose, so every D_m is that
    similarity up to the fp32 roundings of the poses (a dozen of them at <= 16 m, ulp 1.9e-6): a followed point lies
    within 1e-4 m of where sim3_apply puts it, two hundred times below the voxel."""
    import synth_sequence as ss
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapFollower, chunk_transform
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_NONE), **SCENE)
    _create(seq, str(tmp_path / "chunks"))
    rec = _reconstruct(str(tmp_path / "chunks"), str(tmp_path / "rec"), bundle_adjust=False, map_follow_poses=True)
    chunks = rec.reconstructions
    assert len(chunks) == len(seq.chunks) == 3 and all("_poses_created" in c and "dense_depth" in c for c in chunks)
    st = rec.dense_follower.last_stats
    assert st["chunks_followed"] == 3 and st["chunks_fallen_back"] == 0 and st["dropped"] == 0
    metres = seq.chunk_draws(0)["gauge_s"]                   # the world frame is chunk 0's: its unit in metres
    follower, worst = MapFollower(), 0.0
    for c in chunks:
        pts = c["dense_cloud"]["points"].to(DEV, torch.float32).contiguous()
        sim = pts.clone()
        ops.sim3_apply(chunk_transform(c).reshape(16).to(DEV).contiguous(), sim, None)
        moved, _ = follower.apply(c, pts.clone(), None)
        worst = max(worst, float((moved.double() - sim.double()).norm(dim=1).max()) * metres)
    print(f"no bundle adjustment: followed vs similarity, worst point {worst:.3g} m; levels {st}")
    assert st["level1"] >= 0.5 * st["points"]
    assert worst <= 1e-4


# With bundle adjustment on (NOISE_BF16, 70 frames in chunks of 40, 40 and 10):
# the measured figures are in test_the_map_follows_the_bundle_adjusted_poses' docstring.  The level-1 condition (c) is
# checked on the numpy oracle alone (its own counters over the run's chunks) before the device's counters are compared.
@pytest.fixture(scope="module")
def adjusted(tmp_path_factory):
    import synth_sequence as ss
    tmp = tmp_path_factory.mktemp("follow")
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), **SCENE)
    _create(seq, str(tmp / "chunks"))
    runs = {"on": _reconstruct(str(tmp / "chunks"), str(tmp / "on"), map_follow_poses=True),
            "off": _reconstruct(str(tmp / "chunks"), str(tmp / "off"), map_follow_poses=False, map_follow_tolerance=0.03),
            "unasked": _reconstruct(str(tmp / "chunks"), str(tmp / "unasked")),
            "none": _reconstruct(str(tmp / "chunks"), str(tmp / "none"), bundle_adjust=False)}
    return seq, tmp, runs


def test_the_adjustments_were_applied(adjusted):
    """A run in which no adjustment was applied measures nothing."""
    _, _, runs = adjusted
    for name in ("on", "off", "unasked"):
        summary = runs[name].refinement_summary
        print(name, summary)
        assert summary["per_chunk_bundle_adjust"]["applied"] >= 1
        assert summary["prior_constrained_bundle_adjust"]["applied"] >= 1


def test_flag_off_is_byte_identical_to_not_asking(adjusted):
    _, tmp, runs = adjusted
    off, unasked = _tree(tmp / "off"), _tree(tmp / "unasked")
    assert set(off) == set(unasked) and "dense_points.ply" in off and "trajectory_tum.txt" in off
    assert all(off[k] == unasked[k] for k in off)
    assert all("_poses_created" not in c for c in runs["off"].reconstructions + runs["unasked"].reconstructions)
    assert runs["off"].dense_follower is None and runs["unasked"].dense_follower is None
    # the trajectory does not depend on the flag
    on = _tree(tmp / "on")
    assert set(on) == set(off) and all(on[k] == off[k] for k in on if k != "dense_points.ply")
    assert on["dense_points.ply"] != off["dense_points.ply"]


def test_the_map_follows_the_bundle_adjusted_poses(adjusted):
    """(a) dense_points.ply equals the oracle pipeline over the run's chunks; (c) at least half of all cloud points
    follow views that saw them, in the oracle alone and on the device; (d) the map is more consistent with the refined
    trajectory than the map that keeps the chunks' similarities: m = the median |zc - zo| over keyframe_residuals pairs
    with |zc - zo| <= 0.1 zo, keyframes at their final poses.

    Measured on an MI355X (70 frames, chunks of 40, 40 and 10, 3 + 2 adjustments applied; world units = chunk 0's; every
    4th voxel): m_on = 0.0333589 (601 928 pairs), m_off = 0.0334262 (604 887), m_none = 0.0199239 (520 550, bundle_adjust
    =False).  The follower moves the median by 0.2 %: a voxel is already a blend of some twenty views, the adjustment
    moved each of them its own way, and one blended move cannot agree with all of them; what the adjustment does to the
    chunks as wholes the similarity already followed.  Levels: 86 932 of 88 178 cloud points follow views that agree
    with them (0.9859), 17 views that see them, 1 229 the chunk's mean move.  Within 5 mm / 2 cm of a true surface
    (printed, not asserted): on 0.1541 / 0.5868 of 76 334 voxels, off 0.1535 / 0.5863 of 76 918, without adjustment
    0.1994 / 0.7686 of 59 780: the follower makes the map consistent with the trajectory, not better than it.
    The bound on m_on is sqrt(m_on m_off) of that pair: half the gained ratio may erode."""
    seq, tmp, runs = adjusted
    on, off, none = runs["on"], runs["off"], runs["none"]
    # (a)
    exp = _oracle_followed_map(on.reconstructions, VOXEL, normals=False)
    assert open(tmp / "on" / "dense_points.ply", "rb").read() == _ply_bytes(tmp, "oracle_on.ply", exp)
    world_off = cons_gpu._oracle_world(off.reconstructions, VOXEL)
    assert open(tmp / "off" / "dense_points.ply", "rb").read() == _ply_bytes(tmp, "oracle_off.ply", world_off)
    world_none = cons_gpu._oracle_world(none.reconstructions, VOXEL)
    # (c)
    st = on.dense_follower.last_stats
    total = int(exp["levels"].sum())
    share = exp["levels"][1] / total
    print(f"levels (dropped, 1, 2, 3) {exp['levels'].tolist()} of {total} cloud points: level-1 share {share:.4f}")
    assert [st["dropped"], st["level1"], st["level2"], st["level3"]] == exp["levels"].tolist() and st["points"] == total
    assert st["chunks_followed"] == len(seq.chunks) == 3 and st["chunks_fallen_back"] == 0
    assert share >= 0.5
    # (d)
    m_on, n_on = _median_residual(exp["points"], on.reconstructions)
    m_off, n_off = _median_residual(world_off["points"], off.reconstructions)
    m_none, n_none = _median_residual(world_none["points"], none.reconstructions)
    print(f"median |zc - zo|: on {m_on:.6g} ({n_on} pairs), off {m_off:.6g} ({n_off}), without adjustment {m_none:.6g} "
          f"({n_none})")
    for name, pts in (("on", exp["points"]), ("off", world_off["points"]), ("without adjustment", world_none["points"])):
        _, _, d = _surface_distance(pts.astype(np.float64), seq)
        print(f"  {name}: {len(d)} voxels, {float((d <= 0.005).mean()):.4f} within 5 mm of a true surface, "
              f"{float((d <= 0.02).mean()):.4f} within 2 cm")
    assert m_on < m_off
    assert m_on <= M_ON_BOUND


M_ON_BOUND = 0.0333925          # sqrt(0.0333589 * 0.0334262) of the measured pair (the docstring above)
