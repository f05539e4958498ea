"""The post-processing, alignment and ingest kernels (csrc/post.hip, csrc/sim3.hip, csrc/ingest.hip) against the
references of tests/post_kernels_ref.py at the sizes and values where they can go wrong: bit-exact where the
contract is exact (masked ratio median, apply_scale, keypoint matching, the exact projections, ingest), within the
bound the reference derives where it is not (sim3_apply, sim3_compose_prefix, the general projections), and within the
project's tolerances for the Levenberg-Marquardt focal / shift recovery.  tests/test_post_kernels_ref.py checks, without
a GPU, the references themselves and every property of the inputs relied on here."""
import numpy as np
import pytest
import torch

import post_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------- 1. masked ratio median
@pytest.mark.parametrize("kind", R.MEDIAN_KINDS)
def test_ratio_median_is_the_sorted_rank_bit_for_bit(dev, kind):
    from pi3_slam_amd import ops
    cases, outs = [], []
    for n in R.MEDIAN_SIZES:
        for st in R.MEDIAN_STRIDES:
            c = R.median_case(kind, n, st)
            cases.append(c)
            outs.append(ops.masked_ratio_median(_t(c["num"], dev), _t(c["den"], dev), st, _t(c["mask"], dev), n))
            if c["clean"] is not None:                 # the same case without the NaN and the 0/0 under mask == 0
                cl = c["clean"]
                cases.append(cl)
                outs.append(ops.masked_ratio_median(_t(cl["num"], dev), _t(cl["den"], dev), st, _t(cl["mask"], dev), n))
    got = torch.stack(outs).cpu().numpy()
    for c, g in zip(cases, got):
        val, cnt = R.ratio_median_ref(c["num"], c["den"], c["stride"], c["mask"], c["n"])
        say = (kind, c["n"], c["stride"], float(g[0]), float(val), hex(int(R.bits32(g[0])[0])), hex(int(R.bits32(val)[0])))
        assert R.same_median(g[0], val), say
        assert g[1] == cnt, say                        # out[1]: the count, NaN answer or not


# ------------------------------------------------------------------------------------------------- 2. apply_scale
def _apply_scale_case(F_, n3, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n3).astype(np.float32), rng.standard_normal(n3).astype(np.float32),
            R.general_poses(F_, rng))


def _run_apply_scale(dev, s, lp, pts, poses):
    from pi3_slam_amd import ops
    a, b, P = _t(lp, dev), _t(pts, dev), _t(poses, dev)
    ops.apply_scale(torch.tensor([s], dtype=torch.float32, device=dev), a, b, P)
    return a.cpu().numpy(), b.cpu().numpy(), P.cpu().numpy()


@pytest.mark.parametrize("F_,n3", [(100, 300), (3, 4096 * 256 + 771)])
def test_apply_scale_is_the_fp32_product(dev, F_, n3):
    """F = 100 with H = W = 1: 300 translation entries, a second workgroup.  n3 = 4096 * 256 + 771: past the grid cap, the
    stride loop runs (and its tail).  Rotations and fourth rows are general: only [:, :3, 3] may change."""
    lp, pts, poses = _apply_scale_case(F_, n3, 5)
    if F_ == 100:
        lp, pts = lp.reshape(100, 1, 1, 3), pts.reshape(100, 1, 1, 3)
    for s in (1.37, 0.015625, 3.0e-3):
        ea, eb, eP = R.apply_scale_ref(s, lp, pts, poses)
        a, b, P = _run_apply_scale(dev, s, lp, pts, poses)
        assert a.tobytes() == ea.tobytes() and b.tobytes() == eb.tobytes() and P.tobytes() == eP.tobytes(), s
        assert (P[:, :3, 3] != poses[:, :3, 3]).all() and np.array_equal(P[:, :, :3], poses[:, :, :3])


def test_apply_scale_invalid_scales_change_nothing(dev):
    lp, pts, poses = _apply_scale_case(100, 300, 6)
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        a, b, P = _run_apply_scale(dev, bad, lp, pts, poses)
        assert a.tobytes() == lp.tobytes() and b.tobytes() == pts.tobytes() and P.tobytes() == poses.tobytes(), bad


def test_apply_scale_scales_every_pose_when_the_maps_are_shorter(dev):
    """local_points of 3 floats with 100 poses: the grid must cover max(n3, 3 F).  Sized from n3 alone it was one
    workgroup, and poses 85 .. 99 (entries 256 .. 299) kept their translation."""
    lp, pts, poses = _apply_scale_case(100, 3, 7)
    ea, eb, eP = R.apply_scale_ref(1.37, lp, pts, poses)
    a, b, P = _run_apply_scale(dev, 1.37, lp, pts, poses)
    unscaled = np.nonzero((P[:, :3, 3] == poses[:, :3, 3]).any(1))[0]
    assert unscaled.size == 0, unscaled
    assert a.tobytes() == ea.tobytes() and b.tobytes() == eb.tobytes() and P.tobytes() == eP.tobytes()


# -------------------------------------------------------------------------------------------------- 3. sim3_apply
@pytest.mark.parametrize("n,F_", [(0, 5), (7, 0), (5, 300), (1000, 5), (4096 * 256 + 257, 2)])
def test_sim3_apply_within_the_derived_bound(dev, n, F_):
    """(5, 300): F > n, the launcher's blocks * 256 < F correction.  (4096 * 256 + 257, 2): the grid-stride loop."""
    from pi3_slam_amd import ops
    rng = np.random.default_rng(100 + n % 97 + F_)
    M = R.random_similarity(rng, 1.3, 1.3) if n % 2 else R.random_similarity(rng, 0.7, 0.7)
    M[3] = [np.nan, 1e300, -np.inf, 7.0]                       # the fourth row of M must be ignored
    pts = (rng.standard_normal((n, 3)) * 3).astype(np.float32)
    poses = R.general_poses(F_, rng)
    p, pb, P, Pb = R.sim3_apply_ref(M, pts, poses)
    pd, Pd = (_t(pts, dev) if n else None), (_t(poses, dev) if F_ else None)
    ops.sim3_apply(_t(M, dev), pd, Pd)
    if n:
        err = np.abs(pd.cpu().numpy().astype(np.float64) - p)
        assert (err <= pb).all(), (err / pb).max()
    if F_:
        got = Pd.cpu().numpy()
        err = np.abs(got.astype(np.float64) - P)
        assert (err[:, :3] <= Pb[:, :3]).all(), (err[:, :3] / Pb[:, :3]).max()
        assert got[:, 3].tobytes() == poses[:, 3].tobytes()    # the poses' fourth rows: untouched
        Rg = got[:, :3, :3].astype(np.float64)
        D = np.abs(np.swapaxes(Rg, 1, 2) @ Rg - np.eye(3))
        lim = R.rotation_defect_bound(M, poses, P, Pb)
        assert (D <= lim).all(), (D / lim).max()               # still a rotation, to the same bound


# ----------------------------------------------------------------------------------------- 4. sim3_compose_prefix
@pytest.mark.parametrize("n", [1, 2, 64])
def test_sim3_compose_prefix_against_exact_rationals(dev, n):
    from pi3_slam_amd import ops
    T = R.compose_case(n)
    G, bound = R.compose_prefix_ref(T)
    got = ops.sim3_compose_prefix(_t(T.reshape(n, 16), dev)).cpu().numpy().reshape(n, 4, 4)
    assert got[0].tobytes() == T[0].tobytes()                  # G_0 = T_0, a copy
    worst = R.compose_within(got, G, bound)
    assert worst <= 1.0, worst
    assert (got[:, 3] == [0, 0, 0, 1]).all()                   # exact: its bound is 0 off the corner


# --------------------------------------------------------------------------------------------- 5. match_keypoints
@pytest.mark.parametrize("ov,K", R.MATCH_SHAPES)
def test_match_keypoints_equals_the_oracle(dev, ov, K):
    from oracle import post_ref
    from pi3_slam_amd import ops
    kr, kq, planted = R.match_case(ov, K)
    idx = ops.sim3_match_keypoints(_t(kr, dev), _t(kq, dev)).cpu().numpy()
    want = post_ref.match_keypoints(kr, kq)
    assert idx.dtype == np.int32 and np.array_equal(idx, want), np.argwhere(idx != want)[:5]
    for v, facts in planted.items():                           # other view only, -0.0 vs +0.0, NaN with equal bits
        for slot, exp in facts.items():
            assert idx[v, slot] == exp, (v, slot, idx[v, slot], exp)


# ---------------------------------------------------------------------------------------- 6. project_observations
def _project(dev, pts, poses, intr, W, H, max_after):
    from pi3_slam_amd import ops
    uv, valid = ops.project_observations(_t(pts, dev), _t(poses, dev), _t(intr, dev), W, H, max_after)
    return uv.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("K", R.PROJ_KS)
@pytest.mark.parametrize("N,max_after", [(3, 0), (3, 1), (3, 5), (1, 2)])
def test_project_observations_exact_borders(dev, N, max_after, K):
    """Identity poses, power-of-two intrinsics and points: u and v are exact, so every border decision is pinned
    (u = 0 in, u = W out, v = H - 2^-10 in, u = -2^-10 out, v = H out, v = 0 in, zc = 0 out, zc < 0 inside is in)."""
    pts, poses, intr, u, v, inside = R.project_exact_case(N, K)
    uv, valid = _project(dev, pts, poses, intr, R.PROJ_W, R.PROJ_H, max_after)
    assert uv.shape == (N, N, K, 2) and valid.shape == (N, N, K) and valid.dtype == bool
    act = R.active_pairs(N, max_after)
    for s in range(N):
        for t in range(N):
            if act[s, t]:
                assert np.array_equal(uv[s, t, :, 0], u[s].astype(np.float32), equal_nan=True), (s, t)
                assert np.array_equal(uv[s, t, :, 1], v[s].astype(np.float32), equal_nan=True), (s, t)
                assert np.array_equal(valid[s, t], inside[s]), (s, t, np.nonzero(valid[s, t] != inside[s])[0][:5])
            else:                                              # inactive pairs: valid == 0 and uv == 0
                assert not valid[s, t].any() and not uv[s, t].any(), (s, t)
    assert act.any() or N == 1


def test_project_observations_general_rotations(dev):
    g = R.PROJ_GENERAL
    pts, poses, intr = R.project_general_case()
    ruv, rin, _ = R.project_ref(pts, poses, intr, g["W"], g["H"], g["max_after"])
    uv, valid = _project(dev, pts, poses, intr, g["W"], g["H"], g["max_after"])
    act = R.active_pairs(g["N"], g["max_after"])
    err = np.abs(uv.astype(np.float64) - ruv)[act]
    tol = R.project_tolerance(ruv)[act]
    assert (err <= tol).all(), (err / tol).max()
    assert not valid[~act].any() and not uv[~act].any()
    flips = (valid != rin)[act]
    near = R.project_near_border(ruv, g["W"], g["H"])[act]
    assert not (flips & ~near).any(), int((flips & ~near).sum())
    assert near.sum() <= 0.01 * near.size


# ------------------------------------------------------------------------------------------------- 7. focal_shift
@pytest.mark.parametrize("via", ["mask8", "conf"])
@pytest.mark.parametrize("scene", R.FOCAL_SCENES)
@pytest.mark.parametrize("H,W", R.FOCAL_SHAPES)
def test_focal_shift_against_scipy_lm(dev, H, W, scene, via):
    """Three frames a call, a different mask per frame (full, one row, checkerboard / one wave of one batch, two columns,
    lower half / two samples, one sample, a diagonal where single samples exist)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.chunk_creator import _uv_tables_build
    uvx, uvy = _uv_tables_build(H, W, dev)
    lp1 = R.focal_scene(H, W, scene)
    for names, masks in R.focal_batches(H, W):
        lp = np.stack([lp1] * 3)
        ref = R.focal_shift_ref(lp, masks)
        if via == "mask8":
            m8 = np.where(masks, np.array([1, 2, 255], np.uint8)[:, None, None], 0).astype(np.uint8)
            r = ops.focal_shift(_t(lp, dev), None, uvx, uvy, mask=_t(m8, dev))
        else:                                                  # sigmoid(+-5) = 0.993 / 0.0067 against the 0.1 threshold
            conf = np.where(masks, 5.0, -5.0).astype(np.float32)[..., None]
            r = ops.focal_shift(_t(lp, dev), _t(conf, dev), uvx, uvy)
        r = {k: v.cpu().numpy() for k, v in r.items()}
        print(names, "focal", r["focal"], ref["focal"], "shift", r["shift"], ref["shift"])
        np.testing.assert_allclose(r["focal"], ref["focal"], rtol=1e-5, err_msg=str(names))
        np.testing.assert_allclose(r["shift"], ref["shift"], rtol=1e-5, atol=1e-6, err_msg=str(names))
        if "one" in names:                                     # a single valid sample: (1, 0)
            i = names.index("one")
            assert r["focal"][i] == 1.0 and r["shift"][i] == 0.0
        # layout: fx, fy, cx, cy and the row-major 3x3, from the device's own focal in the reference's fp32 order
        lay = R.focal_intrinsics(r["focal"], H, W)
        assert r["fxfycxcy"].tobytes() == lay["fxfycxcy"].tobytes()
        assert r["intrinsics"].tobytes() == lay["K"].tobytes()
        assert (r["fxfycxcy"][:, 2] == W // 2).all() and (r["fxfycxcy"][:, 3] == H // 2).all()
        K = r["intrinsics"]
        assert np.array_equal(K[:, 0, 0], r["fxfycxcy"][:, 0]) and np.array_equal(K[:, 1, 1], r["fxfycxcy"][:, 1])
        assert np.array_equal(K[:, 0, 2], r["fxfycxcy"][:, 2]) and np.array_equal(K[:, 1, 2], r["fxfycxcy"][:, 3])
        np.testing.assert_allclose(r["fxfycxcy"], ref["fxfycxcy"], rtol=1e-5)


# ------------------------------------------------------------------------------------------------------ 8. ingest
@pytest.mark.parametrize("shape", R.INGEST_SHAPES)
@pytest.mark.parametrize("kind", R.INGEST_KINDS)
def test_ingest_bit_exact_at_the_edges(dev, kind, shape):
    """Identity size, a 1 x 1 target, a 1 x 1 source, more than 8x reduction, W1 = 257 (a second workgroup per row
    and a ragged last one); constant 0 / 255 frames, where the 22-bit weights decide the result."""
    from oracle import ingest_ref
    from pi3_slam_amd.image_io import ingest_frames_device
    N, H0, W0, H1, W1 = shape
    frames = R.ingest_case(kind, N, H0, W0)
    out = ingest_frames_device(_t(frames, dev), (H1, W1)).cpu().numpy()
    ref = ingest_ref.ingest_frames(frames, (H1, W1))
    assert out.shape == ref.shape == (N, 3, H1, W1) and out.dtype == np.float32
    assert out.tobytes() == ref.tobytes(), np.argwhere(out != ref)[:5]


# ------------------------------------------------------------------------------------------- 9. argument errors
def _entry_points(dev):
    """name -> (good argument list without the stream, output tensors, [(argument index, bad value)])."""
    f32 = lambda *s: torch.rand(*s, device=dev) + 0.5                                      # noqa: E731
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)                         # noqa: E731
    e = {}
    num, den, mask, out2 = f32(8), f32(8), torch.ones(8, dtype=torch.uint8, device=dev), f32(2)
    e["pi3_masked_ratio_median"] = ([num, den, 1, mask, 8, out2], [out2],
                                    [(0, None), (1, None), (3, None), (5, None), (2, 0), (2, -1), (4, 0), (4, -1)])
    sc, lp, pts, poses = torch.tensor([2.0], device=dev), f32(12), f32(12), f32(2, 4, 4)
    e["pi3_apply_scale"] = ([sc, lp, pts, 12, poses, 2], [lp, pts, poses],
                            [(0, None), (1, None), (2, None), (4, None), (3, 0), (3, -1), (5, 0), (5, -1)])
    M, p3, P = torch.eye(4, dtype=torch.float64, device=dev) * 2, f32(5, 3), f32(2, 4, 4)
    e["pi3_sim3_apply"] = ([M, p3, 5, P, 2], [p3, P],
                           [(0, None), (1, None), (3, None), (2, -1), (4, -1), ((2, 4), (0, 0))])
    T, G = torch.rand(3, 16, dtype=torch.float64, device=dev), torch.rand(3, 16, dtype=torch.float64, device=dev)
    e["pi3_sim3_compose_prefix"] = ([T, G, 3], [G], [(0, None), (1, None), (2, 0), (2, -1)])
    kr = torch.arange(24, device=dev).reshape(2, 6, 2).half()
    idx = torch.full((2, 6), 77, dtype=torch.int32, device=dev)
    e["pi3_sim3_match_keypoints"] = ([kr, kr.clone(), 2, 6, idx], [idx],
                                     [(0, None), (1, None), (4, None), (2, 0), (2, -1), (3, 0), (3, -1)])
    xp = (f32(2, 4, 3) + 1).half()
    po, K3 = torch.eye(4, device=dev).repeat(2, 1, 1), torch.eye(3, device=dev).repeat(2, 1, 1)
    uv, va = f32(2, 2, 4, 2), torch.full((2, 2, 4), 9, dtype=torch.uint8, device=dev)
    e["pi3_project_observations"] = ([xp, po, K3, 2, 4, 8, 8, 1, uv, va], [uv, va],
                                     [(0, None), (1, None), (2, None), (8, None), (9, None), (3, 0), (3, -1), (4, 0),
                                      (4, -1), (5, 0), (5, -1), (6, 0), (6, -1), (7, -1)])
    l4, c4, m4 = f32(1, 4, 4, 3), f32(1, 4, 4, 1), torch.ones(1, 4, 4, dtype=torch.uint8, device=dev)
    ux, uy = f32(4), f32(4)
    fo, sh, fxy, K33 = f32(1) + 5, f32(1) + 5, f32(1, 4) + 5, f32(1, 3, 3) + 5
    e["pi3_focal_shift"] = ([l4, c4, m4, ux, uy, 1, 4, 4, 0.1, fo, sh, fxy, K33], [fo, sh, fxy, K33],
                            [(0, None), ((1, 2), (None, None)), (3, None), (4, None), (9, None), (10, None), (11, None),
                             (12, None), (5, 0), (5, -1), (6, 0), (6, -1), (7, 0), (7, -1)])
    src = torch.randint(0, 256, (1, 4, 4, 3), dtype=torch.uint8, device=dev)
    xb, xk = i32([[0, 2], [2, 2]]), i32([[1 << 21, 1 << 21, 0], [1 << 21, 1 << 21, 0]])
    tmp, dst = torch.full((1, 4, 2, 3), 7, dtype=torch.uint8, device=dev), f32(1, 3, 2, 2) + 5
    e["pi3_ingest_frames"] = ([src, 1, 4, 4, 2, 2, xb, xk, 3, xb.clone(), xk.clone(), 3, tmp, dst], [tmp, dst],
                              [(0, None), (6, None), (7, None), (9, None), (10, None), (12, None), (13, None)]
                              + [(i, b) for i in (1, 2, 3, 4, 5, 8, 11) for b in (0, -1)])
    return e


@pytest.mark.parametrize("name", ["pi3_masked_ratio_median", "pi3_apply_scale", "pi3_sim3_apply",
                                  "pi3_sim3_compose_prefix", "pi3_sim3_match_keypoints", "pi3_project_observations",
                                  "pi3_focal_shift", "pi3_ingest_frames"])
def test_argument_errors_launch_nothing(dev, name):
    """A null pointer or a non-positive size is refused with an error and leaves every output as it was; the good call
    afterwards succeeds and writes."""
    from pi3_slam_amd import lib as L
    good, outs, bads = _entry_points(dev)[name]
    fn = getattr(L.load(), name)
    raw = lambda args: [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args] + [L.stream_ptr()]  # noqa: E731
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()
    for where, bad in bads:
        args = list(good)
        for i, b in zip(where, bad) if isinstance(where, tuple) else [(where, bad)]:
            args[i] = b
        rc = fn(*raw(args))
        assert rc != 0, (name, where, bad)
        with pytest.raises(L.Pi3HipError, match=name):
            L.check(rc, name)
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert o.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
    L.check(fn(*raw(good)), name)
    torch.cuda.synchronize()
    assert any(o.cpu().numpy().tobytes() != b.cpu().numpy().tobytes() for o, b in zip(outs, before)), name
