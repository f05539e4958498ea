"""CPU-only: the references of tests/post_kernels_ref.py against independent implementations (torch.median,
oracle.post_ref, oracle.ingest_ref, Pillow, scipy, exact rationals against numpy), and every property of the seeded
inputs that tests/test_post_kernels_gpu.py relies on - a seed that loses one of them fails here, without a GPU."""
import numpy as np
import pytest
import torch

import post_kernels_ref as R


# ------------------------------------------------------------------------------------------- 1. masked ratio median
def _median_cases(kind):
    for n in R.MEDIAN_SIZES:
        for st in R.MEDIAN_STRIDES:
            yield R.median_case(kind, n, st)


@pytest.mark.parametrize("kind", R.MEDIAN_KINDS)
def test_median_reference_is_torch_median_and_inputs_are_what_they_claim(kind):
    zero_answers = 0
    for c in _median_cases(kind):
        n, st = c["n"], c["stride"]
        val, cnt = R.ratio_median_ref(c["num"], c["den"], st, c["mask"], n)
        sel = R.median_selected(c)
        assert cnt == int((c["mask"] != 0).sum()) == len(sel)
        assert len(c["den"]) == n * st and (st == 1 or np.isnan(c["den"].reshape(n, st)[:, 1:]).all())
        if cnt and not np.isnan(sel).any():
            t = torch.from_numpy(sel.copy()).median()                    # torch: the LOWER median
            assert t.item() == val and not np.isnan(val)
            if val == 0:                                                 # +0 / -0: a sort cannot tell them apart
                zero_answers += 1
                z = sel[sel == 0]
                assert np.signbit(z).all() or not np.signbit(z).any(), "zeros of both signs at the selected rank"
        else:
            assert np.isnan(val)
        if c["expect"] is not None:
            assert R.same_median(val, c["expect"]), (kind, n, st)
        neg, r = int((sel < 0).sum()), (cnt - 1) // 2
        if kind == "all_negative":
            assert neg == n and val < 0
        if kind == "mixed_rank_below_zero":
            assert val < 0 and neg >= r + 1 and (n < 3 or neg < n)
        if kind == "mixed_rank_above_zero":
            assert val > 0 and neg <= r and (n < 3 or neg > 0)
        if kind.startswith("two_"):
            s, uq = np.sort(sel), np.unique(sel)
            a, b = (uq[0], uq[-1]) if len(uq) == 2 else (None, None)
            assert len(uq) == 2 or n <= 2
            if len(uq) == 2:
                assert abs(int(R.bits32(a)[0]) - int(R.bits32(b)[0])) == 1 and a < b     # neighbouring keys
            if "lower_last" in kind:
                assert r + 1 == n or (s[r] == a and s[r + 1] == b)
            else:
                assert r == 0 or (s[r] == b and s[r - 1] == a)
        if kind.startswith("share"):
            top = int(kind[5:kind.index("_")])
            b = R.bits32(sel)
            assert len(np.unique(b >> (32 - top))) == 1 and (n < 3 or len(np.unique(b)) > 1)
            assert (sel < 0).all() == kind.endswith("neg")
            if top == 24 and n >= 1023:
                assert len(np.unique(b)) < n                                       # ties
        if kind == "subnormal":
            assert (np.abs(sel) < 2.0 ** -126).all() and (sel != 0).all() and (n < 3 or 0 < neg < n)
        if kind == "inf_neg":
            assert val == -np.inf and np.sort(sel)[min(r + 1, n - 1)] > -np.inf or n == 1
        if kind == "inf_pos":
            assert val == np.inf and (r == 0 or np.sort(sel)[r - 1] < np.inf)
        if kind == "inf_both":
            assert np.isfinite(val) and (n < 6 or (np.isinf(sel) & (sel > 0)).any() and (np.isinf(sel) & (sel < 0)).any())
        if kind == "mask_bytes":
            assert n < 1023 or {0, 2, 255} <= set(c["mask"].tolist())
        if kind == "nan_masked_off":
            cl = c["clean"]
            off = c["mask"] == 0
            with np.errstate(all="ignore"):
                q = c["num"] / c["den"][::st]
            assert np.isnan(q[off]).sum() == min(2, n - 1) and np.isfinite(cl["num"]).all()
            v2, c2 = R.ratio_median_ref(cl["num"], cl["den"], st, cl["mask"], n)
            assert c2 == cnt and R.same_median(val, v2) and not np.isnan(val)  # unchanged by what is masked off
        if kind == "nan_selected":
            assert np.isnan(val) and cnt >= 1 and np.isnan(sel).sum() == 1
        if kind == "empty":
            assert cnt == 0 and np.isnan(val)
    assert zero_answers == 0            # no case of this suite has a zero for an answer (stated in the summary)


# ------------------------------------------------------------------------------------------------- 2. apply_scale
def test_apply_scale_reference():
    rng = np.random.default_rng(0)
    lp, pts = rng.standard_normal(50).astype(np.float32), rng.standard_normal(50).astype(np.float32)
    poses = R.general_poses(7, rng)
    a, b, P = R.apply_scale_ref(1.37, lp, pts, poses)
    s = torch.tensor(1.37, dtype=torch.float32)
    assert a.dtype == np.float32 and np.array_equal(a, (torch.from_numpy(lp) * s).numpy())
    assert np.array_equal(b, (torch.from_numpy(pts) * s).numpy())
    changed = P != poses
    assert changed[:, :3, 3].all() and not changed[:, :, :3].any() and not changed[:, 3].any()
    assert np.array_equal(P[:, :3, 3], (torch.from_numpy(poses)[:, :3, 3] * s).numpy())
    assert (poses[:, 3] != np.array([0, 0, 0, 1], np.float32)).all()         # the fourth row is not the trivial one
    for bad in (np.nan, 0.0, -1.0, np.inf):
        a, b, P = R.apply_scale_ref(bad, lp, pts, poses)
        assert np.array_equal(a, lp) and np.array_equal(b, pts) and np.array_equal(P, poses)


# -------------------------------------------------------------------------------------------------- 3. sim3_apply
def test_sim3_apply_reference_against_the_oracle():
    from oracle import post_ref
    rng = np.random.default_rng(1)
    M = R.random_similarity(rng, 1.3, 1.3)
    assert abs(np.linalg.norm(M[:3, 0]) - 1.3) < 1e-12 and np.abs(M[:3, :3]).min() > 1e-3     # scale != 1, general R
    pts = rng.standard_normal((500, 3)).astype(np.float32) * 3
    poses = R.general_poses(9, rng)
    p, pb, P, Pb = R.sim3_apply_ref(M, pts, poses)
    p2, P2 = post_ref.apply_sim3(M, pts, poses)
    fp64 = lambda b, ref: b - 0.5 * R.SLACK * R.ulp32(ref)                                       # noqa: E731
    assert (np.abs(p - p2) <= fp64(pb, p)).all()
    assert (np.abs(P[:, :3] - P2[:, :3]) <= fp64(Pb, P)[:, :3]).all()
    assert np.array_equal(P[:, 3], poses[:, 3].astype(np.float64)) and not Pb[:, 3].any()
    garbage = M.copy()
    garbage[3] = [np.nan, 1e300, -np.inf, 7.0]
    for a, b in zip(R.sim3_apply_ref(garbage, pts, poses), (p, pb, P, Pb)):
        assert np.array_equal(a, b)                                                              # the fourth row of M is ignored
    # the bound is about rounding: a handful of fp32 ulps at most, nowhere near a transposed R_cw
    assert (pb <= 0.51 * R.ulp32(p) + 1e-14).all() and (Pb[:, :3] <= 0.51 * R.ulp32(P[:, :3]) + 1e-14).all()
    Pt = poses.copy()
    Pt[:, :3, :3] = np.swapaxes(poses[:, :3, :3], 1, 2)
    assert (np.abs(R.sim3_apply_ref(M, pts, Pt)[2] - P)[:, :3, :3] > 1e3 * Pb[:, :3, :3]).any(axis=(1, 2)).all()
    # the reference's own rotation block is orthonormal to the stated bound (its own error is within P_bound's fp64 part)
    D = np.abs(np.swapaxes(P[:, :3, :3], 1, 2) @ P[:, :3, :3] - np.eye(3))
    assert (D <= R.rotation_defect_bound(M, poses, P, Pb)).all() and D.max() < 1e-6
    # empty inputs
    p, pb, P, Pb = R.sim3_apply_ref(M, np.zeros((0, 3), np.float32), np.zeros((0, 4, 4), np.float32))
    assert p.shape == (0, 3) and P.shape == (0, 4, 4)


def test_ulp32():
    for v in (1.0, 1.5, 2.0, 0.75, 3e-39, 0.0, -1e30, 1 - 2.0 ** -24):
        f = np.float32(v)
        want = float(np.nextafter(np.abs(f), np.float32(np.inf)) - np.abs(f)) if f == v else None
        if want is not None:
            assert R.ulp32(v) == want, v
    assert R.ulp32(1 - 2.0 ** -30) == 2.0 ** -24 and R.ulp32(1 + 2.0 ** -30) == 2.0 ** -23


# ----------------------------------------------------------------------------------------- 4. sim3_compose_prefix
@pytest.mark.parametrize("n", [1, 2, 64])
def test_compose_reference_against_numpy(n):
    T = R.compose_case(n)
    s = np.linalg.norm(T[:, :3, 0], axis=1)
    assert ((s >= 0.8) & (s <= 1.25)).all() and (T[:, 3] == [0, 0, 0, 1]).all()
    G, bound = R.compose_prefix_ref(T)
    g = [T[0]]
    for c in range(1, n):
        g.append(g[-1] @ T[c])
    g = np.stack(g)
    assert R.compose_within(g, G, bound) <= 1.0               # numpy's chained fp64 products: the kernel's error model
    assert np.array_equal(np.array([[float(v) for v in row] for row in G[0]]), T[0]) and not bound[0].any()
    assert np.isfinite(bound).all() and np.abs(g).max() < 1e3  # the chain stays bounded
    if n > 1:
        wrong = g.copy()
        wrong[1] = T[1] @ T[0]                                # the other order of composition is far outside
        assert R.compose_within(wrong, G, bound) > 1e6


# --------------------------------------------------------------------------------------------- 5. match_keypoints
@pytest.mark.parametrize("ov,K", R.MATCH_SHAPES)
def test_match_oracle_is_bit_identity(ov, K):
    from oracle import post_ref
    kr, kq, planted = R.match_case(ov, K)
    idx = post_ref.match_keypoints(kr, kq)
    assert idx.dtype == np.int32 and np.array_equal(idx, R.match_brute(kr, kq))
    for v, facts in planted.items():
        for slot, want in facts.items():
            assert idx[v, slot] == want, (v, slot)
    if K >= 8:
        # -0.0 against +0.0: equal as numbers, different bits -> no match
        assert kq[0, 4, 0] == kr[0, 3, 0] and np.signbit(kq[0, 4, 0]) and not np.signbit(kr[0, 3, 0]) and idx[0, 4] == -1
        # the same NaN bits in both views: unequal as numbers, matched by bits
        assert np.isnan(kq[0, 6, 0]) and kq.view(np.uint16)[0, 6, 0] == kr.view(np.uint16)[0, 5, 0] == R.NAN16
        assert idx[0, 6] == 5
        if ov > 1:                                            # present in another view, absent from its own
            q = kq[0, 2]
            assert (kr[1] == q).all(-1).any() and not (kr[0] == q).all(-1).any() and idx[0, 2] == -1
    if K >= 2:                                                # duplicates inside a reference view: the FIRST wins
        packed = np.ascontiguousarray(kr).view(np.uint32).reshape(ov, K)
        assert all(len(np.unique(packed[v])) < K for v in range(ov))
        j = int(np.nonzero(packed[0] == packed[0, 0])[0][-1])
        assert j > 0 and (idx[0][(np.ascontiguousarray(kq).view(np.uint32).reshape(ov, K)[0] == packed[0, 0])] == 0).all()
    assert (idx >= 0).sum() >= (ov * K) // 2                 # mostly matches


# ---------------------------------------------------------------------------------------- 6. project_observations
@pytest.mark.parametrize("K", R.PROJ_KS)
def test_project_exact_table_is_what_both_references_compute(K):
    from oracle import post_ref
    N = 3
    pts, poses, intr, u, v, inside = R.project_exact_case(N, K)
    for max_after in (0, 1, N + 2):
        act = R.active_pairs(N, max_after)
        with np.errstate(all="ignore"):
            ouv, ovalid = post_ref.project_observations(pts, poses, intr, R.PROJ_W, R.PROJ_H, max_after)
        ruv, rvalid, _ = R.project_ref(pts, poses, intr, R.PROJ_W, R.PROJ_H, max_after)
        assert np.array_equal(ouv, ruv, equal_nan=True) and np.array_equal(ovalid, rvalid)
        assert act.sum() == {0: 3, 1: 5, N + 2: 6}[max_after]
        for s in range(N):
            for t in range(N):
                if act[s, t]:
                    assert np.array_equal(ruv[s, t, :, 0], u[s], equal_nan=True)
                    assert np.array_equal(ruv[s, t, :, 1], v[s], equal_nan=True)
                    assert np.array_equal(rvalid[s, t], inside[s])
                else:
                    assert not ruv[s, t].any() and not rvalid[s, t].any()
    finite = np.isfinite(u)
    assert np.array_equal(u[finite].astype(np.float32).astype(np.float64), u[finite])          # exact in fp32 too
    assert np.array_equal(v[finite].astype(np.float32).astype(np.float64), v[finite])


def test_project_exact_table_pins_each_border():
    t = {(u, v): ins for _, u, v, ins in R.PROJ_EXACT if np.isfinite(u)}
    W, H = R.PROJ_W, R.PROJ_H
    assert t[(0.0, 31.0)] is True and t[(float(W), 31.0)] is False
    assert t[(32.0, H - 2.0 ** -10)] is True and t[(-2.0 ** -10, 31.0)] is False
    assert t[(32.0, float(H))] is False and t[(32.0, 0.0)] is True
    assert any(p[2] == 0 and not ins for p, _, _, ins in R.PROJ_EXACT)
    assert any(p[2] < 0 and ins for p, _, _, ins in R.PROJ_EXACT)


def test_project_general_inputs():
    from oracle import post_ref
    g = R.PROJ_GENERAL
    pts, poses, intr = R.project_general_case()
    uv, inside, zc = R.project_ref(pts, poses, intr, g["W"], g["H"], g["max_after"])
    act = R.active_pairs(g["N"], g["max_after"])
    assert act.sum() == 2 + 3 + 4 + 4 + 4                                      # N = 5, all earlier + 2 after
    assert (np.abs(zc[act]) >= g["min_depth"]).all()
    for P in poses:                                                            # real rotations
        Rm = P[:3, :3].astype(np.float64)
        assert np.abs(Rm - np.eye(3)).max() > 0.05 and np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-6
    # independent implementation: the oracle on poses widened beforehand (its inverse is then LAPACK's fp64 one)
    ouv, ovalid = post_ref.project_observations(pts, poses.astype(np.float64), intr.astype(np.float64), g["W"], g["H"],
                                                g["max_after"])
    assert np.abs(ouv - uv).max() < 1e-10 and np.array_equal(ovalid, inside)
    frac_in = inside[act].mean()
    assert 0.2 < frac_in < 0.9                                                 # both outcomes are well represented
    near = R.project_near_border(uv, g["W"], g["H"])[act]
    assert near.sum() <= 0.01 * near.size
    assert near.sum() == 0                                                     # the count stated in the summary


# ------------------------------------------------------------------------------------------------- 7. focal_shift
def _focal_inputs():
    for (H, W) in R.FOCAL_SHAPES:
        masks = R.focal_masks(H, W)
        for scene in R.FOCAL_SCENES:
            lp = R.focal_scene(H, W, scene)
            for name, m in masks.items():
                yield H, W, scene, name, lp, m


def test_focal_masks_are_what_they_claim():
    for (H, W) in R.FOCAL_SHAPES:
        yy, xx = R.focal_sample_maps(H, W)
        assert yy.min() == 0 and yy.max() <= H - 1 and xx.max() <= W - 1
        m = R.focal_masks(H, W)
        sampled = {k: v[yy][:, xx] for k, v in m.items()}
        assert sampled["full"].all() and len(m) % 3 == 0
        assert sampled["row"].reshape(64, 64).all(1).sum() >= 1 and sampled["row"].all(1).sum() == sampled["row"].any(1).sum()
        if min(H, W) >= 2:
            assert 0.3 < sampled["checker"].mean() < 0.7
        if H >= 64:                 # one sample row = one wave; the other three waves of its batch and all other batches empty
            k = np.nonzero(sampled["last_wave"].reshape(-1))[0]
            assert np.array_equal(k, np.arange(35 * 64, 36 * 64)) and (35 % 4) == 3
        if "two" in m:
            assert sampled["two"].sum() == 2 and sampled["one"].sum() == 1 and sampled["diagonal"].sum() >= 64
    assert "two" in R.focal_masks(64, 64) and "two" in R.focal_masks(100, 37)
    assert "two" not in R.focal_masks(17, 23) and "two" not in R.focal_masks(1, 64)   # every pixel is read several times


def test_focal_reference_is_the_oracle_and_away_from_a_stopping_decision():
    """The oracle stops at ftol = 1e-3: with ftol (1 +- 1e-3) scipy must take the same number of evaluations and land
    within a tenth of the comparison tolerance, or the input sits on a stopping decision and must be replaced."""
    from oracle import post_ref
    checked = 0
    for H, W, scene, name, lp, m in _focal_inputs():
        uv, xyz = R.focal_samples(lp, m)
        if len(uv) < 2:
            assert name == "one"
            continue
        s0, f0, n0 = R.lm_focal_shift(uv, xyz)
        so, fo = post_ref.solve_optimal_focal_shift(uv, xyz)
        assert s0 == so and f0 == fo
        for scale in (1 - 1e-3, 1 + 1e-3):
            s1, f1, n1 = R.lm_focal_shift(uv, xyz, 1e-3 * scale)
            assert n1 == n0, (H, W, scene, name, n0, n1)
            assert abs(f1 - f0) <= 1e-6 * abs(f0) and abs(float(s1) - float(s0)) <= 1e-6 * abs(float(s0)) + 1e-7, (H, W, scene, name)
        if scene == "pinhole" and name != "two":       # the planted answer (two points: a one-parameter family fits exactly)
            assert abs(f0 - R.FOCAL_F0) < 1e-2 * R.FOCAL_F0 and abs(float(s0) - R.FOCAL_SHIFT0) < 1e-2, (H, W, name, f0, s0)
        checked += 1
    assert checked == 2 * (9 + 6 + 6 + 9) - 2 * 2


def test_focal_shift_ref_batches_and_intrinsics():
    from oracle import post_ref
    H, W = 17, 23
    names, masks = R.focal_batches(H, W)[0]
    lp = np.stack([R.focal_scene(H, W, "noisy")] * 3)
    ref = R.focal_shift_ref(lp, masks)
    conf = torch.from_numpy(np.where(masks, 5.0, -5.0).astype(np.float32))[..., None]
    est = post_ref.estimate_camera_parameters(torch.from_numpy(lp), conf)
    assert np.array_equal(ref["focal"], est["focal"][0].numpy()) and np.array_equal(ref["shift"], est["shift"][0].numpy())
    assert np.array_equal(ref["K"], est["intrinsics"].numpy())
    for i, k in enumerate(("fx", "fy", "cx", "cy")):
        assert np.array_equal(ref["fxfycxcy"][:, i], est[k][0].numpy())
    assert len(set(ref["focal"].tolist())) == 3                     # a different mask per frame gives a different answer
    one = R.focal_shift_ref(R.focal_scene(64, 64, "noisy")[None], R.focal_masks(64, 64)["one"][None])
    assert one["focal"][0] == 1.0 and one["shift"][0] == 0.0


def test_focal_intrinsics_is_the_kernels_fp32_expression():
    """post.hip: fx = (((f / 2) * (float)sqrt(1 + ar^2)) / (float)ar) * W, fy = ((f / 2) * (float)sqrt(1 + ar^2)) * H, one
    fp32 rounding per operation: torch's fp32 tensor arithmetic with python scalars must be that, bit for bit."""
    f = np.random.default_rng(3).uniform(0.2, 3.0, 4000).astype(np.float32)
    for (H, W) in R.FOCAL_SHAPES + ((308, 406),):
        ar = W / H
        c1, arf = np.float32(np.sqrt(1.0 + ar * ar)), np.float32(ar)
        half = f / np.float32(2.0)
        fx = ((half * c1) / arf) * np.float32(W)
        fy = (half * c1) * np.float32(H)
        got = R.focal_intrinsics(f, H, W)
        assert got["fxfycxcy"][:, 0].tobytes() == fx.tobytes() and got["fxfycxcy"][:, 1].tobytes() == fy.tobytes()
        assert (got["fxfycxcy"][:, 2] == W // 2).all() and (got["fxfycxcy"][:, 3] == H // 2).all()
        K = got["K"]
        assert np.array_equal(K[:, 0, 0], fx) and np.array_equal(K[:, 1, 1], fy) and (K[:, 2, 2] == 1).all()
        assert np.array_equal(K[:, 0, 2], got["fxfycxcy"][:, 2]) and np.array_equal(K[:, 1, 2], got["fxfycxcy"][:, 3])
        assert not K[:, 0, 1].any() and not K[:, 1, 0].any() and not K[:, 2, :2].any()


# ------------------------------------------------------------------------------------------------------ 8. ingest
@pytest.mark.parametrize("shape", R.INGEST_SHAPES)
@pytest.mark.parametrize("kind", R.INGEST_KINDS)
def test_ingest_oracle_is_pillow(kind, shape):
    from PIL import Image
    from oracle import ingest_ref
    from pi3_slam_amd import image_io
    N, H0, W0, H1, W1 = shape
    frames = R.ingest_case(kind, N, H0, W0)
    assert frames.shape == (N, H0, W0, 3) and frames.dtype == np.uint8
    ref = ingest_ref.ingest_frames(frames, (H1, W1))
    pil = np.stack([np.asarray(Image.fromarray(f).resize((W1, H1), Image.BILINEAR)) for f in frames])
    pil = (pil.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    assert ref.shape == (N, 3, H1, W1) and np.array_equal(ref, pil)
    if kind == "zeros":
        assert not ref.any()
    if kind == "full":
        assert (ref == 1.0).all()                               # the 22-bit weights of every tap row sum to >= 2^22 - 2^21 / 255
    if kind == "frame_constants":
        assert all((ref[f, c] == np.float32(frames[f, 0, 0, c]) / np.float32(255)).all() for f in range(N) for c in range(3))
        assert N == 1 or not np.array_equal(ref[0], ref[1])
    if (H0, W0) == (H1, W1):
        assert np.array_equal(ref, (frames.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))   # identity size
    for a, b in ((W0, W1), (H0, H1)):                           # the host tables the device pass reads
        b0, k0 = ingest_ref.resample_coeffs(a, b)
        b1, k1 = image_io.resample_coeffs(a, b)
        assert np.array_equal(b0, b1) and np.array_equal(k0, k1)


def test_ingest_shapes_cover_the_listed_edges():
    s = R.INGEST_SHAPES
    assert any((h0, w0) == (h1, w1) for _, h0, w0, h1, w1 in s) and any((h1, w1) == (1, 1) for *_, h1, w1 in s)
    assert any((h0, w0) == (1, 1) for _, h0, w0, _, _ in s) and any(h0 > 8 * h1 and w0 > 8 * w1 for _, h0, w0, h1, w1 in s)
    assert any(w1 > 256 and w1 % 256 for *_, w1 in s) and any(n > 1 for n, *_ in s)
