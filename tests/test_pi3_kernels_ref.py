"""tests/pi3_kernels_ref.py pinned to torch's own operators, and every condition the GPU tests of
tests/test_pi3_kernels_gpu.py rely on in their inputs asserted on the references alone (a bad seed fails here)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pi3_kernels_ref as R
from oracle import pi3_ref

DT16 = [torch.bfloat16, torch.float16]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------- formats
def test_ulp16_is_the_spacing_of_the_format():
    for dt, one, tiny, sub in ((torch.bfloat16, 2.0 ** -7, 2.0 ** -133, 1e-39), (torch.float16, 2.0 ** -10, 2.0 ** -24, 1e-6)):
        v = torch.tensor([1.0, -1.0, 1.999, 2.0, 0.75, 0.0, sub], dtype=torch.float64)
        want = torch.tensor([one, one, one, 2 * one, one / 2, tiny, tiny], dtype=torch.float64)
        assert torch.equal(R.ulp16(v, dt), want)
    x = torch.randn(1000, generator=_gen(1)).double() * 50                       # against the format itself
    for dt in DT16:
        lo = x.to(dt)
        step = R.ulp16(lo.double(), dt)
        assert torch.equal((lo.double().abs() + step).to(dt).double(), lo.double().abs() + step)      # the next number up
        assert ((lo.double() - x).abs() <= 0.5 * R.ulp16(x, dt)).all()
        assert (((lo.double().abs() + 0.49 * step).to(dt).double() == lo.double().abs())).all()                # and none in between


@pytest.mark.parametrize("dt", DT16 + [torch.float32])
def test_cast_ref_is_torchs_cast(dt):
    t = torch.cat([torch.tensor(R.CAST_TABLE), torch.randn(4000, generator=_gen(2)) * 100,
                   torch.randn(4000, generator=_gen(3)) * 1e-5]).view(4, -1)
    got, want = R.cast_ref(t, t.shape[1] + 4, t.shape[1], dt), t.to(dt)
    nan = torch.isnan(want)
    assert nan.sum() == 1 and torch.equal(torch.isnan(got[:, :t.shape[1]]), nan)
    bits = {2: torch.int16, 4: torch.int32}[want.element_size()]
    assert torch.equal(got[:, :t.shape[1]].view(bits)[~nan], want.view(bits)[~nan])
    assert torch.equal(got[:, t.shape[1]:].view(bits), torch.zeros(4, 4, dtype=bits))


def test_cast_table_holds_what_its_comments_say():
    t = torch.tensor(R.CAST_TABLE)
    assert len(R.CAST_TABLE) % 4 == 0
    b, h = t.bfloat16().float(), t.half().float()
    at = lambda v: int((t == np.float32(v)).nonzero()[0])
    assert b[at(1 + 2.0 ** -8)] == 1.0 and b[at(1 + 3 * 2.0 ** -8)] == 1 + 2.0 ** -6          # ties to even, both ways
    assert b[at(1 + 2.0 ** -8 + 2.0 ** -23)] == 1 + 2.0 ** -7 and b[at(1 + 3 * 2.0 ** -8 - 2.0 ** -23)] == 1 + 2.0 ** -7
    assert h[at(1 + 2.0 ** -11)] == 1.0 and h[at(1 + 3 * 2.0 ** -11)] == 1 + 2.0 ** -9
    assert h[at(65504.0)] == 65504.0 and h[at(65519.99)] == 65504.0 and h[at(65520.0)] == R.INF and h[at(-65520.0)] == -R.INF
    assert float(t[at(65519.99)]) < 65520.0
    assert h[at(2.0 ** -25)] == 0.0 and h[at(2.0 ** -25 + 2.0 ** -40)] == 2.0 ** -24 and h[at(3 * 2.0 ** -25)] == 2.0 ** -23
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    assert sub.sum() >= 6                                                                   # half subnormals that survive
    mx = at(3.4028234663852886e38)
    assert torch.isfinite(t[mx]) and b[mx] == R.INF and h[mx] == R.INF and b[mx + 1] == -R.INF
    assert torch.isfinite(b[at(3.3895313892515355e38)])
    assert torch.signbit(t[1]) and t[1] == 0


def test_capped_grid_shapes_pass_their_caps():
    """cast_rows: more float4s than one sweep of 4096 workgroups, with and without a quad carry; qknorm_rope: more
    64-vectors than one sweep.  index_values: no two neighbouring rows alike, in any output format."""
    carries = []
    for rows, cols in R.CAST_CAPPED:
        nv = cols // 4
        assert rows * nv > R.CAST_GRID_CAP and rows * cols < 2 ** 24
        carries.append(R.CAST_GRID_CAP % nv != 0)
        x = R.index_values(rows, cols)
        dr = R.CAST_GRID_CAP // nv
        for dt in DT16 + [torch.float32]:
            y = x.to(dt)
            assert not (y[:-1] == y[1:]).all(1).any() and not (y[:-dr] == y[dr:]).all(1).any()
            if nv > 1:
                assert not (y[:, :-4] == y[:, 4:]).all(1).any()
    assert carries == [True, True, False]
    rows, cols, in_cols = R.CAST_CAPPED_FILL
    assert rows * (cols // 4) > R.CAST_GRID_CAP and in_cols < cols and R.CAST_GRID_CAP % (cols // 4) != 0
    assert [r * 2 * h > R.QK_GRID_CAP for r, h, _ in R.QK_SHAPES] == [False, True]


# ----------------------------------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("rows,D", [(5, 260), (3, 4), (2, 2048)])
@pytest.mark.parametrize("kind", ["randn", "offset", "range"])
def test_layernorm_ref_is_layer_norm_in_fp64(rows, D, kind):
    g = _gen(D)
    x = R.layernorm_data(kind, rows, D, g)
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    y, bound = R.layernorm_ref(x, w, b, 1e-6)
    want = F.layer_norm(x.double(), (D,), w.double(), b.double(), float(np.float32(1e-6)))
    assert (y - want).abs().max() <= 1e-12 * (1 + want.abs().max())
    assert torch.isfinite(bound).all() and (bound > 0).all()
    if kind == "randn":                      # the bound stays a rounding bound: far below half a bf16 ulp
        assert (bound <= 2.0 ** -4 * R.ulp16(y, torch.bfloat16)).float().mean() > 0.99
    if kind == "offset":                     # the data set defeats a one-pass variance in fp32
        x32 = x[0]
        one_pass = (x32 * x32).mean() - x32.mean() ** 2
        assert abs(float(one_pass) - float(x[0].double().var(unbiased=False))) > 0.5 * float(x[0].double().var(unbiased=False))
    assert [R.layernorm_vpl(d) for d in (4, 252, 256, 260, 384, 516, 1024, 1028, 2048)] == [1, 1, 1, 2, 2, 4, 4, 8, 8]


# ----------------------------------------------------------------------------------------- patch_gather, resample
def test_patch_gather_ref_is_unfold_of_the_normalised_image():
    from pi3_slam_amd.weights import IMAGE_MEAN, IMAGE_STD
    img = torch.rand(2, 3, 28, 126, generator=_gen(5))
    out, rows = R.patch_gather_ref(img, IMAGE_MEAN, IMAGE_STD, 590, torch.bfloat16)
    mean, std = torch.tensor(IMAGE_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGE_STD).view(1, 3, 1, 1)
    norm = (img - mean) * (1.0 / std)
    assert torch.equal(rows, F.unfold(norm, 14, stride=14).transpose(1, 2).reshape(2 * 18, 588))
    exact = (img.double() - mean.double()) / std.double()
    assert ((norm.double() - exact).abs() <= 3 * R.U * exact.abs() + R.U * mean.double() / std.double()).all()
    assert torch.equal(out[:, :588].view(torch.int16), rows.bfloat16().view(torch.int16)) and not out[:, 588:].any()
    assert rows.unique().numel() > 0.99 * rows.numel()                       # every pixel its own value


def test_resample_ref_is_wy_src_wxt():
    g = _gen(6)
    src, wy, wx = torch.randn(5, 7, 3, generator=g), torch.randn(2, 5, generator=g), torch.randn(3, 7, generator=g)
    wy[0, 1] = 0.0
    dst, bound = R.resample_ref(src, wy, wx)
    for d in range(3):
        assert torch.allclose(dst[..., d], wy.double() @ src[..., d].double() @ wx.double().t(), rtol=0, atol=1e-13)
    assert bound.shape == dst.shape and (bound > 0).all()
    assert bound[0, 0, 0] / bound[1, 0, 0] != 1 and int((wy[0] != 0).sum()) == 4


# ------------------------------------------------------------------------------------------------------ qknorm_rope
@pytest.mark.parametrize("norm,rope", [(True, True), (True, False), (False, True), (False, False)])
def test_qknorm_rope_ref_is_layer_norm_then_rope2d(norm, rope):
    rows, H, T = R.QK_SHAPES[0]
    qkv, pos, cs, nw = R.qk_case(rows, H, T)
    args = nw if norm else [None] * 4
    qs = 0.125 * math.log2(math.e)
    out, bound = R.qknorm_rope_ref(qkv, rows, H, T, pos, cs, *args, 1e-5, qs, rope)
    x = qkv.float().view(rows // T, T, 3, H, 64)
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)
    if norm:
        q, k = F.layer_norm(q, (64,), nw[0], nw[1], 1e-5), F.layer_norm(k, (64,), nw[2], nw[3], 1e-5)
    if rope:
        xpos = pos.long()[None].expand(rows // T, T, 2)
        q, k = pi3_ref.rope2d(q, xpos), pi3_ref.rope2d(k, xpos)
    o = out.view(rows // T, T, 3, H, 64)
    assert torch.allclose(o[:, :, 0].float(), q.transpose(1, 2) * qs, rtol=1e-5, atol=1e-5)
    assert torch.allclose(o[:, :, 1].float(), k.transpose(1, 2), rtol=1e-5, atol=1e-5)
    assert torch.equal(o[:, :, 2].float(), x[:, :, 2]) and not bound[:, 2].any()
    assert (bound[:, :2] <= 2.0 ** -6 * R.ulp16(out[:, :2], torch.bfloat16)).float().mean() > 0.99
    assert (pos[:5] == 0).all() and cs[0, :, 0].eq(1).all() and cs[0, :, 1].eq(0).all()       # (0, 0): the identity
    assert (pos[5:] > 0).all()


# ------------------------------------------------------------------------------------------------ unpatchify_points
def test_unpatchify_ref_is_pixel_shuffle():
    Fr, H, W, nreg = 2, 28, 42, 5
    ph, pw = H // 14, W // 14
    P, T = ph * pw, ph * pw + nreg
    g = _gen(7)
    pfeat, cfeat = torch.randn(Fr * T, 640, generator=g) * 0.5, torch.randn(Fr * T, 256, generator=g)

    def shuffle(f, c):                       # as tests/test_fullsize_gpu.py::test_pointmap_and_camera_heads_full_chunk spells it
        x = f.view(Fr, T, -1)[:, nreg:, :c * 196].transpose(-1, -2).reshape(Fr, c * 196, ph, pw)
        return torch.nn.functional.pixel_shuffle(x, 14).permute(0, 2, 3, 1)
    local, bound, conf = R.unpatchify_ref(pfeat, cfeat, Fr, H, W, T, nreg)
    ret = shuffle(pfeat, 3).double()
    z = torch.exp(ret[..., 2:])
    assert torch.equal(local, torch.cat([ret[..., :2] * z, z], dim=-1))
    assert torch.equal(conf, shuffle(cfeat, 1))
    assert (bound[..., 2] == R.SLACK * 4 * R.U * local[..., 2]).all() and (bound[..., :2] <= 5.01 * R.U * local[..., :2].abs()).all()
    poses = torch.randn(Fr, 4, 4, generator=g)
    pts, pb = R.world_ref(local.float(), poses)
    hom = torch.cat([local.float().double(), torch.ones(Fr, H, W, 1, dtype=torch.float64)], dim=-1)
    assert torch.allclose(pts, torch.einsum("nij,nhwj->nhwi", poses.double(), hom)[..., :3], rtol=0, atol=1e-12)
    assert (pb > 0).all()


# ------------------------------------------------------------------------------------------------------ camera_tail
@pytest.mark.parametrize("D", R.CAM_D)
def test_camera_cases_are_well_conditioned_and_show_both_determinant_signs(D):
    """Every frame of every case: s2 + sign(det) s3 > 0.1; every case: a frame with det < 0 and one with det > 0; the
    inputs do not depend on tok_off; the derived bounds stay rounding bounds."""
    for P in R.CAM_P:
        feat5, T5, w5 = R.camera_case(D, P, 5)
        feat0, T0, w0 = R.camera_case(D, P, 0)
        assert T5 == P + 5 and T0 == P and torch.isnan(feat5.view(3, T5, D)[:, :5]).all()
        assert torch.equal(feat5.view(3, T5, D)[:, 5:], feat0.view(3, P, D)) and all(torch.equal(w5[k], w0[k]) for k in w5)
        ref = R.camera_tail_ref(feat5, 3, P, T5, 5, w5)
        gap = ref["s"][:, 1] + torch.sign(ref["det"]) * ref["s"][:, 2]
        assert float(gap.min()) > 0.1, (D, P, gap)
        assert (ref["det"] > 0).any() and (ref["det"] < 0).any(), (D, P, ref["det"])
        assert float(R.rotation_tolerance(ref).max()) < 1e-3 and float((ref["t_bound"] / (1 + ref["t"].abs())).max()) < 1e-4
        assert float(ref["t"].abs().max()) > 5.0                                   # translations of order 10
        hidden = torch.relu(F.linear(feat0.view(3, P, D).double().mean(1), w0[R.CAM_W[0] + ".weight"].double(), w0[R.CAM_W[0] + ".bias"].double()))
        assert (hidden == 0).any() and (hidden > 0).any()                          # the ReLU cuts some neurons and passes others


def test_camera_tail_ref_is_the_oracles_head():
    D, P = 512, 33
    feat, T, w = R.camera_case(D, P, 5)
    ref = R.camera_tail_ref(feat, 3, P, T, 5, w)
    v = feat.view(3, T, D)[:, 5:].mean(dim=1)
    v = torch.relu(F.linear(v, w[R.CAM_W[0] + ".weight"], w[R.CAM_W[0] + ".bias"]))
    v = torch.relu(F.linear(v, w[R.CAM_W[1] + ".weight"], w[R.CAM_W[1] + ".bias"]))
    t = F.linear(v, w[R.CAM_W[2] + ".weight"], w[R.CAM_W[2] + ".bias"])
    r = F.linear(v, w[R.CAM_W[3] + ".weight"], w[R.CAM_W[3] + ".bias"])
    assert torch.allclose(ref["t"].float(), t, rtol=1e-4, atol=1e-4)
    assert (ref["R"].float() - pi3_ref.svd_orthogonalize(r)).abs().max() < 1e-4
    assert torch.allclose(ref["A"].float(), F.normalize(r.view(3, 3, 3), dim=-1), atol=1e-5)
    RtR = ref["R"].transpose(1, 2) @ ref["R"]
    assert (RtR - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12 and torch.allclose(torch.det(ref["R"]), torch.ones(3, dtype=torch.float64))
    # the nearest rotation maximises tr(R^T A): no rotation nearby does better
    g = _gen(9)
    for f in range(3):
        best = torch.trace(ref["R"][f].t() @ ref["A"][f])
        for _ in range(20):
            k = torch.randn(3, generator=g).double() * 0.05
            K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
            assert torch.trace((torch.matrix_exp(K) @ ref["R"][f]).t() @ ref["A"][f]) <= best + 1e-12
