"""The row / pixel kernels of the MoGe path (csrc/moge.hip, fill_tokens of csrc/elem.hip), each called directly and
compared with the same operation written out in fp64 (or int64) on the host from the same fp32 inputs.

The end-to-end MoGe tests gate these kernels only through the network's output, at twice the reference's own
fp16-autocast deviation; the bounds here are those of fp32 arithmetic: equality where the operation is exact (integer
sums, gathers, casts, adds), otherwise a worst-case rounding bound per element derived from the number of fp32 roundings
(U = 2^-24, the unit roundoff) times the sum of the magnitudes that enter the result.

Poison rule, for every kernel that takes a leading dimension: the pad columns [C, ld) of an input hold NaN (they must
never be read), outputs start as NaN, and the columns beyond a kernel's documented write range must keep their bits.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
NAN = float("nan")
DT16 = [torch.bfloat16, torch.float16]


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns (NaN payloads and the sign of zero included) on the host."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(_bits(a), _bits(b))


def _padded(vals: torch.Tensor, ld: int) -> torch.Tensor:
    """[rows, C] -> [rows, ld] with NaN in the pad columns."""
    out = torch.full((vals.shape[0], ld), NAN, dtype=vals.dtype)
    out[:, :vals.shape[1]] = vals
    return out


# ------------------------------------------------------------------------------------------------ groupnorm_stats
GN_SHAPES = [
    (1, 1, 32, 1, 32),
    (1, 7, 20, 20, 32),
    (1, 129, 32, 1, 40),            # odd HW in the two-pixels-per-wave form
    (1, 513, 64, 2, 64),            # two blocks, the second of one pixel
    (1, 1531, 96, 3, 96),
    (1, 700, 256, 8, 256),
    (1, 300, 520, 5, 528),
    (1, 200, 1024, 1024, 1024),     # sixteen channels per lane, instance norm, 64 groups per wave
    (1, 300001, 32, 1, 32),         # block cap: more than 512 pixels per block
    (3, 1531, 64, 2, 72),           # B > 1, every image its own data
]


@pytest.mark.parametrize("B,HW,C,G,ld", GN_SHAPES)
def test_groupnorm_stats_equal_the_integer_sums(built_lib, B, HW, C, G, ld):
    """Integer-valued data in {-3 ... 3}: every 64-pixel fp32 partial (|sum| <= 192, sum of squares <= 576) and every
    fp64 sum is exact, so the statistics equal the int64 sums; one dropped or double-counted pixel changes them."""
    from pi3_slam_amd import ops
    g = torch.Generator().manual_seed(HW * 31 + C)
    xi = torch.randint(-3, 4, (B * HW, C), generator=g)
    x = _padded(xi.float(), ld).to(DEV)
    stats = torch.full((2 * B * G + 2,), NAN, dtype=torch.float64, device=DEV)
    ops.groupnorm_stats(x, HW, C, G, stats, B=B)
    v = xi.view(B, HW, G, C // G)
    want = torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)       # [B][G][2], int64
    got = stats[:2 * B * G].cpu().view(B, G, 2)
    assert torch.equal(got, want.double()), (got - want.double()).abs().max().item()
    assert _same_bits(stats[2 * B * G:], torch.full((2,), NAN, dtype=torch.float64))


def test_groupnorm_stats_real_valued_within_the_scheme_bound_and_deterministic(built_lib):
    """fp32 inside 64-pixel chunks, fp64 across: at most 64 fp32 roundings touch a term, so |d sum| <= 64 U sum|x| and
    |d sumsq| <= 64 U sum x^2 (the square's own rounding is one of the 64: a chunk adds 63 times).  Two runs agree bit
    for bit (no atomics)."""
    from pi3_slam_amd import ops
    HW, C = 4099, 32
    x = torch.randn(HW, C, generator=torch.Generator().manual_seed(4099)) + 8.0
    xd = x.to(DEV)
    runs = []
    for _ in range(2):
        stats = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
        ops.groupnorm_stats(xd, HW, C, 1, stats)
        runs.append(stats.cpu())
    assert _same_bits(runs[0], runs[1])
    x64 = x.double()
    s, q = x64.sum().item(), (x64 * x64).sum().item()
    ds, dq = abs(runs[0][0].item() - s), abs(runs[0][1].item() - q)
    print(f"groupnorm_stats randn+8: |dsum| {ds:.3e} (bound {64 * U * x64.abs().sum().item():.3e}), "
          f"|dsumsq| {dq:.3e} (bound {64 * U * q:.3e})")
    assert ds <= 64 * U * x64.abs().sum().item()
    assert dq <= 64 * U * q


def test_groupnorm_stats_rejects_bad_arguments(built_lib):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    x = torch.zeros(8, 1040, device=DEV)
    stats = torch.zeros(16, dtype=torch.float64, device=DEV)
    with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):         # PI3_ERR_ARG
        ops.groupnorm_stats(x, 8, 32, 5, stats)                   # C % G != 0
    with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
        ops.groupnorm_stats(x, 8, 1028, 1, stats)                 # C > 1024
    lib = L.load()
    need = int(lib.pi3_groupnorm_ws_doubles(2, 4, 32))
    assert need == 2 * 1 * 2 * 32
    ws = torch.zeros(need, dtype=torch.float64, device=DEV)
    with pytest.raises(L.Pi3HipError, match=r"rc=-3\b"):         # PI3_ERR_WORKSPACE
        L.check(lib.pi3_groupnorm_stats(x.data_ptr(), x.stride(0), 2, 4, 32, 1, stats.data_ptr(), ws.data_ptr(), need - 1,
                                        L.stream_ptr()), "pi3_groupnorm_stats")


# -------------------------------------------------------------------------------------------------- convt_scatter
@pytest.mark.parametrize("B,H,W,Cout,Cs,Cpad,ldg,ldo", [
    (1, 3, 5, 32, 32, 32, 128, 32),
    (1, 4, 70, 8, 8, 64, 32, 64),       # more than 256 quads per output row
    (1, 2, 3, 6, 8, 8, 32, 8),          # vector-eligible source, the last quad ragged
    (1, 2, 3, 6, 6, 8, 24, 12),         # scalar path, ldo > Cpad
    (2, 3, 2, 16, 16, 64, 64, 64),
])
@pytest.mark.parametrize("dt", DT16)
def test_convt_scatter_is_the_gather_with_torchs_cast(built_lib, B, H, W, Cout, Cs, Cpad, ldg, ldo, dt):
    """out[b][2y+dy][2x+dx][co] = cast(g[b][y][x][(dy*2+dx)*Cs + co]): a gather plus round-to-nearest-even, so equality
    with torch's cast (inf beyond the half range, half subnormals kept); channels [Cout, Cpad) are zeros; the source's
    channels [Cout, Cs) of each (dy, dx) slot and its columns past 4 Cs hold NaN and are never read."""
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(H * 100 + W * 10 + Cout)
    g = torch.full((B * H * W, ldg), NAN)
    for s in range(4):
        g[:, s * Cs: s * Cs + Cout] = torch.randn(B * H * W, Cout, generator=gen) * 3
    g[0, :4] = torch.tensor([1e5, -1e5, 65504.0, 6e-8])           # beyond / at the half range, a half subnormal
    g[-1, 3 * Cs + Cout - 2: 3 * Cs + Cout] = torch.tensor([-7e4, 3e-8])
    out = torch.full((B * 4 * H * W, ldo), NAN, dtype=dt, device=DEV)
    ops.convt_scatter(g.to(DEV), H, W, Cout, Cs, Cpad, out, B=B)
    want = g.view(B, H, W, ldg)[..., :4 * Cs].reshape(B, H, W, 2, 2, Cs)[..., :Cout]
    want = want.permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * H * W, Cout).to(dt)      # [b][y][dy][x][dx][co]
    assert _same_bits(out[:, :Cout], want)
    assert _same_bits(out[:, Cout:Cpad], torch.zeros(B * 4 * H * W, Cpad - Cout, dtype=dt))
    assert _same_bits(out[:, Cpad:], torch.full((B * 4 * H * W, ldo - Cpad), NAN, dtype=dt))


# ------------------------------------------------------------------------------------------------------ uv_affine
@pytest.mark.parametrize("B,H,W,C,ld,wofs,ldw,bias,accumulate,offset", [
    (1, 5, 7, 32, 32, 0, 2, True, False, 0),
    (1, 3, 70, 64, 64, 384, 386, False, True, 0),     # 4480 floats per row: two segments, the second partial
    (1, 4, 50, 96, 96, 10, 16, True, True, 0),        # 256 % (C / 4) != 0: weights reloaded per iteration
    (1, 4, 9, 6, 8, 0, 2, True, False, 0),            # scalar path
    (1, 4, 9, 32, 36, 0, 2, True, True, 1),           # base off by one float: misaligned, so the scalar path
    (3, 4, 6, 32, 32, 0, 2, False, True, 0),          # v[y] repeats per image
])
def test_uv_affine_against_fp64(built_lib, B, H, W, C, ld, wofs, ldw, bias, accumulate, offset):
    """x (+)= w[c][wofs] u[x] + w[c][wofs+1] v[y] + bias[c].  Two products, up to three additions: a term passes through
    at most four fp32 roundings (contracted or not), so |error| <= 4 U (|x0| + |w0 u| + |w1 v| + |b|).  Without
    accumulate the destination starts as NaN and must come out finite (it is not read)."""
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
    rows = B * H * W
    x0 = torch.randn(rows, C, generator=gen) if accumulate else torch.full((rows, C), NAN)
    buf = torch.full((rows * ld + offset,), NAN)
    buf[offset:].view(rows, ld)[:, :C] = x0
    buf = buf.to(DEV)
    x = buf[offset:].view(rows, ld)
    assert x.data_ptr() % 16 == (4 * offset) % 16
    w = torch.full((C, ldw), NAN)                                  # only columns wofs, wofs + 1 may be read
    w[:, wofs: wofs + 2] = torch.randn(C, 2, generator=gen)
    b = torch.randn(C, generator=gen) if bias else None
    u = torch.randn(W, generator=gen)
    v = torch.randn(H, generator=gen)
    ops.uv_affine(x, H, W, C, w.to(DEV), wofs, b.to(DEV) if bias else None, u.to(DEV), v.to(DEV), accumulate, B=B)
    t0 = w[:, wofs].double().view(1, 1, 1, C) * u.double().view(1, 1, W, 1)
    t1 = w[:, wofs + 1].double().view(1, 1, 1, C) * v.double().view(1, H, 1, 1)
    tb = (b.double() if bias else torch.zeros(C, dtype=torch.float64)).view(1, 1, 1, C)
    ta = x0.double().view(B, H, W, C) if accumulate else torch.zeros(B, H, W, C, dtype=torch.float64)
    want = ta + t0 + t1 + tb
    bound = 4 * U * (ta.abs() + t0.abs() + t1.abs() + tb.abs())
    got = x.cpu()
    val = got[:, :C].double().view(B, H, W, C)
    assert torch.isfinite(val).all()
    excess = ((val - want).abs() - bound).max().item()
    assert excess <= 0, excess
    assert _same_bits(got[:, C:], torch.full((rows, ld - C), NAN))


# ---------------------------------------------------------------------------------------------------- resize_taps
def _nearest2(n_in):
    """The nearest-neighbour x2 table MoGeEngine._resample builds: src = dst // 2, one tap of weight 1."""
    sc = np.stack([np.arange(2 * n_in) // 2, np.ones(2 * n_in, dtype=np.int64)], 1).astype(np.int32)
    wt = np.zeros((2 * n_in, 8), dtype=np.float32)
    wt[:, 0] = 1.0
    return sc, wt


def _table(spec):
    from pi3_slam_amd.moge import linear_taps
    return _nearest2(spec[1]) if spec[0] == "nearest2" else linear_taps(*spec)


def _dense(sc, wt, n_in):
    """Tap table -> [out, in] fp64 matrix."""
    m = np.zeros((sc.shape[0], n_in))
    for i, (s, n) in enumerate(sc):
        assert 0 <= s and s + n <= n_in and 1 <= n <= wt.shape[1]      # the kernel's reads stay inside the source
        m[i, s:s + n] = wt[i, :n].astype(np.float64)
    return m


def _dev_table(sc, wt):
    """Device copy whose unused weight slots hold NaN: the kernel reads `count` weights per row and no more."""
    wt = wt.copy()
    for i, (_, n) in enumerate(sc):
        wt[i, n:] = np.nan
    return torch.from_numpy(sc).to(DEV), torch.from_numpy(wt).to(DEV)


@pytest.mark.parametrize("C,ih,iw,ytab,xtab,src_layout,dst_layout", [
    (3, 518, 37, (518, 140, True), (37, 14, True), "planar", "planar"),       # 8 taps: the full table
    (3, 37, 518, (37, 14, True), (518, 140, True), "nhwc32", "hwc"),
    (1, 16, 16, (16, 64, False), (16, 64, False), "nhwc8", "planar"),         # one-tap rows at both borders
    (5, 7, 9, ("nearest2", 7), ("nearest2", 9), "nhwc8", "nhwc8"),            # _resample's x2 up-sampling in place
    (3, 16, 11, (16, 64, False), ("nearest2", 11), "nhwc32", "planar"),       # another table per axis
    (3, 60, 72, (60, 840, False), (72, 1000, False), "nhwc32", "hwc"),        # > 256*32*256 outputs: grid-stride loop
])
def test_resize_taps_against_the_tables_in_fp64(built_lib, C, ih, iw, ytab, xtab, src_layout, dst_layout):
    """dst = Wy src Wx^T with the same tables applied in fp64.  An output adds nx products per source row and ny rows:
    at most ny + nx fp32 roundings touch a term, so |error| <= (ny + nx) U sum |wy| |wx| |src|.  The engine's stride
    layouts: planar, NHWC with a channel stride (pad channels NaN: they must not leak), packed HWC."""
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(ih * 1000 + iw + C)
    src = torch.randn(C, ih, iw, generator=gen) * 2 + 0.5
    (ysc, ywt), (xsc, xwt) = _table(ytab), _table(xtab)
    oh, ow = ysc.shape[0], xsc.shape[0]
    Wy, Wx = torch.from_numpy(_dense(ysc, ywt, ih)), torch.from_numpy(_dense(xsc, xwt, iw))

    def place(layout, h, w, vals):
        """-> (device tensor, strides (c, y, x), leading dimension or None)."""
        if layout == "planar":
            t = vals.contiguous() if vals is not None else torch.full((C, h, w), NAN)
            return t.to(DEV), (h * w, w, 1), None
        ld = C if layout == "hwc" else int(layout[4:])
        t = torch.full((h * w, ld), NAN)
        if vals is not None:
            t[:, :C] = vals.permute(1, 2, 0).reshape(h * w, C)
        return t.to(DEV), (1, w * ld, ld), ld

    s, sstr, _ = place(src_layout, ih, iw, src)
    d, dstr, dld = place(dst_layout, oh, ow, None)
    ys, yw = _dev_table(ysc, ywt)
    xs, xw = _dev_table(xsc, xwt)
    ops.resize_taps(s, sstr, C, ys, yw, xs, xw, oh, ow, d, dstr)
    got = d.cpu()
    if dld is not None:
        assert _same_bits(got[:, C:], torch.full((oh * ow, dld - C), NAN))
        got = got[:, :C].reshape(oh, ow, C).permute(2, 0, 1)
    want = Wy @ src.double() @ Wx.t()
    mag = Wy.abs() @ src.double().abs() @ Wx.abs().t()
    nyx = torch.from_numpy(ysc[:, 1].astype(np.float64)).view(1, oh, 1) + torch.from_numpy(xsc[:, 1].astype(np.float64)).view(1, 1, ow)
    assert torch.isfinite(got).all()
    excess = ((got.double() - want).abs() - nyx * U * mag).max().item()
    assert excess <= 0, excess


# ------------------------------------------------------------------------------------------------------ dense_vec
@pytest.mark.parametrize("K,N", [(384, 128), (128, 1), (100, 5), (1, 3), (1000, 129)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", [0, 2])
def test_dense_vec_against_fp64(built_lib, K, N, bias, act):
    """y = act(W x + b): |error| <= K U sum |W| |x| + U |b| (K products summed in some order, then the bias)."""
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(K * 7 + N)
    x = torch.randn(K, generator=gen)
    W = torch.randn(N, K, generator=gen) / K ** 0.5
    b = torch.randn(N, generator=gen) if bias else None
    y = torch.full((N + 1,), NAN, device=DEV)
    ops.dense_vec(x.to(DEV), W.to(DEV), b.to(DEV) if bias else None, act, y)
    want = W.double() @ x.double() + (b.double() if bias else 0.0)
    bound = K * U * (W.double().abs() @ x.double().abs()) + U * (b.double().abs() if bias else 0.0)
    if act == 2:
        want = want.clamp_min(0)                                   # ReLU is 1-Lipschitz: the bound carries over
    got = y.cpu()
    excess = ((got[:N].double() - want).abs() - bound).max().item()
    assert excess <= 0, excess
    assert _same_bits(got[N:], torch.full((1,), NAN))


# ----------------------------------------------------------------------------------------------------- moge_remap
EXP_RTOL = 3e-6         # the project's bound for expf (test_pointmap_and_camera_heads_full_chunk)
# sinhf: the project recorded no bound.  Measured on an MI355X against fp64 sinh on the inputs below: 7.607e-8 relative at
# n = 1000 and 6.606e-8 at n = 257 (0.64 fp32 ulp; four ulp, 4.8e-7, would have been a finding to look into, not a number
# to adopt).  The gate is twice the larger measurement.
SINH_MEASURED = 7.607e-8
SINH_RTOL = 2 * SINH_MEASURED


def _remap_points(n):
    gen = torch.Generator().manual_seed(n)
    pts = torch.rand(n, 3, generator=gen) * 8 - 4
    special = torch.tensor([0.0, 1e-6, -1e-6, 10.0, -10.0])
    for k in range(3):                                             # every special value in every coordinate ...
        pts[:5, k] = special
    pts[5:10, 0] = special                                         # ... and against ordinary partners
    pts[10:15, 2] = special
    return pts


def _rel_err(got, want):
    """max |got - want| / |want|, an exact zero being required where want is zero."""
    got, want = got.double(), want.double()
    zero = want == 0
    assert torch.equal(got[zero], want[zero])
    return ((got[~zero] - want[~zero]).abs() / want[~zero].abs()).max().item() if (~zero).any() else 0.0


@pytest.mark.parametrize("n", [1000, 257])
@pytest.mark.parametrize("remap", [0, 1, 2, 3])
def test_moge_remap_modes_against_fp64(built_lib, n, remap):
    """linear: bits unchanged; exp: z = exp(z), xy *= z; sinh: all three; sinh_exp: xy = sinh(xy), z = exp(z)."""
    from pi3_slam_amd import ops
    p0 = _remap_points(n)
    pts = torch.full((n + 1, 3), NAN)
    pts[:n] = p0
    pts = pts.to(DEV)
    mask = torch.full((n + 1,), 7, dtype=torch.uint8, device=DEV)
    ops.moge_remap(pts, None, n, remap, mask)
    got = pts.cpu()
    assert _same_bits(got[n:], torch.full((1, 3), NAN))
    assert torch.equal(mask.cpu(), torch.cat([torch.ones(n, dtype=torch.uint8), torch.tensor([7], dtype=torch.uint8)]))
    p64 = p0.double()
    if remap == 0:
        assert _same_bits(got[:n], p0)
        return
    if remap == 1:
        z = p64[:, 2].exp()
        ez = _rel_err(got[:n, 2], z)
        exy = _rel_err(got[:n, :2], p64[:, :2] * z[:, None])
        print(f"moge_remap exp n={n}: z rel {ez:.3e}, xy rel {exy:.3e}")
        assert ez <= EXP_RTOL and exy <= EXP_RTOL + U
    elif remap == 2:
        e = _rel_err(got[:n], p64.sinh())
        print(f"moge_remap sinh n={n}: sinhf max rel {e:.3e}")
        assert e <= SINH_RTOL
    else:
        exy = _rel_err(got[:n, :2], p64[:, :2].sinh())
        ez = _rel_err(got[:n, 2], p64[:, 2].exp())
        print(f"moge_remap sinh_exp n={n}: sinhf max rel {exy:.3e}, expf max rel {ez:.3e}")
        assert exy <= SINH_RTOL and ez <= EXP_RTOL

    # mask = None: only the points change
    pts2 = p0.to(DEV)
    ops.moge_remap(pts2, None, n, remap, None)
    assert _same_bits(pts2, got[:n])


@pytest.mark.parametrize("n", [1000, 257])
def test_moge_remap_mask_is_the_sign_of_the_logit(built_lib, n):
    """sigmoid(l) > 0.5 <=> l > 0; NaN gives 0.  Logits in (0, 1e-7) are left out: there the fp32 sigmoid legitimately
    rounds to 0.5.  No flip is allowed anywhere else."""
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(n + 1)
    inf = float("inf")
    l = torch.randn(n, generator=gen) * 3
    l = torch.where(l.abs() < 1e-6, torch.full_like(l, 1e-6), l)
    special = torch.tensor([0.0, -0.0, 1e-6, -1e-6, 0.3, -0.3, 100.0, -100.0, inf, -inf, NAN])
    l[:special.numel()] = special
    p0 = _remap_points(n)
    pts = p0.to(DEV)
    mask = torch.full((n + 1,), 7, dtype=torch.uint8, device=DEV)
    ops.moge_remap(pts, l.to(DEV), n, 0, mask)
    got = mask.cpu()
    assert torch.equal(got[:n], (l > 0).to(torch.uint8)) and got[n].item() == 7
    assert _same_bits(pts, p0)


# ----------------------------------------------------------------------------------------------------- moge_depth
@pytest.mark.parametrize("shift", [-0.25, 0.0])
@pytest.mark.parametrize("with_scale", [True, False])
def test_moge_depth_mask_and_depth(built_lib, shift, with_scale):
    """ok = mask & (fp32(z + shift) > 0); mask_out = ok; depth = +inf where not ok, else (z + shift) exp(log_scale)."""
    from pi3_slam_amd import ops
    n = 1000
    gen = torch.Generator().manual_seed(17)
    z = torch.randn(n, generator=gen) * 0.5
    lo = np.nextafter(np.float32(0.25), np.float32(0))
    hi = np.nextafter(np.float32(0.25), np.float32(1))
    # with shift = -0.25: a pair that cancels to 0 and its two neighbours; with shift = 0: z exactly 0, either sign
    z[:8] = torch.tensor([0.25, float(lo), float(hi), 0.0, -0.0, 0.5, -0.5, -0.25])
    m_in = (torch.rand(n, generator=gen) < 0.7).to(torch.uint8)
    m_in[:8] = 1
    m_in[8:16] = torch.tensor([0, 1] * 4, dtype=torch.uint8)
    z[8:16] = torch.tensor([1.0, 1.0, -1.0, -1.0, 0.25, 0.25, 2.0, 2.0])
    pts = torch.full((n, 3), NAN)                                  # x, y are not this kernel's business
    pts[:, 2] = z
    sh = torch.tensor([shift])
    ls = torch.tensor([0.7]) if with_scale else None
    mask = torch.full((n + 1,), 7, dtype=torch.uint8)
    mask[:n] = m_in
    mask = mask.to(DEV)
    depth = torch.full((n + 1,), NAN, device=DEV)
    ops.moge_depth(pts.to(DEV), sh.to(DEV), ls.to(DEV) if with_scale else None, mask, n, depth)
    d32 = z + sh                                                   # the fp32 sum, rounded as the device rounds it
    ok = m_in.bool() & (d32 > 0)
    assert ok.any() and (~ok).any() and (m_in.bool() & ~ok).any()
    got_m, got_d = mask.cpu(), depth.cpu()
    assert torch.equal(got_m[:n], ok.to(torch.uint8)) and got_m[n].item() == 7
    assert _same_bits(got_d[n:], torch.full((1,), NAN))
    assert _same_bits(got_d[:n][~ok], torch.full((int((~ok).sum()),), float("inf")))
    if with_scale:
        want = (z.double() + sh.double()) * ls.double().exp()
        rel = ((got_d[:n][ok].double() - want[ok]).abs() / want[ok].abs()).max().item()
        print(f"moge_depth shift={shift}: max rel {rel:.3e}")
        assert rel <= 3e-6
    else:
        assert _same_bits(got_d[:n][ok], d32[ok])


# -------------------------------------------------------------------------------------------- add_rows, fill_tokens
@pytest.mark.parametrize("rows,C,ldx,ldy", [(1000, 32, 32, 64), (5, 3, 8, 4), (40000, 64, 64, 64)])   # the last: > 256*32 blocks
def test_add_rows_equals_the_host_sum(built_lib, rows, C, ldx, ldy):
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(rows + C)
    x0, y0 = torch.randn(rows, C, generator=gen), torch.randn(rows, C, generator=gen)
    x = _padded(x0, ldx).to(DEV)
    ops.add_rows(x, _padded(y0, ldy).to(DEV), rows, C)
    got = x.cpu()
    assert _same_bits(got[:, :C], x0 + y0)                          # one IEEE addition per element
    assert _same_bits(got[:, C:], torch.full((rows, ldx - C), NAN))


@pytest.mark.parametrize("F,T,D,t0,nt", [(3, 11, 256, 0, 5), (2, 9, 384, 4, 5), (300, 6, 1024, 0, 5)])   # the last: > 4096 blocks
def test_fill_tokens_writes_its_rows_and_no_others(built_lib, F, T, D, t0, nt):
    from pi3_slam_amd import ops
    gen = torch.Generator().manual_seed(F + T + D)
    x0 = torch.randn(F * T, D, generator=gen)
    vals = torch.randn(nt, D, generator=gen)
    x = x0.to(DEV)
    ops.fill_tokens(x, F, T, t0, vals.to(DEV))
    want = x0.clone().view(F, T, D)
    want[:, t0:t0 + nt] = vals
    assert _same_bits(x, want.view(F * T, D))


def test_fill_tokens_rejects_rows_past_the_frame(built_lib):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    x = torch.zeros(2 * 9, 64, device=DEV)
    with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
        ops.fill_tokens(x, 2, 9, 5, torch.zeros(5, 64, device=DEV))           # t0 + nt = 10 > T
    assert not x.any()
