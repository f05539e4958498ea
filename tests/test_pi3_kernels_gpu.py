"""The row and head kernels of the Pi3 path (csrc/elem.hip, csrc/heads.hip), each called directly through
pi3_slam_amd.ops and compared with the same operation written out in fp64 (tests/pi3_kernels_ref.py, pinned to torch by
tests/test_pi3_kernels_ref.py) from the same fp32 / bf16 inputs.

Bounds are per element: equality where the operation is exact (casts, gathers, a subtraction followed by a product),
otherwise k U (sum of the magnitudes entering that element), U = 2^-24, with k counted from the roundings in the kernel
source (the count stands in each reference's docstring and is repeated in the test's).  rsqrtf and expf get 2 ulp: HIP's
own statement of their error is not at hand.  A 16-bit output is held to |out - ref64| <= ulp16(ref64) / 2 + that fp32
bound, which a truncating pack breaks on about half the elements.

Poison rule: input pad columns [C, ld), input rows beyond `rows`, register-token rows that must be skipped and input
columns at and beyond in_cols hold NaN; outputs start as NaN; everything outside the documented write range keeps its bits.
"""
import math

import pytest
import torch

import pi3_kernels_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
DT16 = [torch.bfloat16, torch.float16]
DT = [torch.float32] + DT16
QSCALE = 0.125 * math.log2(math.e)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)
    return torch.device("cuda:0")


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns (NaN payloads and the sign of zero included) on the host."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(_bits(a), _bits(b))


def _same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit, except that a NaN matches any NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def _is_nan_fill(t: torch.Tensor) -> bool:
    """Untouched since torch.full(..., NaN)."""
    return _same_bits(t, torch.full(t.shape, NAN, dtype=t.dtype))


def _padded(vals: torch.Tensor, ld: int, extra_rows: int = 0) -> torch.Tensor:
    """[rows, C] -> [rows + extra_rows, ld] with NaN in the pad columns and the extra rows."""
    out = torch.full((vals.shape[0] + extra_rows, ld), NAN, dtype=vals.dtype)
    out[:vals.shape[0], :vals.shape[1]] = vals
    return out


def _within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> None:
    """|got - ref| <= bound on every element (fp32 result); for a 16-bit result half an ulp of the format at ref more."""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), what
    if got.dtype != torch.float32:
        bound = bound + 0.5 * R.ulp16(ref, got.dtype)
    excess = (got.double() - ref).abs() - bound
    i = int(excess.argmax())
    assert excess.max().item() <= 0, (what, i, got.flatten()[i].item(), ref.flatten()[i].item(), bound.flatten()[i].item())


# ------------------------------------------------------------------------------------------------------ layernorm
LN_D = [4, 252, 256, 260, 384, 516, 1024, 1028, 2048]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_against_fp64(dev, D, dt):
    """rows in {1, 5, 9} of a buffer one row longer (its last row NaN), ldx = D + 4, ldo = D + 8, three data sets.
    k: the mean sees VPL + 9 roundings, the variance VPL + 11 (+ 2 for the centred value), rsqrtf 2 ulp, the output
    three on the product and one on the sum - assembled in pi3_kernels_ref._ln_core."""
    from pi3_slam_amd import ops
    g = torch.Generator().manual_seed(D)
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    wd, bd = w.to(dev), b.to(dev)
    for rows in (1, 5, 9):
        for kind in ("randn", "offset", "range"):
            x = R.layernorm_data(kind, rows, D, g)
            xb = _padded(x, D + 4, 1).to(dev)
            ob = torch.full((rows + 1, D + 8), NAN, dtype=dt, device=dev)
            ops.layernorm(xb[:, :D], wd, bd, ob[:, :D], rows=rows)
            ref, bound = R.layernorm_ref(x, w, b, 1e-6)
            got = ob.cpu()
            _within(got[:rows, :D], ref, bound, (rows, kind))
            assert _is_nan_fill(got[:rows, D:]) and _is_nan_fill(got[rows:])


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("D", [4, 256, 1024, 2048])
def test_layernorm_zero_variance_rows_return_the_bias(dev, D, dt):
    """x constant at a small integer, D a power of two: sum, mean and x - mean are exact, so y = 0 rstd w + b = b."""
    from pi3_slam_amd import ops
    g = torch.Generator().manual_seed(D + 1)
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    assert (b != 0).all()
    x = torch.tensor([3.0, -2.0, 7.0, 0.0, 1.0]).view(5, 1).expand(5, D).contiguous()
    xb = _padded(x, D + 4, 1).to(dev)
    ob = torch.full((6, D + 8), NAN, dtype=dt, device=dev)
    ops.layernorm(xb[:, :D], w.to(dev), b.to(dev), ob[:, :D], rows=5)
    got = ob.cpu()
    assert _same_bits(got[:5, :D], b.to(dt).expand(5, D))
    assert _is_nan_fill(got[:5, D:]) and _is_nan_fill(got[5:])


@pytest.mark.parametrize("T,ns,rows", [(11, 5, 25), (4, 4, 9)])
@pytest.mark.parametrize("D", [256, 516])
def test_layernorm_special_rows_are_copies(dev, T, ns, rows, D):
    """Rows with row % T < ns are special[row % T] bit for bit (-0.0 included) and their x rows (NaN) are not read; every
    other row - the one after the last special row among them - is normalised."""
    from pi3_slam_amd import ops
    g = torch.Generator().manual_seed(T * 100 + D)
    w, b = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    sp = torch.randn(ns, D, generator=g)
    sp[:, ::7] = -0.0
    x = torch.randn(rows, D, generator=g) * 3 + 1
    t = torch.arange(rows) % T
    x[t < ns] = NAN
    xb = _padded(x, D + 4, 1).to(dev)
    ob = torch.full((rows + 1, D + 8), NAN, device=dev)
    ops.layernorm(xb[:, :D], w.to(dev), b.to(dev), ob[:, :D], rows=rows, T=T, nspecial=ns, special=sp.to(dev))
    got = ob.cpu()
    assert _same_bits(got[:rows, :D][t < ns], sp[t[t < ns]])
    normal = t >= ns
    assert bool(normal[ns]) == (ns < T) and bool(normal.any()) == (ns < T)
    if normal.any():
        ref, bound = R.layernorm_ref(x[normal], w, b, 1e-6)
        _within(got[:rows, :D][normal], ref, bound)
    assert _is_nan_fill(got[:rows, D:]) and _is_nan_fill(got[rows:])


def test_layernorm_rejects_bad_arguments(dev):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    for D, dt, ns in ((6, torch.float32, 0), (2052, torch.float32, 0), (256, torch.bfloat16, 2), (256, torch.float16, 2)):
        x = torch.zeros(4, D + 4 - D % 4, device=dev)[:, :D]
        out = torch.full((4, D + 8 - D % 4), NAN, dtype=dt, device=dev)
        w = torch.ones(D, device=dev)
        with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
            ops.layernorm(x, w, w, out[:, :D], T=4, nspecial=ns, special=torch.zeros(2, D, device=dev) if ns else None)
        assert _is_nan_fill(out)


# ------------------------------------------------------------------------------------------------------ cast_rows
def _cast_case(dev, x, rows, cols, in_cols, ldi, ldo, dt):
    """x [rows, in_cols] -> run cast_rows on poisoned buffers one row longer than `rows`; checks the whole output."""
    from pi3_slam_amd import ops
    xb = _padded(x, ldi, 1).to(dev)
    ob = torch.full((rows + 1, ldo), NAN, dtype=dt, device=dev)
    ops.cast_rows(xb, ob, rows=rows, cols=cols, in_cols=in_cols)
    got = ob.cpu()
    assert _same_values(got[:rows, :cols], R.cast_ref(x, cols, in_cols, dt))
    assert _same_values(got[:rows, :in_cols], x.to(dt))                            # torch's own cast
    assert _is_nan_fill(got[:rows, cols:]) and _is_nan_fill(got[rows:])


@pytest.mark.parametrize("dt", DT)
def test_cast_rows_value_table(dev, dt):
    """Round to nearest even like torch's cast: signed zeros, infinities, NaN (as a NaN), bf16 and half ties either way,
    the half overflow threshold, half subnormals, +-max fp32."""
    n = len(R.CAST_TABLE)
    _cast_case(dev, torch.tensor(R.CAST_TABLE).view(1, n), 1, n, n, n, n, dt)
    _cast_case(dev, torch.tensor(R.CAST_TABLE).view(n // 4, 4), n // 4, 8, 4, 8, 12, dt)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,cols,in_cols,ldi,ldo", R.CAST_SHAPES)
def test_cast_rows_shapes_pads_and_zero_fill(dev, rows, cols, in_cols, ldi, ldo, dt):
    """Columns [in_cols, cols) come out as zero bits and their inputs (NaN) are not read; [cols, ldo) keep their bits."""
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, in_cols, generator=g) * 10
    x[0, :4] = torch.tensor([65520.0, -1e-7, 1 + 2.0 ** -8, -0.0])
    _cast_case(dev, x, rows, cols, in_cols, ldi, ldo, dt)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,cols", R.CAST_CAPPED)
def test_cast_rows_capped_grid_walk(dev, rows, cols, dt):
    """More float4s than 4096 workgroups cover in one sweep: every thread walks (row, quad) with a carry (12 and 20
    columns) or without one (2048).  Values come from the flat index, so a slipped row or quad shows."""
    _cast_case(dev, R.index_values(rows, cols), rows, cols, cols, cols + 4, cols + 4, dt)


@pytest.mark.parametrize("dt", DT)
def test_cast_rows_capped_grid_zero_fill(dev, dt):
    """in_cols < cols on the capped grid: a thread's second and later steps write zeros too (a value kept from its
    previous step would show), and the input columns [in_cols, ldi) - NaN - are not read on any step."""
    rows, cols, in_cols = R.CAST_CAPPED_FILL
    _cast_case(dev, R.index_values(rows, in_cols), rows, cols, in_cols, in_cols + 4, cols + 4, dt)


def test_cast_rows_rejects_bad_arguments(dev):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    x = torch.ones(2, 16, device=dev)
    out = torch.full((2 * 16 + 4,), NAN, dtype=torch.bfloat16, device=dev)
    o = out[:32].view(2, 16)
    for kw in (dict(cols=8, in_cols=12), dict(cols=6, in_cols=4)):
        with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
            ops.cast_rows(x, o, **kw)
    mis = out[1:33].view(2, 16)
    assert mis.data_ptr() % 8 == 2
    with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
        ops.cast_rows(x, mis)
    assert _is_nan_fill(out)


# ---------------------------------------------------------------------------------------------------- patch_gather
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("KP", [588, 590, 640])
@pytest.mark.parametrize("F,H,W,offset", [(1, 14, 14, 0), (2, 28, 126, 0), (1, 14, 238, 0), (2, 28, 126, 1)])
def test_patch_gather_is_the_normalised_gather_with_torchs_cast(dev, F, H, W, offset, KP, dt):
    """(img - mean) * (float32(1) / float32(std)): a subtraction, then a product - nothing to contract - so the fp32
    value is the host's and the output equals torch's cast of it; pw = 1, 9 = 8 + 1, 17 = 8 + 8 + 1 patches per row.
    offset = 1: the image starts one float into its buffer (rows no longer 8-byte aligned: scalar loads)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.weights import IMAGE_MEAN, IMAGE_STD
    g = torch.Generator().manual_seed(H * W + KP)
    img = torch.rand(F, 3, H, W, generator=g)
    n = img.numel()
    buf = torch.full((n + 2 * offset,), NAN)
    buf[offset: offset + n] = img.flatten()
    buf = buf.to(dev)
    imgd = buf[offset: offset + n].view(F, 3, H, W)
    assert imgd.data_ptr() % 8 == 4 * offset
    P = F * (H // 14) * (W // 14)
    ob = torch.full((P + 1, KP), NAN, dtype=dt, device=dev)
    ops.patch_gather(imgd, ob[:P], IMAGE_MEAN, IMAGE_STD)
    want, rows = R.patch_gather_ref(img, IMAGE_MEAN, IMAGE_STD, KP, dt)
    got = ob.cpu()
    assert _same_bits(got[:P, :588], rows.to(dt))
    assert _same_bits(got[:P], want)                                               # pad columns: zero bits
    assert _is_nan_fill(got[P:])


# --------------------------------------------------------------------------------------------------- resample_grid
@pytest.mark.parametrize("D", [1, 128, 300, 1024])
@pytest.mark.parametrize("Mi,Mj,oh,ow", [(5, 7, 2, 3), (37, 37, 22, 29)])
@pytest.mark.parametrize("taps", ["random", "bicubic"])
def test_resample_grid_against_fp64(dev, Mi, Mj, oh, ow, D, taps):
    """dst = wy src wx^T.  Zero taps are skipped; a term passes through its product, at most nzx(x) row additions, the
    product with wy and at most nzy(y) additions: k = nzy(y) + nzx(x) + 2.  Random dense taps carry exact zeros and
    negative entries; `bicubic` is the engine's own table."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.engine import bicubic_aa_taps
    g = torch.Generator().manual_seed(Mi * 100 + D)
    src = torch.randn(Mi, Mj, D, generator=g) * 2 + 0.5
    if taps == "random":
        wy, wx = torch.randn(oh, Mi, generator=g), torch.randn(ow, Mj, generator=g)
        wy[torch.rand(oh, Mi, generator=g) < 0.3] = 0.0
        wx[torch.rand(ow, Mj, generator=g) < 0.3] = 0.0
        wy[0], wx[-1, 1:] = 0.0, 0.0                                                # an all-zero row, a one-tap row
        wy[-1, 0], wx[0, 0] = -0.75, -1.25
        assert (wy < 0).any() and (wx < 0).any()
    else:
        wy, wx = torch.from_numpy(bicubic_aa_taps(Mi, oh)), torch.from_numpy(bicubic_aa_taps(Mj, ow))
    got = ops.resample_grid(src.to(dev), wy.to(dev), wx.to(dev))
    ref, bound = R.resample_ref(src, wy, wx)
    assert got.shape == (oh, ow, D)
    _within(got, ref, bound)
    if taps == "random":
        assert _same_bits(got[0], torch.zeros(ow, D))


# ----------------------------------------------------------------------------------------------------- qknorm_rope
@pytest.mark.parametrize("rows,H,T", R.QK_SHAPES)
@pytest.mark.parametrize("norm,rope", [(True, True), (True, False), (False, True), (False, False)])
def test_qknorm_rope_against_fp64(dev, rows, H, T, norm, rope):
    """fp64 from the bf16 inputs and the same cos / sin table.  Norm: k_mean = 11 (8 adds, 3 shuffle levels), k_var = 13,
    rsqrtf 2 ulp; RoPE: 2 U (|x c| + |p s|) on top of the inputs' errors; q * qscale one rounding; then half a bf16 ulp.
    v keeps its bits everywhere, and so does the buffer's last row (beyond `rows`).  Without norm: tokens at (0, 0) are
    rotated by the identity, so their k keeps its bits and their q is the rounded fp32 product q * qscale - as is every
    q, and k too, when there is no rotation either."""
    from pi3_slam_amd import ops
    qkv0, pos, cs, nw = R.qk_case(rows, H, T)
    buf = torch.cat([qkv0, torch.full((1, 3 * H * 64), NAN, dtype=torch.bfloat16)]).to(dev)
    args = [t.to(dev) for t in nw] if norm else [None] * 4
    ops.qknorm_rope(buf, rows, H, T, pos.to(dev) if rope else None, cs.to(dev) if rope else None, *args, eps=1e-5,
                    qscale=QSCALE, do_rope=rope)
    got = buf.cpu()
    assert _is_nan_fill(got[rows:])
    got = got[:rows].view(rows, 3, H, 64)
    x0 = qkv0.view(rows, 3, H, 64)
    assert _same_bits(got[:, 2], x0[:, 2])
    ref, bound = R.qknorm_rope_ref(qkv0, rows, H, T, pos, cs, *(nw if norm else [None] * 4), 1e-5, QSCALE, rope)
    _within(got[:, :2], ref[:, :2], bound[:, :2], (norm, rope))
    if not norm:
        ident = torch.ones(rows, dtype=torch.bool) if not rope else (pos[torch.arange(rows) % T] == 0).all(1)
        assert ident.any()
        qs = (x0[:, 0].float() * torch.tensor(QSCALE, dtype=torch.float32)).bfloat16()
        assert _same_bits(got[:, 0][ident], qs[ident]) and _same_bits(got[:, 1][ident], x0[:, 1][ident])


# ----------------------------------------------------------------------------------------------- unpatchify_points
def _unp_case(dev, F, H, W, tok_off, extra, ldp, ldc, offset=0):
    from pi3_slam_amd import ops
    P = (H // 14) * (W // 14)
    T = tok_off + P + extra
    g = torch.Generator().manual_seed(H * W + T + ldp)

    def feats(C, ld, scale):
        v = torch.full((F, T, C), NAN)
        v[:, tok_off: tok_off + P] = torch.randn(F, P, C, generator=g) * scale
        flat = torch.full((F * T * ld + offset,), NAN)
        flat[offset:].view(F * T, ld)[:, :C] = v.view(F * T, C)
        d = flat.to(dev)[offset:].view(F * T, ld)
        assert d.data_ptr() % 16 == (4 * offset) % 16
        return v.view(F * T, C), d
    pf, pfd = feats(588, ldp, 0.5)
    cf, cfd = feats(196, ldc, 2.0)
    q, _ = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))
    poses = torch.zeros(F, 4, 4)
    poses[:, :3, :3], poses[:, :3, 3], poses[:, 3, 3] = q, torch.randn(F, 3, generator=g) * 10, 1.0
    lp = torch.full((F + 1, H, W, 3), NAN, device=dev)
    pts = torch.full((F + 1, H, W, 3), NAN, device=dev)
    conf = torch.full((F + 1, H, W, 1), NAN, device=dev)
    ops.unpatchify_points(pfd, cfd, poses.to(dev), F, H, W, T, tok_off, lp, pts, conf)
    lp, pts, conf = lp.cpu(), pts.cpu(), conf.cpu()
    for t in (lp, pts, conf):
        assert _is_nan_fill(t[F:])
    local, bound, cref = R.unpatchify_ref(pf, cf, F, H, W, T, tok_off)
    assert _same_bits(conf[:F], cref)
    _within(lp[:F], local, bound, "local")
    wref, wbound = R.world_ref(lp[:F], poses)
    _within(pts[:F], wref, wbound, "world")


@pytest.mark.parametrize("ldp,ldc", [(588, 196), (589, 197), (640, 256)])
@pytest.mark.parametrize("tok_off,extra", [(0, 0), (5, 0), (5, 4)])
@pytest.mark.parametrize("F,H,W", [(1, 14, 14), (2, 28, 126), (1, 42, 238)])
def test_unpatchify_points_against_fp64(dev, F, H, W, tok_off, extra, ldp, ldc):
    """conf: the gather, bit for bit.  z: fp64 exp at expf's 2 ulp; x z, y z one rounding more.  World points: fp64 from
    the kernel's own local points, 4 U (|t0 lx| + |t1 ly| + |t2 z| + |t3|).  T = tok_off + P + extra: the register rows in
    front and the rows behind hold NaN, like the pads [588, ldp), [196, ldc); ld 589 / 197 take the scalar staging path."""
    _unp_case(dev, F, H, W, tok_off, extra, ldp, ldc)


def test_unpatchify_points_with_a_misaligned_base(dev):
    """ld % 4 == 0, but the buffers start one float off a 16-byte boundary: the scalar staging path again."""
    _unp_case(dev, 2, 28, 126, 5, 4, 640, 256, offset=1)


def test_unpatchify_points_rejects_bad_arguments(dev):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    z = lambda *s: torch.zeros(*s, device=dev)
    outs = [torch.full((1, 28, 28, c), NAN, device=dev) for c in (3, 3, 1)]
    for H, ldp, T in ((15, 640, 9), (28, 584, 9), (28, 640, 8)):                  # H % 14, ldp < 588, T < tok_off + P
        with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
            ops.unpatchify_points(z(9, ldp), z(9, 256), z(1, 4, 4), 1, H, 28, T, 5, *outs)
    assert all(_is_nan_fill(o) for o in outs)


# ----------------------------------------------------------------------------------------------------- camera_tail
@pytest.mark.parametrize("tok_off", [0, 5])
@pytest.mark.parametrize("P", R.CAM_P)
@pytest.mark.parametrize("D", R.CAM_D)
def test_camera_tail_against_fp64(dev, D, P, tok_off):
    """Three frames, ld = D + 4 (pads NaN), register rows NaN.  Translation: the forward bound of camera_tail_ref (pool
    k = ceil(P / np) + np + 3, every layer k = ceil(D / 64) + 8, errors carried through |W|).  Rotation: against the SVD
    orthogonalisation of the fp64 pre-rotation matrix within 2 ||dA||_F / (s2 + sign(det) s3) + U; the cases (both signs
    of det, gap > 0.1 in every frame) are asserted in tests/test_pi3_kernels_ref.py.  np = 8, 8, 8, 5, 4 for the five
    widths; P = 1, 3 leave row phases empty."""
    from oracle.pi3_ref import svd_orthogonalize
    from pi3_slam_amd import ops
    Fr = 3
    feat, T, w = R.camera_case(D, P, tok_off)
    fd = _padded(feat, D + 4).to(dev)
    wd = {k: v.to(dev).contiguous() for k, v in w.items()}
    poses = torch.full((Fr + 1, 4, 4), NAN, device=dev)
    ops.camera_tail(fd[:, :D], T, tok_off, Fr, P, wd, poses)
    got = poses.cpu()
    assert _is_nan_fill(got[Fr:]) and torch.isfinite(got[:Fr]).all()
    ref = R.camera_tail_ref(feat, Fr, P, T, tok_off, w)
    _within(got[:Fr, :3, 3], ref["t"], ref["t_bound"], "translation")
    Rg = got[:Fr, :3, :3].double()
    tol = R.rotation_tolerance(ref)
    err = (Rg - ref["R"]).abs().amax((1, 2))
    assert (err <= tol).all(), (err, tol)
    assert (ref["R"] - svd_orthogonalize(ref["A"].reshape(Fr, 9))).abs().max() < 1e-12
    assert (Rg.transpose(1, 2) @ Rg - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-6
    assert (torch.det(Rg) - 1).abs().max() <= 1e-6
    assert _same_bits(got[:Fr, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(Fr, 4))


def test_camera_tail_rejects_bad_arguments(dev):
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    poses = torch.full((2, 4, 4), NAN, device=dev)
    for D, ld in ((1028, 1028), (6, 8), (8, 10)):                                 # D > 1024, D % 4, ld % 4
        feat = torch.zeros(2 * 3, ld, device=dev)[:, :D]
        w = {}
        for name, n in zip(R.CAM_W, (D, D, 3, 9)):
            w[name + ".weight"], w[name + ".bias"] = torch.zeros(n, D, device=dev), torch.zeros(n, device=dev)
        with pytest.raises(L.Pi3HipError, match=r"rc=-1\b"):
            ops.camera_tail(feat, 3, 0, 2, 3, w, poses)
    assert _is_nan_fill(poses)
