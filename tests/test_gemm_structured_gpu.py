"""pi3_gemm, pi3_gemm_qkv and pi3_conv3x3 on operands whose exact result is known (tests/gemm_patterns.py), through
every kernel and template instance the product build dispatches to.

The accuracy tests of the GEMM family compare Gaussian operands under max|d| / max|ref| <= 6e-3: one lost k element of
1024, a residual row from the neighbour or a q-scale boundary one column group off is far below that.  Here every such
fault is a wrong integer, and every comparison but GELU is bit for bit (gemm_patterns.check_exact) against fp64
arithmetic on the numbers the kernel reads, rounded once by torch's cast where the output is a 16-bit type.

Every operand is a column slice of a wider buffer filled with NaN (lda > K, ldw > K, ldo > N, ldr != ldo, ldadd != N): a
read outside the slice poisons the result.  Every output is prefilled with NaN where the kernel must write and with a
sentinel everywhere else - the columns beside the slice, the rows a row remap skips, the rows behind the last one -
and the sentinels must come back untouched.

Shapes (gemm_patterns.GEMM_SHAPES ... CONV_CASES; tests/test_gemm_patterns.py checks that they reach every kernel
and every dispatched instance): the 128x128 kernel at one, two, three and ten K steps and M around its tile height; the
narrow kernel at both tile widths and M around 256; the 256x256 kernel at M = 1024 ... 1281 (the last row panel of a
wave, the last tile), both tile orders (N / 256 <= 4 or not), one to sixteen K steps, and 272 tiles for the persistent
walk; its two decline cases, which the 128x128 kernel must answer with the same bits; the row remap with rpg = 37
(dividing no tile height), goff = 3, gstride = 45 on both fp32-output kernels; pi3_gemm_qkv fused and two-pass, batch
seams inside a tile and inside a wave's rows, row % T wrapping inside a tile; pi3_conv3x3 from 1x1 to 19x23x2 images.

GELU: the pre-activations are 0 or integers of magnitude >= 8; the bound is the absolute figure that
test_gelu_epilogue_accuracy_on_ten_million_samples asserts against the fp64 truth at sigma = 1 (read from that test),
plus one rounding of the 16-bit store (attn_patterns.STORE_TOL)."""
import pytest
import torch

import gemm_patterns as gp

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 8                 # elements on either side of every sliced operand: 16 bytes of a 16-bit type, 32 of fp32
GELU_FORM_DEFAULT = 0   # knob gelu_form: 0 the exp2 form, 1 the sigmoid form of the tanh approximation


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pi3_slam_amd import lib
    lib.load(require_gpu=True)
    return torch.device("cuda:0")


def gelu_abs_bound():
    """max_vs_truth of the sigma = 1 row of test_gelu_epilogue_accuracy_on_ten_million_samples."""
    import test_kernels_gpu
    mark = [m for m in test_kernels_gpu.test_gelu_epilogue_accuracy_on_ten_million_samples.pytestmark
            if m.name == "parametrize"][0]
    names = [s.strip() for s in mark.args[0].split(",")]
    rows = [dict(zip(names, r)) for r in mark.args[1]]
    return [r["max_vs_truth"] for r in rows if r["sigma"] == 1.0][0]


def sliced(values, dtype, dev, pad=PAD, extra_rows=0):
    """A [R, C] view, holding `values`, into a wider buffer full of NaN."""
    R, Cn = values.shape
    big = torch.full((R + extra_rows, Cn + 2 * pad), NAN, device=dev, dtype=dtype)
    view = big[:R, pad:pad + Cn]
    view.copy_(values.to(dev))
    return view


class Out:
    """[rows, N] output slice of a [rows + 2, N + 2 PAD] buffer: NaN on `written` rows, the sentinel everywhere else."""

    def __init__(self, rows, N, dtype, dev, written):
        self.big = torch.full((rows + 2, N + 2 * PAD), gp.SENTINEL, device=dev, dtype=dtype)
        self.view = self.big[:rows, PAD:PAD + N]
        self.view[written.to(dev)] = NAN
        self.N = N
        assert self.view.data_ptr() % 16 == 0 and self.big.stride(0) % 4 == 0

    def surroundings_intact(self):
        rows = self.view.shape[0]
        return bool((self.big[:, :PAD] == gp.SENTINEL).all()) and bool((self.big[:, PAD + self.N:] == gp.SENTINEL).all()) \
            and bool((self.big[rows:] == gp.SENTINEL).all())


class Uploaded:
    """A GemmCase's operands on the device, each a slice of a wider NaN buffer, in the operands' type."""

    def __init__(self, case, in_dtype, dev):
        self.case = case
        self.A = sliced(case.A, in_dtype, dev)
        self.W = sliced(case.W, in_dtype, dev)
        assert torch.equal(self.A.float().cpu(), case.A) and self.A.stride(0) > case.K and self.W.stride(0) > case.K
        self.bias = case.bias.to(dev) if case.bias is not None else None
        self.gamma = case.gamma.to(dev) if case.gamma is not None else None
        # fp32 rows read 16 bytes at a time: 4 floats beside the residual (ldr = N + 8, the output's ldo = N + 16), 4 behind
        # a row of the table (ldadd = N + 4)
        self.resid = sliced(case.resid, torch.float32, dev, pad=4) if case.resid is not None else None
        self.addtab = None
        if case.addtab is not None:
            big = torch.full((case.addtab.shape[0], case.N + 4), NAN, device=dev)
            self.addtab = big[:, :case.N]
            self.addtab.copy_(case.addtab.to(dev))
        self.exact = gp.gemm_reference(case)
        self.written = gp.remapped_rows(case)


def run_gemm(dev, up, out_dtype, qcols=None):
    from pi3_slam_amd import ops
    c = up.case
    out = Out(c.out_rows, c.N, out_dtype, dev, up.written)
    if up.resid is not None:
        assert up.resid.stride(0) != out.big.stride(0)
    ops.gemm(up.A, up.W, out.view, M=c.M, K=c.K, bias=up.bias, gamma=up.gamma, resid=up.resid, act=c.act, rpg=c.rpg,
             gstride=c.gstride, goff=c.goff, addtab=up.addtab, qscale=c.qscale, qcols=c.qcols if qcols is None else qcols)
    torch.cuda.synchronize()
    return out


def _shape_id(s):
    return f"{s[0]}-M{s[1]}-N{s[2]}-K{s[3]}"


@pytest.mark.parametrize("shape", gp.GEMM_SHAPES, ids=_shape_id)
def test_patterns_plain(dev, shape):
    """tally, both address pairs and rounding with no epilogue operand, into the 16-bit type and into fp32."""
    dt, M, N, K = shape
    in_dtype = gp.DTYPES[dt]
    out16 = torch.bfloat16 if dt == "f32" else in_dtype
    cases = [("tally", gp.tally(M, N, K)), ("address0", gp.address(M, N, K, 0))]
    if M * N <= (1 << 22):      # the 272-tile case is about which tile lands where: the first two patterns say it
        cases += [("address1", gp.address(M, N, K, 1)), ("rounding", gp.rounding(M, N, K, out16))]
    for name, case in cases:
        up = Uploaded(case, in_dtype, dev)
        for out_dtype in (out16, torch.float32):
            out = run_gemm(dev, up, out_dtype)
            ok, msg = gp.check_exact(out.view, up.exact)
            assert ok, (name, str(out_dtype), msg)
            assert out.surroundings_intact(), (name, str(out_dtype), "wrote outside the output slice")


@pytest.mark.parametrize("spec", gp.EPILOGUE_CASES, ids=lambda s: s.name)
def test_epilogue(dev, spec):
    from pi3_slam_amd import lib
    case = gp.epilogue(spec.M, spec.N, spec.K, act=spec.act, **spec.kwargs())
    for pair in (0, 1):
        if pair:
            case = gp.epilogue(spec.M, spec.N, spec.K, act=spec.act, pair=1, **spec.kwargs())
        up = Uploaded(case, gp.DTYPES[spec.in_dtype], dev)
        try:
            lib.set_knob("gelu_form", spec.gelu_form)
            out = run_gemm(dev, up, gp.DTYPES[spec.out_dtype])
        finally:
            lib.set_knob("gelu_form", GELU_FORM_DEFAULT)
        assert out.surroundings_intact(), "wrote outside the output slice"
        if spec.act != 1:
            ok, msg = gp.check_exact(out.view, up.exact)
            assert ok, (spec.name, pair, msg)
            continue
        rows = up.written.to(dev)
        skipped = torch.ones(case.out_rows, dtype=torch.bool, device=dev)
        skipped[rows] = False
        assert bool((out.view[skipped] == gp.SENTINEL).all())
        ok, worst, msg = gp.check_gelu(out.view[rows], up.exact[up.written], gelu_abs_bound())
        print(f"{spec.name} pair {pair}: {msg}")
        assert ok, (spec.name, pair, msg)


@pytest.mark.parametrize("dt,M,N,K", [("bf16", 129, 384, 64), ("f16", 257, 96, 64), ("f32", 129, 128, 32), ("bf16", 1153, 512, 64)])
def test_qcols_off_the_column_groups_is_refused(dev, dt, M, N, K):
    """A boundary inside a group of 4 columns would scale the whole group: pi3_gemm refuses it (and a negative one, and
    one beyond N) before any launch, and the output keeps its prefill."""
    from pi3_slam_amd import lib, ops
    case = gp.epilogue(M, N, K, qscale=0.5, qcols=20)
    up = Uploaded(case, gp.DTYPES[dt], dev)
    for bad in (-4, 2, 21, N - 1, N + 4):
        out = Out(case.out_rows, N, torch.float32, dev, up.written)
        before = out.big.clone()
        with pytest.raises(lib.Pi3HipError, match="qcols"):
            ops.gemm(up.A, up.W, out.view, M=M, K=K, bias=up.bias, qscale=0.5, qcols=bad)
        torch.cuda.synchronize()
        assert torch.equal(out.big.view(torch.int32), before.view(torch.int32)), (bad, "a refused call wrote")
    for good in (0, 4, 20, N - 4, N):       # the boundary cases stay exact
        c = gp.epilogue(M, N, K, qscale=0.5, qcols=good)
        ok, msg = gp.check_exact(run_gemm(dev, Uploaded(c, gp.DTYPES[dt], dev), torch.float32).view, gp.gemm_reference(c))
        assert ok, (good, msg)


@pytest.mark.parametrize("B,S,T,mode", gp.QKV_CASES)
def test_qkv(dev, B, S, T, mode):
    from pi3_slam_amd import ops
    H, K = gp.QKV_H, gp.QKV_K
    case = gp.qkv(B, S, K, H, T, mode)
    M, N = case.M, 3 * H * 64
    exact, k2exact = gp.qkv_reference(case)
    A = sliced(case.A, torch.bfloat16, dev)
    W = sliced(case.W, torch.bfloat16, dev)
    qkv = torch.full((M + 3, N), NAN, device=dev, dtype=torch.bfloat16)
    qkv[M:] = gp.SENTINEL
    k2 = torch.full((B * H + 2,), NAN, device=dev)
    k2[B * H:] = gp.SENTINEL
    ln = {}
    if case.qb is not None:
        zero = torch.zeros(64, device=dev)
        ln = dict(qw=zero, qb=case.qb.to(dev), kw=zero.clone(), kb=case.kb.to(dev))
    ops.gemm_qkv(A, W, qkv[:M], M=M, H=H, bias=case.bias.to(dev), T=T, pos=case.pos.to(dev) if case.pos is not None else None,
                 cs=case.cs.to(dev) if case.cs is not None else None, qscale=case.qscale, k2max=k2[:B * H], attn_B=B,
                 attn_S=S, **ln)
    torch.cuda.synchronize()
    kernel = gp.expected_kernel(M, N, K, "bf16", "bf16", 0, qkv_H=H, k2max=True, attn_S=S)
    ok, msg = gp.check_exact(qkv[:M], exact)
    assert ok, (kernel, msg)
    assert bool((qkv[M:] == gp.SENTINEL).all()) and bool((k2[B * H:] == gp.SENTINEL).all())
    want = k2exact.float().to(dev)
    assert torch.equal(k2[:B * H], want), (kernel, "k2max [batch, head]", k2[:B * H].view(B, H).tolist(), want.view(B, H).tolist())


def _conv_id(c):
    return f"{c[0]}-B{c[1]}-{c[2]}x{c[3]}-C{c[4]}-N{c[5]}-{c[6]}-act{c[7]}" + ("-resid" if c[9] else "")


@pytest.mark.parametrize("spec", gp.CONV_CASES, ids=_conv_id)
def test_conv(dev, spec):
    from pi3_slam_amd import ops
    dt, B, H, W, C, N, out_name, act, bias, resid = spec
    dtype, out_dtype = gp.DTYPES[dt], gp.DTYPES[out_name]
    P = B * H * W
    every = torch.arange(P)

    def run(case, odt):
        img = sliced(case.img.reshape(P, C), dtype, dev)
        wgt = gp.conv_packed_weights(case).to(dtype).to(dev)
        out = Out(P + 1, N, odt, dev, every)
        rs = sliced(case.resid, torch.float32, dev, pad=4) if case.resid is not None else None
        ops.conv3x3(img, H, W, C, wgt, case.bias.to(dev) if case.bias is not None else None, out.view, resid=rs, act=case.act, B=B)
        torch.cuda.synchronize()
        exact = torch.cat((gp.conv_reference(case), torch.full((1, N), gp.SENTINEL, dtype=torch.float64)))
        ok, msg = gp.check_exact(out.view, exact)
        return ok and out.surroundings_intact(), msg

    ok, msg = run(gp.conv(B, H, W, C, N, bias=bias, resid=resid, act=act), out_dtype)
    assert ok, ("integer weights", msg)
    for tap in range(9):        # the image shifted by (dy, dx) and clamped at its own border
        for odt in (dtype, torch.float32):
            ok, msg = run(gp.conv(B, H, W, C, N, tap=tap), odt)
            assert ok, (f"one-hot tap {tap} (dy {tap // 3 - 1}, dx {tap % 3 - 1})", str(odt), msg)
