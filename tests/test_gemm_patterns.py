"""The exact-answer GEMM patterns keep their promises (tests/gemm_patterns.py): representable operands, partial sums
below 2^24, closed forms equal to the fp64 product, residues that tell every row and column of the GPU case table
apart; every comparator accepts the exact answer and rejects each injected fault that CATCHES assigns to its pattern;
and the GPU case table reaches every kernel and every template instance the three entry points dispatch to.  CPU only."""
import math

import pytest
import torch

import gemm_patterns as gp
from attn_patterns import assert_16bit_exact

SHAPES = [(5, 128, 32), (129, 384, 64), (257, 160, 192), (300, 256, 640)]


def _acc(case):
    return case.A.double() @ case.W.double().T


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_builders_keep_their_promises(M, N, K):
    t = gp.tally(M, N, K)
    assert set(t.A.unique().tolist()) <= {-1.0, 1.0} and set(t.W.unique().tolist()) <= {-1.0, 1.0}
    acc = _acc(t)
    assert torch.equal(acc, gp.tally_exact(M, N)) and float(acc.abs().max()) <= 256
    assert bool((acc[1:] != acc[:-1]).all()) and bool((acc[:, 1:] != acc[:, :-1]).all()), "neighbours share a tally"
    for pair in (0, 1):
        a = gp.address(M, N, K, pair)
        acc = _acc(a)
        assert torch.equal(acc, gp.address_exact(M, N, pair)) and float(acc.abs().max()) <= 256
        # the payload sits in every block of 32 columns, at a position that changes from block to block
        r, _ = gp.address_codes(M, N, pair)
        assert K // gp.BLK < 4 or len(set(gp.slot_positions(K // gp.BLK)[:, 0].tolist())) >= 4
        assert float(gp.assert_exact_sum(a.A, a.W)) < gp.LIMIT
    for dtype in (torch.bfloat16, torch.float16):
        c = gp.rounding(M, N, K, dtype)
        acc = _acc(c)
        assert torch.equal(acc, gp.rounding_exact(M, N, dtype))
        u = acc.abs() - gp.rounding_offset(dtype) * (1 + torch.arange(N) % 2)
        assert 257 <= float(u.min()) and float(u.max()) <= 1023
        tie = gp.is_store_tie(acc, dtype)
        assert 0.45 <= float(tie.float().mean()) <= 0.55
        # a tie is not representable, and torch's cast takes it to the even neighbour
        stored = gp.round_to(acc, dtype).double()
        assert bool((stored[tie] != acc[tie]).all())
        step = (stored[tie] - acc[tie]).abs()
        assert bool((torch.remainder(stored[tie] / (2 * step), 2) == 0).all())
        assert bool((acc < 0).any()) and bool((acc > 0).any())


def test_address_residues_tell_every_row_and_column_of_the_gpu_table_apart():
    rows = [p[0] for p in gp.ADDRESS_PAIRS]
    cols = [p[2] for p in gp.ADDRESS_PAIRS]
    assert math.gcd(*rows) == 1 and math.gcd(*cols) == 1
    assert all(math.gcd(p[1], p[2]) == 1 for p in gp.ADDRESS_PAIRS)
    shapes = [(M, N) for _, M, N, _ in gp.GEMM_SHAPES] + [(s.M, s.N) for s in gp.EPILOGUE_CASES] + \
             [(B * S, 3 * 64 * gp.QKV_H) for B, S, _, _ in gp.QKV_CASES]
    for M, N in shapes:
        assert not gp.confusable(M, rows) and not gp.confusable(N, cols), (M, N)
    # and by enumeration at the largest shape: the pair of codes is unique per row and per column
    M, N = max(s[0] for s in shapes), max(s[1] for s in shapes)
    r0, c0 = gp.address_codes(M, N, 0)
    r1, c1 = gp.address_codes(M, N, 1)
    assert len(set(zip(r0.tolist(), r1.tolist()))) == M and len(set(zip(c0.tolist(), c1.tolist()))) == N


def test_epilogue_operands_show_their_column_and_stay_exact():
    for act, qscale in ((2, 0.5), (1, 2.0), (0, 0.25)):
        c = gp.epilogue(257, 384, 128, act=act, qcols=20, qscale=qscale, **{k: v for k, v in gp.FULL.items() if k != "qscale"})
        assert_16bit_exact(c.A, c.W)
        for v in (c.bias, c.gamma):
            assert bool((v[1:] != v[:-1]).all()) and torch.equal(v, v.round())
        for v in (c.resid, c.addtab):
            assert bool((v[1:] != v[:-1]).all()) and bool((v[:, 1:] != v[:, :-1]).all()) and torch.equal(v, v.round())
        assert c.resid.shape[0] == c.out_rows and c.addtab.shape[0] == c.rpg
        pre = _acc(c) + c.bias.double()
        pre[:, :c.qcols] *= qscale
        if act == 1:
            assert torch.equal(pre, pre.round()) and bool(((pre == 0) | (pre.abs() >= 8)).all()) and bool((pre == 0).any())
        full = gp.gemm_reference(c)
        m = torch.arange(c.M)
        orow = (m // c.rpg) * c.gstride + c.goff + m % c.rpg
        untouched = torch.ones(c.out_rows, dtype=torch.bool)
        untouched[orow] = False
        assert int(untouched.sum()) > c.M // c.rpg and bool((full[untouched] == gp.SENTINEL).all())
        if act != 1:
            assert torch.equal(full.float().double(), full) and float(full.abs().max()) < gp.LIMIT


def _gemm_case(pattern):
    if pattern == "tally":
        return gp.tally(257, 384, 192)
    if pattern == "address":
        return gp.address(257, 384, 192, 1)
    if pattern == "rounding":
        return gp.rounding(257, 384, 192)
    return gp.epilogue(257, 384, 192, act=2, qcols=20, **gp.FULL)


@pytest.mark.parametrize("pattern", ["tally", "address", "rounding", "epilogue"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_gemm_comparator_accepts_the_answer_and_rejects_assigned_faults(pattern, dtype):
    case = _gemm_case(pattern) if not (pattern == "rounding" and dtype == torch.float16) else gp.rounding(257, 384, 192, dtype)
    exact = gp.gemm_reference(case)
    ok, msg = gp.check_exact(gp.round_to(exact, dtype), exact)
    assert ok, msg
    poisoned = gp.round_to(exact, dtype)
    poisoned[3, 5] = float("nan")
    assert not gp.check_exact(poisoned, exact)[0]
    for fault in gp.CATCHES[pattern]:
        wrong = gp.gemm_reference(case, fault)
        ok, msg = gp.check_exact(wrong.float().to(dtype), exact)
        assert not ok, (pattern, fault, "not caught")
        assert "row" in msg and "column" in msg


@pytest.mark.parametrize("mode", gp.QKV_MODES)
def test_qkv_pattern_and_its_faults(mode):
    case = gp.qkv(3, 129, 128, gp.QKV_H, 37, mode)
    assert_16bit_exact(case.A, case.W, case.bias)
    out, k2 = gp.qkv_reference(case)
    assert torch.equal(out, out.float().bfloat16().double()), "an expected q / k / v value is not a bf16 number"
    assert bool((out != 0).all()) and k2.shape == (3 * gp.QKV_H,)
    ok, _ = gp.check_exact(out.float().bfloat16(), out)
    assert ok
    proj = case.A.double() @ case.W.double().T + case.bias.double()
    assert float(proj.abs().max()) <= 256 and bool((proj != 0).all())
    H = gp.QKV_H
    assert torch.equal(out[:, 2 * H * 64:], proj[:, 2 * H * 64:])
    if mode == "plain":
        assert torch.equal(out[:, :H * 64], proj[:, :H * 64] * case.qscale)
        assert len(set(k2.tolist())) == k2.numel(), "two (batch, head) share a maximum"
    if mode == "ln_rope":       # q and k are the LayerNorm biases, turned: a permutation with signs of their 64 values
        q = out[:, :64] / case.qscale
        assert torch.equal(q.abs().sort(dim=1).values, case.qb.double().abs().sort().values.expand(case.M, 64))
    for fault in gp.CATCHES["qkv"]:
        if mode == "ln_rope" and fault != "swap_rows":
            continue            # bias-only LayerNorm hides the projection and makes every key row the same size
        wout, wk2 = gp.qkv_reference(case, fault)
        caught = not gp.check_exact(wout.float().bfloat16(), out)[0] or not torch.equal(wk2, k2)
        assert caught, (mode, fault)
        if fault == "k2max_next_batch":
            assert torch.equal(wout, out) and not torch.equal(wk2, k2)


def test_quarter_turn_rope_is_a_signed_permutation_with_the_oracle_pairing():
    from oracle import pi3_ref
    cs = gp.quarter_turn_table()
    assert set(map(tuple, cs.reshape(-1, 2).tolist())) == {(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)}
    g = torch.Generator().manual_seed(5)
    B, Hh, S, npos = 2, 3, 21, 6
    tok = torch.randn(B, Hh, S, 64, generator=g)
    pos = torch.randint(0, npos, (B, S, 2), generator=g)
    pos[0, 0] = npos - 1
    want = pi3_ref.rope2d(tok, pos)                 # base 100: angle = position * 100^(-f / 16)
    ang = torch.arange(npos).double().view(npos, 1) * (100.0 ** (-torch.arange(16).double() / 16)).view(1, 16)
    real = torch.stack((ang.cos(), ang.sin()), dim=-1)
    x = tok.permute(0, 2, 1, 3).reshape(B * S, Hh, 64).double()
    got = gp.rope_with_table(x, pos.reshape(B * S, 2), real).view(B, S, Hh, 64).permute(0, 2, 1, 3)
    assert float((got - want.double()).abs().max()) < 1e-5
    # the quarter-turn table: every output is +- one input of the same row and head
    turned = gp.rope_with_table(x, pos.reshape(B * S, 2) % gp.QKV_NPOS, cs)
    assert torch.equal(turned.abs().sort(dim=-1).values, x.abs().sort(dim=-1).values)


@pytest.mark.parametrize("C,N", [(32, 96), (64, 128)])
def test_conv_pattern_and_its_faults(C, N):
    case = gp.conv(2, 5, 7, C, N, bias=True, resid=True, act=2)
    exact = gp.conv_reference(case)
    plain = gp.conv(2, 5, 7, C, N)
    want = torch.nn.functional.conv2d(
        torch.nn.functional.pad(plain.img.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate"),
        plain.wgt.double().view(N, 3, 3, C).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(-1, N)
    assert torch.equal(gp.conv_reference(plain), want)
    assert gp.conv_packed_weights(case).shape == (N, 320 if C == 32 else 9 * C)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert gp.check_exact(gp.round_to(exact, dtype), exact)[0]
        for fault in gp.CATCHES["conv"]:
            assert not gp.check_exact(gp.conv_reference(case, fault).float().to(dtype), exact)[0], (fault, dtype)
    for tap in range(9):        # one-hot tap: the image shifted by (dy, dx), clamped at its own border
        one = gp.conv(2, 5, 7, C, N, tap=tap)
        dy, dx = tap // 3 - 1, tap % 3 - 1
        y = (torch.arange(5) + dy).clamp(0, 4)
        x = (torch.arange(7) + dx).clamp(0, 6)
        shifted = one.img[:, y][:, :, x].double()           # [B, H, W, C]
        n = torch.arange(N)
        g = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[(n // C) % 4]
        out = gp.conv_reference(one)
        assert torch.equal(out, shifted.reshape(-1, C)[:, n % C] * g)
        for fault in gp.CATCHES["conv"]:
            differs = not torch.equal(gp.conv_reference(one, fault), out)
            expect = {"conv_transpose_tap": dy != dx, "conv_zero_pad": tap != 4, "conv_seam": dy != 0}[fault]
            assert differs == expect, (tap, fault)


def test_every_fault_is_caught_by_some_pattern():
    caught = {f for faults in gp.CATCHES.values() for f in faults}
    assert caught == set(gp.FAULTS)


def test_gelu_comparator():
    c = gp.epilogue(129, 128, 64, act=1, qscale=2.0, qcols=20)
    exact = gp.gemm_reference(c)
    for dtype in (torch.bfloat16, torch.float16):
        ok, worst, msg = gp.check_gelu(exact.float().to(dtype), exact, 5e-4)
        assert ok and worst < 1e-12, msg         # gelu(-8) = -5e-15 stores as -0 in half
        wrong = gp.gemm_reference(c, "bias_shift")
        assert not gp.check_gelu(wrong.float().to(dtype), exact, 5e-4)[0]


def _reached():
    kernels, instances = set(), set()
    for dt, M, N, K in gp.GEMM_SHAPES:
        out16 = "bf16" if dt == "f32" else dt
        for out in (out16, "f32"):
            k = gp.expected_kernel(M, N, K, dt, out, 0)
            kernels.add(k)
            instances.add(gp.instance_of(k, dt, out, 0))
    for s in gp.EPILOGUE_CASES:
        kernels.add(s.kernel())
        instances.add(gp.instance_of(s.kernel(), s.in_dtype, s.out_dtype, s.act, gelu_form=s.gelu_form))
    for B, S, T, mode in gp.QKV_CASES:
        k = gp.expected_kernel(B * S, 3 * 64 * gp.QKV_H, gp.QKV_K, "bf16", "bf16", 0, qkv_H=gp.QKV_H, k2max=True, attn_S=S)
        kernels.add(k)
        if k == "g256_qk":
            instances.add(gp.instance_of(k, "bf16", "bf16", 0))
    for dt, B, H, W, C, N, out, act, bias, resid in gp.CONV_CASES:
        k = gp.expected_kernel(B * H * W, N, 0, dt, out, act, conv_C=C)
        kernels.add(k)
        instances.add(gp.instance_of(k, dt, out, act, conv=True))
    return kernels, instances


def test_gpu_table_reaches_every_kernel_and_every_dispatched_instance():
    kernels, instances = _reached()
    assert kernels == {"tn128", "narrow32", "narrow64", "g256", "g256_qk", "two_pass"}
    assert len(set(gp.INSTANCES)) == 22
    missing = set(gp.INSTANCES) - instances
    assert not missing, missing
    assert instances <= set(gp.INSTANCES), instances - set(gp.INSTANCES)


def test_dispatch_mirror_at_its_thresholds():
    ek = gp.expected_kernel
    assert ek(1023, 256, 64, "bf16", "bf16", 0) == "tn128" and ek(1024, 256, 64, "bf16", "bf16", 0) == "g256"
    assert ek(1024, 384, 64, "bf16", "bf16", 0) == "tn128" and ek(1024, 256, 64, "f16", "f16", 0) == "tn128"
    assert ek(1024, 256, 64, "bf16", "bf16", 0, resid=True) == "tn128" and ek(1024, 256, 64, "bf16", "f32", 0, resid=True) == "g256"
    assert ek(1024, 256, 64, "bf16", "bf16", 0, qcols=20) == "tn128" and ek(1024, 256, 64, "bf16", "bf16", 0, qcols=32) == "g256"
    assert ek(1024, 256, 64, "bf16", "f32", 2) == "tn128" and ek(1024, 256, 64, "bf16", "bf16", 2) == "tn128"
    assert ek(4096, 96, 64, "bf16", "f32", 0) == "narrow32" and ek(4096, 192, 64, "f16", "f32", 0) == "narrow64"
    assert ek(4096, 128, 32, "f32", "f32", 0) == "tn128"
    assert ek(1152, 768, 128, "bf16", "bf16", 0, qkv_H=4, k2max=True, attn_S=128) == "g256_qk"
    assert ek(1143, 768, 128, "bf16", "bf16", 0, qkv_H=4, k2max=True, attn_S=127) == "two_pass"
    assert ek(1143, 768, 128, "bf16", "bf16", 0, qkv_H=4, k2max=False, attn_S=127) == "g256_qk"
    assert ek(1000, 768, 128, "bf16", "bf16", 0, qkv_H=4) == "two_pass"
    assert ek(900, 128, 0, "bf16", "f32", 0, conv_C=64) == "tn128" and ek(900, 128, 0, "bf16", "f32", 0, conv_C=32) == "narrow64"
    assert ek(900, 96, 0, "f16", "f16", 2, conv_C=128) == "narrow32"
