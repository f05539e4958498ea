"""GEMM, qkv and 3x3-convolution operands whose exact result is known, and on which ONE mishandled k element, row, column
or epilogue index is a wrong integer.

Gaussian operands spread an output over K products: a k element that is lost or counted twice, a residual row taken
from the neighbour, a q-scale boundary one column group off move an output by a few percent of a standard deviation,
against a tolerance that has to leave room for bf16 rounding.  Every pattern here has an exact answer instead:

  * every operand value is a small integer times a power of two, exactly representable in bf16 AND IEEE half (asserted);
  * the sum over k of |a| |w| stays below 2^24 for every output (asserted), so every partial sum, in any order and with
    or without fma contraction, is an integer (times one power of two) that fp32 holds exactly: the accumulator does not
    depend on the kernel's summation order;
  * the expectation is fp64 arithmetic on the very numbers the kernel reads, rounded once by torch's own
    round-to-nearest-even cast where the output is a 16-bit type; the comparison is bit for bit.

Patterns (K is cut into blocks of 32 columns; a bf16 K step of 64 holds two blocks, an fp32 K step one):
  tally     +-1 operands, every product +-1.  Base products alternate (-1)^k; row m flips a(m) = m mod 13 of its even
            columns, column n flips c(n) = n mod 11 of its odd ones, one per block, round robin from block m // 13 (n // 11):
            out = 2 (c(n) - a(m)), |out| <= 24.  One lost or doubled k element moves every output by exactly 1.
  address   two payload columns per block, at block-dependent permuted positions: one carries a share of r(m) against 1,
            one 1 against a share of c(n); the other 30 columns are cancelling pairs (a, a) x (w, -w).  out = sgn(m)
            (r(m) + c(n)).  Two residue pairs, ADDRESS_PAIRS: rows m, m' collide under both only if m = m' mod 127 * 128,
            columns only if n = n' mod 125 * 123, beyond every shape of the GPU table (asserted).  r - c is not constant,
            so a transposed block is seen too.
  rounding  address with r + c in 257 .. 511, odd columns doubled, a third of the rows negated: |out| in 257 .. 1022 with
            half of the values ties of the bf16 store (odd below 512, = 2 mod 4 above).  Half holds these integers
            exactly, so for IEEE half a constant 1792 joins r + c: 2049 .. 2303 and, doubled, 4098 .. 4606, where half
            is as coarse as bf16 is at 257 .. 1022, with the same values odd.
  epilogue  address accumulators under integer bias / gamma / resid / addtab and a power-of-two qscale, with the row remap.
  qkv       integer q, k, v projections for pi3_gemm_qkv, a quarter-turn RoPE table, bias-only LayerNorm.
  conv      integer NHWC image with pixel and channel codes, integer or one-hot-tap weights, for pi3_conv3x3.

The references take a `fault`: one bookkeeping error applied to the reference computation.  CATCHES says which pattern
must reject which fault (tests/test_gemm_patterns.py checks it); every fault of FAULTS is caught by at least one pattern.

expected_kernel / instance_of mirror the dispatch of pi3_gemm, pi3_gemm_qkv, pi3_conv3x3, launch_narrow and
pi3_gemm256_try (csrc/gemm.hip, csrc/gemm256.hip) as they read in the product build; GEMM_SHAPES ... CONV_CASES are the
case tables of tests/test_gemm_structured_gpu.py, kept here so that the CPU tests can check what they reach.

Plain torch; runs on the CPU, and the comparators also accept device tensors."""
from dataclasses import dataclass
from typing import Optional

import torch

from attn_patterns import STORE_TOL, assert_16bit_exact

BLK = 32                        # columns per block: the K step of the fp32 kernel, half a K step of the 16-bit ones
LIMIT = float(1 << 24)          # integers below it are exact in fp32
SENTINEL = 77.0                 # prefill of everything a kernel must not write
ADDRESS_PAIRS = ((127, 7, 125), (128, 5, 123))      # (row modulus, column multiplier, column modulus)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}

FAULTS = ("drop_k", "repeat_kstep", "swap_rows", "swap_cols", "bias_shift", "qcols_shift4", "qcols_shift16", "goff_off1",
          "resid_before_remap", "conv_transpose_tap", "conv_zero_pad", "conv_seam", "k2max_next_batch")
CATCHES = {
    "tally": ("drop_k", "repeat_kstep"),
    "address": ("drop_k", "swap_rows", "swap_cols"),
    "rounding": ("drop_k", "swap_rows"),
    "epilogue": ("swap_cols", "bias_shift", "qcols_shift4", "qcols_shift16", "goff_off1", "resid_before_remap"),
    "qkv": ("drop_k", "swap_rows", "bias_shift", "k2max_next_batch"),
    "conv": ("conv_transpose_tap", "conv_zero_pad", "conv_seam"),
}


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class GemmCase:
    """One fully specified pi3_gemm problem.  A [M, K], W [N, K] fp32 holding 16-bit-exact values; epilogue operands
    fp32 or None; resid has out_rows rows (it is indexed by the remapped row), addtab max(rpg, 1) rows."""
    kind: str
    M: int
    N: int
    K: int
    A: torch.Tensor
    W: torch.Tensor
    bias: Optional[torch.Tensor] = None
    gamma: Optional[torch.Tensor] = None
    resid: Optional[torch.Tensor] = None
    addtab: Optional[torch.Tensor] = None
    qscale: float = 1.0
    qcols: int = 0
    act: int = 0                # 0 none, 1 GELU (erf), 2 ReLU
    rpg: int = 0
    gstride: int = 0
    goff: int = 0

    @property
    def out_rows(self):
        """Rows of the output buffer: the last remapped row, and one more that nothing may write."""
        if self.rpg == 0:
            return self.M + 1
        return ((self.M - 1) // self.rpg) * self.gstride + self.goff + self.rpg + 1


def assert_exact_sum(A, W):
    """sum_k |a| |w| < 2^24 for every output: every partial sum of the K loop is exact in fp32 in any order."""
    bound = float((A.double().abs() @ W.double().abs().T).max())
    assert bound < LIMIT, f"sum |a||w| = {bound} >= 2^24"
    return bound


def _split(v, nb):
    """[L] non-negative int64 -> [L, nb] shares floor((v + t) / nb), which sum to v."""
    return (v.view(-1, 1) + torch.arange(nb).view(1, nb)) // nb


def slot_positions(nb):
    """[nb, 32]: the column, inside block t, of slot j - a fixed permutation that differs from block to block."""
    return (torch.arange(BLK).view(1, BLK) * 5 + 3 * torch.arange(nb).view(nb, 1) + 1) % BLK


def payload_operands(M, N, K, r, c, rowmul, wmul=None, offset=0):
    """A [M, K], W [N, K] (fp32) with A[m] . W[n] == rowmul[m] * (r[m] + c[n] + offset) * wmul[n].  Slot 0 of every block: a
    share of r(m) against 1; slot 1: 1 against a share of c(n); slots 2 .. 31: pairs (a, a) x (w, -w) with a in 1 .. 3
    and w in 1 .. 2, which depend on the row, the column, the pair and the block.  offset (a 16-bit-exact constant):
    the first pair of block 0 becomes (1, 1) x (offset, 0)."""
    assert K % BLK == 0 and int(r.min()) >= 0 and int(c.min()) >= 0
    nb = K // BLK
    m = torch.arange(M).view(M, 1, 1)
    n = torch.arange(N).view(N, 1, 1)
    t = torch.arange(nb).view(1, nb, 1)
    i = torch.arange(15).view(1, 1, 15)
    a_s = torch.zeros(M, nb, BLK, dtype=torch.int64)
    w_s = torch.zeros(N, nb, BLK, dtype=torch.int64)
    fa = 1 + (m + i + t) % 3
    fw = (1 + (n + i) % 2).expand(N, nb, 15)
    a_s[:, :, 2::2] = fa
    a_s[:, :, 3::2] = fa
    w_s[:, :, 2::2] = fw
    w_s[:, :, 3::2] = -fw
    a_s[:, :, 0] = _split(r, nb)
    w_s[:, :, 0] = 1
    a_s[:, :, 1] = 1
    w_s[:, :, 1] = _split(c, nb)
    if offset:
        a_s[:, 0, 2:4] = 1
        w_s[:, 0, 2] = offset
        w_s[:, 0, 3] = 0
    a_s *= rowmul.view(M, 1, 1)
    if wmul is not None:
        w_s *= wmul.view(N, 1, 1)
    pos = slot_positions(nb)
    A = torch.zeros(M, nb, BLK, dtype=torch.int64).scatter_(2, pos.expand(M, nb, BLK), a_s).reshape(M, K).float()
    W = torch.zeros(N, nb, BLK, dtype=torch.int64).scatter_(2, pos.expand(N, nb, BLK), w_s).reshape(N, K).float()
    assert_16bit_exact(A, W)
    assert_exact_sum(A, W)
    return A, W


def _rowsign(M, period=3):
    m = torch.arange(M)
    return torch.where(m % period == period - 1, -1, 1)


def tally(M, N, K):
    assert K % BLK == 0
    nb = K // BLK
    m, n = torch.arange(M), torch.arange(N)
    a, c = m % 13, n % 11
    A = torch.ones(M, K)
    W = torch.ones(N, K)
    W[:, 1::2] = -1.0
    for j in range(12):         # flip j of row m: block (m // 13 + j) mod nb, even column 2 (j // nb) of it
        rows = a > j
        col = ((m // 13 + j) % nb) * BLK + 2 * (j // nb)
        A[m[rows], col[rows]] = -1.0
    for j in range(10):
        rows = c > j
        col = ((n // 11 + j) % nb) * BLK + 2 * (j // nb) + 1
        W[n[rows], col[rows]] = 1.0
    assert_16bit_exact(A, W)
    assert_exact_sum(A, W)
    assert bool((A != 0).all()) and bool((W != 0).all())
    return GemmCase("tally", M, N, K, A, W)


def tally_exact(M, N):
    return (2 * ((torch.arange(N) % 11).view(1, N) - (torch.arange(M) % 13).view(M, 1))).double()


def address_codes(M, N, pair):
    pm, mul, pn = ADDRESS_PAIRS[pair]
    return torch.arange(M) % pm, (torch.arange(N) * mul) % pn


def address(M, N, K, pair=0):
    r, c = address_codes(M, N, pair)
    A, W = payload_operands(M, N, K, r, c, _rowsign(M))
    return GemmCase("address", M, N, K, A, W)


def address_exact(M, N, pair=0):
    r, c = address_codes(M, N, pair)
    return (_rowsign(M).view(M, 1) * (r.view(M, 1) + c.view(1, N))).double()


def confusable(L, moduli):
    """True if two indices below L share their residue under every modulus (the moduli are pairwise coprime)."""
    period = 1
    for p in moduli:
        period *= p
    return L > period


def rounding_offset(dtype):
    """bf16 keeps 8 significant bits, half 11: 1792 = 7 * 256 moves 257 .. 511 to 2049 .. 2303, where half is as coarse as
    bf16 is at 257 .. 511 (and the doubled columns to 4098 .. 4606), without changing which values are odd."""
    return 1792 if dtype == torch.float16 else 0


def rounding(M, N, K, dtype=torch.bfloat16):
    m, n = torch.arange(M), torch.arange(N)
    r = 128 + m % 128
    c = 129 + (n // 2) % 128
    A, W = payload_operands(M, N, K, r, c, _rowsign(M), 1 + n % 2, rounding_offset(dtype))
    return GemmCase("rounding", M, N, K, A, W)


def rounding_exact(M, N, dtype=torch.bfloat16):
    m, n = torch.arange(M).view(M, 1), torch.arange(N).view(1, N)
    return (_rowsign(M).view(M, 1) * (257 + rounding_offset(dtype) + m % 128 + (n // 2) % 128) * (1 + n % 2)).double()


def is_store_tie(v, dtype):
    """v (fp64 integers of the rounding pattern) exactly half way between two neighbours of the 16-bit type."""
    u = v.abs().long()
    fine = 4096 if dtype == torch.float16 else 512         # below it the type's step is 2, from it on 4
    return ((u < fine) & (u % 2 == 1)) | ((u >= fine) & (u % 4 == 2))


def epilogue(M, N, K, *, pair=0, bias=True, gamma=False, resid=False, addtab=False, qscale=1.0, qcols=0, act=0, rpg=0,
             gstride=0, goff=0):
    """address accumulators + 16 (a fifth of the rows all zero) under the whole epilogue.  Every vector differs between
    neighbouring columns, resid and addtab also between neighbouring rows.  act == 1 (GELU): the bias is 8 ((n mod 3) - 1),
    so that every pre-activation is 0 or an integer multiple of qscale with |acc + bias| >= 8."""
    r, c = address_codes(M, N, pair)
    m, n = torch.arange(M), torch.arange(N)
    rowmul = _rowsign(M) * (m % 5 != 4)
    A, W = payload_operands(M, N, K, r + 16, c, rowmul)
    case = GemmCase("epilogue", M, N, K, A, W, qscale=qscale, qcols=qcols, act=act, rpg=rpg, gstride=gstride, goff=goff)
    if bias:
        case.bias = (8 * (n % 3 - 1) if act == 1 else n % 9 - 4).float()
    if gamma:
        case.gamma = torch.tensor([1, -2, 3, -1, 2, -3])[n % 6].float()
    if resid:
        o = torch.arange(case.out_rows).view(-1, 1)
        case.resid = ((o * 7 + n.view(1, N) * 3) % 101 - 50).float()
    if addtab:
        t = torch.arange(max(rpg, 1)).view(-1, 1)
        case.addtab = ((t * 5 + n.view(1, N)) % 31 - 15).float()
    assert qscale in (0.25, 0.5, 1.0, 2.0, 4.0)
    return case


def remapped_rows(case):
    """[M] int64: the output row of row m, as include/pi3slam_hip.h states it."""
    m = torch.arange(case.M)
    return (m // case.rpg) * case.gstride + case.goff + m % case.rpg if case.rpg else m


def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x * 0.7071067811865476)


def gemm_reference(case, fault=None):
    """The whole output buffer [out_rows, N] in fp64: rows that pi3_gemm does not write hold SENTINEL.  `fault`: one
    bookkeeping error of the K loop or the epilogue."""
    M, N, K = case.M, case.N, case.K
    A, W = case.A.double(), case.W.double()
    if fault == "drop_k":
        A = A.clone()
        A[:, (2 * K) // 3] = 0.0
    elif fault == "repeat_kstep":       # the second 64-column K step (32 for fp32 operands) is read from the first
        step = 64 if K >= 128 else BLK
        assert K >= 2 * step
        A, W = A.clone(), W.clone()
        A[:, step:2 * step] = A[:, :step]
        W[:, step:2 * step] = W[:, :step]
    x = A @ W.T
    if case.bias is not None:
        b = case.bias.double()
        x = x + (b.roll(1) if fault == "bias_shift" else b)
    qcols = case.qcols + {"qcols_shift4": 4, "qcols_shift16": 16}.get(fault, 0)
    x[:, :min(qcols, N)] *= case.qscale
    if case.act == 1:
        x = gelu64(x)
    elif case.act == 2:
        x = x.clamp_min(0.0)
    if case.gamma is not None:
        x = x * case.gamma.double()
    m = torch.arange(M)
    goff = case.goff + (1 if fault == "goff_off1" else 0)
    orow = (m // case.rpg) * case.gstride + goff + m % case.rpg if case.rpg else m
    trow = m % case.rpg if case.rpg else torch.zeros_like(m)
    if case.resid is not None:
        x = x + case.resid.double()[m if fault == "resid_before_remap" else orow]
    if case.addtab is not None:
        x = x + case.addtab.double()[trow]
    if fault == "swap_rows":
        x[[M // 2, M // 2 - 1]] = x[[M // 2 - 1, M // 2]]
    elif fault == "swap_cols":
        x[:, [N // 2, N // 2 + 1]] = x[:, [N // 2 + 1, N // 2]]
    full = torch.full((case.out_rows, N), SENTINEL, dtype=torch.float64)
    full[orow] = x
    return full


# ---------------------------------------------------------------------------------------------------------------------
# pi3_gemm_qkv
# ---------------------------------------------------------------------------------------------------------------------
QKV_MODES = ("plain", "rope", "ln_rope")
QKV_NPOS = 9


@dataclass
class QkvCase:
    mode: str
    M: int
    K: int
    H: int
    T: int
    attn_B: int
    attn_S: int
    A: torch.Tensor
    W: torch.Tensor
    bias: torch.Tensor
    qscale: float
    pos: Optional[torch.Tensor] = None          # int32 [T, 2] (y, x)
    cs: Optional[torch.Tensor] = None           # fp32 [npos, 16, 2] (cos, sin)
    qb: Optional[torch.Tensor] = None           # fp32 [64]; the LayerNorm weights are zero
    kb: Optional[torch.Tensor] = None


def quarter_turn_table(npos=QKV_NPOS):
    """cs[p, f] = (cos, sin) of ((2 f + 1) p + f) quarter turns: only (1, 0), (0, 1), (-1, 0), (0, -1)."""
    p = torch.arange(npos).view(npos, 1)
    f = torch.arange(16).view(1, 16)
    q = ((2 * f + 1) * p + f) % 4
    turns = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    return turns[q].contiguous()


def rope_with_table(x, pos_rows, cs):
    """RoPE-2D with a caller-owned table, the pairing of oracle/pi3_ref.rope2d (tests/test_gemm_patterns.py checks it
    against that function): dims f and f + 16 (f < 16) turn by the y position, 32 + f and 48 + f by the x position,
    (u, v) -> (u cos - v sin, v cos + u sin).  x [M, H, 64] fp64, pos_rows [M, 2] int64, cs [npos, 16, 2]."""
    cs = cs.double()

    def rot(u, v, t):
        co, si = t[:, None, :, 0], t[:, None, :, 1]
        return u * co - v * si, v * co + u * si

    y0, y1 = rot(x[..., 0:16], x[..., 16:32], cs[pos_rows[:, 0]])
    x0, x1 = rot(x[..., 32:48], x[..., 48:64], cs[pos_rows[:, 1]])
    return torch.cat((y0, y1, x0, x1), dim=-1)


def qkv_peak(b):
    return 30 + 10 * ((2 * b) % 3)


def qkv(attn_B, attn_S, K, H, T, mode, qscale=0.25):
    """Projections sgn(m) (r(m) + c(n)) + bias(n), non-zero integers of at most 154.  r is 6 .. 10 inside a batch,
    peak(b) = 30, 50, 40, 30 ... on its last row and peak(b) - 3 on its first: a key row credited to the neighbouring
    batch changes a maximum."""
    assert mode in QKV_MODES and attn_S >= 2
    M, N = attn_B * attn_S, 3 * H * 64
    m, n = torch.arange(M), torch.arange(N)
    s, b = m % attn_S, m // attn_S
    r = 6 + s % 5
    r = torch.where(s == attn_S - 1, qkv_peak(b), r)
    r = torch.where(s == 0, qkv_peak(b) - 3, r)
    c = (n * 7) % 101
    A, W = payload_operands(M, N, K, r, c, _rowsign(M, 4))
    case = QkvCase(mode, M, K, H, T, attn_B, attn_S, A, W, (n % 9 - 4).float(), qscale)
    if mode != "plain":
        t = torch.arange(T)
        case.pos = torch.stack(((t * 3) % 7, (t * 5) % QKV_NPOS), dim=1).int().contiguous()
        case.cs = quarter_turn_table()
    if mode == "ln_rope":
        d = torch.arange(64)
        case.qb = ((d * 3) % 11 + 1).float()
        case.kb = (-((d * 5) % 13) - 1).float()
    return case


def qkv_reference(case, fault=None):
    """(qkv [M, 3 H 64], k2max [attn_B * H]) in fp64."""
    M, H, S, B = case.M, case.H, case.attn_S, case.attn_B
    A = case.A.double()
    if fault == "drop_k":
        A = A.clone()
        A[:, (2 * case.K) // 3] = 0.0
    bias = case.bias.double()
    x = (A @ case.W.double().T + (bias.roll(1) if fault == "bias_shift" else bias)).view(M, 3, H, 64)
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    if case.qb is not None:     # LayerNorm with zero weights: the bias, whatever the row holds
        q = case.qb.double().expand(M, H, 64)
        k = case.kb.double().expand(M, H, 64)
    if case.pos is not None:
        pr = case.pos.long()[torch.arange(M) % case.T]
        q, k = rope_with_table(q, pr, case.cs), rope_with_table(k, pr, case.cs)
    q = q * case.qscale
    out = torch.stack((q, k, v), dim=1).reshape(M, 3 * H * 64)
    if fault == "swap_rows":
        out[[M // 2, M // 2 - 1]] = out[[M // 2 - 1, M // 2]]
    k2 = (k * k).sum(-1)                            # [M, H]
    if fault == "k2max_next_batch":                 # the last row of a batch is credited to the next one
        batch = ((torch.arange(M) + 1) // S).clamp_max(B - 1)
        k2max = torch.stack([k2[batch == bb].amax(dim=0) for bb in range(B)])
    else:
        k2max = k2.view(B, S, H).amax(dim=1)
    assert float(k2max.max()) < LIMIT
    return out, k2max.reshape(B * H)


# ---------------------------------------------------------------------------------------------------------------------
# pi3_conv3x3
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ConvCase:
    B: int
    H: int
    W: int
    C: int
    N: int
    img: torch.Tensor           # [B, H, W, C] fp32
    wgt: torch.Tensor           # [N, 9, C] fp32, tap = (dy + 1) * 3 + (dx + 1)
    bias: Optional[torch.Tensor] = None
    resid: Optional[torch.Tensor] = None        # [B H W, N]
    act: int = 0


def conv_image(B, H, W, C):
    """img[b, y, x, ci] = +- (pixel code + 29 * channel code): pixel code (3 x + 7 y + 11 b) mod 29, channel code ci mod 8,
    negative where (ci // 8) is odd; |value| <= 231."""
    b = torch.arange(B).view(B, 1, 1, 1)
    y = torch.arange(H).view(1, H, 1, 1)
    x = torch.arange(W).view(1, 1, W, 1)
    ci = torch.arange(C).view(1, 1, 1, C)
    val = (3 * x + 7 * y + 11 * b) % 29 + 29 * (ci % 8)
    img = (val * (1 - 2 * ((ci // 8) % 2))).float()
    assert_16bit_exact(img)
    return img


def conv_weights(N, C, tap=None):
    """tap None: integers ((5 n + 3 tap + ci) mod 7) - 3.  tap 0 .. 8: one-hot - output channel n reads input channel
    n mod C of that tap alone, times (1, -1, 2, -2)[(n // C) mod 4], so the output is the shifted image."""
    n = torch.arange(N).view(N, 1, 1)
    tp = torch.arange(9).view(1, 9, 1)
    ci = torch.arange(C).view(1, 1, C)
    if tap is None:
        w = (5 * n + 3 * tp + ci) % 7 - 3
    else:
        g = torch.tensor([1, -1, 2, -2])[(n // C) % 4]
        w = g * ((tp == tap) & (ci == n % C))
    w = w.float()
    assert_16bit_exact(w)
    return w


def conv(B, H, W, C, N, tap=None, bias=False, resid=False, act=0):
    case = ConvCase(B, H, W, C, N, conv_image(B, H, W, C), conv_weights(N, C, tap), act=act)
    n = torch.arange(N)
    if bias:
        case.bias = (n % 9 - 4).float()
    if resid:
        case.resid = ((torch.arange(B * H * W).view(-1, 1) * 7 + n.view(1, N) * 3) % 101 - 50).float()
    assert 9 * C * float(case.img.abs().max()) * float(case.wgt.abs().max()) < LIMIT
    return case


def conv_packed_weights(case):
    """The layout pi3_conv3x3 reads: [N, 9 C], or for C == 32 [N, 10 * 32] with a tenth tap of zeros."""
    w = case.wgt.reshape(case.N, 9 * case.C)
    if case.C == 32:
        w = torch.cat((w, torch.zeros(case.N, 32)), dim=1)
    return w.contiguous()


def conv_reference(case, fault=None):
    """[B H W, N] fp64: the convolution with replicate padding, each image clamped at its own border."""
    B, H, W, C, N = case.B, case.H, case.W, case.C, case.N
    img = case.img.double()
    tall = img.reshape(B * H, W, C)
    b = torch.arange(B).view(B, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    out = torch.zeros(B * H * W, N, dtype=torch.float64)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if fault == "conv_transpose_tap":
            dy, dx = dx, dy
        yy, xx = y + dy, x + dx
        inside = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).expand(B, H, W)
        xx = xx.clamp(0, W - 1)
        if fault == "conv_seam":        # the rows of all images as one tall image
            src = tall[(b * H + yy).clamp(0, B * H - 1), xx]
        else:
            src = img[b, yy.clamp(0, H - 1), xx]
        if fault == "conv_zero_pad":
            src = src * inside.unsqueeze(-1)
        out += src.reshape(B * H * W, C) @ case.wgt[:, tap].double().T
    if case.bias is not None:
        out = out + case.bias.double()
    if case.act == 2:
        out = out.clamp_min(0.0)
    if case.resid is not None:
        out = out + case.resid.double()
    assert float(out.abs().max()) < LIMIT
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparators: (ok, message).  `got` is what the kernel left in the buffer, `exact` the fp64 expectation of the same
# shape (SENTINEL where nothing may be written).
# ---------------------------------------------------------------------------------------------------------------------
def round_to(exact, dtype):
    """torch's round-to-nearest-even cast of the exact value (fp64 -> fp32 is exact for these integers)."""
    f = exact.float()
    assert torch.equal(f.double(), exact), "expectation not exact in fp32"
    return f.to(dtype)


def check_exact(got, exact):
    exp = round_to(exact, got.dtype).to(got.device)
    if got.shape == exp.shape and torch.equal(got, exp):
        return True, "bitwise equal"
    assert got.shape == exp.shape, (got.shape, exp.shape)
    ne = ~(got == exp)          # NaN counts as different
    rows = torch.nonzero(ne.any(dim=1)).flatten()
    r0 = int(rows[0])
    c0 = int(torch.nonzero(ne[r0]).flatten()[0])
    return False, (f"{int(ne.sum())} elements in {rows.numel()} rows differ; first: row {r0} column {c0}: got "
                   f"{float(got[r0, c0])!r}, expected {float(exp[r0, c0])!r}")


def check_gelu(got, exact, abs_tol):
    """|got - exact| <= abs_tol + STORE_TOL |exact| (fp64 erf-GELU; one rounding of the 16-bit store); rows that hold
    SENTINEL in `exact` are compared exactly by the caller."""
    g, e = got.double(), exact.to(got.device)
    if not bool(torch.isfinite(g).all()):
        return False, float("inf"), "non-finite output"
    err = (g - e).abs() - STORE_TOL[got.dtype] * e.abs()
    worst = float(err.max())
    i = int(err.argmax())
    return worst <= abs_tol, worst, (f"worst |got - gelu| - store rounding = {worst:.3e} (bound {abs_tol:.1e}) at row "
                                     f"{i // e.shape[1]} column {i % e.shape[1]}: got {float(g.flatten()[i])!r}, exact "
                                     f"{float(e.flatten()[i])!r}")


# ---------------------------------------------------------------------------------------------------------------------
# dispatch mirror (csrc/gemm.hip, csrc/gemm256.hip, product build)
# ---------------------------------------------------------------------------------------------------------------------
def _g256_applies(M, N, K, out16, act, *, resid, addtab, qcols, lda=None, ldw=None):
    lda = K if lda is None else lda
    ldw = K if ldw is None else ldw
    if N % 256 or K % 64 or M < 1024:
        return False
    if qcols % 16:
        return False
    if out16 and (resid or addtab):
        return False
    if M * lda * 2 >= (1 << 32) or N * ldw * 2 >= (1 << 32):
        return False
    return (out16 and act in (0, 1)) or (not out16 and act == 0)


def expected_kernel(M, N, K, in_dtype, out_dtype, act, *, resid=False, addtab=False, gamma=False, rpg=0, qcols=0,
                    qkv_H=0, k2max=False, attn_S=0, conv_C=0):
    """The kernel that serves the call: "tn128", "narrow32", "narrow64", "g256", "g256_qk" or "two_pass" (pi3_gemm_qkv
    only: the plain projection followed by the stand-alone q/k passes).  conv_C > 0: pi3_conv3x3 (K is ignored);
    qkv_H > 0: pi3_gemm_qkv (N = 3 * 64 * qkv_H); else pi3_gemm.  Dtypes "bf16" / "f16" / "f32"."""
    out16 = out_dtype != "f32"
    if conv_C:
        if N % 128 or conv_C == 32:
            return "narrow64" if N % 64 == 0 else "narrow32"
        return "tn128"
    if qkv_H:
        assert N == 3 * 64 * qkv_H and in_dtype == "bf16" and out_dtype == "bf16" and act == 0
        fused = _g256_applies(M, N, K, True, 0, resid=False, addtab=False, qcols=0) and not (k2max and attn_S < 128)
        return "g256_qk" if fused else "two_pass"
    if in_dtype != "f32" and N % 128 and N % 32 == 0:
        return "narrow64" if N % 64 == 0 else "narrow32"
    if in_dtype == "bf16" and _g256_applies(M, N, K, out16, act, resid=resid, addtab=addtab, qcols=qcols):
        return "g256"
    return "tn128"


# every (kernel, 16-bit operands, 16-bit output, act) template instance the three entry points dispatch to in the product
# build: the pair lists of csrc/gemm.hip (Linear16Pairs and LinearF32Pairs for launch_gemm, Linear16Pairs for launch_narrow
# from pi3_gemm, ConvPairs for both families from pi3_conv3x3, "conv" appended) and the five launch256 instances at the end
# of pi3_gemm256_try (G256Pairs; act 3 = GELU under the knob gelu_form = 1; "qk" = the fused epilogue)
INSTANCES = (
    ("tn128", True, True, 0), ("tn128", True, True, 1), ("tn128", True, False, 0), ("tn128", True, False, 2),
    ("tn128", False, False, 0), ("tn128", False, False, 2), ("tn128", False, True, 0),
    ("narrow", True, True, 0), ("narrow", True, True, 1), ("narrow", True, False, 0), ("narrow", True, False, 2),
    ("narrow_conv", True, True, 0), ("narrow_conv", True, False, 0), ("narrow_conv", True, True, 2),
    ("tn128_conv", True, True, 0), ("tn128_conv", True, False, 0), ("tn128_conv", True, True, 2),
    ("g256", True, True, 0), ("g256", True, True, 1), ("g256", True, True, 3), ("g256", True, False, 0),
    ("g256_qk", True, True, 0),
)


def instance_of(kernel, in_dtype, out_dtype, act, *, conv=False, gelu_form=0):
    if kernel == "g256" and act == 1 and gelu_form == 1:
        act = 3
    family = kernel[:6] if kernel.startswith("narrow") else kernel
    return (family + ("_conv" if conv else ""), in_dtype != "f32", out_dtype != "f32", act)


# ---------------------------------------------------------------------------------------------------------------------
# the case tables of tests/test_gemm_structured_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
# (in_dtype, M, N, K): every pattern, plain epilogue, the operands' 16-bit type (bf16 for fp32 operands) and fp32 output
GEMM_SHAPES = (
    [(dt, M, N, K) for dt in ("bf16", "f16") for M in (1, 127, 128, 129, 257) for N in (128, 384) for K in (64, 128, 192, 640)]
    + [("f32", M, N, K) for M in (1, 127, 128, 129, 257) for N in (128, 384) for K in (32, 64, 96)]
    + [(dt, M, N, K) for dt in ("bf16", "f16") for M in (1, 255, 256, 257, 513) for N in (32, 64, 96, 160) for K in (64, 192)]
    + [("bf16", M, N, K) for M in (1024, 1025, 1151, 1153, 1281) for N in (256, 512, 1280) for K in (64, 128, 192)]
    + [("bf16", 1025, 256, 1024), ("bf16", 1153, 512, 1024), ("bf16", 1281, 1280, 1024)]
    + [("bf16", 4352, 4096, 64)]        # 17 x 16 = 272 tiles: more than compute units, a workgroup walks several
)

REMAP = dict(rpg=37, gstride=45, goff=3)        # 37 divides neither 128 nor 256; rows 40 .. 44 of a group stay untouched


@dataclass(frozen=True)
class EpiSpec:
    """One epilogue case: shape, types, activation and the keyword arguments of gemm_patterns.epilogue."""
    name: str
    in_dtype: str
    out_dtype: str
    M: int
    N: int
    K: int
    act: int = 0
    gelu_form: int = 0
    kw: tuple = ()              # sorted (key, value) pairs

    def kwargs(self):
        return dict(self.kw)

    def kernel(self):
        k = self.kwargs()
        return expected_kernel(self.M, self.N, self.K, self.in_dtype, self.out_dtype, self.act, resid=k.get("resid", False),
                               addtab=k.get("addtab", False), gamma=k.get("gamma", False), rpg=k.get("rpg", 0),
                               qcols=k.get("qcols", 0))


def _epi(name, in_dtype, out_dtype, M, N, K, act=0, gelu_form=0, **kw):
    return EpiSpec(name, in_dtype, out_dtype, M, N, K, act, gelu_form, tuple(sorted(kw.items())))


FULL = dict(gamma=True, resid=True, addtab=True, qscale=0.5, **REMAP)


def _epilogue_cases():
    cases = []
    # ---- 128x128 kernel: M = 257 is three row panels, N = 384 three column tiles
    for dt in ("bf16", "f16"):
        for qc in (4, 20, 380, 384):
            cases.append(_epi(f"tn128-{dt}-f32-relu-full-q{qc}", dt, "f32", 257, 384, 128, act=2, qcols=qc, **FULL))
        cases.append(_epi(f"tn128-{dt}-f32-full", dt, "f32", 257, 384, 128, qcols=20, **FULL))
        cases.append(_epi(f"tn128-{dt}-16-resid", dt, dt, 257, 384, 128, gamma=True, resid=True, qscale=0.5, qcols=4))
        cases.append(_epi(f"tn128-{dt}-16-gelu", dt, dt, 257, 384, 128, act=1, qscale=2.0, qcols=20))
    cases.append(_epi("tn128-f32-f32-relu-full", "f32", "f32", 257, 384, 96, act=2, qcols=20, **FULL))
    cases.append(_epi("tn128-f32-f32-full", "f32", "f32", 257, 384, 96, qcols=380, **FULL))
    cases.append(_epi("tn128-f32-bf16-resid", "f32", "bf16", 257, 384, 96, gamma=True, resid=True, qscale=0.5, qcols=4))
    # ---- narrow kernel: N = 96 (32-column tiles) and 160 (32), 64 (64-column tiles); its four instances
    for dt in ("bf16", "f16"):
        for N in (64, 96, 160):
            for qc in (4, 20, N - 4, N):
                cases.append(_epi(f"narrow-{dt}-f32-relu-full-N{N}-q{qc}", dt, "f32", 513, N, 192, act=2, qcols=qc, **FULL))
            cases.append(_epi(f"narrow-{dt}-f32-full-N{N}", dt, "f32", 513, N, 192, qcols=20, **FULL))
            cases.append(_epi(f"narrow-{dt}-16-resid-N{N}", dt, dt, 513, N, 192, gamma=True, resid=True, qscale=0.5, qcols=4))
            cases.append(_epi(f"narrow-{dt}-16-gelu-N{N}", dt, dt, 513, N, 192, act=1, qscale=2.0, qcols=20))
    # ---- 256x256 kernel: M = 1153 is five row panels (the last of 129 rows), N = 512
    g = dict(in_dtype="bf16", M=1153, N=512, K=128)
    cases.append(_epi("g256-bf16-plain", out_dtype="bf16", gamma=True, qscale=0.5, qcols=16, **g))
    cases.append(_epi("g256-bf16-plain-q496", out_dtype="bf16", gamma=True, qscale=0.5, qcols=496, **g))
    cases.append(_epi("g256-bf16-gelu-form0", out_dtype="bf16", act=1, gelu_form=0, qscale=2.0, qcols=32, **g))
    cases.append(_epi("g256-bf16-gelu-form1", out_dtype="bf16", act=1, gelu_form=1, qscale=2.0, qcols=32, **g))
    cases.append(_epi("g256-f32-gamma-resid", out_dtype="f32", gamma=True, resid=True, qscale=0.5, qcols=16, **g))
    cases.append(_epi("g256-f32-remap-addtab", out_dtype="f32", addtab=True, qscale=0.5, qcols=512, **REMAP, **g))
    cases.append(_epi("g256-f32-full", out_dtype="f32", qcols=48, **FULL, **g))
    # the two decline cases: the 128x128 kernel must give the same exact answer
    cases.append(_epi("decline-bf16-resid", out_dtype="bf16", gamma=True, resid=True, qscale=0.5, qcols=16, **g))
    cases.append(_epi("decline-qcols20", out_dtype="bf16", gamma=True, qscale=0.5, qcols=20, **g))
    cases.append(_epi("decline-f32-relu", out_dtype="f32", act=2, qcols=16, **FULL, **g))
    return cases


EPILOGUE_CASES = _epilogue_cases()

# (attn_B, attn_S, T): H = 4 (N = 768 = 3 column tiles of 256), K = 128.  Fused form: M just above 1024, batch seams inside
# a 256-row tile and inside a wave's 128 rows (129, 400) or on them (128); T = 50 and 37 wrap inside a tile.
QKV_H, QKV_K = 4, 128
QKV_SHAPES = ((9, 128, 50), (8, 129, 37), (3, 400, 50),       # fused
              (3, 129, 37),                                    # M = 387 < 1024: two-pass
              (11, 100, 50))                                   # M = 1100, attn_S < 128: two-pass (with k2max)
QKV_CASES = [(B, S, T, mode) for B, S, T in QKV_SHAPES for mode in QKV_MODES]

# (dtype, B, H, W, C, N, out_dtype, act, bias, resid); every one also runs the nine one-hot tap sets
CONV_CASES = (
    [("bf16", 1, h, w, 64, 32, "f32", 0, True, False) for h, w in ((1, 1), (3, 3), (1, 300), (300, 1))]
    + [("f16", 1, h, w, 32, 96, "f16", 0, True, False) for h, w in ((1, 1), (3, 3), (1, 300), (300, 1))]
    + [(dt, 2, 19, 23, C, N, out if out == "f32" else dt, act, True, resid)
       for dt in ("bf16", "f16") for C in (32, 64, 128) for N in (32, 96, 128)
       for out, act, resid in (("f32", 0, True), ("16", 0, False), ("16", 2, True))]
)
