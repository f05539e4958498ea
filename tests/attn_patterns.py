"""Attention inputs whose exact answer is known, and on which ONE mishandled key or row is an O(1) error.

Gaussian q/k/v spread a softmax row over many keys: a key that is dropped, counted twice or read from the wrong row
shows only as far as some row happens to weight it, against a tolerance that has to leave room for bf16 arithmetic.  The
three patterns here make such a fault an O(1) error against an exact answer instead (all scores in the exp2 domain: q
arrives pre-scaled, pi3_attention computes exp2(q.k)):

  census    every score equals one constant c, V is a one-hot class indicator: out[b, i, h, d] = n[b, h, d] / S, the share
            of keys in class d.  Every p is the same power of two, so l = S 2^c and the accumulators n 2^c are exact in
            fp32 and the only rounding is the 16-bit store.  A key lost or counted twice moves one element by 1 / n
            relatively (n ~ S / 64).  Blind to any permutation of the keys, by construction.
  selector  q_i and k_j are +-1 codes of the key index: row i scores `match` against key pi(i) and at least `margin` >= 64
            less against every other key, so the softmax is one-hot and out[b, i, h, :] == V[b, pi(i), h, :] BIT FOR BIT.
            Every key is selected by exactly one row: a wrong key, row, head or batch index is a whole wrong V row.
            Blind to a duplicated key (the copy carries the same V row).
  peaked    the selector's codes scaled down so that |q| max|k| <= 90 (the bound of the loop without a running maximum):
            match 60 / 78, margin 12.  Expected = fp64 softmax of the same inputs.

Every generated value is exactly representable in bf16 AND IEEE half (asserted), so one builder serves both kernels'
types and the fp64 reference sees the very numbers the kernel reads.

Plain torch; runs on the CPU, and the comparators also accept device tensors.  tests/test_attn_patterns.py checks the
builders, the tolerances and that the comparators reject injected faults; tests/test_attention_structured_gpu.py runs
the patterns through every dispatch path of pi3_attention."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

D = 64
CENSUS_SCORES = (0, 48, -48)
CENSUS_MAPS = ("A", "B")
CENSUS_MAX_MIN_COUNT = 71       # a single-key fault moves an element by >= 1 / 71 = 1.4e-2 = 3.6 x the bf16 tolerance
SELECTOR_MIN_MARGIN = 64
PEAKED_SCALES = {643: (1.0, 1.0), 4131: (1.5, 1.0)}       # S -> (q scale, k scale)
PEAKED_BOUND = 90.0             # |q| max|k| of the bounded-score loop (attn64.hip)
FAULTS = ("drop_last", "dup_last", "roll_k")
# which injected faults a pattern must catch (see the blind spots above); every fault is caught by at least two patterns
CATCHES = {"census": ("drop_last", "dup_last"), "selector": ("drop_last", "roll_k"), "peaked": ("drop_last", "roll_k")}

# relative error of a round-to-nearest store is at most u / (1 + u) < u with u = 2^-8 (bf16: 8 significant bits) and
# u = 2^-11 (half: 11); the fp32 division and multiply in front of it add ~2^-23
STORE_TOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


@dataclass
class Pattern:
    kind: str
    B: int
    S: int
    H: int
    q: torch.Tensor             # [B, S, H, 64] fp32 holding 16-bit-exact values
    k: torch.Tensor
    v: torch.Tensor
    counts: Optional[torch.Tensor] = None       # census: [B, H, 64] int64, keys per class
    perm: Optional[torch.Tensor] = None         # selector / peaked: [B, H, S] int64, row i selects key perm[b, h, i]
    match: float = 0.0
    margin: float = 0.0
    qk_bound: float = 0.0       # max |q| * max |k|

    def qkv(self, dtype):
        """Packed [B * S, 3 * H * 64] in `dtype`, the layout pi3_attention reads."""
        x = torch.stack((self.q, self.k, self.v), dim=2).reshape(self.B * self.S, 3 * self.H * D)
        return x.to(dtype)


def assert_16bit_exact(*tensors):
    for t in tensors:
        assert torch.equal(t.to(torch.bfloat16).float(), t), "value not representable in bf16"
        assert torch.equal(t.to(torch.float16).float(), t), "value not representable in IEEE half"


def _bh_grid(B, H):
    b = torch.arange(B).view(B, 1, 1)
    h = torch.arange(H).view(1, 1, H)
    return b, h


def census_classes(B, S, H, cmap):
    """cls[b, j, h]: map A = (j + 7 h + 13 b) mod 64 (every tile holds every class); map B = contiguous blocks
    floor(64 j / S) (a lost tile empties a class), shifted by the same 7 h + 13 b so that heads and batches differ."""
    assert cmap in CENSUS_MAPS
    b, h = _bh_grid(B, H)
    j = torch.arange(S).view(1, S, 1)
    base = j if cmap == "A" else (64 * j) // S
    return (base + 7 * h + 13 * b) % D


def census(B, S, H, c, cmap):
    assert c in CENSUS_SCORES
    u = torch.zeros(D)
    u[:48] = 1.0
    # c = 0: q = 0 makes every score 0 whatever k holds (k = u keeps max |k|^2 non-zero for the a-priori test)
    q = (u if c != 0 else torch.zeros(D)).expand(B, S, H, D).clone()
    k = (u * (-1.0 if c < 0 else 1.0)).expand(B, S, H, D).clone()
    cls = census_classes(B, S, H, cmap)
    v = torch.nn.functional.one_hot(cls, D).float()
    counts = v.sum(dim=1).long()                 # [B, H, 64]
    assert_16bit_exact(q, k, v)
    assert float((q[0, 0, 0] * k[0, 0, 0]).sum()) == float(c)
    assert int(counts.sum(-1).min()) == S and int(counts.sum(-1).max()) == S
    nz = counts[counts > 0]
    assert int(nz.min()) <= CENSUS_MAX_MIN_COUNT, "a single key would move every element by less than 1 / 71"
    return Pattern("census", B, S, H, q, k, v, counts=counts, qk_bound=float(q[0, 0, 0].norm() * k[0, 0, 0].norm()))


def selector_codes(S):
    """[S, 64] codes: the +-1 vector of j's nb bits, repeated floor(64 / nb) times, zero padded."""
    nb = max(1, math.ceil(math.log2(S)))
    assert (1 << nb) >= S and (nb == 1 or (1 << (nb - 1)) < S)
    reps = D // nb
    j = torch.arange(S).view(S, 1)
    bits = ((j >> torch.arange(nb).view(1, nb)) & 1).float() * 2.0 - 1.0
    code = torch.zeros(S, D)
    code[:, :nb * reps] = bits.repeat(1, reps)
    return code, nb, reps


def selector(B, S, H, seed=0, q_scale=4.0, k_scale=2.0, kind="selector"):
    code, nb, reps = selector_codes(S)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * S + 31 * H + B)
    perm = torch.stack([torch.stack([torch.randperm(S, generator=g) for _ in range(H)]) for _ in range(B)])   # [B, H, S]
    q = (q_scale * code)[perm].permute(0, 2, 1, 3).contiguous()             # [B, S, H, 64]
    k = (k_scale * code).view(1, S, 1, D).expand(B, S, H, D).clone()
    # +- m / 32, m in 1 .. 127: no zeros (a bitwise comparison of a zero would see the 2^-64 leak of the other keys)
    m = torch.randint(1, 128, (B, S, H, D), generator=g).float()
    sgn = torch.randint(0, 2, (B, S, H, D), generator=g).float() * 2.0 - 1.0
    v = sgn * m / 32.0
    assert_16bit_exact(q, k, v)
    match = q_scale * k_scale * reps * nb
    margin = 2.0 * q_scale * k_scale * reps       # one flipped bit, reps copies
    qk = q_scale * k_scale * reps * nb            # |q| |k| = scale^2 * (number of non-zero entries): the codes are +-1
    p = Pattern(kind, B, S, H, q, k, v, perm=perm, match=match, margin=margin, qk_bound=qk)
    if kind == "selector":
        assert margin >= SELECTOR_MIN_MARGIN, f"S = {S}: margin {margin} < {SELECTOR_MIN_MARGIN}"
    return p


def peaked(B, S, H, seed=0):
    qs, ks = PEAKED_SCALES[S]
    p = selector(B, S, H, seed, qs, ks, kind="peaked")
    assert p.qk_bound <= PEAKED_BOUND and p.margin == 12.0
    return p


def scores_of(p, b, h, q=None, k=None):
    q = p.q if q is None else q
    k = p.k if k is None else k
    return q[b, :, h].double() @ k[b, :, h].double().T


def inject(p, fault):
    """(k, v) [B, S', H, 64] with one bookkeeping fault of the key sweep applied."""
    k, v = p.k, p.v
    if fault is None:
        return k, v
    if fault == "drop_last":
        return k[:, :-1], v[:, :-1]
    if fault == "dup_last":
        return torch.cat((k, k[:, -1:]), 1), torch.cat((v, v[:, -1:]), 1)
    if fault == "roll_k":
        return k.roll(1, dims=1), v
    raise ValueError(fault)


def softmax_ref(q, k, v, chunk=1024):
    """fp64 softmax(q k^T) v in the exp2 domain; q [B, Sq, H, 64], k / v [B, Sk, H, 64] -> [B * Sq, H * 64] float64."""
    B, Sq, H, _ = q.shape
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))        # [B, H, S, 64]
    out = torch.empty(B, H, Sq, D, dtype=torch.float64, device=q.device)
    for r0 in range(0, Sq, chunk):
        s = qd[:, :, r0:r0 + chunk] @ kd.transpose(-1, -2)
        s = s - s.amax(dim=-1, keepdim=True)
        w = torch.exp2(s)
        out[:, :, r0:r0 + chunk] = (w @ vd) / w.sum(-1, keepdim=True)
    return out.permute(0, 2, 1, 3).reshape(B * Sq, H * D)


def emulate(q, k, v, dtype, chunk=1024):
    """The kernels' arithmetic on the CPU: fp32 scores, p = exp2(s - row max) rounded to the 16-bit type, fp32 row sum
    and accumulation, fp32 divide, 16-bit store.  -> [B * Sq, H * 64] in `dtype`."""
    B, Sq, H, _ = q.shape
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    out = torch.empty(B, H, Sq, D, dtype=torch.float32)
    for r0 in range(0, Sq, chunk):
        s = qf[:, :, r0:r0 + chunk] @ kf.transpose(-1, -2)
        s = s - s.amax(dim=-1, keepdim=True)
        w = torch.exp2(s).to(dtype).float()
        out[:, :, r0:r0 + chunk] = (w @ vf) / w.sum(-1, keepdim=True)
    return out.permute(0, 2, 1, 3).reshape(B * Sq, H * D).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# expected results and comparators.  `got` is the kernel's [B * S, H * 64] output in its 16-bit type.  Each comparator
# returns (ok, worst, message): worst = the largest error in units of the tolerance (census, peaked) or the number of
# differing elements (selector).
# ---------------------------------------------------------------------------------------------------------------------
def census_expected(p, device=None):
    """[B * S, H * 64] float64: n / S on every row."""
    e = (p.counts.double() / p.S).view(p.B, 1, p.H, D).expand(p.B, p.S, p.H, D).reshape(p.B * p.S, p.H * D)
    return e.to(device) if device is not None else e


def check_census(got, p):
    tol = STORE_TOL[got.dtype]
    exp = census_expected(p, got.device)
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return False, float("inf"), "non-finite output"
    zero = exp == 0
    if bool((g[zero] != 0).any()):
        return False, float("inf"), f"{int((g[zero] != 0).sum())} elements of empty classes are not exactly 0"
    err = (g - exp).abs() / exp.clamp_min(1e-300)
    err[zero] = 0.0
    worst = float(err.max())
    i = int(err.argmax())
    return worst <= tol, worst / tol, (f"worst |got - n/S| / (n/S) = {worst:.3e} (tolerance {tol:.3e}) at row {i // exp.shape[1]} "
                                       f"column {i % exp.shape[1]}: got {float(g.flatten()[i])!r}, expected {float(exp.flatten()[i])!r}")


def selector_expected(p, dtype, device=None):
    """[B * S, H * 64] in `dtype`: V[b, perm[b, h, i], h, :]."""
    idx = p.perm.permute(0, 2, 1).unsqueeze(-1).expand(p.B, p.S, p.H, D)            # [B, S(i), H, 64] -> key index
    e = torch.gather(p.v, 1, idx).reshape(p.B * p.S, p.H * D).to(dtype)
    return e.to(device) if device is not None else e


def check_selector(got, p):
    exp = selector_expected(p, got.dtype, got.device)
    ne = got.view(torch.int16) != exp.view(torch.int16)
    n = int(ne.sum())
    if n == 0:
        return True, 0.0, "bitwise equal"
    rows = torch.nonzero(ne.any(dim=1)).flatten()
    r0 = int(rows[0])
    c0 = int(torch.nonzero(ne[r0]).flatten()[0])
    return False, float(n), (f"{n} elements in {rows.numel()} rows differ from V[perm]; first: row {r0} (batch {r0 // p.S}, token "
                             f"{r0 % p.S}) column {c0} (head {c0 // D}): got {float(got[r0, c0])!r}, expected {float(exp[r0, c0])!r}")


def peaked_tolerance(p):
    """P rounding and output rounding each contribute <= 2^-9 max|V| (8 significant bits, round to nearest); the
    tolerance is twice their sum."""
    return 2.0 ** -7 * float(p.v.abs().max())


def check_peaked(got, p, ref):
    """ref: softmax_ref(p.q, p.k, p.v) (float64, same device as got)."""
    tol = peaked_tolerance(p)
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return False, float("inf"), "non-finite output"
    err = (g - ref).abs()
    worst = float(err.max())
    i = int(err.argmax())
    return worst <= tol, worst / tol, (f"worst |got - ref| = {worst:.3e} (tolerance {tol:.3e}) at row {i // ref.shape[1]} column "
                                       f"{i % ref.shape[1]}")
