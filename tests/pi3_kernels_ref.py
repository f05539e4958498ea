"""fp64 references of the Pi3 row and head kernels (csrc/elem.hip, csrc/heads.hip), written out from the kernels'
documented contracts and taking the fp32 (or bf16) inputs the kernel gets.  Each returns, next to the value, the
per-element error bound of the kernel's fp32 arithmetic: k U (sum of the magnitudes entering the element), k counted
from the roundings in the kernel source, U = 2^-24.  tests/test_pi3_kernels_ref.py pins every function to torch's own
operator; tests/test_pi3_kernels_gpu.py holds the kernels to these values and bounds.

Library functions: the ulp figures HIP's math documentation states for rsqrtf / expf could not be consulted when these
tests were written, so each is allowed 2 ulp (one ulp of a binary32 result is a relative 2^-23 = 2 U at most).  sqrtf and the division are
correctly rounded (hipcc's default), one rounding each.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
ULP32 = 2.0 * U                     # largest relative size of one binary32 ulp
RSQRT_ULPS = 2
EXP_ULPS = 2
SLACK = 1.0 + 2.0 ** -10            # covers the second-order terms (products of two relative errors, each < 2^-10)


# ------------------------------------------------------------------------------------------------------- formats
def ulp16(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` (bfloat16 or float16) numbers around the fp64 values `ref` (subnormal spacing below the
    smallest normal)."""
    emin, p = (-126, 7) if dtype == torch.bfloat16 else (-14, 10)
    _, e = torch.frexp(ref.abs().double())                      # |ref| = m 2^e, m in [0.5, 1)
    fl = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (fl - p).double())


def cast_ref(x: torch.Tensor, cols: int, in_cols: int, dtype: torch.dtype) -> torch.Tensor:
    """out[r, :in_cols] = round-to-nearest-even(x[r, :in_cols]), out[r, in_cols:cols] = +0.  bf16 by integer arithmetic
    on the fp32 bits (NaN -> a quiet NaN), half through numpy's IEEE conversion, fp32 a copy."""
    x = x[:, :in_cols].contiguous()
    out = torch.zeros(x.shape[0], cols, dtype=dtype)
    if dtype == torch.float32:
        out[:, :in_cols] = x
    elif dtype == torch.bfloat16:
        b = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
        r = torch.where(torch.isnan(x), torch.full_like(r, 0x7FC0), r)
        r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
        out[:, :in_cols] = r.view(torch.bfloat16)
    else:
        with np.errstate(over="ignore"):
            out[:, :in_cols] = torch.from_numpy(x.numpy().astype(np.float16))
    return out


# ----------------------------------------------------------------------------------------------------- layernorm
def _ln_core(x, w, b, eps, k_mean, k_var):
    """LayerNorm rows in fp64 + the bound of the two-pass fp32 form  y = ((x - m) rstd) w + b:
      m^ = m + dm,           |dm| <= k_mean U mean|x|              (k_mean roundings touch a term of the sum, the division included)
      d^ = fl(x - m^) = (d - dm)(1 + e),  sum d = 0  =>  sum (d - dm)^2 = sum d^2 + D dm^2   (no first-order term)
      V^ = fl(sum d^^2 / D + eps) = (var + eps)(1 + rv),   |rv| <= (k_var + 2) U + dm^2 / (var + eps)
      rstd^ = rsqrtf(V^):    relative error rr <= rv / 2 (1 + rv) + RSQRT_ULPS ulp
      y^: three more roundings on the product (d^ rounding, two multiplies), one on the sum (a contraction only removes one):
      |y^ - y| <= |w| rstd (|d| (rr + 3 U) + dm) + U (|d rstd w| + |b|), times SLACK for the second-order terms."""
    x, w, b = x.double(), w.double(), b.double()
    eps = float(np.float32(eps))
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    V = var + eps
    r = V.rsqrt()
    t = d * r * w
    y = t + b
    dm = k_mean * U * x.abs().mean(-1, keepdim=True)
    rv = (k_var + 2) * U + dm * dm / V
    assert float(rv.max()) < 2.0 ** -10, "second-order terms would not fit SLACK"
    rr = 0.5 * rv * (1 + rv) + RSQRT_ULPS * ULP32
    bound = SLACK * (w.abs() * r * (d.abs() * (rr + 3 * U) + dm) + U * (t.abs() + b.abs()))
    return y, bound


def layernorm_vpl(D: int) -> int:
    """Vectors per lane of the kernel instance pi3_layernorm picks for width D."""
    vpl = (D // 4 + 63) // 64
    return 1 if vpl <= 1 else 2 if vpl <= 2 else 4 if vpl <= 4 else 8


def layernorm_ref(x, w, b, eps=1e-6):
    """x [rows, D] fp32 -> (y, bound) fp64.  A lane sums VPL float4s: two roundings inside a float4's pair sum, VPL
    sequential adds, six wave-reduction levels, the division by D: k_mean = VPL + 9.  The variance adds the square's
    rounding and the + eps: k_var = VPL + 11."""
    vpl = layernorm_vpl(x.shape[-1])
    return _ln_core(x, w, b, eps, vpl + 9, vpl + 11)


# ----------------------------------------------------------------------------------------------------- patch_gather
def patch_rows(t: torch.Tensor) -> torch.Tensor:
    """[F, C, H, W] -> [F * P, C * 196]: row f*P + py*pw + px, column c*196 + ky*14 + kx = t[f, c, py*14 + ky, px*14 + kx]."""
    F, C, H, W = t.shape
    ph, pw = H // 14, W // 14
    return t.view(F, C, ph, 14, pw, 14).permute(0, 2, 4, 1, 3, 5).reshape(F * ph * pw, C * 196)


def patch_gather_ref(img, mean, std, KP, dtype):
    """((img - mean) * (float32(1) / float32(std))) in fp32 - a subtraction, then a product: nothing to contract, so the
    value is the kernel's bit for bit - gathered into patch rows, cast, columns [588, KP) zero.  -> (out, fp32 rows)."""
    m = torch.tensor([np.float32(v) for v in mean], dtype=torch.float32).view(1, 3, 1, 1)
    istd = torch.tensor([np.float32(1.0) / np.float32(v) for v in std], dtype=torch.float32).view(1, 3, 1, 1)
    rows = patch_rows(((img - m) * istd).contiguous())
    return cast_ref(rows, KP, 588, dtype), rows


# ---------------------------------------------------------------------------------------------------- resample_grid
def resample_ref(src, wy, wx):
    """dst[y, x, d] = sum_ij wy[y, i] wx[x, j] src[i, j, d] in fp64.  The kernel skips zero taps; a term passes through
    its product's rounding, at most nzx(x) row additions, the multiplication by wy and at most nzy(y) additions:
    k = nzy(y) + nzx(x) + 2.  -> (dst, bound)."""
    s, a, b = src.double(), wy.double(), wx.double()
    dst = torch.einsum("yi,ijd,xj->yxd", a, s, b)
    mag = torch.einsum("yi,ijd,xj->yxd", a.abs(), s.abs(), b.abs())
    k = (a != 0).sum(1).view(-1, 1, 1) + (b != 0).sum(1).view(1, -1, 1) + 2
    return dst, k.double() * U * mag


# ------------------------------------------------------------------------------------------------------ qknorm_rope
def rope_table(npos: int, base: float = 100.0) -> torch.Tensor:
    """The engine's fp32 table [npos][16][2] = (cos, sin)(pos * base^(-j/16)), built as RoPE2D builds its own."""
    inv = 1.0 / (base ** (torch.arange(0, 32, 2).float() / 32))
    ang = torch.arange(npos).float()[:, None] * inv[None]
    return torch.stack([ang.cos(), ang.sin()], -1).contiguous()


def qknorm_rope_ref(qkv, rows, H, T, pos, cs, qw, qb, kw, kb, eps, qscale, do_rope):
    """qkv [>= rows, 3 H 64] bf16 -> (out fp64 [rows, 3, H, 64], fp32 bound of the same shape; v: the input, bound 0).
    Norm: 8 sequential adds and 3 shuffle levels (the 1/64 is exact): k_mean = 11; + the square and + eps: k_var = 13.
    RoPE  x' = x c + sgn p s  from the given fp32 table: the errors of x and of its partner p pass through |c| and |s|,
    two products and a sum round: 2 U (|x c| + |p s|).  q * qscale: one rounding."""
    x = qkv[:rows].float().double().view(rows, 3, H, 64)
    out = x.clone()
    bound = torch.zeros_like(out)
    for part, (nw, nb) in enumerate(((qw, qb), (kw, kb))):
        v, e = x[:, part], torch.zeros(rows, H, 64, dtype=torch.float64)
        if nw is not None:
            v, e = _ln_core(v, nw, nb, eps, 11, 13)
        if do_rope:
            t = torch.arange(rows) % T
            c = torch.empty(rows, 64, dtype=torch.float64)
            s = torch.empty(rows, 64, dtype=torch.float64)
            for half in range(2):                                    # dims 0..31 use y, 32..63 use x
                tab = cs.double()[pos[t, half].long()]               # [rows, 16, 2]
                c[:, 32 * half: 32 * half + 32] = torch.cat([tab[..., 0], tab[..., 0]], -1)
                s[:, 32 * half: 32 * half + 32] = torch.cat([tab[..., 1], tab[..., 1]], -1)
            c, s = c[:, None, :], s[:, None, :]

            def partner(a, sign):
                a = a.view(rows, H, 2, 2, 16)                        # [half][low / high 16][j]
                lo, hi = a[..., 0, :], a[..., 1, :]
                return torch.stack([sign * hi, lo], -2).reshape(rows, H, 64)
            xc, ps = v * c, partner(v, -1.0) * s
            e = SLACK * (c.abs() * e + s.abs() * partner(e, 1.0) + 2 * U * (xc.abs() + ps.abs()))
            v = xc + ps
        sc = float(np.float32(qscale)) if part == 0 else 1.0
        out[:, part] = v * sc
        bound[:, part] = SLACK * (abs(sc) * e + (U * (v * sc).abs() if part == 0 else 0.0))
    return out, bound


# ------------------------------------------------------------------------------------------------ unpatchify_points
def pixel_gather(feat, ld_cols, F, H, W, T, tok_off):
    """feat [F * T, >= ld_cols] -> [F, H, W, ld_cols / 196]:  out[f, y, x, c] = feat[f T + tok_off + (y / 14) pw + x / 14]
    [c 196 + (y % 14) 14 + x % 14]."""
    ph, pw = H // 14, W // 14
    C = ld_cols // 196
    v = feat.reshape(F, T, -1)[:, tok_off: tok_off + ph * pw, :ld_cols]
    return v.reshape(F, ph, pw, C, 14, 14).permute(0, 1, 4, 2, 5, 3).reshape(F, H, W, C)


def unpatchify_ref(pfeat, cfeat, F, H, W, T, tok_off):
    """-> local fp64 [F, H, W, 3] = (x z, y z, z = exp(z)), its bound (expf: EXP_ULPS ulp; x z, y z one more rounding),
    conf fp32 [F, H, W, 1] (a gather: exact)."""
    p = pixel_gather(pfeat, 588, F, H, W, T, tok_off).double()
    z = p[..., 2:].exp()
    local = torch.cat([p[..., :2] * z, z], -1)
    bz = EXP_ULPS * ULP32 * z
    bound = SLACK * torch.cat([(EXP_ULPS * ULP32 + U) * (p[..., :2] * z).abs(), bz], -1)
    return local, bound, pixel_gather(cfeat, 196, F, H, W, T, tok_off)


def world_ref(local, poses):
    """points = pose[:3] . [local, 1] in fp64 from the fp32 local points, and 4 U (|t0 lx| + |t1 ly| + |t2 z| + |t3|):
    two additions and the last one round every term at most four times with its product."""
    l, t = local.double(), poses.double()[:, :3]
    hom = torch.cat([l, torch.ones_like(l[..., :1])], -1)
    pts = torch.einsum("fij,fhwj->fhwi", t, hom)
    mag = torch.einsum("fij,fhwj->fhwi", t.abs(), hom.abs())
    return pts, 4 * U * mag


# ------------------------------------------------------------------------------------------------------ camera_tail
CAM_W = ("camera_head.more_mlps.0", "camera_head.more_mlps.2", "camera_head.fc_t", "camera_head.fc_rot")


def _linear_ref(W, b, x, ex, D):
    """y = W x + b with input error ex: a lane adds ceil(D / 64) products, six wave levels, the bias:
    k = ceil(D / 64) + 8 on sum |W| |x| + |b|, plus |W| ex."""
    W, b = W.double(), b.double()
    y = x @ W.t() + b
    k = (D + 63) // 64 + 8
    e = SLACK * (k * U * (x.abs() @ W.abs().t() + b.abs()) + ex @ W.abs().t())
    return y, e


def camera_tail_ref(feat, F, P, T, tok_off, w):
    """feat [F * T, D] fp32 (patch rows tok_off .. tok_off + P of each frame) -> dict:
      t, t_bound [F, 3];  A [F, 3, 3] the row-normalised fc_rot output;  R [F, 3, 3] its nearest rotation (SVD with the
      determinant fix, in fp64);  dA [F] the bound on ||A^ - A||_F;  s [F, 3] singular values of A;  det [F] = det A.
    Pool: with np = min(8, 1024 / (D / 4)) row phases a term sees at most ceil(P / np) accumulator additions, two to
    combine the four accumulators, np phase additions and the division: k = ceil(P / np) + np + 3.  ReLU is 1-Lipschitz.
    Rows of A: v -> v / |v| has the Jacobian (I - n n^T) / |v| of norm 1 / |v|; |v| itself (three squares, two sums, sqrtf)
    and the division add 5 U to every element."""
    from oracle.pi3_ref import svd_orthogonalize
    D = feat.shape[1]
    npz = min(8, 1024 // (D // 4))
    x = feat.double().view(F, T, D)[:, tok_off: tok_off + P]
    v = x.mean(1)
    ev = (math.ceil(P / npz) + npz + 3) * U * x.abs().mean(1)
    for name in CAM_W[:2]:
        v, ev = _linear_ref(w[name + ".weight"], w[name + ".bias"], v, ev, D)
        ev = torch.where(v + ev <= 0, torch.zeros_like(ev), ev)     # cut on both sides: an exact zero
        v = v.clamp_min(0)
    t, et = _linear_ref(w[CAM_W[2] + ".weight"], w[CAM_W[2] + ".bias"], v, ev, D)
    r, er = _linear_ref(w[CAM_W[3] + ".weight"], w[CAM_W[3] + ".bias"], v, ev, D)
    r, er = r.view(F, 3, 3), er.view(F, 3, 3)
    nrm = r.norm(dim=-1)
    A = r / nrm[..., None]
    rel = er.norm(dim=-1) / nrm
    assert float(rel.max()) < 2.0 ** -10
    dA = (SLACK * rel + 5 * U * math.sqrt(3.0)).norm(dim=-1)
    return {"t": t, "t_bound": et, "A": A, "R": svd_orthogonalize(r), "dA": dA,
            "s": torch.linalg.svdvals(A), "det": torch.det(A)}


def rotation_tolerance(ref) -> torch.Tensor:
    """[F]: 2 ||dA||_F / (s2 + sign(det) s3), the perturbation bound of the orthogonal polar factor restricted to SO(3),
    plus U: the pose is stored in fp32 and |R_ij| <= 1."""
    gap = ref["s"][:, 1] + torch.sign(ref["det"]) * ref["s"][:, 2]
    return 2 * ref["dA"] / gap + U


CAM_D = (4, 8, 512, 768, 1024)
CAM_P = (1, 3, 31, 32, 33, 70)
# seed per (D, P): every frame has s2 + sign(det) s3 > 0.1 and both signs of det occur (tests/test_pi3_kernels_ref.py)
CAM_SEEDS = {(4, 1): 10, (4, 3): 6, (4, 33): 2, (8, 1): 4, (8, 3): 7, (8, 33): 1, (8, 70): 5, (512, 32): 1, (768, 31): 3,
             (768, 70): 3, (1024, 1): 2, (1024, 3): 1, (1024, 33): 2}           # every other case: seed 0


def camera_case(D, P, tok_off, F=3):
    """Inputs of one camera_tail case: feat [F * T, D] (register rows NaN), T, weights.
    The bound of camera_tail_ref pushes errors through |W|, so it is as tight as the layers are free of cancellation:
    features are positive, and the two hidden layers are 0.7 x a permutation plus small, mostly positive noise
    (sum |w| |x| stays within a few percent of |sum w x|); every fourth hidden neuron has a bias of -3 and is cut by the
    ReLU.  Every frame lights its own random half of the channels, so the frames differ after the pool whatever P is.
    fc_t and fc_rot are signed (translations of order 10)."""
    g = torch.Generator().manual_seed(CAM_SEEDS.get((D, P), 0) * 100003 + D * 101 + P)
    T = P + tok_off
    feat = torch.full((F, T, D), float("nan"))
    feat[:, tok_off:] = torch.rand(F, P, D, generator=g) * 0.5 + 2.0 * (torch.rand(F, 1, D, generator=g) < 0.5).float()

    def hidden():
        W = (torch.rand(D, D, generator=g) - 0.1) * (0.3 / (0.4 * D))
        W[torch.arange(D), torch.randperm(D, generator=g)] += 0.7
        b = torch.randn(D, generator=g) * 0.1
        b[::4] -= 3.0
        return W, b
    def signed(n, scale):
        """Dense small weights (every column counts) plus up to eight large ones per row: the sum cancels like eight
        terms, not like D."""
        W = torch.randn(n, D, generator=g) * (0.05 / D ** 0.5)
        for r in range(n):
            cols = torch.randperm(D, generator=g)[:8]
            W[r, cols] += torch.randn(len(cols), generator=g) * scale
        return W
    (w1, b1), (w2, b2) = hidden(), hidden()
    w = {CAM_W[0] + ".weight": w1, CAM_W[0] + ".bias": b1, CAM_W[1] + ".weight": w2, CAM_W[1] + ".bias": b2,
         CAM_W[2] + ".weight": signed(3, 4.0), CAM_W[2] + ".bias": torch.randn(3, generator=g),
         CAM_W[3] + ".weight": signed(9, 0.4), CAM_W[3] + ".bias": torch.randn(9, generator=g) * 0.3}
    return feat.view(F * T, D), T, w


# ------------------------------------------------------------------------------------------- inputs shared by the tests
def layernorm_data(kind: str, rows: int, D: int, g: torch.Generator) -> torch.Tensor:
    """"randn": randn * 3 + 1;  "offset": mean 1e3 with a spread of 1e-1 (E[x^2] - E[x]^2 in fp32 has no digit left);
    "range": like randn, but row 0 spans twelve decades."""
    if kind == "offset":
        return 1e3 + 1e-1 * torch.randn(rows, D, generator=g)
    x = torch.randn(rows, D, generator=g) * 3 + 1
    if kind == "range":
        x[0] = torch.randn(D, generator=g) * torch.pow(torch.tensor(10.0), torch.rand(D, generator=g) * 12 - 6)
    return x


INF = float("inf")
CAST_TABLE = [
    0.0, -0.0, INF, -INF, float("nan"), 1.0, -1.0, 0.1,
    1 + 2.0 ** -8, -(1 + 2.0 ** -8),                 # bf16 tie, the neighbour below is even: down to 1
    1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8),         # bf16 tie, the neighbour below is odd: up to 1 + 2^-6
    1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 1 + 3 * 2.0 ** -8 - 2.0 ** -23,     # one fp32 ulp off a tie
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,              # the same two ties in half
    65504.0, 65519.99, 65520.0, -65520.0, 1e5,       # half: the largest, just under the tie to inf, the tie, beyond
    6.1e-5, 6e-5, 3.1e-5, 6e-8, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, -1e-7, 1e-9,     # half subnormals
    3.4028234663852886e38, -3.4028234663852886e38,   # +-max fp32: inf in both 16-bit formats
    3.3895313892515355e38,                           # the largest bf16
    1.1754943508222875e-38,                          # the smallest normal fp32 (a normal bf16 too)
]
CAST_TABLE += [1.0] * (-len(CAST_TABLE) % 4)

CAST_SHAPES = [(1, 4, 4, 4, 4), (7, 12, 12, 16, 20), (5, 24, 8, 12, 28), (3, 640, 588, 588, 640)]   # rows, cols, in_cols, ldi, ldo
CAST_CAPPED = [(350000, 12), (220000, 20), (2100, 2048)]
CAST_CAPPED_FILL = (220000, 20, 12)        # rows, cols, in_cols: the zero fill on the second and later steps of the walk
CAST_GRID_CAP = 4096 * 256          # float4s one sweep of the capped grid covers
QK_SHAPES = [(33, 2, 11), (4100, 16, 41)]                          # rows, H, T
QK_GRID_CAP = 4096 * 32             # 64-vectors one sweep of the capped grid covers


def index_values(rows: int, cols: int) -> torch.Tensor:
    """[rows, cols] fp32 made from the flat index by a multiplicative hash (odd modulus: no
    power-of-two stride repeats it): eleven significant bits (exact in half,
    rounded by bf16), so that an element taken from another row or quad differs."""
    i = torch.arange(rows * cols, dtype=torch.int64)
    h = (i * 2654435761) % 1000003 % 2048 - 1024
    return (h.float() / 16).view(rows, cols)


def qk_case(rows, H, T, seed=0):
    """bf16 qkv, positions (five register tokens at (0, 0), then a grid from (1, 1)), table, norm weights."""
    g = torch.Generator().manual_seed(rows + H + seed)
    qkv = (torch.randn(rows, 3 * H * 64, generator=g) * 2 + 0.25).bfloat16()
    side = max(1, math.isqrt(T - 5))
    pos = torch.zeros(T, 2, dtype=torch.int32)
    for t in range(5, T):
        pos[t, 0], pos[t, 1] = (t - 5) // side + 1, (t - 5) % side + 1
    cs = rope_table(int(pos.max()) + 1)
    nw = [torch.randn(64, generator=g) * 0.2 + (1 if i % 2 == 0 else 0) for i in range(4)]
    return qkv, pos, cs, nw
