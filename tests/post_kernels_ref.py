"""References and seeded inputs for the post-processing, alignment and ingest kernels (csrc/post.hip, csrc/sim3.hip,
csrc/ingest.hip): plain numpy / torch, no GPU.  Each reference is written from the kernel's documented contract and
takes the inputs the kernel takes; where the result is not exact it returns the per-element bound next to the value,
with the roundings counted from the kernel source.  tests/test_post_kernels_ref.py pins every reference to an
independent implementation (torch.median, oracle.post_ref, oracle.ingest_ref, Pillow, scipy) and asserts, on the
references alone, every property of the inputs that tests/test_post_kernels_gpu.py relies on.

The inputs are built here, by name and shape, so that both test files see the same arrays.
"""
import zlib
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

U53 = 2.0 ** -53                    # unit roundoff of binary64
SLACK = 1.0 + 2.0 ** -20            # second-order terms: k U53 / (1 - k U53) and the fp64 evaluation of the bound itself


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def ulp32(ref):
    """Spacing of the binary32 numbers around the fp64 values `ref` (the subnormal spacing below 2^-126)."""
    a = np.abs(np.asarray(ref, np.float64))
    _, e = np.frexp(a)                                           # a = m 2^e, m in [0.5, 1)
    fl = np.maximum(np.where(a == 0, -126, e - 1), -126)
    return np.ldexp(1.0, fl - 23)


def bits32(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def random_rotation(rng):
    """A general rotation (fp64) from a random unit quaternion: no axis is special, no entry is 0 or 1."""
    w, x, y, z = (q := rng.standard_normal(4)) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def general_poses(F_, rng, fourth_row=(0.25, -3.0, 7.0, 2.0)):
    """fp32 [F,4,4]: a general rotation, a translation and a NON-trivial fourth row per pose (no kernel here may read
    or write that row)."""
    P = np.zeros((F_, 4, 4), np.float32)
    for f in range(F_):
        P[f, :3, :3] = random_rotation(rng)
        P[f, :3, 3] = rng.standard_normal(3) * 2
        P[f, 3] = np.asarray(fourth_row, np.float32) * (f + 1)
    return P


def random_similarity(rng, smin=0.8, smax=1.25):
    """fp64 4x4 [[sR, t], [0, 0, 0, 1]] with a general rotation and s in [smin, smax]."""
    M = np.eye(4)
    M[:3, :3] = rng.uniform(smin, smax) * random_rotation(rng)
    M[:3, 3] = rng.standard_normal(3)
    return M


# ------------------------------------------------------------------------------------------- 1. masked ratio median
MEDIAN_SIZES = (1, 2, 3, 1023, 1024, 1025, 2049, 5000)
MEDIAN_STRIDES = (1, 3)
MEDIAN_KINDS = ("all_negative", "mixed_rank_below_zero", "mixed_rank_above_zero", "all_equal",
                "two_lower_last_pos", "two_upper_first_pos", "two_lower_last_neg", "two_upper_first_neg",
                "share8_pos", "share16_pos", "share24_pos", "share8_neg", "share16_neg", "share24_neg",
                "subnormal", "inf_neg", "inf_pos", "inf_both", "mask_bytes", "nan_masked_off", "nan_selected", "empty")


def ratio_median_ref(num, den, stride, mask, n):
    """The kernel's contract (post.hip): the quotients num[i] / den[i * stride] in fp32 (the device division is
    correctly rounded, so numpy's float32 division is the same number, subnormal results included), those with
    mask[i] != 0 sorted, the element of rank (count - 1) // 2 (torch's LOWER median).  A NaN among the selected
    quotients, or an empty selection, gives NaN.  Exact: no bound.  -> (float32 value, count)."""
    with np.errstate(all="ignore"):
        q = num[:n].astype(np.float32) / den[:n * stride:stride].astype(np.float32)
    sel = q[mask[:n] != 0]
    c = len(sel)
    if c == 0 or np.isnan(sel).any():
        return np.float32(np.nan), c
    return np.sort(sel)[(c - 1) // 2], c


def median_selected(case):
    """The selected fp32 quotients of a case, unsorted."""
    n, st = case["n"], case["stride"]
    with np.errstate(all="ignore"):
        q = case["num"][:n] / case["den"][:n * st:st]
    return q[case["mask"][:n] != 0]


def median_case(kind, n, stride):
    """-> dict(num [n], den [n * stride] with NaN between the strided entries (a stride slip poisons the result),
    mask uint8 [n], n, stride, expect = the value the construction plants or None, clean = the same case without its
    masked-off NaNs or None)."""
    rng = _rng("median", kind, n, stride)
    r = (n - 1) // 2
    pos = lambda k: (rng.random(k) + 0.1).astype(np.float32)                     # noqa: E731
    mask = np.ones(n, np.uint8)
    den = np.ones(n, np.float32)
    expect = clean = None

    def mixed(nneg):
        sign = np.ones(n, np.float32)
        sign[:nneg] = -1
        rng.shuffle(sign)
        flip = rng.choice(np.array([-1, 1], np.float32), n)                      # negative denominators as well
        return pos(n) * sign * flip, pos(n) * flip

    if kind == "all_negative":
        num, den = -pos(n), pos(n)
    elif kind == "mixed_rank_below_zero":                                         # r + 1 <= nneg: the rank is a negative
        num, den = mixed(r + 1 + (n - r - 1) // 2)
    elif kind == "mixed_rank_above_zero":                                         # nneg <= r: the rank is a positive
        num, den = mixed((r + 1) // 2)
    elif kind == "all_equal":
        num, den = np.full(n, 3.5, np.float32), np.full(n, 2.0, np.float32)
        expect = np.float32(1.75)
    elif kind.startswith("two_"):
        a = np.float32(1.5) if kind.endswith("pos") else np.float32(-1.5)
        b = np.nextafter(a, np.float32(2.0))                                      # the next float above a, either sign
        na = r + 1 if "lower_last" in kind else r                                 # the rank is the last a / the first b
        vals = np.array([a] * na + [b] * (n - na), np.float32)
        rng.shuffle(vals)
        num, den = vals * np.float32(0.5), np.full(n, 0.5, np.float32)            # exact
        expect = a if "lower_last" in kind else b
    elif kind.startswith("share"):
        top = int(kind[5:kind.index("_")])
        base = {8: 0x3F000000, 16: 0x3FC00000, 24: 0x3FC01200}[top] | (0x80000000 if kind.endswith("neg") else 0)
        bits = (base | rng.integers(0, 1 << (32 - top), n)).astype(np.uint32)     # keys built from integer bit patterns
        num = bits.view(np.float32).copy()
    elif kind == "subnormal":
        num, den = mixed(n // 3)
        num, den = num * np.float32(1e-30), den * np.float32(2e10)                # |quotient| about 1e-41 .. 5e-40
    elif kind.startswith("inf_"):
        if kind == "inf_neg":
            nlo, nhi = r + 1, 0                                                   # the rank is the last -inf
        elif kind == "inf_pos":
            nlo, nhi = 0, n - r                                                   # the rank is the first +inf
        else:
            nlo, nhi = min(r, n // 3), min(n - r - 1, n // 3)                     # the rank is finite
        num, den = mixed((n - nlo - nhi) // 2)
        where = rng.permutation(n)
        for j, i in enumerate(where[:nlo + nhi]):
            sgn = np.float32(-1.0 if j < nlo else 1.0)
            if j % 2:
                num[i], den[i] = sgn * np.float32(np.inf), np.float32(0.75)       # inf / finite
            else:
                num[i], den[i] = sgn, np.float32(0.0)                             # finite / +0
    elif kind == "mask_bytes":
        num, den = mixed(n // 2)
        mask = rng.choice(np.array([0, 1, 2, 128, 255], np.uint8), n)
        mask[0] = 255
    elif kind in ("nan_masked_off", "nan_selected"):
        num, den = mixed(n // 2)
        mask = (rng.random(n) > 0.3).astype(np.uint8)
        mask[0] = 1
        k = min(2, n - 1)                                                         # n = 1 has nothing to mask off
        mask[n - k:] = 0
        num[n - k:] = 1.0
        den[n - k:] = 1.0
        clean = dict(num=num.copy(), den=den.copy(), mask=mask.copy())
        if k >= 1:
            num[n - 1] = np.float32(np.nan)                                       # a NaN under a zero mask byte ...
        if k == 2:
            num[n - 2] = den[n - 2] = np.float32(0.0)                             # ... and a 0 / 0
        if kind == "nan_selected":                                                # the same NaN, selected
            num[n - 1] = np.float32(np.nan)
            mask[n - 1] = 1
            clean = None
    elif kind == "empty":
        num, den = mixed(n // 2)
        mask[:] = 0
    else:
        raise ValueError(kind)

    def strided(d):
        full = np.full(n * stride, np.nan, np.float32)
        full[::stride] = d
        return full

    case = dict(kind=kind, num=np.ascontiguousarray(num, np.float32), den=strided(den), mask=mask, n=n, stride=stride,
                expect=expect, clean=None)
    if clean is not None:
        case["clean"] = dict(kind=kind, num=clean["num"], den=strided(clean["den"]), mask=clean["mask"], n=n,
                             stride=stride)
    return case


def same_median(got, ref):
    """`==` on the values, the bit patterns as well wherever the answer is not a zero (+0 and -0 are distinct keys to
    the kernel's radix select but equal to a sort); NaN matches NaN."""
    got, ref = np.float32(got), np.float32(ref)
    if np.isnan(ref):
        return bool(np.isnan(got))
    if ref == 0:
        return bool(got == 0)
    return bool(got == ref) and int(bits32(got)[0]) == int(bits32(ref)[0])


# ------------------------------------------------------------------------------------------------- 2. apply_scale
def apply_scale_ref(scale, lp, pts, poses):
    """lp, pts (any shape, fp32) and poses[:, :3, 3] times s in fp32: one correctly rounded multiplication per float,
    so numpy's float32 product is the kernel's bit for bit.  s that is NaN, not positive or infinite counts as 1.
    Nothing else of the poses may change.  Exact: no bound."""
    s = np.float32(scale)
    if not (s > 0) or np.isinf(s):
        s = np.float32(1.0)
    P = poses.copy()
    P[:, :3, 3] = P[:, :3, 3] * s
    return lp * s, pts * s, P


# -------------------------------------------------------------------------------------------------- 3. sim3_apply
def sim3_apply_ref(M, pts, poses):
    """X' = A X + t on fp32 points [n,3] and, on cam->world poses [F,4,4] fp32, R_cw' = (A / sc) R_cw with sc = the
    norm of A's first column, c' = A c + t; the fourth rows of M and of every pose take no part.  Evaluated in fp64 in
    the kernel's expression order.  -> (p, p_bound, P, P_bound), fp64; P_bound is 0 on the fourth rows (untouched).

    Roundings, U = 2^-53, counted in sim3.hip for the uncontracted form (a contraction removes some, adds none):
      point / translation   A0 x + A1 y + A2 z + A3: the first product passes its own rounding and three additions, no
                            term passes more: 4 U sum|terms|.  This reference rounds the same expression the same way:
                            another 4.  k = 8.
      rotation              sc: three squares, two additions, the square root: the sum has 3 U, the root halves it and
                            adds one: 2.5 U relative.  Numerator: 3 U sum|terms|.  The division: 1 U.  In all at most
                            (3 + 2.5 + 1) U sum|terms| / sc <= 7 U ...; twice for kernel and reference: k = 14.
    then the conversion to fp32: half an ulp of the reference.  (A computed value on the other side of a power of two
    from the reference rounds to that power of two or nearer, so the reference's own ulp is the right one.)"""
    A = np.asarray(M, np.float64).reshape(4, 4)[:3]
    x = np.asarray(pts, np.float64).reshape(-1, 3)
    terms = A[None, :, :3] * x[:, None, :]                                        # [n, r, k] = A[r, k] x[k]
    p = ((terms[..., 0] + terms[..., 1]) + terms[..., 2]) + A[:, 3]
    pb = SLACK * (0.5 * ulp32(p) + 8 * U53 * (np.abs(terms).sum(-1) + np.abs(A[:, 3])))
    sc = np.sqrt(A[0, 0] * A[0, 0] + A[1, 0] * A[1, 0] + A[2, 0] * A[2, 0])
    Pin = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    P, Pb = Pin.copy(), np.zeros_like(Pin)
    t = A[None, :, :3, None] * Pin[:, None, :3, :]                                # [F, r, k, c] = A[r, k] P[k, c]
    s3 = (t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]                                   # [F, r, c]
    a3 = np.abs(t).sum(2)
    P[:, :3, :3] = s3[:, :, :3] / sc
    P[:, :3, 3] = s3[:, :, 3] + A[:, 3]
    Pb[:, :3, :3] = SLACK * (0.5 * ulp32(P[:, :3, :3]) + 14 * U53 * a3[:, :, :3] / sc)
    Pb[:, :3, 3] = SLACK * (0.5 * ulp32(P[:, :3, 3]) + 8 * U53 * (a3[:, :, 3] + np.abs(A[:, 3])))
    return p, pb, P, Pb


def rotation_defect_bound(M, poses_in, P_ref, P_bound):
    """Bound on |R'^T R' - I| (elementwise, [F,3,3]) for rotation blocks R' = Q + E, |E| <= P_bound, Q = R R_cw:
    Q^T Q - I = R_cw^T (R^T R - I) R_cw + (R_cw^T R_cw - I), so
      |R'^T R' - I| <= |R_cw^T R_cw - I|  (the fp32 input's own defect, evaluated here in fp64)
                     + 3 max|R^T R - I|   (the similarity's; columns of R_cw have 1-norm <= sqrt 3)
                     + |Q|^T b + b^T |Q| + b^T b  (the kernel's error, the same bound sim3_apply_ref states)
                     + 16 U53             (this evaluation and the test's)."""
    A = np.asarray(M, np.float64).reshape(4, 4)[:3, :3]
    R = A / np.sqrt((A[:, 0] ** 2).sum())
    dR = np.abs(R.T @ R - np.eye(3)).max()
    Rin = np.asarray(poses_in, np.float64)[:, :3, :3]
    d_in = np.abs(np.swapaxes(Rin, 1, 2) @ Rin - np.eye(3))
    Q, b = np.abs(P_ref[:, :3, :3]), P_bound[:, :3, :3]
    Qt, bt = np.swapaxes(Q, 1, 2), np.swapaxes(b, 1, 2)
    return d_in + 4 * dR + SLACK * (Qt @ b + bt @ Q + bt @ b) + 16 * U53


# ----------------------------------------------------------------------------------------- 4. sim3_compose_prefix
def compose_prefix_ref(T):
    """G_0 = T_0, G_c = G_{c-1} T_c in exact rational arithmetic.  T [n,4,4] fp64 -> (G as nested lists of Fraction,
    bound [n,4,4] fp64).  The kernel forms each entry as 0 + a b + a b + a b + a b in fp64: four roundings at most on
    a term (its product and the additions after it; 0 + x is exact), so one step adds 4 U |G_{c-1}| |T_c| to the error it
    inherits, |E_{c-1}| |T_c|.  By induction |E_c| <= c 4 U (1 + ...) |T_0| ... |T_c|; the factor 8 leaves the
    second-order terms a whole factor of two.  bound_c = c 8 U prod_{i <= c} |T_i|; step 0 is a copy (bound 0)."""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    Ts = [[[Fraction(float(v)) for v in row] for row in t] for t in T]
    G = [Ts[0]]
    for c in range(1, len(Ts)):
        g, t = G[-1], Ts[c]
        G.append([[sum(g[r][j] * t[j][k] for j in range(4)) for k in range(4)] for r in range(4)])
    bound = np.zeros_like(T)
    ap = np.abs(T[0])
    for c in range(1, len(T)):
        ap = ap @ np.abs(T[c])
        bound[c] = c * 8 * U53 * ap * SLACK
    return G, bound


def compose_within(got, G, bound):
    """max over entries of |got - G| / bound (0 / 0 counts as 0), evaluated exactly."""
    worst = Fraction(0)
    for c in range(len(G)):
        for r in range(4):
            for k in range(4):
                err = abs(Fraction(float(got[c, r, k])) - G[c][r][k])
                b = Fraction(float(bound[c, r, k]))
                if err == 0:
                    continue
                if b == 0:
                    return float("inf")
                worst = max(worst, err / b)
    return float(worst)


def compose_case(n):
    rng = _rng("compose", n)
    return np.stack([random_similarity(rng) for _ in range(n)])


# --------------------------------------------------------------------------------------------- 5. match_keypoints
MATCH_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (3, 171), (2, 600))
NAN16 = 0x7E01                                                                    # a NaN with a payload bit


def match_case(ov, K):
    """-> (kp_ref, kp_qry) fp16 [ov,K,2] and the planted facts {view: {qry slot: expected index}}.  Coordinates come
    from a small integer range, so reference views hold duplicates; the query is a permutation of its reference view.
    From K >= 8 on, per view v:
      qry slot 2 = (1000 + v, 7), present in reference view (v + 1) % ov only (when ov > 1)          -> -1
      qry slot 4 = (-0.0, 900) against reference slot 3 = (+0.0, 900): equal values, different bits  -> -1
      qry slot 6 = (NaN 0x7e01, 901) = reference slot 5, the same bits                               ->  5"""
    rng = _rng("match", ov, K)
    ref = rng.integers(0, max(3, K // 8), (ov, K, 2)).astype(np.float16)
    if K >= 2:
        ref[:, K - 1] = ref[:, 0]                                                 # at least one duplicate per view
    qry = np.stack([ref[v, rng.permutation(K)] for v in range(ov)])
    planted = {v: {} for v in range(ov)}
    if K >= 8:
        r16, q16 = ref.view(np.uint16), qry.view(np.uint16)
        for v in range(ov):
            if ov > 1:
                ref[(v + 1) % ov, 1] = (1000 + v, 7)
                qry[v, 2] = (1000 + v, 7)
                planted[v][2] = -1
            ref[v, 3] = (0.0, 900)
            qry[v, 4] = (-0.0, 900)
            planted[v][4] = -1
            ref[v, 5, 1] = qry[v, 6, 1] = 901
            r16[v, 5, 0] = q16[v, 6, 0] = NAN16
            planted[v][6] = 5
    return np.ascontiguousarray(ref), np.ascontiguousarray(qry), planted


def match_brute(kp_ref, kp_qry):
    """All-pairs comparison of the packed 32-bit patterns; first hit in the same view."""
    ov, K = kp_ref.shape[:2]
    r = np.ascontiguousarray(kp_ref).view(np.uint32).reshape(ov, K)
    q = np.ascontiguousarray(kp_qry).view(np.uint32).reshape(ov, K)
    eq = q[:, :, None] == r[:, None, :]
    return np.where(eq.any(-1), eq.argmax(-1), -1).astype(np.int32)


# ---------------------------------------------------------------------------------------- 6. project_observations
PROJ_KS = (1, 127, 128, 129, 300)
PROJ_W, PROJ_H = 64, 32
# identity pose, K = [[64, 0, 0], [0, 1, 31], [0, 0, 1]]: u = 64 x / z, v = y / z + 31, every operation exact.
PROJ_EXACT = (  # point (fp16-exact), u, v, inside
    ((0.0, 0.0, 1.0), 0.0, 31.0, True),                             # u = 0 is in
    ((1.0, 0.0, 1.0), 64.0, 31.0, False),                           # u = W is out
    ((0.5, 1.0 - 2.0 ** -10, 1.0), 32.0, 32.0 - 2.0 ** -10, True),  # v = H - 2^-10 is in
    ((-2.0 ** -14, 0.0, 4.0), -2.0 ** -10, 31.0, False),            # u = -2^-10 is out
    ((0.5, 1.0, 1.0), 32.0, 32.0, False),                           # v = H is out
    ((0.5, -31.0, 1.0), 32.0, 0.0, True),                           # v = 0 is in
    ((0.5, 0.0, 0.0), np.nan, np.nan, False),                       # zc = 0: inf and 0/0, out
    ((-0.5, -0.5, -1.0), 32.0, 31.5, True),                         # zc < 0 landing inside is in (no z > 0 test)
    ((0.25, 0.5, 2.0), 8.0, 31.25, True),
)


def project_exact_case(N, K):
    """points fp16 [N,K,3] cycling through PROJ_EXACT (shifted by the frame index, so frames differ), identity poses
    and the exact intrinsics -> (points, poses, intr, u [N,K], v [N,K], inside [N,K]) for any active pair."""
    # frame 1 starts at the table's first row: with K = 1 the earliest source frame still pins u = 0, frame 2 u = W
    sel = (np.arange(K)[None, :] + np.arange(N)[:, None] - 1) % len(PROJ_EXACT)
    tab = np.array([p for p, _, _, _ in PROJ_EXACT], np.float16)
    pts = tab[sel]
    assert np.array_equal(pts.astype(np.float64), np.array([p for p, _, _, _ in PROJ_EXACT])[sel]), "fp16-exact"
    poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    intr = np.tile(np.array([[64, 0, 0], [0, 1, 31], [0, 0, 1]], np.float32), (N, 1, 1))
    u = np.array([e[1] for e in PROJ_EXACT])[sel]
    v = np.array([e[2] for e in PROJ_EXACT])[sel]
    inside = np.array([e[3] for e in PROJ_EXACT])[sel]
    return np.ascontiguousarray(pts), poses, intr, u, v, inside


def active_pairs(N, max_after):
    a = np.zeros((N, N), bool)
    for s in range(N):
        a[s, :s] = True
        a[s, s + 1:s + 1 + max_after] = True
    return a


def project_ref(points, poses, intr, W, H, max_after):
    """The kernel's contract (sim3.hip): for every active (source, target) pair x = T_t^-1 X with the fp32 pose widened
    to fp64 and inverted there, (xn, yn, zn) = x / zc, u = K0 . (xn, yn, zn), v = K1 . (xn, yn, zn), inside = 0 <= u < W
    and 0 <= v < H; inactive pairs are 0.  -> (uv [N,N,K,2] fp64, inside [N,N,K] bool, zc [N,N,K] fp64)."""
    N, K = points.shape[:2]
    X = np.concatenate([points.astype(np.float64), np.ones((N, K, 1))], -1)
    uv, inside, zc = np.zeros((N, N, K, 2)), np.zeros((N, N, K), bool), np.zeros((N, N, K))
    act = active_pairs(N, max_after)
    with np.errstate(all="ignore"):
        for s in range(N):
            for t in range(N):
                if not act[s, t]:
                    continue
                x = X[s] @ np.linalg.inv(poses[t].astype(np.float64)).T
                n3 = x[:, :3] / x[:, 2:3]
                pr = n3 @ intr[t].astype(np.float64).T
                uv[s, t], zc[s, t] = pr[:, :2], x[:, 2]
                inside[s, t] = (pr[:, 0] >= 0) & (pr[:, 0] < W) & (pr[:, 1] >= 0) & (pr[:, 1] < H)
    return uv, inside, zc


PROJ_GENERAL = dict(N=5, K=300, W=64, H=48, max_after=2, min_depth=0.5)


def project_general_case():
    """Five cameras with real rotations (up to 0.5 rad about random axes) around a scene 4 units ahead; per source
    frame the first K of 6 K candidates whose depth in EVERY camera is at least 0.5 in magnitude."""
    g = PROJ_GENERAL
    N, K = g["N"], g["K"]
    rng = _rng("project", "general")
    poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    for f in range(N):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        th = rng.uniform(0.2, 0.5)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        poses[f, :3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        poses[f, :3, 3] = rng.standard_normal(3) * 0.3
    intr = np.tile(np.array([[40, 0, 32], [0, 40, 24], [0, 0, 1]], np.float32), (N, 1, 1))
    intr[:, 0, 0] += np.arange(N, dtype=np.float32)                               # per-target intrinsics differ
    intr[:, 0, 1] = 0.5                                                           # a skew: K[1] is read
    pts = np.zeros((N, K, 3), np.float16)
    inv = [np.linalg.inv(p.astype(np.float64)) for p in poses]
    for s in range(N):
        cand = (rng.standard_normal((6 * K, 3)) * np.array([2.5, 2.0, 1.5]) + np.array([0, 0, 4.0])).astype(np.float16)
        X = np.concatenate([cand.astype(np.float64), np.ones((6 * K, 1))], -1)
        ok = np.all([np.abs(X @ iv[2]) >= g["min_depth"] + 1e-3 for iv in inv], 0)
        assert ok.sum() >= K
        pts[s] = cand[ok][:K]
    return pts, poses, intr


def project_tolerance(uv_ref):
    return 2.0 ** -23 * np.maximum(1.0, np.abs(uv_ref))


def project_near_border(uv_ref, W, H):
    """Observations whose reference u or v lies within the tolerance of a border: the flag may go either way."""
    tol = project_tolerance(uv_ref)
    u, v = uv_ref[..., 0], uv_ref[..., 1]
    return (np.minimum(np.abs(u), np.abs(u - W)) <= tol[..., 0]) | (np.minimum(np.abs(v), np.abs(v - H)) <= tol[..., 1])


# ------------------------------------------------------------------------------------------------- 7. focal_shift
FOCAL_SHAPES = ((64, 64), (17, 23), (1, 64), (100, 37))
FOCAL_SCENES = ("pinhole", "noisy")
FOCAL_F0, FOCAL_SHIFT0 = 0.9, 0.3
FS_N = 64


def focal_sample_maps(H, W):
    """Pixel row / column each of the 64 x 64 samples reads: F.interpolate(mode='nearest') applied to index images."""
    yy = F.interpolate(torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W).contiguous(),
                       (FS_N, FS_N), mode="nearest")[0, 0, :, 0].long().numpy()
    xx = F.interpolate(torch.arange(W, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W).contiguous(),
                       (FS_N, FS_N), mode="nearest")[0, 0, 0, :].long().numpy()
    return yy, xx


def focal_scene(H, W, scene):
    """local_points fp32 [H,W,3].  'pinhole': a smooth surface seen by a pinhole of focal FOCAL_F0 on the normalised
    view plane, its z then moved by -FOCAL_SHIFT0: recover_focal_shift's residual is exactly 0 at shift = FOCAL_SHIFT0,
    focal = FOCAL_F0.  'noisy': the same with 1 % gaussian noise on all three coordinates."""
    from oracle import post_ref
    uv = post_ref.normalized_view_plane_uv(W, H).numpy().astype(np.float64)
    z = 2.0 + 0.5 * np.sin(3.0 * uv[..., 0] + 1.0) + 0.4 * np.cos(4.0 * uv[..., 1]) + 0.3 * uv[..., 0] * uv[..., 1]
    lp = np.concatenate([uv * z[..., None] / FOCAL_F0, (z - FOCAL_SHIFT0)[..., None]], -1)
    if scene == "noisy":
        lp = lp + 0.01 * _rng("focal", H, W).standard_normal(lp.shape) * np.abs(lp).mean()
    return lp.astype(np.float32)


def focal_masks(H, W):
    """Pixel masks by name (bool [H,W]), in a fixed order.  'last_wave' is the pixel row that sample row 35 reads (the
    kernel compacts 256 samples = 4 sample rows at a time, one 64-lane wave per row; 35 % 4 == 3): where H >= 64 no
    other sample row reads it, so in that batch three waves are empty and every other batch is.  'two' and 'one' exist
    only where pixels can be found that exactly one sample reads (H, W >= 64 or a column hit once)."""
    yy, xx = focal_sample_maps(H, W)
    m = {}
    m["full"] = np.ones((H, W), bool)
    m["row"] = np.zeros((H, W), bool)
    m["row"][yy[32]] = True
    m["checker"] = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    m["last_wave"] = np.zeros((H, W), bool)
    m["last_wave"][yy[35]] = True
    m["two_cols"] = np.zeros((H, W), bool)                   # two, so that H = 1 still leaves two distinct points
    m["two_cols"][:, xx[21]] = m["two_cols"][:, xx[45]] = True
    m["lower_half"] = np.zeros((H, W), bool)
    m["lower_half"][H // 2:] = True
    once_y = [i for i in range(FS_N) if (yy == yy[i]).sum() == 1]
    once_x = [j for j in range(FS_N) if (xx == xx[j]).sum() == 1]
    if len(once_y) >= 8 and len(once_x) >= 8:
        (ya, yb), (xa, xb) = (once_y[2], once_y[-3]), (once_x[3], once_x[-2])
        m["two"] = np.zeros((H, W), bool)
        m["two"][yy[ya], xx[xa]] = m["two"][yy[yb], xx[xb]] = True
        m["one"] = np.zeros((H, W), bool)
        m["one"][yy[ya], xx[xa]] = True
        m["diagonal"] = np.zeros((H, W), bool)
        for i in range(FS_N):
            m["diagonal"][yy[i], xx[i]] = True
    return m


def focal_samples(lp, mask):
    """The point list recover_focal_shift hands the solver: (uv [n,2], xyz [n,3]) fp32, row-major over the samples."""
    from oracle import post_ref
    H, W = mask.shape
    yy, xx = focal_sample_maps(H, W)
    uv = post_ref.normalized_view_plane_uv(W, H).numpy()
    sel = mask[yy][:, xx]
    return uv[yy][:, xx][sel], lp[yy][:, xx][sel]


def lm_focal_shift(uv, xyz, ftol=1e-3):
    """solve_optimal_focal_shift (utils/geometry_numpy.py:79-96) with the stopping tolerance exposed and the number of
    residual evaluations returned.  -> (shift float32, focal float64, nfev)."""
    from scipy.optimize import least_squares
    uv, xy, z = uv.reshape(-1, 2), xyz[..., :2].reshape(-1, 2), xyz[..., 2].reshape(-1)

    def fn(shift):
        xy_proj = xy / (z + shift)[:, None]
        f = (xy_proj * uv).sum() / np.square(xy_proj).sum()
        return (f * xy_proj - uv).ravel()

    sol = least_squares(fn, x0=0, ftol=ftol, method="lm")
    shift = sol["x"].squeeze().astype(np.float32)
    xy_proj = xy / (z + shift)[:, None]
    return shift, (xy_proj * uv).sum() / np.square(xy_proj).sum(), int(sol["nfev"])


def focal_shift_ref(lp, mask):
    """lp fp32 [F,H,W,3], mask bool [F,H,W] -> dict of numpy fp32: focal [F], shift [F] (oracle.post_ref: scipy LM),
    fxfycxcy [F,4] and K [F,3,3] by camera_estimation.py:47-57 in fp32.  Tolerances are the project's: focal rtol
    1e-5, shift rtol 1e-5 with atol 1e-6 (the device restates MINPACK's iteration in fp64; no bound is derived)."""
    from oracle import post_ref
    focal, shift = post_ref.recover_focal_shift(torch.from_numpy(lp), torch.from_numpy(mask))
    return dict(focal=focal.numpy(), shift=shift.numpy(), **focal_intrinsics(focal, lp.shape[1], lp.shape[2]))


def focal_intrinsics(focal, H, W):
    """fx, fy, cx, cy and the 3x3 from an fp32 focal, torch fp32 arithmetic in the reference's operation order."""
    focal = torch.as_tensor(focal, dtype=torch.float32)
    ar = W / H
    fx = focal / 2 * (1 + ar ** 2) ** 0.5 / ar * W
    fy = focal / 2 * (1 + ar ** 2) ** 0.5 * H
    cx, cy = torch.full_like(fx, W // 2), torch.full_like(fy, H // 2)
    K = torch.zeros(len(focal), 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = fx, fy, cx, cy, 1.0
    return dict(fxfycxcy=torch.stack([fx, fy, cx, cy], 1).numpy(), K=K.numpy())


def focal_batches(H, W):
    """[(names, masks bool [3,H,W])]: the masks of focal_masks three to a call, a different one per frame."""
    m = focal_masks(H, W)
    names = list(m)
    assert len(names) % 3 == 0
    return [(names[i:i + 3], np.stack([m[k] for k in names[i:i + 3]])) for i in range(0, len(names), 3)]


# ------------------------------------------------------------------------------------------------------ 8. ingest
INGEST_SHAPES = ((1, 7, 9, 7, 9), (2, 5, 3, 1, 1), (1, 1, 1, 4, 5), (1, 69, 130, 8, 15), (3, 10, 300, 13, 257))
INGEST_KINDS = ("random", "zeros", "full", "checker", "frame_constants")


def ingest_case(kind, N, H0, W0):
    """uint8 [N,H0,W0,3]."""
    if kind == "random":
        return _rng("ingest", N, H0, W0).integers(0, 256, (N, H0, W0, 3), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((N, H0, W0, 3), np.uint8)
    if kind == "full":
        return np.full((N, H0, W0, 3), 255, np.uint8)
    if kind == "checker":
        c = ((np.add.outer(np.arange(H0), np.arange(W0)) % 2) * 255).astype(np.uint8)
        return np.broadcast_to(c[None, :, :, None], (N, H0, W0, 3)).copy()
    if kind == "frame_constants":                                                 # a frame-stride slip mixes these
        v = (37 + 83 * np.arange(N)[:, None] + 29 * np.arange(3)[None, :]).astype(np.uint8)
        return np.broadcast_to(v[:, None, None, :], (N, H0, W0, 3)).copy()
    raise ValueError(kind)
