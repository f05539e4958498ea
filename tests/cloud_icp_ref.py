"""numpy f64 oracle of the ICP normal equations (pi3_slam_amd/csrc/cloud_icp.hip), an ICP loop of its own around it
(scipy's k-d tree for the search), and the planted room the ICP tests run on.

The equations are formed straight from their definition: for every pair that takes part the 3 x 7 Jacobian
J = [ -[x]x | x | I ] is built as a matrix and the sums are einsums over (pair, row); nothing of the kernel's written-out
J^T J is restated here.  Every sum comes with its MAJORANT: the same sum with every factor replaced by its absolute
value before multiplying (|J|, |n|, |e| component-wise), the scale against which two differently ordered f64 sums may
differ.  What IS the kernel's arithmetic: which pairs take part, and how a normal is prepared (rotation row by row as
(R0 a0 + R1 a1) + R2 a2, l2 = (a0 a0 + a1 a1) + a2 a2, n = a / sqrt(l2)): the counters must agree exactly.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

SPAN = 4096          # queries per workgroup of the kernel (ops.CLOUD_ICP_SPAN)
TRI = np.triu_indices(7)


def jacobians(x: np.ndarray) -> np.ndarray:
    """x (P,3) -> J (P,3,7) = [ -[x]x | x | I ]: d(p + w x x + l x + t) / d(w, l, t) at 0."""
    P = len(x)
    J = np.zeros((P, 3, 7))
    cross = np.zeros((P, 3, 3))                      # [x]x
    cross[:, 0, 1], cross[:, 0, 2] = -x[:, 2], x[:, 1]
    cross[:, 1, 0], cross[:, 1, 2] = x[:, 2], -x[:, 0]
    cross[:, 2, 0], cross[:, 2, 1] = -x[:, 1], x[:, 0]
    J[:, :, 0:3] = -cross
    J[:, :, 3] = x
    J[:, :, 4:7] = np.eye(3)
    return J


def prepare_normals(raw: np.ndarray, Rn: Optional[np.ndarray]):
    """raw (P,3) -> (ok (P,), n (P,3) unit where ok) with the kernel's operation order."""
    a = np.asarray(raw, np.float64)
    with np.errstate(all="ignore"):
        if Rn is not None:
            R = np.asarray(Rn, np.float64).reshape(3, 3)
            a = np.stack([(R[k, 0] * a[:, 0] + R[k, 1] * a[:, 1]) + R[k, 2] * a[:, 2] for k in range(3)], 1)
        l2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        ok = (l2 > 0.0) & (l2 < np.inf)
        n = a / np.sqrt(np.where(ok, l2, 1.0))[:, None]
    return ok, n


def pair_equations(queries, points, idx, d2, trim_dist: float, centre, normals=None, normals_of: int = 0, Rn=None) -> Dict:
    """-> sums (37,) = A's upper triangle row-major (28), b (7), r2, sum of e.e; majorant (37,) likewise; counters
    dict(used, unmatched, trimmed, normal_rejected).  queries may be f32 (what the kernel sees) or f64 (the oracle's
    own ICP loop)."""
    q = np.asarray(queries).astype(np.float64).reshape(-1, 3)
    pts = np.asarray(points).astype(np.float64).reshape(-1, 3)
    idx = np.asarray(idx).astype(np.int64).reshape(-1)
    d2 = np.asarray(d2, np.float64).reshape(-1)
    m, n = len(q), len(pts)
    c = np.asarray(centre, np.float64).reshape(3)
    matched = (idx >= 0) & (idx < n)
    with np.errstate(invalid="ignore"):
        near = d2 <= float(trim_dist) * float(trim_dist)
    take = matched & near
    rejected = np.zeros(m, bool)
    nrm = None
    if normals_of:
        raw = np.asarray(normals).astype(np.float64).reshape(-1, 3)
        rows = np.where(take, idx, 0) if normals_of == 1 else np.arange(m)
        ok, nrm = prepare_normals(raw[rows] if len(raw) else np.zeros((m, 3)), Rn if normals_of == 2 else None)
        rejected = take & ~ok
        take = take & ok
    counters = dict(used=int(take.sum()), unmatched=int((~matched).sum()), trimmed=int((matched & ~near).sum()),
                    normal_rejected=int(rejected.sum()))
    p = q[take]
    e = p - pts[idx[take]]
    x = p - c
    J = jacobians(x)
    aJ, ae = np.abs(J), np.abs(e)
    if normals_of == 0:
        A, b, r2 = np.einsum("pka,pkb->ab", J, J), np.einsum("pka,pk->a", J, e), np.einsum("pk,pk->", e, e)
        Am, bm, r2m = np.einsum("pka,pkb->ab", aJ, aJ), np.einsum("pka,pk->a", aJ, ae), np.einsum("pk,pk->", ae, ae)
    else:
        nn = nrm[take]
        an = np.abs(nn)
        j, r = np.einsum("pka,pk->pa", J, nn), np.einsum("pk,pk->p", nn, e)
        jm, rm = np.einsum("pka,pk->pa", aJ, an), np.einsum("pk,pk->p", an, ae)
        A, b, r2 = np.einsum("pa,pb->ab", j, j), np.einsum("pa,p->a", j, r), np.einsum("p,p->", r, r)
        Am, bm, r2m = np.einsum("pa,pb->ab", jm, jm), np.einsum("pa,p->a", jm, rm), np.einsum("p,p->", rm, rm)
    ee = np.einsum("pk,pk->", e, e)
    eem = np.einsum("pk,pk->", ae, ae)
    return dict(sums=np.concatenate([A[TRI], b, [r2, ee]]), majorant=np.concatenate([Am[TRI], bm, [r2m, eem]]),
                counters=counters, A=A, b=b)


# ------------------------------------------------------------------------------------------------ the oracle's ICP
def increment(x, centre) -> np.ndarray:
    """The 4x4 similarity of the step x = (w, l, t) about centre, through scipy's rotation vector."""
    from scipy.spatial.transform import Rotation
    x = np.asarray(x, np.float64)
    c = np.asarray(centre, np.float64)
    sR = np.exp(x[3]) * Rotation.from_rotvec(x[:3]).as_matrix()
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = sR, c + x[4:] - sR @ c
    return D


def icp(est, ref, mode: str, est_normals=None, ref_normals=None, with_scale=False, max_dist=0.25, iterations=30,
        tolerance=1e-7, init=None) -> Dict:
    """The algorithm of map_eval.icp_refine in numpy f64 throughout: the moved estimate is never rounded to fp32."""
    from scipy.spatial import cKDTree
    e0 = np.asarray(est).astype(np.float64).reshape(-1, 3)
    r = np.asarray(ref).astype(np.float64).reshape(-1, 3)
    tree = cKDTree(r)
    centre = r.mean(0)
    M = np.eye(4) if init is None else np.array(init, np.float64)
    sel = np.arange(7) if with_scale else np.array([0, 1, 2, 4, 5, 6])
    history, status = [], "max_iterations"
    for _ in range(iterations):
        moved = e0 @ M[:3, :3].T + M[:3, 3]
        d, i = tree.query(moved, distance_upper_bound=max_dist)
        hit = np.isfinite(d)
        idx = np.where(hit, i, -1)
        d2 = np.where(hit, d, np.inf) ** 2                   # the tree already stopped at max_dist: no further trim
        if mode == "point":
            eq = pair_equations(moved, r, idx, d2, 1e150, centre)
        elif ref_normals is not None:
            eq = pair_equations(moved, r, idx, d2, 1e150, centre, ref_normals, 1)
        else:
            Rn = M[:3, :3] / np.cbrt(np.linalg.det(M[:3, :3]))
            eq = pair_equations(moved, r, idx, d2, 1e150, centre, est_normals, 2, Rn)
        pairs = eq["counters"]["used"]
        history.append(dict(pairs=pairs, rms=float(np.sqrt(eq["sums"][35] / max(pairs, 1))),
                            point_rms=float(np.sqrt(eq["sums"][36] / max(pairs, 1)))))
        if pairs < 16:
            status = "too_few_pairs"
            break
        A, b = eq["A"][np.ix_(sel, sel)], eq["b"][sel]
        x = np.zeros(7)
        x[sel] = np.linalg.solve(A, -b)
        M = increment(x, centre) @ M
        history[-1]["step"] = float(np.linalg.norm(x))
        if history[-1]["step"] < tolerance:
            status = "converged"
            break
    return dict(transform=M, status=status, iterations=len(history), history=history)


# ------------------------------------------------------------------------------------------------ the planted room
ROOM = np.array([4.0, 3.0, 2.5])                 # the box, centred on the origin
CABINET = np.array([1.0, 1.0, 1.2])              # in the corner at -ROOM / 2
ROOM_SEED = 5
TRUTH_AXIS = np.array([0.3, -0.5, 0.8])
TRUTH_DEG = 3.0
TRUTH_T = np.array([0.08, -0.048, 0.032])


def sample_room(count: int, rng) -> tuple:
    """`count` points uniform by area on the inside of the box and on the three free faces of the cabinet, with the
    normals that point into the room.  -> (points f64 (count,3), normals f64 (count,3))."""
    lo, hi = -ROOM / 2.0, ROOM / 2.0
    cab = lo + CABINET
    faces = []                                    # (axis, coordinate, normal sign, lo2, hi2) over the other two axes
    for ax in range(3):
        faces.append((ax, lo[ax], 1.0, lo, hi))
        faces.append((ax, hi[ax], -1.0, lo, hi))
        faces.append((ax, cab[ax], 1.0, lo, cab))                                      # a free face of the cabinet
    areas = np.array([np.prod(np.delete(h - l, ax)) for ax, _, _, l, h in faces])
    pts, nrm = [], []
    have = 0
    while have < count:
        which = rng.choice(len(faces), size=count, p=areas / areas.sum())
        u = rng.random((count, 3))
        P, N = np.zeros((count, 3)), np.zeros((count, 3))
        for f, (ax, at, sign, l, h) in enumerate(faces):
            rows = which == f
            P[rows] = l + u[rows] * (h - l)
            P[rows, ax] = at
            N[rows, ax] = sign
        inside = np.all(P < cab - 1e-9, axis=1)                                       # wall or floor behind the cabinet
        pts.append(P[~inside])
        nrm.append(N[~inside])
        have += int((~inside).sum())
    return np.concatenate(pts)[:count], np.concatenate(nrm)[:count]


def truth(scale: float = 1.0) -> np.ndarray:
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = scale * Rotation.from_rotvec(np.deg2rad(TRUTH_DEG) * TRUTH_AXIS / np.linalg.norm(TRUTH_AXIS)).as_matrix()
    T[:3, 3] = TRUTH_T
    return T


def planted_room(scale: float = 1.0, noise: float = 0.0, n_ref: int = 20000, n_est: int = 10000, seed: int = ROOM_SEED) -> Dict:
    """The reference (n_ref points, with normals), an independent sample of the same room as the estimate (n_est points,
    with normals) moved by the INVERSE of truth(scale) and given Gaussian noise of `noise` metres: the ICP must find
    truth(scale).  All arrays fp32, as the device receives them."""
    rng = np.random.default_rng(seed)
    ref, ref_n = sample_room(n_ref, rng)
    est, est_n = sample_room(n_est, rng)
    T = truth(scale)
    R = T[:3, :3] / scale
    moved = (est - T[:3, 3]) @ T[:3, :3] / scale ** 2                                  # T^-1 p, row-wise
    if noise:
        moved = moved + noise * rng.standard_normal(moved.shape)
    return dict(ref=ref.astype(np.float32), ref_normals=ref_n.astype(np.float32), est=moved.astype(np.float32),
                est_normals=(est_n @ R).astype(np.float32), est_unmoved=est.astype(np.float32), truth=T)


def alignment_error(M, T) -> Dict:
    """How far the similarity M is from the truth T: rotation angle (degrees), displacement of the room's centre (the
    origin) in metres, scale error."""
    M, T = np.asarray(M, np.float64), np.asarray(T, np.float64)
    sm, st = np.cbrt(np.linalg.det(M[:3, :3])), np.cbrt(np.linalg.det(T[:3, :3]))
    dR = (M[:3, :3] / sm) @ (T[:3, :3] / st).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return dict(rotation_deg=float(ang), centre_m=float(np.linalg.norm(M[:3, 3] - T[:3, 3])), scale=float(abs(sm - st)))
