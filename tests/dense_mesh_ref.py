"""numpy oracle of the dense map's surface mesh (pi3_slam_amd/csrc/voxel_mesh.hip, pi3_slam_amd/dense_map.MapMesher).

An oriented-point signed field (Hoppe '92) on the lattice of the fused voxel table, meshed by surface nets.  Inputs are
the table's integer sums (dense_map_ref.merge: keys, W, U, C) and the normal sums (dense_normals_ref.accumulate: keys,
acc = Nx, Ny, Nz, cnt).  All arithmetic is f64 / int64, every operation rounded on its own, in the order written:

  source voxel   keep (when a mask is given), W >= 1, cnt > 0 and (Nx, Ny, Nz) != 0
                 c = k + U / (W * 2^24) per axis (voxel units), n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz),
                 colour_u = (C + W // 2) // W
  cell           a voxel index i with every biased field in 1 .. 2^21 - 1 and a source voxel among the 27 voxels
                 i - 1 .. i + 1 (x-major order: dx outermost, dz innermost)
  corner         g = i + (a, b, c), a, b, c in {0, 1}; f(g) = (sum over the source voxels among g - 1 .. g, in x-major
                 order, of (nx (gx - cx) + ny (gy - cy)) + nz (gz - cz)) / their number; undefined without one
  edge           EDGES below: axis 0's four, then axis 1's, then axis 2's; a crossing when both ends are defined and
                 exactly one has f < 0; its point is the lower end with t = f_a / (f_a - f_b) added along the axis
  vertex         a cell with a crossing: the sum of its crossings in edge order / their number, times the voxel size in
                 f64, rounded to fp32; normal = S / sqrt((Sx Sx + Sy Sy) + Sz Sz) of the sum S of the 27 voxels' unit
                 normals in x-major order (0 when the square is not positive); colour = (sum colour_u + cnt // 2) // cnt
  quad           the edge from a cell's corner 0 along axis a, when it is a crossing and the cells i - e_b, i - e_c,
                 i - e_b - e_c exist (b = (a + 1) % 3, c = (a + 2) % 3): ring q0 = i - e_b - e_c, q1 = i - e_c, q2 = i,
                 q3 = i - e_b, counter-clockwise seen from +a; flip = the lower end is not negative (the surface faces -a).
                 Triangles (q0, q1, q2), (q0, q2, q3), or with flip (q0, q2, q1), (q0, q3, q2).
  ambiguous      the cell faces through corner 0 whose four corners are defined with alternating signs (four crossings:
                 a non-manifold edge)

Vertices in ascending cell-key order, quads by (owner key, axis).  Test infrastructure only: the product never imports
it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

BIAS = 1 << 20
FIELD_MAX = (1 << 21) - 1
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]      # x-major
CORNERS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]                        # index 4a + 2b + c
# (axis, lower corner index, upper corner index)
EDGES = ([(0, 2 * b + c, 4 + 2 * b + c) for b in (0, 1) for c in (0, 1)]
         + [(1, 4 * a + c, 4 * a + 2 + c) for a in (0, 1) for c in (0, 1)]
         + [(2, 4 * a + 2 * b, 4 * a + 2 * b + 1) for a in (0, 1) for b in (0, 1)])


def fields(keys: np.ndarray) -> np.ndarray:
    """keys u64 (n,) -> biased fields int64 (n,3)."""
    k = np.asarray(keys, np.uint64)
    return np.stack([((k >> np.uint64(42 - 21 * a)) & np.uint64(FIELD_MAX)).astype(np.int64) for a in range(3)], 1)


def pack(f: np.ndarray) -> np.ndarray:
    f = np.asarray(f, np.int64).astype(np.uint64)
    return (f[..., 0] << np.uint64(42)) | (f[..., 1] << np.uint64(21)) | f[..., 2]


def sources(table: Dict[str, np.ndarray], nacc: Dict[str, np.ndarray], keep: Optional[np.ndarray] = None):
    """-> the source voxels in ascending key order: keys u64 (S,), c f64 (S,3), n f64 (S,3), colour int64 (S,3)."""
    keys = np.asarray(table["keys"], np.uint64)
    W = np.asarray(table["W"], np.uint64)
    sums = np.zeros((len(keys), 4), np.int64)
    if len(nacc["keys"]) and len(keys):
        at = np.minimum(np.searchsorted(nacc["keys"], keys), len(nacc["keys"]) - 1)
        hit = nacc["keys"][at] == keys
        sums[hit] = nacc["acc"][at[hit]]
    src = (W >= 1) & (sums[:, 3] > 0) & (sums[:, :3] != 0).any(1)
    if keep is not None:
        src &= np.asarray(keep).reshape(-1).astype(bool)
    keys, W, sums = keys[src], W[src], sums[src]
    U, C = np.asarray(table["U"], np.uint64)[src], np.asarray(table["C"], np.uint64)[src]
    k = (fields(keys) - BIAS).astype(np.float64)
    den = W.astype(np.float64) * 16777216.0
    c = k + U.astype(np.float64) / den[:, None]
    d = sums[:, :3].astype(np.float64)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    n = d / ln[:, None]
    col = ((C + W[:, None] // np.uint64(2)) // np.maximum(W[:, None], np.uint64(1))).astype(np.int64)
    return keys, c, n, col


def mesh(table: Dict[str, np.ndarray], nacc: Dict[str, np.ndarray], voxel_size: float,
         keep: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """-> keys u64 (V,), vertices f32 (V,3), normals f32 (V,3), colors u8 (V,3), faces i32 (F,3), quad_keys u64 (Q,),
    quad_codes i32 (Q,) (axis | flip << 2), vertices_f64 (V,3) (the vertices in voxel units before the fp32 rounding),
    and the counts sources / cells / quads / ambiguous."""
    skeys, sc, sn, scol = sources(table, nacc, keep)
    S = len(skeys)
    empty = dict(keys=np.zeros(0, np.uint64), vertices=np.zeros((0, 3), np.float32), normals=np.zeros((0, 3), np.float32),
                 colors=np.zeros((0, 3), np.uint8), faces=np.zeros((0, 3), np.int32), quad_keys=np.zeros(0, np.uint64),
                 quad_codes=np.zeros(0, np.int32), vertices_f64=np.zeros((0, 3), np.float64), sources=S, cells=0, quads=0, ambiguous=0)
    if S == 0:
        return empty
    sf = fields(skeys)
    off = np.asarray(OFFSETS, np.int64)
    cand = (sf[:, None, :] + off[None, :, :]).reshape(-1, 3)
    cand = cand[((cand >= 1) & (cand <= FIELD_MAX)).all(1)]
    ckeys = np.unique(pack(cand))
    cf = fields(ckeys)                                      # (M,3) biased
    M = len(ckeys)
    # the 27 voxels of every cell: index into the sources, or -1
    nf = cf[:, None, :] + off[None, :, :]                   # (M,27,3)
    exists = ((nf >= 1) & (nf <= FIELD_MAX)).all(2)
    nk = pack(np.where(exists[..., None], nf, 1))
    at = np.minimum(np.searchsorted(skeys, nk), S - 1)
    nb = np.where(exists & (skeys[at] == nk), at, -1)       # (M,27)
    has = nb >= 0
    nbs = np.where(has, nb, 0)
    i0 = (cf - BIAS).astype(np.float64)                     # the cell's index = its corner 0

    # corners
    f = np.zeros((M, 8), np.float64)
    cnt = np.zeros((M, 8), np.int64)
    for ci, (a, b, c) in enumerate(CORNERS):
        g = i0 + np.array([a, b, c], np.float64)
        for j, (dx, dy, dz) in enumerate(OFFSETS):
            if not (a - 1 <= dx <= a and b - 1 <= dy <= b and c - 1 <= dz <= c):
                continue
            cc, nn = sc[nbs[:, j]], sn[nbs[:, j]]
            term = (nn[:, 0] * (g[:, 0] - cc[:, 0]) + nn[:, 1] * (g[:, 1] - cc[:, 1])) + nn[:, 2] * (g[:, 2] - cc[:, 2])
            f[:, ci] = f[:, ci] + np.where(has[:, j], term, 0.0)
            cnt[:, ci] += has[:, j]
    defined = cnt > 0
    f = np.where(defined, f / np.maximum(cnt, 1).astype(np.float64), 0.0)
    neg = defined & (f < 0.0)

    # crossings and the vertex
    psum = np.zeros((M, 3), np.float64)
    ncross = np.zeros(M, np.int64)
    crossing = np.zeros((M, 12), bool)
    for e, (axis, lo, hi) in enumerate(EDGES):
        x = defined[:, lo] & defined[:, hi] & (neg[:, lo] != neg[:, hi])
        crossing[:, e] = x
        with np.errstate(all="ignore"):
            t = f[:, lo] / (f[:, lo] - f[:, hi])
        p = i0 + np.asarray(CORNERS[lo], np.float64)
        p[:, axis] = p[:, axis] + np.where(x, t, 0.0)
        psum = psum + np.where(x[:, None], p, 0.0)
        ncross += x
    vert = ncross > 0
    pos64 = psum / np.maximum(ncross, 1).astype(np.float64)[:, None]        # voxel units
    pos = (float(voxel_size) * pos64).astype(np.float32)

    # normal and colour over the 27 voxels
    ns = np.zeros((M, 3), np.float64)
    cs = np.zeros((M, 3), np.int64)
    for j in range(27):
        ns = ns + np.where(has[:, j, None], sn[nbs[:, j]], 0.0)
        cs += np.where(has[:, j, None], scol[nbs[:, j]], 0)
    l2 = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]
    some = l2 > 0.0
    nrm = np.where(some[:, None], ns / np.sqrt(np.where(some, l2, 1.0))[:, None], 0.0).astype(np.float32)
    n27 = has.sum(1).astype(np.int64)
    col = ((cs + (n27 // 2)[:, None]) // np.maximum(n27, 1)[:, None]).astype(np.uint8)

    # quads: the three edges from corner 0 (EDGES 0, 4, 8)
    qk, qc = [], []
    for axis, e in ((0, 0), (1, 4), (2, 8)):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        ok = crossing[:, e] & (cf[:, b] - 1 >= 1) & (cf[:, c] - 1 >= 1)
        flip = ~neg[:, 0]
        qk.append(ckeys[ok])
        qc.append((axis | (flip[ok].astype(np.int64) << 2)).astype(np.int32))
    qk, qc = np.concatenate(qk), np.concatenate(qc)
    order = np.lexsort((qc & 3, qk))
    qk, qc = qk[order], qc[order]

    # ambiguous faces through corner 0: perpendicular to `axis`, corners with that bit clear
    amb = 0
    for axis in range(3):
        bit = 4 >> axis
        o1, o2 = [x for x in (4, 2, 1) if x != bit]
        quad = [0, o1, o1 + o2, o2]
        alld = defined[:, quad].all(1)
        alt = (neg[:, quad[0]] == neg[:, quad[2]]) & (neg[:, quad[1]] == neg[:, quad[3]]) & (neg[:, quad[0]] != neg[:, quad[1]])
        amb += int((alld & alt).sum())

    vkeys = ckeys[vert]
    out = dict(keys=vkeys, vertices=pos[vert], normals=nrm[vert], colors=col[vert], quad_keys=qk, quad_codes=qc,
               vertices_f64=pos64[vert], sources=S, cells=M, quads=len(qk), ambiguous=amb)
    out["faces"] = quad_faces(vkeys, qk, qc)
    return out


def quad_ring(quad_keys: np.ndarray, quad_codes: np.ndarray) -> np.ndarray:
    """The four cell keys q0..q3 of every quad, u64 (Q,4)."""
    f = fields(quad_keys)
    axis = np.asarray(quad_codes, np.int64) & 3
    rows = np.arange(len(f))
    ring = np.repeat(f[:, None, :], 4, 1)                   # q2 = the owner
    b, c = (axis + 1) % 3, (axis + 2) % 3
    ring[rows, 0, b] -= 1
    ring[rows, 0, c] -= 1
    ring[rows, 1, c] -= 1
    ring[rows, 3, b] -= 1
    return pack(ring)


def quad_faces(vertex_keys: np.ndarray, quad_keys: np.ndarray, quad_codes: np.ndarray) -> np.ndarray:
    """Triangles i32 (2 Q,3) into the ascending vertex keys; every ring key must be a vertex."""
    if len(quad_keys) == 0:
        return np.zeros((0, 3), np.int32)
    ring = quad_ring(quad_keys, quad_codes)
    idx = np.searchsorted(vertex_keys, ring)
    assert (idx < len(vertex_keys)).all() and (vertex_keys[np.minimum(idx, len(vertex_keys) - 1)] == ring).all(), \
        "a quad names a cell without a vertex"
    flip = (np.asarray(quad_codes, np.int64) >> 2 & 1).astype(bool)
    q0, q1, q2, q3 = idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]
    t1 = np.where(flip[:, None], np.stack([q0, q2, q1], 1), np.stack([q0, q1, q2], 1))
    t2 = np.where(flip[:, None], np.stack([q0, q3, q2], 1), np.stack([q0, q2, q3], 1))
    return np.stack([t1, t2], 1).reshape(-1, 3).astype(np.int32)


# ---------------------------------------------------------------------------------------------- inputs for the tests
def fused(points: np.ndarray, normals: np.ndarray, colors: Optional[np.ndarray], voxel_size: float):
    """Oriented points f32 (n,3) + unit normals f32 (n,3) [+ colours u8], weight 1 each, identity rotation ->
    (table, nacc) as the map and normal oracles fuse them."""
    import dense_map_ref as dm
    import dense_normals_ref as dn
    inv_v = dm.inv_voxel(voxel_size)
    keys, w, wu, wc, _ = dm.contributions_points(points, colors, None, inv_v)
    table = dm.merge(keys, w, wu, wc)
    part = dn.point_normals(points, normals, np.ones(len(points), np.int32), np.eye(3).reshape(9), inv_v)
    return table, dn.accumulate([part])


def sphere_samples(radius: float, centre, n: int, seed: int = 0):
    """n points on a sphere (a Fibonacci spiral, so every voxel the surface crosses is hit when n is large) with their
    outward normals and a colour that varies over the surface."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    p = (np.asarray(centre, np.float64) + radius * d).astype(np.float32)
    col = np.clip(np.rint(127.5 * (d + 1.0)), 0, 255).astype(np.uint8)
    return p, d.astype(np.float32), col


PLANE_Q = (11.0, 8.0, 32.0)             # the plane patch's normal direction: about (0.316, 0.230, 0.920)


def plane_samples(voxel_size: float, half_extent: float = 15.0, step: float = 0.125, origin=(0.3125, 0.4375, 0.28125)):
    """A patch of the plane q . (s - origin) = 0 in voxel units s, q = PLANE_Q: a grid of (sx, sy) at `step` spacing within
    +-half_extent voxels of the origin, sz solved for.  With a power-of-two voxel size, step and origin every coordinate
    is a multiple of 2^-24 voxels, so the fused centroids lie on the plane exactly; the normals are q / 64, which the
    2^15 fixed point of the normal sums holds exactly.  -> points f32 (metres), normals f32, colours u8, and the plane
    (origin, unit normal) in voxel units, f64."""
    q = np.asarray(PLANE_Q, np.float64)
    o = np.asarray(origin, np.float64)
    g = np.arange(-half_extent, half_extent + 0.5 * step, step)
    a, b = np.meshgrid(g, g, indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    s = np.stack([o[0] + a, o[1] + b, o[2] - (q[0] * a + q[1] * b) / q[2]], 1)
    p = (s * float(voxel_size)).astype(np.float32)
    assert (p.astype(np.float64) / float(voxel_size) == s).all(), "the plane's samples must be exact in fp32"
    nr = np.repeat((q / 64.0)[None], len(p), 0).astype(np.float32)
    col = np.stack([np.full(len(p), 200.0), 128 + 100 * a / half_extent, 128 + 100 * b / half_extent], 1).astype(np.uint8)
    return p, nr, col, (o, q / np.linalg.norm(q))


def plane_rim_distance(x: np.ndarray, half_extent: float = 15.0, origin=(0.3125, 0.4375, 0.28125)) -> np.ndarray:
    """The distance (voxel units) of the points x f64 (n,3) from the rim of plane_samples' patch: its four sides."""
    q = np.asarray(PLANE_Q, np.float64)
    o = np.asarray(origin, np.float64)
    h = float(half_extent)
    cor = [o + np.array([a, b, -(q[0] * a + q[1] * b) / q[2]]) for a, b in ((-h, -h), (h, -h), (h, h), (-h, h))]
    best = np.full(len(x), np.inf)
    for i in range(4):
        p0, d = cor[i], cor[(i + 1) % 4] - cor[i]
        t = np.clip(((x - p0) @ d) / (d @ d), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(x - (p0 + t[:, None] * d), axis=1))
    return best


def edge_uses(faces: np.ndarray):
    """-> (undirected edges (E,2) sorted, the number of triangles on each)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(1)
    return np.unique(e, axis=0, return_counts=True)
