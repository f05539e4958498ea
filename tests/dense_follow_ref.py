"""numpy oracle of the follow kernel (pi3_slam_amd/csrc/cloud_follow.hip) and of dense_map.MapFollower.chunk_moves,
element-wise in f64, every product and sum rounded on its own in the kernel's order, the views in order.

  follow   per point X (fp32 widened to f64), per view m (views (M,20): rigid frame->camera 3x4 row-major, fx fy cx cy,
           0, [17] = the plane's unit; moves (M,12): D_m 3x4 row-major; planes fp16 (M,H',W')):
             Y = ((d0 x + d1 y) + d2 z) + d3, ..;   Nn = (d0 nx + d1 ny) + d2 nz, ..;   S3 += Y, N3 += Nn;
             xc = ((c0 x + c1 y) + c2 z) + c3, likewise yc, zc;  next view unless zc > 0 and all finite;
             u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rint(u / S), pv = rint(v / S), inside the plane;
             w = 1 / (zc zc);  S2 += w Y, W2 += w, N2 += w Nn, ++n2;
             zo = c17 plane[m, pv, pu], next view when 0 or not finite;
             |zc - zo| <= rel_tol zo + margin:  S1 += w Y, W1 += w, N1 += w Nn, ++n1;
           level = 1 when n1 > 0, else 2 when n2 > 0, else 3;  out = S_l / W_l (level 3: S3 / M);  normal = N_l /
           sqrt((Nx Nx + Ny Ny) + Nz Nz) when that is positive and finite, else 0;  a point that is not finite is
           copied, level 0.
  moves    D = [s R_f Rt_o | s R_f t_o + c_f]: (Rt_o, t_o) the rigid frame->camera of the created pose, (R_f, c_f) the
           rotation (scale divided out) and centre of the final pose, s the cube root of the determinant of the chunk
           transform's 3x3 block.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

import dense_carve_ref as cref

SCALE_AT = cref.SCALE_AT


def _project(c, plane, x, y, z, S: float):
    """The carver's projection of (x, y, z) into view c -> (zc, inside the plane, zo where inside else 0)."""
    Hp, Wp = plane.shape
    xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3]
    yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7]
    zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11]
    ok = (zc > 0) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
    u = c[12] * (xc / zc) + c[14]
    v = c[13] * (yc / zc) + c[15]
    pu = np.rint(u / S)
    pv = np.rint(v / S)
    ok &= (pu >= 0) & (pu <= Wp - 1) & (pv >= 0) & (pv <= Hp - 1)
    iu = np.where(ok, pu, 0).astype(np.int64)
    iv = np.where(ok, pv, 0).astype(np.int64)
    zo = c[SCALE_AT] * plane[iv, iu].astype(np.float64)
    return zc, ok, zo


def follow(points, normals, views, moves, planes, stride: int, rel_tol: float, margin: float) -> Dict[str, np.ndarray]:
    """points f32 (P,3), normals f32 (P,3) or None, views f64 (M,20), moves f64 (M,12), planes fp16 (M,H',W') ->
    points f32 (P,3), normals f32 (P,3) or None, level u8 (P,), support i32 (P,), counters i64 (4,) = not finite,
    level 1, 2, 3."""
    Xf = np.asarray(points, np.float32).reshape(-1, 3)
    X = Xf.astype(np.float64)
    P = len(X)
    views = np.asarray(views, np.float64).reshape(-1, 20)
    moves = np.asarray(moves, np.float64).reshape(-1, 12)
    planes = np.asarray(planes)
    M = len(views)
    assert M >= 1 and len(moves) == M and planes.dtype == np.float16 and planes.ndim == 3 and len(planes) == M
    with_n = normals is not None
    Nf = np.asarray(normals, np.float32).reshape(-1, 3) if with_n else np.zeros((P, 3), np.float32)
    N = Nf.astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    live = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    S1, S2, S3 = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3))
    N1, N2, N3 = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3))
    W1, W2 = np.zeros(P), np.zeros(P)
    n1, n2 = np.zeros(P, np.int64), np.zeros(P, np.int64)
    S, tol, mar = float(stride), float(rel_tol), float(margin)
    for d, c, plane in zip(moves, views, planes):
        with np.errstate(all="ignore"):
            Y = np.stack([((d[0] * x + d[1] * y) + d[2] * z) + d[3],
                          ((d[4] * x + d[5] * y) + d[6] * z) + d[7],
                          ((d[8] * x + d[9] * y) + d[10] * z) + d[11]], 1)
            Nn = np.stack([(d[0] * nx + d[1] * ny) + d[2] * nz,
                           (d[4] * nx + d[5] * ny) + d[6] * nz,
                           (d[8] * nx + d[9] * ny) + d[10] * nz], 1)
            S3 = S3 + Y
            N3 = N3 + Nn
            zc, seen, zo = _project(c, plane, x, y, z, S)
            seen &= live
            w = 1.0 / (zc * zc)
            wY = w[:, None] * Y
            wN = w[:, None] * Nn
            S2 = np.where(seen[:, None], S2 + wY, S2)
            W2 = np.where(seen, W2 + w, W2)
            N2 = np.where(seen[:, None], N2 + wN, N2)
            n2 += seen
            lim = tol * zo + mar
            agree = seen & (zo != 0) & np.isfinite(zo) & (np.abs(zc - zo) <= lim)
            S1 = np.where(agree[:, None], S1 + wY, S1)
            W1 = np.where(agree, W1 + w, W1)
            N1 = np.where(agree[:, None], N1 + wN, N1)
            n1 += agree
    level = np.where(~live, 0, np.where(n1 > 0, 1, np.where(n2 > 0, 2, 3))).astype(np.uint8)
    l1, l2 = (level == 1)[:, None], (level == 2)[:, None]
    with np.errstate(all="ignore"):
        Sl = np.where(l1, S1, np.where(l2, S2, S3))
        Wl = np.where(level == 1, W1, np.where(level == 2, W2, float(M)))
        out = (Sl / Wl[:, None]).astype(np.float32)
        Nl = np.where(l1, N1, np.where(l2, N2, N3))
        q = (Nl[:, 0] * Nl[:, 0] + Nl[:, 1] * Nl[:, 1]) + Nl[:, 2] * Nl[:, 2]
        ok = (q > 0) & np.isfinite(q)
        nrm = np.where(ok[:, None], Nl / np.sqrt(q)[:, None], 0.0).astype(np.float32)
    out = np.where(live[:, None], out, Xf)
    nrm = np.where(live[:, None], nrm, Nf)
    counters = np.array([int((~live).sum())] + [int((level == k).sum()) for k in (1, 2, 3)], np.int64)
    return dict(points=out, normals=nrm if with_n else None, level=level,
                support=np.where(live, n1, 0).astype(np.int32), counters=counters)


def depth_scale(chunk: Dict) -> float:
    """The cube root of the determinant of the 3x3 block of the chunk's transform ('_sim3_dense', else '_sim3_global',
    else the identity)."""
    G = chunk.get("_sim3_dense")
    if G is None:
        G = chunk.get("_sim3_global")
    if G is None:
        return 1.0
    return float(np.cbrt(np.linalg.det(np.asarray(G, np.float64).reshape(4, 4)[:3, :3])))


def _frames_and_k(chunk: Dict):
    dd = chunk["dense_depth"]
    frames = np.asarray(dd["frames"], np.int64).reshape(-1)
    return frames, np.asarray(dd["fxfycxcy"], np.float64).reshape(-1, 4)


def chunk_moves(chunk: Dict):
    """-> (views (M,20) at the created poses with [17] = 1, moves (M,12), planes fp16 (M,H',W'), stride) or None."""
    if chunk.get("dense_depth") is None or chunk.get("_poses_created") is None:
        return None
    frames, K = _frames_and_k(chunk)
    if len(frames) == 0:
        return None
    created = np.asarray(chunk["_poses_created"], np.float64).reshape(-1, 4, 4)[frames]
    final = np.asarray(chunk["camera_poses"], np.float64).reshape(-1, 4, 4)[frames]
    views = cref.pack_views(created, K, 1.0)
    rigid = views[:, :12].reshape(-1, 3, 4)
    A = final[:, :3, :3]
    Rf = A / np.cbrt(np.linalg.det(A))[:, None, None]
    cf = final[:, :3, 3]
    sR = depth_scale(chunk) * Rf
    moves = np.zeros((len(frames), 3, 4))
    moves[:, :, :3] = np.einsum("mij,mjk->mik", sR, rigid[:, :, :3])
    moves[:, :, 3] = np.einsum("mij,mj->mi", sR, rigid[:, :, 3]) + cf
    planes = np.ascontiguousarray(np.asarray(chunk["dense_depth"]["depth"])).astype(np.float16)
    return views, moves.reshape(-1, 12), planes, int(chunk["dense_depth"]["pixel_stride"])


def follow_chunk(chunk: Dict, rel_tol: float, margin_voxels: float = 1.0) -> Optional[Dict[str, np.ndarray]]:
    """The chunk's dense_cloud moved by follow(); None when chunk_moves gives nothing."""
    got = chunk_moves(chunk)
    if got is None:
        return None
    views, moves, planes, stride = got
    cl = chunk["dense_cloud"]
    nrm = cl.get("normals")
    return follow(np.asarray(cl["points"]), None if nrm is None else np.asarray(nrm), views, moves, planes, stride,
                  rel_tol, margin_voxels * float(cl["voxel_size"]))


def keyframe_residuals(points_world, chunks):
    """For every (map point, keyframe of every chunk at its FINAL pose, its plane scaled by the chunk's s): (zc, zo)
    wherever the carver's projection gives an in-plane, non-zero, finite sample -> two f64 arrays."""
    X = np.asarray(points_world, np.float32).astype(np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    zcs, zos = [], []
    for chunk in chunks:
        if chunk.get("dense_depth") is None:
            continue
        frames, K = _frames_and_k(chunk)
        if len(frames) == 0:
            continue
        final = np.asarray(chunk["camera_poses"], np.float64).reshape(-1, 4, 4)[frames]
        views = cref.pack_views(final, K, depth_scale(chunk))
        planes = np.asarray(chunk["dense_depth"]["depth"]).astype(np.float16)
        S = float(chunk["dense_depth"]["pixel_stride"])
        for c, plane in zip(views, planes):
            with np.errstate(all="ignore"):
                zc, ok, zo = _project(c, plane, x, y, z, S)
                ok &= (zo != 0) & np.isfinite(zo)
            zcs.append(zc[ok])
            zos.append(zo[ok])
    if not zcs:
        return np.zeros(0), np.zeros(0)
    return np.concatenate(zcs), np.concatenate(zos)
