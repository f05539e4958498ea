"""numpy oracle of the depth keyframes (pi3_slam_amd/csrc/dense_filter.hip: pi3_dense_depth_planes) and of the carve
kernel (pi3_slam_amd/csrc/voxel_carve.hip), element-wise, every product and sum rounded on its own in the kernels' order.

  planes   the candidates of the consistency filter (dense_consistency_ref.candidates) on the frames 0, K, 2K, .. and
           the pixels (S y', S x'): local z (fp32) rounded to fp16 nearest-even, 0 for a non-candidate and for a value
           that rounds to 0 or inf;
  carve    per voxel centroid X (the fp32 rows of the extraction, widened to f64) and view m (20 doubles: rigid
           world->camera 3x4 row-major, fx fy cx cy, 0, [17] = depth scale s):
             xc = ((r00 x + r01 y) + r02 z) + t0, likewise yc, zc;  no vote unless zc > 0 and all finite;
             u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rint(u / S), pv = rint(v / S), inside the plane;
             zo = s plane[m, pv, pu], no vote when 0 or not finite;  r = zc - zo, lim = rel_tol zo + margin;
             agree |r| <= lim, conflict r < -lim;
           carved = conflict >= min_conflicts and conflict > agree.
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict

import numpy as np

import dense_consistency_ref as cref

SCALE_AT = 17


def depth_planes(points, local_points, conf, masks, conf_logit_thr: float, every: int, stride: int):
    """-> (depth fp16 (Nk,H',W'), the number of non-zero samples)."""
    cand = cref.candidates(points, local_points, conf, masks, conf_logit_thr)
    z = np.where(cand, np.asarray(local_points, np.float32)[..., 2], np.float32(0)).astype(np.float32)
    sub = z[::int(every), ::int(stride), ::int(stride)]
    with np.errstate(over="ignore"):
        h = sub.astype(np.float16)
    h = np.where(np.isfinite(h), h, np.float16(0)).astype(np.float16)
    return np.ascontiguousarray(h), int(np.count_nonzero(h))


def pack_views(poses_c2w, fxfycxcy, scale=1.0) -> np.ndarray:
    """cam->world poses (M,4,4) (a scale in the 3x3 block is divided out) + intrinsics (M,4) + depth scale -> f64 (M,20)."""
    P = np.asarray(poses_c2w, np.float64).reshape(-1, 4, 4)
    K = np.asarray(fxfycxcy, np.float64).reshape(-1, 4)
    A = P[:, :3, :3]
    R = A / np.cbrt(np.linalg.det(A))[:, None, None]
    Rt = np.transpose(R, (0, 2, 1))
    t = -np.einsum("mij,mj->mi", Rt, P[:, :3, 3])
    views = np.zeros((len(P), 20))
    views[:, :12] = np.concatenate([Rt, t[:, :, None]], 2).reshape(-1, 12)
    views[:, 12:16] = K
    views[:, SCALE_AT] = scale
    return views


def carve(points, views, planes, stride: int, rel_tol: float, margin: float, min_conflicts: int) -> Dict[str, np.ndarray]:
    """points f32 (V,3), views f64 (M,20), planes fp16 (M,H',W') -> per voxel agree / conflict uint32, carved bool, and
    stats = {voxels, carved, unvoted}."""
    X = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    views = np.asarray(views, np.float64).reshape(-1, 20)
    planes = np.asarray(planes)
    assert planes.dtype == np.float16 and planes.ndim == 3 and len(planes) == len(views)
    Hp, Wp = planes.shape[1:]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    agree = np.zeros(len(X), np.uint32)
    conflict = np.zeros(len(X), np.uint32)
    S, tol, mar = float(stride), float(rel_tol), float(margin)
    for c, plane in zip(views, planes):
        with np.errstate(all="ignore"):
            xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3]
            yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7]
            zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11]
            ok = (zc > 0) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
            u = c[12] * (xc / zc) + c[14]
            v = c[13] * (yc / zc) + c[15]
            pu, pv = np.rint(u / S), np.rint(v / S)
            ok &= (pu >= 0) & (pu <= Wp - 1) & (pv >= 0) & (pv <= Hp - 1)
            iu = np.where(ok, pu, 0).astype(np.int64)
            iv = np.where(ok, pv, 0).astype(np.int64)
            zo = c[SCALE_AT] * plane[iv, iu].astype(np.float64)
            ok &= (zo != 0) & np.isfinite(zo)
            r = zc - zo
            lim = tol * zo + mar
            a = ok & (np.abs(r) <= lim)
            k = ok & ~a & (r < -lim)
        agree += a
        conflict += k
    carved = (conflict >= np.uint32(min_conflicts)) & (conflict > agree)
    return dict(agree=agree, conflict=conflict, carved=carved,
                stats={"voxels": len(X), "carved": int(carved.sum()), "unvoted": int(((agree + conflict) == 0).sum())})
