"""float32 numpy oracle of the multi-view depth consistency filter (pi3_slam_amd/csrc/dense_filter.hip).

Same arithmetic, step for step, every product and sum rounded to fp32 on its own in the kernel's order:
  candidate   mask != 0, conf > conf_logit_thr, the three world coordinates finite, local z finite and > 0;
  zplane      local z of a candidate, else 0;
  neighbour   j = i +- s * stride, s = 1..radius, inside [0, N); R, t = poses[j] (cam->world):
              d = X - t;  xc = (R00 dx + R10 dy) + R20 dz, yc / zc from columns 1 / 2;  no vote unless zc > 0, all finite;
              u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rint(u), pv = rint(v) (half to even), inside the image;
              zo = zplane[j, pv, pu] != 0;  r = zc - zo, lim = rel_tol zo;  agree |r| <= lim, conflict r < -lim;
  keep        agree >= min_views and conflict <= agree.
Vectorised over frames and pixels, one loop over the 2 * radius neighbours.  Test infrastructure only: the product
never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

F = np.float32


def candidates(points, local_points, conf, masks, conf_logit_thr: float) -> np.ndarray:
    P = np.asarray(points, F)
    z = np.asarray(local_points, F)[..., 2]
    cand = np.isfinite(P).all(-1) & np.isfinite(z)
    with np.errstate(invalid="ignore"):
        cand &= z > 0
        if conf is not None:
            cand &= np.asarray(conf, F).reshape(z.shape) > F(conf_logit_thr)
    if masks is not None:
        cand &= np.asarray(masks).reshape(z.shape).astype(bool)
    return cand


def consistency(points, local_points, conf, masks, poses, fxfycxcy, conf_logit_thr: float, radius: int, stride: int,
                min_views: int, rel_tol: float) -> Dict[str, np.ndarray]:
    """-> mask u8 (N,H,W), counts u8 (N,H,W,2) [agree, conflict], stats i64 (2,) [candidates, kept]."""
    P = np.asarray(points, F)
    N, H, W = P.shape[:3]
    T = np.asarray(poses, F).reshape(N, 4, 4)
    K = np.asarray(fxfycxcy, F).reshape(N, 4)
    cand = candidates(P, local_points, conf, masks, conf_logit_thr)
    zplane = np.where(cand, np.asarray(local_points, F)[..., 2], F(0)).astype(F)
    agree = np.zeros((N, H, W), np.int32)
    conflict = np.zeros((N, H, W), np.int32)
    tol = F(rel_tol)
    for s in range(1, int(radius) + 1):
        for sign in (-1, 1):
            off = sign * s * int(stride)
            src = np.arange(max(0, -off), min(N, N - off))       # frames i with j = i + off inside [0, N)
            if len(src) == 0:
                continue
            a, c = _votes(P[src], T[src + off], K[src + off], zplane[src + off], H, W, tol)
            agree[src] += a & cand[src]
            conflict[src] += c & cand[src]
    keep = cand & (agree >= int(min_views)) & (conflict <= agree)
    counts = np.stack([np.minimum(agree, 255), np.minimum(conflict, 255)], -1).astype(np.uint8)
    return dict(mask=keep.astype(np.uint8), counts=counts, candidates=cand,
                stats=np.array([int(cand.sum()), int(keep.sum())], np.int64))


def _votes(X, T, K, zj, H: int, W: int, tol):
    """X (n,H,W,3) world points, T (n,4,4) / K (n,4) / zj (n,H,W) of their target views -> (agree, conflict) bool."""
    def col(v):
        return v[:, None, None]
    with np.errstate(all="ignore"):
        dx, dy, dz = X[..., 0] - col(T[:, 0, 3]), X[..., 1] - col(T[:, 1, 3]), X[..., 2] - col(T[:, 2, 3])
        xc = (col(T[:, 0, 0]) * dx + col(T[:, 1, 0]) * dy) + col(T[:, 2, 0]) * dz
        yc = (col(T[:, 0, 1]) * dx + col(T[:, 1, 1]) * dy) + col(T[:, 2, 1]) * dz
        zc = (col(T[:, 0, 2]) * dx + col(T[:, 1, 2]) * dy) + col(T[:, 2, 2]) * dz
        ok = (zc > 0) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
        u = col(K[:, 0]) * (xc / zc) + col(K[:, 2])
        v = col(K[:, 1]) * (yc / zc) + col(K[:, 3])
        pu, pv = np.rint(u), np.rint(v)
        ok &= (pu >= 0) & (pu <= F(W - 1)) & (pv >= 0) & (pv <= F(H - 1))
        iu = np.where(ok, pu, F(0)).astype(np.int64)
        iv = np.where(ok, pv, F(0)).astype(np.int64)
        zo = zj[np.arange(len(zj))[:, None, None], iv, iu]
        ok &= zo != 0
        r = zc - zo
        lim = tol * zo
        assert r.dtype == F and lim.dtype == F and u.dtype == F
        agree = ok & (np.abs(r) <= lim)
        conflict = ok & ~agree & (r < -lim)
    return agree, conflict


# ------------------------------------------------------------------------------------------------ analytic test scene
def plane_scene(N: int, H: int, W: int, seed: int = 0, noise_rel: float = 0.0):
    """Cameras that translate along x with a small yaw and look at a tilted plane; pinhole rays from the intrinsics.
    -> dict(points, local_points f32 (N,H,W,3), poses f32 (N,4,4), fxfycxcy f32 (N,4), depth f64 (N,H,W)).  The maps are
    formed in f64 and rounded once; points = pose . local in f64 of the ROUNDED pose and local points (what a network's
    outputs satisfy up to fp32), with the optional multiplicative depth noise on the local points."""
    rng = np.random.default_rng(seed)
    fx = fy = 0.9 * W
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    n0, d0 = np.array([0.15, -0.1, -1.0]), -3.0            # plane n0 . x = d0, about 3 m in front, tilted
    n0 = n0 / np.linalg.norm(n0)
    poses = np.tile(np.eye(4), (N, 1, 1))
    for i in range(N):
        yaw = 0.02 * (i - (N - 1) / 2.0)
        poses[i, :3, :3] = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        poses[i, :3, 3] = [0.08 * i, 0.01 * i, 0.0]
    poses32 = poses.astype(F)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, float)], -1)          # (H,W,3), z = 1
    local = np.zeros((N, H, W, 3))
    for i in range(N):
        R, t = poses32[i, :3, :3].astype(float), poses32[i, :3, 3].astype(float)
        dw = ray @ R.T
        depth = (d0 - n0 @ t) / (dw @ n0)                                                # along z: local = depth * ray
        local[i] = depth[..., None] * ray
    if noise_rel > 0:
        local = local * (1.0 + noise_rel * rng.standard_normal((N, H, W, 1)))
    local32 = local.astype(F)
    pts = np.einsum("nij,nhwj->nhwi", poses32[:, :3, :3].astype(float), local32.astype(float)) \
        + poses32[:, None, None, :3, 3].astype(float)
    K = np.tile(np.array([fx, fy, cx, cy], F), (N, 1))
    return dict(points=pts.astype(F), local_points=local32, poses=poses32, fxfycxcy=K)


def scale_block(scene: Dict[str, np.ndarray], frame: int, rows: slice, cols: slice, factor: float) -> None:
    """Pull (factor < 1) or push (> 1) a rectangle of one frame along its rays; the world points follow the pose."""
    lp = scene["local_points"]
    lp[frame, rows, cols] = (lp[frame, rows, cols].astype(float) * factor).astype(F)
    R = scene["poses"][frame, :3, :3].astype(float)
    t = scene["poses"][frame, :3, 3].astype(float)
    scene["points"][frame, rows, cols] = (lp[frame, rows, cols].astype(float) @ R.T + t).astype(F)


def inside_count(scene: Dict[str, np.ndarray], radius: int, stride: int, margin: float = 1.0) -> np.ndarray:
    """(N,H,W) int: in how many neighbour views a pixel's point projects at least `margin` pixels inside the image
    (f64 geometry: used with exact data to say which pixels MUST be kept)."""
    P = scene["points"].astype(float)
    N, H, W = P.shape[:3]
    T, K = scene["poses"].astype(float), scene["fxfycxcy"].astype(float)
    cnt = np.zeros((N, H, W), int)
    for s in range(1, radius + 1):
        for sign in (-1, 1):
            for i in range(N):
                j = i + sign * s * stride
                if not 0 <= j < N:
                    continue
                d = (P[i] - T[j, :3, 3]) @ T[j, :3, :3]
                with np.errstate(all="ignore"):
                    u = K[j, 0] * d[..., 0] / d[..., 2] + K[j, 2]
                    v = K[j, 1] * d[..., 1] / d[..., 2] + K[j, 3]
                    cnt[i] += (d[..., 2] > 0) & (u >= margin - 0.5) & (u <= W - 0.5 - margin) & (v >= margin - 0.5) \
                        & (v <= H - 0.5 - margin)
    return cnt
