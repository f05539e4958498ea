"""float32 numpy oracle of the dense voxel map (pi3_slam_amd/csrc/voxel.hip, pi3_slam_amd/dense_map.py).

Same arithmetic, step for step: s = p * inv_v (fp32), k = floor(s), u = min(trunc((s - k) * 2^24), 2^24 - 1); keys pack
k + 2^20 at 21 bits per axis; integer sums of w, w u and w rgb per key; centroid v (k + U / (W 2^24)) in f64 -> fp32,
colour (C + W // 2) // W.  Output in ascending key order.  Test infrastructure only: the product never imports it."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

BIAS = 1 << 20
FIX = np.float32(16777216.0)


def conf_logit(thr: float) -> np.float32:
    if thr <= 0.0:
        return np.float32(-np.inf)
    if thr >= 1.0:
        return np.float32(np.inf)
    return np.float32(math.log(thr / (1.0 - thr)))


def quantise(points: np.ndarray, inv_v: float):
    """points f32 (n,3) -> (ok (n,), keys u64 (n,), u u64 (n,3)); ok = finite and |k| < 2^20 on every axis."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = p * np.float32(inv_v)
        k = np.floor(s)
        ok = np.isfinite(p).all(1) & (np.abs(k) < np.float32(BIAS)).all(1)
        uf = (s - k) * FIX
    uf = np.where(ok[:, None], uf, np.float32(0))
    u = np.minimum(uf.astype(np.uint64), np.uint64(0xFFFFFF))
    kb = (np.where(ok[:, None], k, 0).astype(np.int64) + BIAS).astype(np.uint64)
    keys = (kb[:, 0] << np.uint64(42)) | (kb[:, 1] << np.uint64(21)) | kb[:, 2]
    return ok, keys, u


def colour_u8(c: np.ndarray) -> np.ndarray:
    v = np.asarray(c, np.float32) * np.float32(255.0)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 255, 255, np.where(v > 0, np.trunc(np.nan_to_num(v, nan=0.0)), 0)).astype(np.uint64)


def merge(keys: np.ndarray, w: np.ndarray, wu: np.ndarray, wc: np.ndarray) -> Dict[str, np.ndarray]:
    """Integer sums per key (uint64, exact), in ascending key order."""
    if len(keys) == 0:
        return dict(keys=np.zeros(0, np.uint64), W=np.zeros(0, np.uint64), U=np.zeros((0, 3), np.uint64),
                    C=np.zeros((0, 3), np.uint64))
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    return dict(keys=ks[starts], W=np.add.reduceat(w[order], starts), U=np.add.reduceat(wu[order], starts, axis=0),
                C=np.add.reduceat(wc[order], starts, axis=0))


def finalise(acc: Dict[str, np.ndarray], voxel_size: float) -> Dict[str, np.ndarray]:
    keys, W, U, C = acc["keys"], acc["W"], acc["U"], acc["C"]
    k = np.stack([((keys >> np.uint64(42 - 21 * a)) & np.uint64(0x1FFFFF)).astype(np.int64) - BIAS for a in range(3)], 1)
    den = W.astype(np.float64)[:, None] * 16777216.0
    pts = (float(voxel_size) * (k.astype(np.float64) + U.astype(np.float64) / den)).astype(np.float32)
    cols = ((C + W[:, None] // np.uint64(2)) // np.maximum(W[:, None], np.uint64(1))).astype(np.uint8)
    return dict(keys=keys, points=pts.reshape(-1, 3), colors=cols.reshape(-1, 3),
                weights=np.minimum(W, np.uint64(2 ** 31 - 1)).astype(np.int32))


def contributions_pixels(points, conf, masks, imgs, conf_threshold: float, inv_v: float):
    """One chunk's maps -> (keys, w, w u, w rgb, dropped)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    sel = np.ones(n, bool)
    if masks is not None:
        sel &= np.asarray(masks).reshape(-1).astype(bool)
    if conf is not None:
        sel &= np.asarray(conf, np.float32).reshape(-1) > conf_logit(conf_threshold)
    ok, keys, u = quantise(p, inv_v)
    dropped = int(np.sum(sel & ~ok))
    sel &= ok
    if imgs is not None:
        im = np.asarray(imgs, np.float32)
        N, _, H, W = im.shape
        rgb = colour_u8(im.transpose(0, 2, 3, 1).reshape(-1, 3))
    else:
        rgb = np.zeros((n, 3), np.uint64)
    return keys[sel], np.ones(int(sel.sum()), np.uint64), u[sel], rgb[sel], dropped


def contributions_points(points, colors, weights, inv_v: float):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    w = np.ones(len(p), np.int64) if weights is None else np.asarray(weights, np.int64).reshape(-1)
    ok, keys, u = quantise(p, inv_v)
    cand = w > 0
    dropped = int(np.sum(cand & ~ok))
    sel = cand & ok
    wu = w[sel].astype(np.uint64)
    rgb = (np.zeros((len(p), 3), np.uint64) if colors is None
           else np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.uint64))
    return keys[sel], wu, wu[:, None] * u[sel], wu[:, None] * rgb[sel], dropped


def inv_voxel(v: float) -> float:
    return float(np.float32(1.0 / float(v)))


def fuse_pixels(points, conf, masks, imgs, conf_threshold: float, voxel_size: float) -> Dict[str, np.ndarray]:
    keys, w, wu, wc, dropped = contributions_pixels(points, conf, masks, imgs, conf_threshold, inv_voxel(voxel_size))
    out = finalise(merge(keys, w, wu, wc), voxel_size)
    out["dropped"] = dropped
    return out


def fuse_points(points, colors, weights, voxel_size: float) -> Dict[str, np.ndarray]:
    keys, w, wu, wc, dropped = contributions_points(points, colors, weights, inv_voxel(voxel_size))
    out = finalise(merge(keys, w, wu, wc), voxel_size)
    out["dropped"] = dropped
    return out


def fuse_point_sets(sets, voxel_size: float) -> Dict[str, np.ndarray]:
    """Several (points, colors, weights) lists into one table (dense_map.fuse_chunks after the transforms)."""
    parts = [contributions_points(p, c, w, inv_voxel(voxel_size)) for p, c, w in sets]
    if not parts:
        return finalise(merge(np.zeros(0, np.uint64), None, None, None), voxel_size)
    cat = [np.concatenate([q[i] for q in parts]) for i in range(4)]
    return finalise(merge(*cat), voxel_size)


def transformed(points: np.ndarray, M4: Optional[np.ndarray]) -> np.ndarray:
    """Host-side f64 similarity (not bit-identical to the device transform: tests pass device-transformed points)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if M4 is None:
        return p.astype(np.float32)
    M = np.asarray(M4, np.float64).reshape(4, 4)
    return (p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
