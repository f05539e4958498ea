"""numpy oracle of the dense map's surface normals (pi3_slam_amd/csrc/voxel_normals.hip).

Same arithmetic, step for step, in f64 / int64 with np.rint (half to even) and np.add.at:

  pixel_normals    candidates under fuse_pixels' predicate; a = P(y,x+1) - P(y,x-1), b = P(y+1,x) - P(y-1,x), n = b x a,
                   l2 = (nx nx + ny ny) + nz nz, q = rint((n / sqrt(l2)) * 2^15); (qx, qy, qz, 1) per contributing pixel
  point_normals    q = w * limit(rint(((r_a0 nx + r_a1 ny) + r_a2 nz) * 2^15), +-2^31), w per row
  accumulate       int64 sums per key
  extract          rows for a list of voxel keys: N / sqrt((Nx Nx + Ny Ny) + Nz Nz) as fp32, min(cnt, 2^31 - 1)
  shade            the camera-frame normal as RGB and the headlight shading per pixel of an index image

Counters as the kernels' stats: [contributions, candidates that could not contribute, degenerate normals, lost].
Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

import dense_map_ref as dm

UNIT = 32768.0
LIMIT = 2147483648.0


def candidates(points, conf, masks, conf_threshold: float, inv_v: float):
    """One chunk's maps (N,H,W,..) -> (cand bool (N,H,W), keys u64 (N,H,W)): fuse_pixels' predicate."""
    p = np.asarray(points, np.float32)
    N, H, W = p.shape[:3]
    sel = np.ones(N * H * W, bool)
    if masks is not None:
        sel &= np.asarray(masks).reshape(-1).astype(bool)
    if conf is not None:
        sel &= np.asarray(conf, np.float32).reshape(-1) > dm.conf_logit(conf_threshold)
    ok, keys, _ = dm.quantise(p.reshape(-1, 3), inv_v)
    return (sel & ok).reshape(N, H, W), keys.reshape(N, H, W)


def full_neighbourhood(cand: np.ndarray) -> np.ndarray:
    """Interior candidates whose four neighbours (y, x +- 1), (y +- 1, x) of the same frame are candidates."""
    full = np.zeros_like(cand)
    if cand.shape[1] >= 3 and cand.shape[2] >= 3:
        full[:, 1:-1, 1:-1] = (cand[:, 1:-1, 1:-1] & cand[:, 1:-1, :-2] & cand[:, 1:-1, 2:] & cand[:, :-2, 1:-1]
                               & cand[:, 2:, 1:-1])
    return full


def pixel_normals(points, conf, masks, conf_threshold: float, inv_v: float) -> Dict[str, np.ndarray]:
    """-> keys u64 (n,), q int64 (n,4) of the contributing pixels, stats int64 (4,), and the per-pixel maps cand / full
    / contributes (N,H,W) for tests that reason about single pixels."""
    p32 = np.asarray(points, np.float32)
    cand, keys = candidates(p32, conf, masks, conf_threshold, inv_v)
    full = full_neighbourhood(cand)
    P = p32.astype(np.float64)
    f, y, x = np.nonzero(full)
    with np.errstate(all="ignore"):
        a = P[f, y, x + 1] - P[f, y, x - 1]
        b = P[f, y + 1, x] - P[f, y - 1, x]
        nx = b[:, 1] * a[:, 2] - b[:, 2] * a[:, 1]
        ny = b[:, 2] * a[:, 0] - b[:, 0] * a[:, 2]
        nz = b[:, 0] * a[:, 1] - b[:, 1] * a[:, 0]
        l2 = (nx * nx + ny * ny) + nz * nz
        good = (l2 > 0.0) & np.isfinite(l2)
        ln = np.sqrt(np.where(good, l2, 1.0))
        q = np.stack([np.rint((c / ln) * UNIT) for c in (nx, ny, nz)], 1)
    q = np.where(good[:, None], q, 0.0).astype(np.int64)
    q = np.concatenate([q, np.ones((len(q), 1), np.int64)], 1)[good]
    contributes = np.zeros_like(cand)
    contributes[f[good], y[good], x[good]] = True
    stats = np.array([int(good.sum()), int(cand.sum() - full.sum()), int((~good).sum()), 0], np.int64)
    return dict(keys=keys[f[good], y[good], x[good]], q=q, stats=stats, cand=cand, full=full, contributes=contributes)


def fixed_component(x: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        r = np.rint(x * UNIT)
    r = np.where(r >= -LIMIT, r, -LIMIT)
    return np.where(r > LIMIT, LIMIT, r).astype(np.int64)


def point_normals(points, normals, nweights, rot9, inv_v: float) -> Dict[str, np.ndarray]:
    """points f32 (n,3) in the world frame, normals f32 (n,3), nweights i32 (n,), rot9 f64 (9,) -> keys, q, stats."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).reshape(-1, 3)
    w = np.asarray(nweights, np.int64).reshape(-1)
    R = np.asarray(rot9, np.float64).reshape(3, 3)
    ok, keys, _ = dm.quantise(p, inv_v)
    has = w > 0
    fine = np.isfinite(nr).all(1) & (nr != 0).any(1)
    sel = has & fine & ok
    n = nr[sel].astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.stack([fixed_component((R[a, 0] * n[:, 0] + R[a, 1] * n[:, 1]) + R[a, 2] * n[:, 2]) for a in range(3)], 1)
    ws = w[sel]
    q = np.concatenate([ws[:, None] * q, ws[:, None]], 1).astype(np.int64)
    stats = np.array([int(sel.sum()), int((has & fine & ~ok).sum()), int((has & ~fine).sum()), 0], np.int64)
    return dict(keys=keys[sel], q=q, stats=stats)


def accumulate(parts: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """Integer sums per key over several pixel_normals / point_normals results; keys ascending."""
    keys = np.concatenate([p["keys"] for p in parts]) if parts else np.zeros(0, np.uint64)
    q = np.concatenate([p["q"] for p in parts]) if parts else np.zeros((0, 4), np.int64)
    uniq, inv = np.unique(keys, return_inverse=True)
    acc = np.zeros((len(uniq), 4), np.int64)
    np.add.at(acc, inv.reshape(-1), q)
    return dict(keys=uniq, acc=acc)


def extract(voxel_keys: np.ndarray, acc: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """One row per key of `voxel_keys` (the map's occupied or kept voxels, ascending): normals f32 (V,3), normal_weights
    i32 (V,).  A voxel without sums gets (0,0,0) and 0."""
    vk = np.asarray(voxel_keys, np.uint64)
    sums = np.zeros((len(vk), 4), np.int64)
    if len(acc["keys"]):
        at = np.searchsorted(acc["keys"], vk)
        at = np.minimum(at, len(acc["keys"]) - 1)
        hit = acc["keys"][at] == vk
        sums[hit] = acc["acc"][at[hit]]
    d = sums[:, :3].astype(np.float64)
    some = (sums[:, 3] != 0) & (sums[:, :3] != 0).any(1)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    nrm = np.where(some[:, None], d / np.where(some, ln, 1.0)[:, None], 0.0).astype(np.float32)
    nw = np.clip(sums[:, 3], 0, 2 ** 31 - 1).astype(np.int32)
    return dict(keys=vk, normals=nrm, normal_weights=nw, nonzero=int(some.sum()))


def to_u8(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.where(v > 0.0, np.where(v >= 255.0, 255.0, v), 0.0).astype(np.uint8)


def shade(index, normals, cams) -> Dict[str, np.ndarray]:
    """index i32 (M,H,W), normals f32 (V,3), cams f64 (M,20) -> normal u8 (M,H,W,3), shaded u8 (M,H,W), pixels."""
    idx = np.asarray(index, np.int64)
    M, H, W = idx.shape
    nr = np.asarray(normals, np.float32).reshape(-1, 3)
    c = np.asarray(cams, np.float64).reshape(M, -1)
    V = len(nr)
    inside = (idx >= 0) & (idx < V)
    n = nr[np.where(inside, idx, 0)] if V else np.zeros((M, H, W, 3), np.float32)
    lit = inside & np.isfinite(n).all(-1) & (n != 0).any(-1)
    n = np.where(lit[..., None], n, 0).astype(np.float64)
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    k = lambda j: c[:, j][:, None, None]       # noqa: E731
    with np.errstate(all="ignore"):
        nc = [(k(4 * a) * x + k(4 * a + 1) * y) + k(4 * a + 2) * z for a in range(3)]
        rgb = np.stack([to_u8(np.rint((v + 1.0) * 127.5)) for v in nc], -1)
        light = -nc[2]
        sh = to_u8(np.rint(255.0 * np.where(light > 0.0, light, 0.0)))
    rgb = np.where(lit[..., None], rgb, 0).astype(np.uint8)
    sh = np.where(lit, sh, 0).astype(np.uint8)
    return dict(normal=rgb, shaded=sh, pixels=int(lit.sum()))


def fuse_pixels_normals(points, conf, masks, conf_threshold: float, voxel_size: float,
                        voxel_keys: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """Stage 1 of one chunk: rows for the cloud's voxels (dense_map_ref.fuse_pixels' keys unless given) + stats."""
    inv_v = dm.inv_voxel(voxel_size)
    part = pixel_normals(points, conf, masks, conf_threshold, inv_v)
    if voxel_keys is None:
        voxel_keys = dm.fuse_pixels(points, conf, masks, None, conf_threshold, voxel_size)["keys"]
    out = extract(voxel_keys, accumulate([part]))
    out["stats"] = part["stats"]
    return out
