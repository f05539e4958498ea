"""numpy oracle of the occupancy grid and the clearance field (pi3_slam_amd/csrc/occupancy.hip), operation for
operation: the f32 voxel quantiser of the mark kernel, the f64 projection of the observe kernel (the carve kernel's,
tests/dense_carve_ref.py), and the windowed, clamped three-pass distance transform.

  grid     cell size c, integer origin (ox, oy, oz), dimensions (nx, ny, nz); arrays are (nz, ny, nx), x fastest;
           state 0 unknown, 1 free, 2 occupied;
  mark     k = floor(fl32(p * inv_c)) per axis, dropped when p is not finite or |k| >= 2^20; i = k - o; state = 2 inside;
  observe  per cell that is not occupied: X = c ((double)(o + i) + 0.5); per view the carver's xc, yc, zc, u, v, pu, pv,
           zo; r = zc - zo, lim = rel_tol zo + margin; r < -lim free, |r| <= lim hit;
           state = 1 when free >= min_free_views and free > hit, else 0; then the unknown cells that hold a view's
           camera centre (floor(-R^T t / c), f64) become free: `freed` of them;
  edt_ref  sites 0, everything else 0xFFFF; per axis x, y, z: out[i] = min over |d| <= R of in[i + d] + d^2, values above
           R^2 clamped to 0xFFFF.
Also the box-room scene of the tests and its geometry.  Test infrastructure only: the product never imports it."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

import dense_carve_ref as carve_ref
import dense_map_ref as mref

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
FAR = 0xFFFF
SCALE_AT = carve_ref.SCALE_AT


def inv_cell(cell: float) -> np.float32:
    return np.float32(1.0 / float(cell))


def point_cells(points, cell: float) -> Tuple[np.ndarray, np.ndarray]:
    """points f32 (P,3) -> (ok (P,), k int64 (P,3)): the quantiser's cell index per axis (0 where not ok)."""
    ok, keys, _ = mref.quantise(points, inv_cell(cell))
    k = np.stack([((keys >> np.uint64(42 - 21 * a)) & np.uint64(0x1FFFFF)).astype(np.int64) - mref.BIAS
                  for a in range(3)], 1)
    return ok, np.where(ok[:, None], k, 0)


def mark(points, cell: float, origin, dims) -> Dict:
    """-> state u8 (nz,ny,nx) with 2 in the cells that hold a point, stats = {marked, dropped, outside}."""
    nx, ny, nz = (int(v) for v in dims)
    ok, k = point_cells(points, cell)
    i = k - np.asarray(origin, np.int64)[None, :]
    inside = ok & (i >= 0).all(1) & (i[:, 0] < nx) & (i[:, 1] < ny) & (i[:, 2] < nz)
    state = np.zeros((nz, ny, nx), np.uint8)
    state[i[inside, 2], i[inside, 1], i[inside, 0]] = OCCUPIED
    return dict(state=state, stats={"marked": int(inside.sum()), "dropped": int((~ok).sum()),
                                    "outside": int((ok & ~inside).sum())})


def cell_centres(cell: float, origin, dims) -> np.ndarray:
    """f64 (nz,ny,nx,3): c ((double)(o + i) + 0.5) per axis."""
    nx, ny, nz = (int(v) for v in dims)
    ax = [float(cell) * ((np.arange(n, dtype=np.int64) + int(o)).astype(np.float64) + 0.5)
          for n, o in zip((nx, ny, nz), origin)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([X, Y, Z], -1)


def observe(state, cell: float, origin, views, planes, stride: int, rel_tol: float, margin: float,
            min_free_views: int) -> Dict:
    """state u8 (nz,ny,nx) (2 = occupied, anything else is decided here) -> state, free / hit uint32 (nz,ny,nx),
    seen uint32 (the views in whose plane the centre projects: oracle only), voted_free bool (free by the vote alone:
    oracle only), stats = {cells, occupied, free, unknown, unvoted, camera_cells_freed}."""
    state = np.asarray(state, np.uint8)
    nz, ny, nx = state.shape
    views = np.asarray(views, np.float64).reshape(-1, 20)
    planes = np.asarray(planes)
    assert planes.dtype == np.float16 and planes.ndim == 3 and len(planes) == len(views)
    Hp, Wp = planes.shape[1:]
    C = cell_centres(cell, origin, (nx, ny, nz)).reshape(-1, 3)
    x, y, z = C[:, 0], C[:, 1], C[:, 2]
    occupied = state.reshape(-1) == OCCUPIED
    free = np.zeros(len(C), np.uint32)
    hit = np.zeros(len(C), np.uint32)
    seen = np.zeros(len(C), np.uint32)
    S, tol, mar = float(stride), float(rel_tol), float(margin)
    for c, plane in zip(views, planes):
        with np.errstate(all="ignore"):
            xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3]
            yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7]
            zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11]
            ok = ~occupied & (zc > 0) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
            u = c[12] * (xc / zc) + c[14]
            v = c[13] * (yc / zc) + c[15]
            pu, pv = np.rint(u / S), np.rint(v / S)
            ok &= (pu >= 0) & (pu <= Wp - 1) & (pv >= 0) & (pv <= Hp - 1)
            seen += ok
            iu = np.where(ok, pu, 0).astype(np.int64)
            iv = np.where(ok, pv, 0).astype(np.int64)
            zo = c[SCALE_AT] * plane[iv, iu].astype(np.float64)
            ok &= (zo != 0) & np.isfinite(zo)
            r = zc - zo
            lim = tol * zo + mar
            h = ok & (np.abs(r) <= lim)
            f = ok & ~h & (r < -lim)
        hit += h
        free += f
    is_free = ~occupied & (free >= np.uint32(min_free_views)) & (free > hit)
    shape = (nz, ny, nx)
    out = np.where(occupied, OCCUPIED, np.where(is_free, FREE, UNKNOWN)).astype(np.uint8).reshape(shape)
    freed = 0
    if len(views):
        with np.errstate(all="ignore"):
            kf = np.floor(view_centres(views) / float(cell))
            kf = kf[(np.abs(kf) < float(1 << 20)).all(1)]                      # NaN falls out
        k = np.unique(kf.astype(np.int64) - np.asarray(origin, np.int64), axis=0).reshape(-1, 3)
        k = k[(k >= 0).all(1) & (k[:, 0] < nx) & (k[:, 1] < ny) & (k[:, 2] < nz)]
        k = k[out[k[:, 2], k[:, 1], k[:, 0]] == UNKNOWN]
        out[k[:, 2], k[:, 1], k[:, 0]] = FREE
        freed = len(k)
    stats = {"cells": len(C), "occupied": int(occupied.sum()), "free": int(is_free.sum()) + freed,
             "unknown": int((~occupied & ~is_free).sum()) - freed, "unvoted": int((~occupied & (free + hit == 0)).sum()),
             "camera_cells_freed": freed}
    return dict(state=out, free=free.reshape(shape), hit=hit.reshape(shape), seen=seen.reshape(shape),
                voted_free=is_free.reshape(shape), stats=stats)


def edt_ref(state, radius: int, unknown_is_obstacle: bool = False) -> np.ndarray:
    """-> d2 uint16 (nz,ny,nx): three passes x, y, z of the windowed minimum, clamped after each."""
    state = np.asarray(state, np.uint8)
    R = int(radius)
    assert state.ndim == 3 and 1 <= R <= 255
    site = state == OCCUPIED
    if unknown_is_obstacle:
        site |= state == UNKNOWN
    g = np.where(site, 0, FAR).astype(np.int64)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (R, R)
        p = np.pad(g, pad, constant_values=FAR)
        best = np.full(g.shape, FAR + R * R + 1, np.int64)
        for d in range(-R, R + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(R + d, R + d + n)
            best = np.minimum(best, p[tuple(sl)] + d * d)
        g = np.where(best > R * R, FAR, best)
    return g.astype(np.uint16)


def clearance(d2, cell: float) -> np.ndarray:
    """float32(cell sqrt(d2)), inf for the far mark."""
    d2 = np.asarray(d2, np.uint16)
    with np.errstate(all="ignore"):
        out = (float(cell) * np.sqrt(d2.astype(np.float64))).astype(np.float32)
    out[d2 == FAR] = np.float32(np.inf)
    return out


def view_centres(views) -> np.ndarray:
    """The camera centres of pack_cameras rows: -R^T t, f64 (M,3)."""
    v = np.asarray(views, np.float64).reshape(-1, 20)
    t0, t1, t2 = v[:, 3:4], v[:, 7:8], v[:, 11:12]
    return -((v[:, 0:3] * t0 + v[:, 4:7] * t1) + v[:, 8:11] * t2)             # the kernel's order of operations


def centre_cells(views, cell: float) -> np.ndarray:
    """int64 (M,3): the cell that holds each camera centre, floor(centre / cell) in f64."""
    return np.floor(view_centres(views) / float(cell)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the box room
ROOM = dict(size=(4.0, 3.0, 2.5), H=48, W=64, f=40.0, n_views=12, ring=0.8, cell=0.1, pad=5,
            rel_tol=0.03, min_free_views=2)


def box_room(cfg=None) -> Dict:
    """A convex room [0, sx] x [0, sy] x [0, sz] seen from n_views cameras on a horizontal circle around its centre,
    alternately looking outwards and across; the depth of a pixel is the analytic ray / box distance along the optical
    axis, rounded to fp16.  -> views f64 (M,20), planes fp16 (M,H,W), points f32 (M H W, 3) (the planes' pixels
    back-projected), cell, origin, dims, margin, size."""
    cfg = dict(ROOM, **(cfg or {}))
    size = np.asarray(cfg["size"], np.float64)
    H, W, f, M = cfg["H"], cfg["W"], cfg["f"], cfg["n_views"]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    mid = size / 2.0
    poses = np.zeros((M, 4, 4))
    for i in range(M):
        phi = 2.0 * np.pi * i / M
        radial = np.array([np.cos(phi), np.sin(phi), 0.0])
        fwd = radial if i % 2 == 0 else -radial          # the camera's z axis
        down = np.array([0.0, 0.0, -1.0])                # its y axis (image rows grow downwards)
        right = np.cross(down, fwd)                      # its x axis
        poses[i, :3, 0], poses[i, :3, 1], poses[i, :3, 2] = right, down, fwd
        poses[i, :3, 3] = mid + cfg["ring"] * radial
        poses[i, 3, 3] = 1.0
    K = np.tile(np.array([f, f, cx, cy]), (M, 1))
    views = carve_ref.pack_views(poses, K, 1.0)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(uu - cx) / f, (vv - cy) / f, np.ones_like(uu)], -1)          # camera frame, z = 1
    planes = np.zeros((M, H, W), np.float16)
    pts = []
    for i in range(M):
        d = rays @ poses[i, :3, :3].T                    # world directions per unit of depth
        o = poses[i, :3, 3]
        with np.errstate(all="ignore"):
            t = np.where(d > 0, (size - o) / d, np.where(d < 0, (0.0 - o) / d, np.inf))
        depth = t.min(-1)
        planes[i] = depth.astype(np.float16)
        pts.append(o + d * planes[i].astype(np.float64)[..., None])
    cell, pad = float(cfg["cell"]), int(cfg["pad"])
    dims = tuple(int(round(s / cell)) + 2 * pad for s in size)
    return dict(views=views, planes=planes, points=np.concatenate([p.reshape(-1, 3) for p in pts]).astype(np.float32),
                cell=cell, origin=(-pad, -pad, -pad), dims=dims, margin=1.0 * cell, size=size, poses=poses,
                rel_tol=cfg["rel_tol"], min_free_views=cfg["min_free_views"])


def wall_distance(room: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """-> (inside bool (nz,ny,nx): the cell's centre lies inside the box; dist f64: its distance to the nearest wall,
    meaningful where inside)."""
    C = cell_centres(room["cell"], room["origin"], room["dims"])
    size = room["size"]
    inside = ((C > 0) & (C < size)).all(-1)
    return inside, np.minimum(C, size - C).min(-1)


def room_invariants(room: Dict, state, free, hit, seen, clear) -> Dict[str, int]:
    """The five conditions a convex room imposes, as counts of violations (all 0 on a correct grid), with the sizes of
    the sets they range over.  clear: the clearance field to the occupied cells, f32, inf beyond its radius."""
    cell = room["cell"]
    inside, dist = wall_distance(room)
    z_max = float(room["planes"].astype(np.float64).max())
    d_min = (room["rel_tol"] * z_max + room["margin"]) / np.cos(np.pi / 4) + cell
    deep_seen = inside & (dist >= d_min) & (seen >= room["min_free_views"])
    cams = centre_cells(room["views"], cell) - np.asarray(room["origin"], np.int64)
    cam_state = state[cams[:, 2], cams[:, 1], cams[:, 0]]
    return {"free_outside": int(((state == FREE) & ~inside).sum()),
            "deep_seen": int(deep_seen.sum()), "deep_seen_not_free": int((deep_seen & (state != FREE)).sum()),
            "cameras": len(cams), "cameras_not_free": int((cam_state != FREE).sum()),
            "occupied_deep": int(((state == OCCUPIED) & inside & (dist > 2.0 * cell)).sum()),
            "clearance_short": int((inside & (clear.astype(np.float64) < dist - (np.sqrt(3.0) / 2.0) * cell)).sum()),
            "z_max": z_max, "d_min": float(d_min)}
