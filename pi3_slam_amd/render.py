"""Camera views of the dense voxel map (csrc/render.hip): depth, colour and a top-down overview.

The fused map of dense_map.fuse_chunks is projected into cameras with correct occlusion by a z-buffered splat
renderer on the device: every voxel is drawn as a square of half-width `splat_scale * voxel_size * fx / z` pixels and
each pixel keeps the nearest voxel (64-bit atomicMin of depth bits | row).  The result does not depend on the order in
which the atomics land; tests/render_ref.py reproduces it bit for bit.

  pack_cameras      cam->world poses + intrinsics (index coordinates: pixel i has its centre at i) -> f64 (M,20)
  MapRenderer       uploads a map once, renders batches of cameras -> depth f32 / color u8 / index i32; with the map's
                    normals also normal u8 (camera-frame normal as RGB) / shaded u8 (csrc/voxel_normals.hip)
  overview_camera   an orthographic camera looking along the trajectory's mean image-down axis, framed on the map
  render_overview   the map + the camera centres as red voxels through that camera
  write_depth_png   16-bit PNG in millimetres (0 = empty), write_color_png

Limitation (inherited from the map): a chunk's cloud follows its chunk's similarity, not the per-view
corrections of a bundle adjustment, so with bundle adjustment on a depth image is as misplaced as the map is.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

CAM_DOUBLES = ops.RENDER_CAM_DOUBLES
# z-buffers of the cameras of one launch: a quarter of the 256 MiB Infinity Cache.  More cameras per launch measured
# faster up to all 20 of the chess-room run (20 MiB); the cap only bounds the buffer for long camera lists
ZBUF_BATCH_BYTES = 64 << 20
DEPTH_PNG_SCALE = 1000.0


def _np(x, dtype) -> np.ndarray:
    """A tensor (any device) or an array-like as a host array of `dtype`."""
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype)


def pack_cameras(poses_c2w, K, ortho=False) -> np.ndarray:
    """cam->world poses (M,4,4) (or one (4,4)), K (3,3) or (M,3,3) in index coordinates -> f64 (M,20): world->camera
    3x4 row-major, fx, fy, cx, cy, ortho flag, 3 spare.  A scale in the 3x3 block (a pose that went through a
    similarity) is divided out, so world->camera is rigid and depths are in map units."""
    P = _np(poses_c2w, np.float64).reshape(-1, 4, 4)
    Km = _np(K, np.float64)
    M = P.shape[0]
    Km = np.broadcast_to(Km.reshape(-1, 3, 3), (M, 3, 3))
    A = P[:, :3, :3]
    det = np.linalg.det(A)
    if not np.all(np.isfinite(det)) or np.any(det <= 0.0):
        raise ValueError("pack_cameras: a pose's 3x3 block is not a scaled rotation (determinant <= 0 or not finite)")
    R = A / np.cbrt(det)[:, None, None]
    Rt = np.transpose(R, (0, 2, 1))
    t = -np.einsum("mij,mj->mi", Rt, P[:, :3, 3])
    cams = np.zeros((M, CAM_DOUBLES), np.float64)
    cams[:, :12] = np.concatenate([Rt, t[:, :, None]], axis=2).reshape(M, 12)
    cams[:, 12], cams[:, 13], cams[:, 14], cams[:, 15] = Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2]
    cams[:, 16] = np.broadcast_to(np.asarray(ortho, bool), (M,)).astype(np.float64)
    return cams


def default_batch(M: int, H: int, W: int) -> int:
    """Cameras per launch: as many as keep their z-buffers (8 B per pixel) within ZBUF_BATCH_BYTES, at least one."""
    return max(1, min(int(M), ZBUF_BATCH_BYTES // (8 * int(H) * int(W))))


class MapRenderer:
    """A voxel map on the device (uploaded once) and a z-buffer that is re-used between batches of cameras."""

    def __init__(self, points, colors, weights, voxel_size: float, device="cuda", normals=None):
        v = float(voxel_size)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError(f"voxel size must be a positive finite length, got {voxel_size!r}")
        self.voxel_size = v
        self.device = torch.device(device)
        self.points = torch.as_tensor(points).reshape(-1, 3).to(self.device, torch.float32).contiguous()
        V = int(self.points.shape[0])
        if V >= 1 << 31:
            raise ValueError("a voxel's row index must fit 32 bits")
        self.colors = (torch.zeros(V, 3, dtype=torch.uint8, device=self.device) if colors is None
                       else torch.as_tensor(colors).reshape(-1, 3).to(self.device, torch.uint8).contiguous())
        self.weights = (None if weights is None
                        else torch.as_tensor(weights).reshape(-1).to(self.device, torch.int32).contiguous())
        if int(self.colors.shape[0]) != V or (self.weights is not None and int(self.weights.shape[0]) != V):
            raise ValueError("points, colors and weights must have one row per voxel")
        # world-frame unit normals f32 (V,3), (0,0,0) = none: render() then also shades (pi3_render_shade)
        self.normals = (None if normals is None
                        else torch.as_tensor(normals).reshape(-1, 3).to(self.device, torch.float32).contiguous())
        if self.normals is not None and int(self.normals.shape[0]) != V:
            raise ValueError("normals must have one row per voxel")
        self.shade_stats = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._zbuf: Optional[torch.Tensor] = None
        self.last_stats: Dict[str, int] = {}

    def render(self, cams, H: int, W: int, min_weight: int = 1, splat_scale: float = 1.0, near: float = 0.05,
               far: float = float("inf"), batch: Optional[int] = None, to_host: bool = True) -> Dict[str, torch.Tensor]:
        """cams f64 (M,20) (pack_cameras) -> {'depth' f32 (M,H,W), 0 = empty; 'color' u8 (M,H,W,3); 'index' i32
        (M,H,W), the voxel's row or -1}, on the host (to_host) or on the device.  Sets last_stats.  A renderer with
        normals adds 'normal' u8 (M,H,W,3) = the camera-frame normal, (n + 1) * 127.5, and 'shaded' u8 (M,H,W) =
        255 max(0, -n_z), a headlight along the optical axis; both 0 where empty, and last_stats['shaded'] pixels."""
        cams = torch.as_tensor(cams, dtype=torch.float64).reshape(-1, CAM_DOUBLES)
        M, H, W = int(cams.shape[0]), int(H), int(W)
        if M == 0:
            raise ValueError("no camera to render")
        batch = default_batch(M, H, W) if batch is None else max(1, min(int(batch), M))
        cams_dev = cams.to(self.device).contiguous()
        if self._zbuf is None or self._zbuf.numel() < batch * H * W:
            self._zbuf = None
            self._zbuf = torch.empty(batch * H * W, dtype=torch.int64, device=self.device)
        depth = torch.empty(M, H, W, dtype=torch.float32, device=self.device)
        color = torch.empty(M, H, W, 3, dtype=torch.uint8, device=self.device)
        index = torch.empty(M, H, W, dtype=torch.int32, device=self.device)
        nrgb = shaded = None
        if self.normals is not None:
            nrgb = torch.empty(M, H, W, 3, dtype=torch.uint8, device=self.device)
            shaded = torch.empty(M, H, W, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self.stats.zero_()
            self.shade_stats.zero_()
            for a in range(0, M, batch):
                b = min(M, a + batch)
                ops.render_splat(self.points, self.weights, cams_dev[a:b], self._zbuf, self.stats, H, W, self.voxel_size,
                                 splat_scale, min_weight, near, far)
                ops.render_resolve(self._zbuf, self.colors, self.stats, b - a, H, W,
                                   out=(depth[a:b], color[a:b], index[a:b]))
                if self.normals is not None:
                    ops.render_shade(index[a:b], self.normals, cams_dev[a:b], self.shade_stats,
                                     out=(nrgb[a:b], shaded[a:b]))
            st = self.stats.cpu().numpy()
        self.last_stats = {"culled": int(st[0]), "clamped": int(st[1]), "pixels": int(st[2]), "atomics": int(st[3])}
        out = {"depth": depth, "color": color, "index": index}
        if self.normals is not None:
            self.last_stats["shaded"] = int(self.shade_stats.cpu()[0])
            out["normal"], out["shaded"] = nrgb, shaded
        return {k: t.cpu() for k, t in out.items()} if to_host else out


def overview_camera(poses_c2w, points, H: int, W: int, near: float = 0.05, margin: float = 0.05,
                    border_px: float = 4.0) -> Tuple[np.ndarray, np.ndarray]:
    """An orthographic camera for a floor plan: -> (cam->world pose (4,4), K (3,3): fx = fy = pixels per map unit).

    The world frame is chunk 0's camera frame, so there is no gravity vector; the mean image-down (camera y) axis of the
    trajectory is the nearest thing to 'down' and becomes the view axis.  The frame is the 1st-99th percentile box of
    the map in the image plane, widened to hold every camera centre, at one scale for both axes.  Seen from above, a
    room shows its ceiling first: the camera sits so that its `near` plane lies `margin` above the highest camera
    centre, which cuts away everything over the trajectory (render with the same `near`)."""
    P = _np(poses_c2w, np.float64).reshape(-1, 4, 4)
    X = _np(points, np.float64).reshape(-1, 3)
    X = X[np.isfinite(X).all(1)]
    C = P[:, :3, 3]
    down = P[:, :3, 1] / np.maximum(np.linalg.norm(P[:, :3, 1], axis=1, keepdims=True), 1e-300)
    z = down.mean(0)
    if not np.linalg.norm(z) > 1e-6:          # cameras that roll all the way round: fall back on the first one
        z = down[0]
    z = z / np.linalg.norm(z)
    e = np.eye(3)[int(np.argmin(np.abs(z)))]  # the world axis most perpendicular to the view axis -> image x
    x = e - z * float(e @ z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)           # columns: the camera's axes in the world
    lat = X @ R[:, :2] if len(X) else C @ R[:, :2]
    lo, hi = np.percentile(lat, 1.0, axis=0), np.percentile(lat, 99.0, axis=0)
    cl = C @ R[:, :2]
    lo, hi = np.minimum(lo, cl.min(0)), np.maximum(hi, cl.max(0))
    span = np.maximum(hi - lo, 1e-6)
    f = float(min((W - 1 - 2 * border_px) / span[0], (H - 1 - 2 * border_px) / span[1]))
    mid = 0.5 * (lo + hi)
    depth0 = float((C @ z).min()) - (float(near) + float(margin))
    pose = np.eye(4)
    pose[:3, :3] = R
    pose[:3, 3] = R[:, 0] * mid[0] + R[:, 1] * mid[1] + z * depth0
    K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    return pose, K


def render_overview(points, colors, weights, voxel_size: float, poses_c2w, H: int, W: int, min_weight: int = 1,
                    splat_scale: float = 1.0, near: float = 0.05, device="cuda", normals=None) -> Dict:
    """The map seen through overview_camera, with the camera centres appended as red voxels of weight `min_weight` (so
    the trajectory is drawn by the same kernel) -> {'color' u8 (H,W,3), 'depth', 'index', 'pose', 'K', 'near'}.
    normals (V,3): also 'shaded' u8 (H,W,3), the headlight shading in grey with the trajectory painted red (the camera
    centres have no normal)."""
    P = _np(poses_c2w, np.float64).reshape(-1, 4, 4)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    pose, K = overview_camera(P, pts, H, W, near=near)
    n = len(P)
    cols = np.zeros((len(pts), 3), np.uint8) if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3)
    w = np.ones(len(pts), np.int32) if weights is None else np.asarray(weights, np.int32).reshape(-1)
    red = np.tile(np.array([[255, 0, 0]], np.uint8), (n, 1))
    nrm = None if normals is None else np.concatenate(
        [np.asarray(normals, np.float32).reshape(-1, 3), np.zeros((n, 3), np.float32)], 0)
    r = MapRenderer(np.concatenate([pts, P[:, :3, 3].astype(np.float32)], 0), np.concatenate([cols, red], 0),
                    np.concatenate([w, np.full(n, int(min_weight), np.int32)], 0), voxel_size, device, normals=nrm)
    out = r.render(pack_cameras(pose[None], K, ortho=True), H, W, min_weight=min_weight, splat_scale=splat_scale,
                   near=near)
    res = {"color": out["color"][0], "depth": out["depth"][0], "index": out["index"][0], "pose": pose, "K": K,
           "near": float(near), "stats": r.last_stats}
    if nrm is not None:
        grey = out["shaded"][0].numpy()
        img = np.repeat(grey[:, :, None], 3, axis=2)
        img[out["index"][0].numpy() >= len(pts)] = (255, 0, 0)
        res["shaded"] = torch.from_numpy(img)
    return res


def depth_to_u16(depth, scale: float = DEPTH_PNG_SCALE) -> np.ndarray:
    """depth (H,W) in map units -> uint16 of round(depth * scale) (half to even, f64), saturating at 65535; empty
    pixels (0, or not finite) stay 0."""
    d = _np(depth, np.float64)
    d = np.where(np.isfinite(d) & (d > 0.0), d, 0.0)
    return np.minimum(np.rint(d * float(scale)), 65535.0).astype(np.uint16)


def write_depth_png(depth, path: str, scale: float = DEPTH_PNG_SCALE) -> None:
    """16-bit greyscale PNG: depth * scale (millimetres for metric maps), 0 = empty, 65535 = that far or farther."""
    from PIL import Image
    Image.fromarray(depth_to_u16(depth, scale).astype("<u2")).save(path, format="PNG")


def write_grey_png(grey, path: str) -> None:
    """8-bit greyscale PNG of a uint8 (H,W) image."""
    from PIL import Image
    g = _np(grey, np.uint8)
    Image.fromarray(np.ascontiguousarray(g.reshape(g.shape[0], g.shape[1]))).save(path, format="PNG")


def write_color_png(color, path: str) -> None:
    from PIL import Image
    c = _np(color, np.uint8)
    Image.fromarray(np.ascontiguousarray(c.reshape(c.shape[0], c.shape[1], 3))).save(path, format="PNG")
