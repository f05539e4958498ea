"""Tensor-level wrappers over the C-ABI (one Python function per entry point of include/pi3slam_hip.h).

Each wrapper only validates shapes/dtypes, allocates the output through torch's allocator and forwards raw device
pointers + the current stream.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import lib as _L

BF16, F32, F16 = 0, 1, 2
_16BIT = (torch.bfloat16, torch.float16)
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
QSCALE = 0.125 * math.log2(math.e)  # head_dim^-0.5 * log2(e), folded into q (attn.hip works in the exp2 domain)


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:       # IEEE half: the MoGe path (the reference runs it under fp16 autocast)
        return F16
    raise _L.Pi3HipError(f"unsupported dtype {t.dtype}")


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, M: Optional[int] = None, K: Optional[int] = None,
         bias: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None,
         resid: Optional[torch.Tensor] = None, act: int = ACT_NONE, rpg: int = 0, gstride: int = 0, goff: int = 0,
         addtab: Optional[torch.Tensor] = None, qscale: float = 1.0, qcols: int = 0) -> torch.Tensor:
    """out[orow(m), :N] = resid + gamma * act((a[m] . w^T + bias) * qscale[n < qcols]) + addtab[m % rpg].

    a: [>=M, lda] (bf16 or f32), w: [N, ldw] same dtype, out: 2-D bf16/f32 with row stride out.stride(0).
    """
    lib = _L.load()
    assert a.dim() == 2 and w.dim() == 2 and out.dim() == 2 and a.dtype == w.dtype
    assert a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    M = a.shape[0] if M is None else M
    K = w.shape[1] if K is None else K
    N = w.shape[0]
    rc = lib.pi3_gemm(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), M, N, K, _dt(a),
                      _L.ptr(bias), _L.ptr(gamma), _L.ptr(resid), resid.stride(0) if resid is not None else 0,
                      out.data_ptr(), out.stride(0), _dt(out), act, rpg, gstride, goff,
                      _L.ptr(addtab), addtab.stride(0) if addtab is not None else 0, float(qscale), int(qcols),
                      _L.stream_ptr())
    _L.check(rc, "pi3_gemm")
    return out


def gemm_qkv(a: torch.Tensor, w: torch.Tensor, qkv: torch.Tensor, *, M: int, H: int, bias: Optional[torch.Tensor],
             T: int, pos: Optional[torch.Tensor] = None, cs: Optional[torch.Tensor] = None, qw=None, qb=None, kw=None,
             kb=None, eps: float = 1e-5, qscale: float = QSCALE, k2max: Optional[torch.Tensor] = None,
             attn_B: int = 0, attn_S: int = 0) -> torch.Tensor:
    """qkv projection + per-head q/k LayerNorm(64) + RoPE-2D + softmax-scale fold (+ max |k|^2 per (batch, head) into
    k2max) in one launch where the 256x256 kernel applies, else projection + the stand-alone passes."""
    lib = _L.load()
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and qkv.dtype == torch.bfloat16
    assert a.stride(1) == 1 and w.stride(1) == 1 and qkv.is_contiguous() and qkv.shape[1] == 3 * H * 64
    assert w.shape[0] == 3 * H * 64
    if pos is not None:
        assert pos.dtype == torch.int32 and pos.is_contiguous() and cs is not None
    rc = lib.pi3_gemm_qkv(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), M, w.shape[1], H, _L.ptr(bias),
                          qkv.data_ptr(), qkv.stride(0), T, _L.ptr(pos), _L.ptr(cs) if pos is not None else None,
                          _L.ptr(qw), _L.ptr(qb), _L.ptr(kw), _L.ptr(kb), float(eps), float(qscale), _L.ptr(k2max),
                          attn_B, attn_S, _L.stream_ptr())
    _L.check(rc, "pi3_gemm_qkv")
    return qkv


def attention(qkv: torch.Tensor, out: torch.Tensor, B: int, S: int, H: int,
              k2max: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv: packed [B*S, 3*H*64] bf16 (q pre-scaled by QSCALE); out: [B*S, H*64] bf16.
    k2max: f32 [B*H] already holding max_s |k|^2 per (batch, head) (written by the fused qkv epilogue); None -> a
    workspace is taken from torch's allocator and the call fills it with its own pre-pass."""
    lib = _L.load()
    assert qkv.dtype in _16BIT and out.dtype == qkv.dtype and qkv.dim() == 2 and out.dim() == 2
    assert qkv.shape[0] >= B * S and qkv.shape[1] == 3 * H * 64 and qkv.stride(1) == 1 and out.stride(1) == 1
    ts = qkv.stride(0)
    base = qkv.data_ptr()
    ready = 1
    if k2max is None:
        ready = 0
        k2max = torch.empty(B * H, device=qkv.device, dtype=torch.float32) \
            if S >= 4096 and qkv.dtype == torch.bfloat16 else None
    else:
        assert k2max.dtype == torch.float32 and k2max.numel() >= B * H and k2max.is_contiguous()
    rc = lib.pi3_attention(base, base + 2 * H * 64, base + 4 * H * 64, ts, S * ts, out.data_ptr(), out.stride(0),
                           S * out.stride(0), B, S, H, 64, _dt(qkv), _L.ptr(k2max), ready, _L.stream_ptr())
    _L.check(rc, "pi3_attention")
    return out


def attention_path_counters(counters: Optional[torch.Tensor]) -> None:
    """Register (or, with None, remove) the diagnostic counter block of pi3_attention's 64-row kernel: int32 [2, 2, 32]
    on the device, zeroed by the caller = [eight-wave (global) | four-wave (frame-wise)] x [bounded-score loop |
    online-max loop] x 32 slots; `counters.sum(-1)` are waves.  Synchronise before changing it."""
    lib = _L.load()
    if counters is not None:
        assert counters.is_cuda and counters.dtype == torch.int32 and counters.numel() == 128 and counters.is_contiguous()
    _L.check(lib.pi3_attention_path_counters(_L.ptr(counters)), "pi3_attention_path_counters")


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor, eps: float = 1e-6, *,
              rows: Optional[int] = None, T: int = 0, nspecial: int = 0,
              special: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _L.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and out.stride(1) == 1
    rows = x.shape[0] if rows is None else rows
    rc = lib.pi3_layernorm(x.data_ptr(), x.stride(0), rows, x.shape[1], w.data_ptr(), b.data_ptr(), float(eps),
                           out.data_ptr(), out.stride(0), _dt(out), T, nspecial, _L.ptr(special), _L.stream_ptr())
    _L.check(rc, "pi3_layernorm")
    return out


def qknorm_rope(qkv: torch.Tensor, rows: int, H: int, T: int, pos: Optional[torch.Tensor],
                cs: Optional[torch.Tensor], qw=None, qb=None, kw=None, kb=None, eps: float = 1e-6,
                qscale: float = QSCALE, do_rope: bool = True) -> torch.Tensor:
    lib = _L.load()
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.shape[1] == 3 * H * 64
    if pos is not None:
        assert pos.dtype == torch.int32 and pos.is_contiguous()
    rc = lib.pi3_qknorm_rope(qkv.data_ptr(), rows, H, T, _L.ptr(pos), _L.ptr(cs), _L.ptr(qw), _L.ptr(qb),
                             _L.ptr(kw), _L.ptr(kb), float(eps), float(qscale), int(do_rope), _L.stream_ptr())
    _L.check(rc, "pi3_qknorm_rope")
    return qkv


_ROPE_DT = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}


def rope_2d(tokens: torch.Tensor, positions: torch.Tensor, base: float, fwd: float) -> None:
    """`curope.rope_2d(tokens, positions, base, fwd)` (pi3/models/curope/curope.cpp:49-68): IN PLACE on tokens
    (B, N, H, D) - any strides with the last dim contiguous - with positions (B, N, 2) int64 = (y, x).  The argument
    checks and their messages are the reference's TORCH_CHECKs (curope.cpp:54-59, kernels.cu:11-14, 91-94), raised as
    RuntimeError like a failing TORCH_CHECK is; one is relaxed: kernels.cu:91 also wants stride(2) == D, which the
    transposed view `cuRoPE2D.forward` makes of a contiguous (B, heads, N, D) tensor does not have."""
    lib = _L.load()
    if tokens.dim() != 4:
        raise RuntimeError("tokens must have 4 dimensions")
    if positions.dim() != 3:
        raise RuntimeError("positions must have 3 dimensions")
    if tokens.size(0) != positions.size(0):
        raise RuntimeError("batch size differs between tokens & positions")
    if tokens.size(1) != positions.size(1):
        raise RuntimeError("seq_length differs between tokens & positions")
    if positions.size(2) != 2:
        raise RuntimeError("positions.shape[2] must be equal to 2")
    if tokens.is_cuda != positions.is_cuda:
        raise RuntimeError("tokens and positions are not on the same device")
    if not tokens.is_cuda:
        raise _L.Pi3HipError("pi3_rope_2d runs on the GPU only (the reference's rope_2d_cpu is restated in oracle/)")
    B, N, H, D = tokens.shape
    if tokens.stride(3) != 1:
        raise RuntimeError("tokens are not contiguous")
    if not positions.is_contiguous():
        raise RuntimeError("positions are not contiguous")
    if D % 4 != 0:
        raise RuntimeError("token dim must be multiple of 4")
    if tokens.dtype not in _ROPE_DT or positions.dtype != torch.int64:
        raise RuntimeError(f"rope_2d: unsupported dtypes {tokens.dtype} / {positions.dtype}")
    rc = lib.pi3_rope_2d(tokens.data_ptr(), positions.data_ptr(), B, N, H, D, tokens.stride(0), tokens.stride(1),
                         tokens.stride(2), float(base), float(fwd), _ROPE_DT[tokens.dtype], _L.stream_ptr())
    _L.check(rc, "pi3_rope_2d")


class cuRoPE2D(torch.nn.Module):
    """Drop-in for `models.curope.cuRoPE2D` (pi3/models/curope/curope2d.py:33-40; selected by pos_embed.py:104-106 when
    the extension is importable): forward(tokens (B, heads, ntokens, dim), positions (B, ntokens, 2)) rotates `tokens` in
    place through the transposed view and returns it.  Inference only (the reference's autograd wrapper calls the same
    entry with fwd = -F0 for the backward pass; `rope_2d(..., -F0)` is available for that)."""

    def __init__(self, freq: float = 100.0, F0: float = 1.0):
        super().__init__()
        self.base = freq
        self.F0 = F0

    def forward(self, tokens: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        rope_2d(tokens.transpose(1, 2), positions, self.base, self.F0)
        return tokens


def cast_rows(x: torch.Tensor, out: torch.Tensor, rows: Optional[int] = None, cols: Optional[int] = None,
              in_cols: Optional[int] = None):
    """out[r, :cols] = x[r, :cols]; with in_cols < cols only x[r, :in_cols] is read and out[r, in_cols:cols] = 0."""
    lib = _L.load()
    assert x.dtype == torch.float32 and x.stride(1) == 1 and out.stride(1) == 1
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    in_cols = cols if in_cols is None else in_cols
    assert in_cols <= x.shape[1] and cols <= out.shape[1]
    rc = lib.pi3_cast_rows_pad(x.data_ptr(), x.stride(0), in_cols, out.data_ptr(), out.stride(0), rows, cols, _dt(out),
                               _L.stream_ptr())
    _L.check(rc, "pi3_cast_rows")
    return out


def patch_gather(imgs: torch.Tensor, out: torch.Tensor, mean, std) -> torch.Tensor:
    """imgs: [F, 3, H, W] f32 -> out: [F*P, KP] bf16 normalised patch rows."""
    lib = _L.load()
    assert imgs.dtype == torch.float32 and imgs.is_contiguous() and out.dtype in _16BIT and out.is_contiguous()
    F, _, H, W = imgs.shape
    m3 = (C.c_float * 3)(*[float(v) for v in mean])
    s3 = (C.c_float * 3)(*[float(v) for v in std])
    rc = lib.pi3_patch_gather(imgs.data_ptr(), F, H, W, out.data_ptr(), out.shape[1], _dt(out), m3, s3, _L.stream_ptr())
    _L.check(rc, "pi3_patch_gather")
    return out


def resample_grid(src: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor) -> torch.Tensor:
    """src [Mi, Mj, D] f32, wy [oh, Mi], wx [ow, Mj] -> [oh, ow, D]."""
    lib = _L.load()
    Mi, Mj, D = src.shape
    oh, ow = wy.shape[0], wx.shape[0]
    dst = torch.empty(oh, ow, D, device=src.device, dtype=torch.float32)
    rc = lib.pi3_resample_grid(src.data_ptr(), Mi, Mj, D, wy.data_ptr(), wx.data_ptr(), oh, ow, dst.data_ptr(),
                               _L.stream_ptr())
    _L.check(rc, "pi3_resample_grid")
    return dst


def fill_tokens(x: torch.Tensor, F: int, T: int, t0: int, vals: torch.Tensor) -> None:
    lib = _L.load()
    assert x.dtype == torch.float32 and vals.dtype == torch.float32 and vals.is_contiguous()
    rc = lib.pi3_fill_tokens(x.data_ptr(), F, T, x.shape[1], t0, vals.shape[0], vals.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_fill_tokens")


def recipe_fill(out: torch.Tensor, seed: int, offset: float, scale: float) -> torch.Tensor:
    lib = _L.load()
    assert out.is_contiguous() and out.dtype != torch.float16      # bf16 / f32 only (half weights: fill f32, then .half())
    rc = lib.pi3_recipe_fill(out.data_ptr(), out.numel(), C.c_ulonglong(seed), float(offset), float(scale), _dt(out),
                             _L.stream_ptr())
    _L.check(rc, "pi3_recipe_fill")
    return out


def unpatchify_points(pfeat: torch.Tensor, cfeat: torch.Tensor, poses: torch.Tensor, F: int, H: int, W: int, T: int,
                      tok_off: int, local_points: torch.Tensor, points: torch.Tensor, conf: torch.Tensor) -> None:
    lib = _L.load()
    for t in (pfeat, cfeat, poses, local_points, points, conf):
        assert t.dtype == torch.float32
    assert poses.is_contiguous() and local_points.is_contiguous() and points.is_contiguous() and conf.is_contiguous()
    rc = lib.pi3_unpatchify_points(pfeat.data_ptr(), pfeat.stride(0), cfeat.data_ptr(), cfeat.stride(0),
                                   poses.data_ptr(), F, H, W, T, tok_off, local_points.data_ptr(), points.data_ptr(),
                                   conf.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_unpatchify_points")


def camera_tail(feat: torch.Tensor, T: int, tok_off: int, F: int, P: int, w: dict, poses: torch.Tensor) -> None:
    """feat: [F*T, C] fp32 (output of the ResConv blocks); patch tokens start at row tok_off of each frame."""
    lib = _L.load()
    assert feat.dtype == torch.float32 and feat.stride(1) == 1 and poses.is_contiguous()
    ld = feat.stride(0)
    base = feat.data_ptr() + tok_off * ld * 4
    g = lambda n: w[n].data_ptr()
    rc = lib.pi3_camera_tail(base, ld, T * ld, F, P, feat.shape[1],
                             g("camera_head.more_mlps.0.weight"), g("camera_head.more_mlps.0.bias"),
                             g("camera_head.more_mlps.2.weight"), g("camera_head.more_mlps.2.bias"),
                             g("camera_head.fc_t.weight"), g("camera_head.fc_t.bias"),
                             g("camera_head.fc_rot.weight"), g("camera_head.fc_rot.bias"),
                             poses.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_camera_tail")


# ----------------------------------------------------------------------------------------------- post-processing
def compute_masks(conf: torch.Tensor, local_points: torch.Tensor, conf_thr: float = 0.1,
                  rtol: float = 0.03) -> torch.Tensor:
    """conf [F,H,W,1] or [F,H,W], local_points [F,H,W,3] (f32, contiguous) -> uint8 mask [F,H,W]."""
    lib = _L.load()
    F, H, W = local_points.shape[:3]
    assert conf.is_contiguous() and local_points.is_contiguous() and conf.numel() == F * H * W
    out = torch.empty(F, H, W, device=conf.device, dtype=torch.uint8)
    rc = lib.pi3_compute_masks(conf.data_ptr(), local_points.data_ptr(), F, H, W, float(conf_thr), float(rtol),
                               out.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_compute_masks")
    return out


def masked_ratio_median(num: torch.Tensor, den: torch.Tensor, den_stride: int, mask: torch.Tensor,
                        n: int) -> torch.Tensor:
    """-> device tensor [median, count] (f32).  den is addressed as den_ptr[i * den_stride]; mask uint8/bool."""
    lib = _L.load()
    assert num.dtype == torch.float32 and den.dtype == torch.float32 and mask.dtype in (torch.uint8, torch.bool)
    out = torch.empty(2, device=num.device, dtype=torch.float32)
    rc = lib.pi3_masked_ratio_median(num.data_ptr(), den.data_ptr(), den_stride, mask.data_ptr(), n, out.data_ptr(),
                                     _L.stream_ptr())
    _L.check(rc, "pi3_masked_ratio_median")
    return out


def apply_scale(scale_dev: torch.Tensor, local_points: torch.Tensor, points: torch.Tensor,
                poses: torch.Tensor) -> None:
    lib = _L.load()
    assert local_points.is_contiguous() and points.is_contiguous() and poses.is_contiguous()
    F = poses.numel() // 16
    rc = lib.pi3_apply_scale(scale_dev.data_ptr(), local_points.data_ptr(), points.data_ptr(), local_points.numel(),
                             poses.data_ptr(), F, _L.stream_ptr())
    _L.check(rc, "pi3_apply_scale")


def gather_keypoints(points, local_points, conf, masks, images, keypoints):
    """Dense maps [F,H,W,*] (masks uint8/bool) + keypoints f32 [F,K,2] -> dict of packed per-keypoint tensors
    (fp16 / bool)."""
    lib = _L.load()
    F, H, W = points.shape[:3]
    K = keypoints.shape[1]
    dev = points.device
    for t in (points, local_points, conf, masks, keypoints):
        assert t.is_contiguous()
    assert keypoints.dtype == torch.float32 and masks.dtype in (torch.uint8, torch.bool)
    o_points = torch.empty(F, K, 3, device=dev, dtype=torch.float16)
    o_local = torch.empty(F, K, 3, device=dev, dtype=torch.float16)
    o_conf = torch.empty(F, K, 1, device=dev, dtype=torch.float16)
    o_mask = torch.empty(F, K, 1, device=dev, dtype=torch.uint8)
    o_kps = torch.empty(F, K, 2, device=dev, dtype=torch.float16)
    o_colors = torch.empty(F, K, 3, device=dev, dtype=torch.float16) if images is not None else None
    if images is not None:
        assert images.is_contiguous() and images.dtype == torch.float32 and tuple(images.shape) == (F, 3, H, W)
    rc = lib.pi3_gather_keypoints(points.data_ptr(), local_points.data_ptr(), conf.data_ptr(), masks.data_ptr(),
                                  _L.ptr(images), keypoints.data_ptr(), F, H, W, K, o_points.data_ptr(),
                                  o_local.data_ptr(), o_conf.data_ptr(), o_mask.data_ptr(), _L.ptr(o_colors),
                                  o_kps.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_gather_keypoints")
    return dict(points=o_points, local_points=o_local, conf=o_conf, masks=o_mask.bool(), colors=o_colors,
                keypoints=o_kps)


# ----------------------------------------------------------------------------------------------- Sim(3) alignment
def sim3_match_keypoints(kp_ref: torch.Tensor, kp_qry: torch.Tensor) -> torch.Tensor:
    """kp_*: f16 [ov, K, 2] -> int32 [ov, K] (index into the ref view's keypoints or -1)."""
    lib = _L.load()
    assert kp_ref.dtype == torch.float16 and kp_qry.dtype == torch.float16 and kp_ref.shape == kp_qry.shape
    kp_ref, kp_qry = kp_ref.contiguous(), kp_qry.contiguous()
    ov, K = kp_ref.shape[:2]
    idx = torch.empty(ov, K, device=kp_ref.device, dtype=torch.int32)
    rc = lib.pi3_sim3_match_keypoints(kp_ref.data_ptr(), kp_qry.data_ptr(), ov, K, idx.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_sim3_match_keypoints")
    return idx


def sim3_umeyama(pts_ref: torch.Tensor, pts_qry: torch.Tensor, idx: torch.Tensor, last_ref_pose: torch.Tensor,
                 w_ref: Optional[torch.Tensor] = None, w_qry: Optional[torch.Tensor] = None,
                 use_filter: bool = True) -> torch.Tensor:
    """-> f64 device tensor [33]: s, R(9), t(3), M(16), n_used, n_common, median, rms.
    w_ref / w_qry [ov, K]: uint8 validity (a pair takes part or not) or float32 weights (the weighted Umeyama:
    pair weight = w_ref[ref track] * w_qry[qry keypoint]); both of one kind."""
    lib = _L.load()
    assert pts_ref.dtype == pts_qry.dtype and pts_ref.dtype in (torch.float16, torch.float32) and idx.dtype == torch.int32
    pts_ref, pts_qry, idx = pts_ref.contiguous(), pts_qry.contiguous(), idx.contiguous()
    flags = int(bool(use_filter)) | (2 if pts_ref.dtype == torch.float32 else 0)
    assert last_ref_pose.dtype == torch.float32
    last_ref_pose = last_ref_pose.contiguous()
    ov, K = idx.shape
    assert pts_ref.numel() == pts_qry.numel() == ov * K * 3
    kinds = {w.dtype for w in (w_ref, w_qry) if w is not None}
    assert kinds <= {torch.uint8} or kinds <= {torch.float32}, "w_ref / w_qry: both uint8 validity or both float32 weights"
    for w in (w_ref, w_qry):
        assert w is None or (w.is_contiguous() and w.numel() == ov * K and w.device == idx.device)
    out = torch.empty(33, device=idx.device, dtype=torch.float64)
    fn, name = ((lib.pi3_sim3_umeyama_weighted, "pi3_sim3_umeyama_weighted") if torch.float32 in kinds
                else (lib.pi3_sim3_umeyama, "pi3_sim3_umeyama"))
    rc = fn(pts_ref.data_ptr(), pts_qry.data_ptr(), idx.data_ptr(), _L.ptr(w_ref), _L.ptr(w_qry),
            ov, K, last_ref_pose.data_ptr(), flags, out.data_ptr(), _L.stream_ptr())
    _L.check(rc, name)
    return out


def sim3_apply(M4: torch.Tensor, pts: Optional[torch.Tensor], poses: Optional[torch.Tensor]) -> None:
    lib = _L.load()
    assert M4.dtype == torch.float64 and M4.numel() >= 16
    n = 0 if pts is None else pts.numel() // 3
    F = 0 if poses is None else poses.numel() // 16
    rc = lib.pi3_sim3_apply(M4.data_ptr(), _L.ptr(pts), n, _L.ptr(poses), F, _L.stream_ptr())
    _L.check(rc, "pi3_sim3_apply")


def sim3_compose_prefix(T: torch.Tensor) -> torch.Tensor:
    lib = _L.load()
    assert T.dtype == torch.float64 and T.is_contiguous()
    n = T.numel() // 16
    G = torch.empty_like(T)
    rc = lib.pi3_sim3_compose_prefix(T.data_ptr(), G.data_ptr(), n, _L.stream_ptr())
    _L.check(rc, "pi3_sim3_compose_prefix")
    return G


def focal_shift(local_points: torch.Tensor, conf: Optional[torch.Tensor], uvx: torch.Tensor, uvy: torch.Tensor,
                conf_thr: float = 0.1, mask: Optional[torch.Tensor] = None):
    """local_points [F,H,W,3], conf [F,H,W,(1)] f32 (or mask uint8 [F,H,W]) -> dict(focal [F], shift [F],
    fxfycxcy [F,4], intrinsics [F,3,3])."""
    lib = _L.load()
    F, H, W = local_points.shape[:3]
    assert local_points.is_contiguous() and uvx.numel() == W and uvy.numel() == H
    assert (conf is not None and conf.is_contiguous()) or (mask is not None and mask.is_contiguous())
    dev = local_points.device
    focal = torch.empty(F, device=dev, dtype=torch.float32)
    shift = torch.empty(F, device=dev, dtype=torch.float32)
    fxy = torch.empty(F, 4, device=dev, dtype=torch.float32)
    K = torch.empty(F, 3, 3, device=dev, dtype=torch.float32)
    rc = lib.pi3_focal_shift(local_points.data_ptr(), _L.ptr(conf), _L.ptr(mask), uvx.data_ptr(), uvy.data_ptr(), F, H, W,
                             float(conf_thr), focal.data_ptr(), shift.data_ptr(), fxy.data_ptr(), K.data_ptr(),
                             _L.stream_ptr())
    _L.check(rc, "pi3_focal_shift")
    return dict(focal=focal, shift=shift, fxfycxcy=fxy, intrinsics=K)


# ----------------------------------------------------------------------------------------------- MoGe conv pyramid
def conv3x3(img: torch.Tensor, H: int, W: int, C: int, wgt: torch.Tensor, bias: Optional[torch.Tensor],
            out: torch.Tensor, resid: Optional[torch.Tensor] = None, act: int = ACT_NONE, *, B: int = 1) -> torch.Tensor:
    """img bf16 NHWC [B*H*W, ldc] (B images, each replicate-padded on its own), wgt bf16 [N, 9*C] (C % 64 == 0) or [N, 10*32] (C == 32: ten tap slots, the
    tenth zero); out [B*H*W, >=N] f32/bf16."""
    lib = _L.load()
    assert img.dtype in _16BIT and wgt.dtype == img.dtype and wgt.shape[1] == (320 if C == 32 else 9 * C)
    rc = lib.pi3_conv3x3(img.data_ptr(), img.stride(0), B, H, W, C, wgt.data_ptr(), wgt.shape[0], _L.ptr(bias),
                         _L.ptr(resid), resid.stride(0) if resid is not None else 0, out.data_ptr(), out.stride(0),
                         _dt(img), _dt(out), act, _L.stream_ptr())
    _L.check(rc, "pi3_conv3x3")
    return out


def groupnorm_stats(x: torch.Tensor, HW: int, C: int, G: int, stats: torch.Tensor, *, B: int = 1) -> None:
    """x f32 [B*HW, ldx] -> stats f64 [B][G][2] (sum, sum of squares per group)."""
    lib = _L.load()
    assert x.dtype == torch.float32 and stats.dtype == torch.float64 and stats.numel() >= 2 * B * G
    n_ws = int(lib.pi3_groupnorm_ws_doubles(B, HW, C))
    ws = torch.empty(n_ws, device=x.device, dtype=torch.float64)     # per-block channel partials (deterministic sum)
    rc = lib.pi3_groupnorm_stats(x.data_ptr(), x.stride(0), B, HW, C, G, stats.data_ptr(), ws.data_ptr(), n_ws,
                                 _L.stream_ptr())
    _L.check(rc, "pi3_groupnorm_stats")


ACT_LEAKY, ACT_SILU, ACT_ELU = 3, 4, 5


def groupnorm_apply(x, HW, C, Cpad, G, stats, gamma, beta, eps, act, out, *, B: int = 1) -> None:
    """G = 0: no normalisation; gamma / beta None: no affine (InstanceNorm2d).  x [B*HW, ldx], stats [B][G][2]."""
    lib = _L.load()
    assert out.dtype in _16BIT and out.shape[1] >= Cpad
    rc = lib.pi3_groupnorm_apply(x.data_ptr(), x.stride(0), B, HW, C, Cpad, G, _L.ptr(stats), _L.ptr(gamma),
                                 _L.ptr(beta), float(eps), act, out.data_ptr(), out.stride(0), _dt(out), _L.stream_ptr())
    _L.check(rc, "pi3_groupnorm_apply")


def add_rows(x: torch.Tensor, y: torch.Tensor, rows: int, C: int) -> None:
    lib = _L.load()
    assert x.dtype == torch.float32 and y.dtype == torch.float32
    rc = lib.pi3_add_rows(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), rows, C, _L.stream_ptr())
    _L.check(rc, "pi3_add_rows")


def convt_scatter(g: torch.Tensor, H: int, W: int, Cout: int, Cs: int, Cpad: int, out: torch.Tensor, *,
                  B: int = 1) -> None:
    lib = _L.load()
    assert g.dtype == torch.float32 and out.dtype in _16BIT
    rc = lib.pi3_convt_scatter(g.data_ptr(), g.stride(0), B, H, W, Cout, Cs, Cpad, out.data_ptr(), out.stride(0),
                               _dt(out), _L.stream_ptr())
    _L.check(rc, "pi3_convt_scatter")


def uv_affine(x, H, W, C, w, wofs, bias, uvx, uvy, accumulate: bool, *, B: int = 1) -> None:
    lib = _L.load()
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and w.stride(1) == 1
    rc = lib.pi3_uv_affine(x.data_ptr(), x.stride(0), B, H, W, C, w.data_ptr(), w.stride(0), wofs, _L.ptr(bias),
                           uvx.data_ptr(), uvy.data_ptr(), int(accumulate), _L.stream_ptr())
    _L.check(rc, "pi3_uv_affine")


def resize_taps(src, sstr, C, ys, yw, xs, xw, oh, ow, dst, dstr) -> None:
    lib = _L.load()
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and ys.dtype == torch.int32
    rc = lib.pi3_resize_taps(src.data_ptr(), sstr[0], sstr[1], sstr[2], C, ys.data_ptr(), yw.data_ptr(),
                             xs.data_ptr(), xw.data_ptr(), oh, ow, dst.data_ptr(), dstr[0], dstr[1], dstr[2],
                             _L.stream_ptr())
    _L.check(rc, "pi3_resize_taps")


def dense_vec(x, W, b, act, y) -> None:
    lib = _L.load()
    assert W.dtype == torch.float32 and W.is_contiguous() and x.is_contiguous()
    rc = lib.pi3_dense_vec(x.data_ptr(), W.data_ptr(), _L.ptr(b), W.shape[1], W.shape[0], act, y.data_ptr(),
                           _L.stream_ptr())
    _L.check(rc, "pi3_dense_vec")


def moge_remap(pts, mask_logit, n, remap, mask) -> None:
    lib = _L.load()
    rc = lib.pi3_moge_remap(pts.data_ptr(), _L.ptr(mask_logit), n, remap, _L.ptr(mask), _L.stream_ptr())
    _L.check(rc, "pi3_moge_remap")


def moge_depth(pts, shift, log_scale, mask, n, depth) -> None:
    lib = _L.load()
    rc = lib.pi3_moge_depth(pts.data_ptr(), shift.data_ptr(), _L.ptr(log_scale), mask.data_ptr(), n,
                            depth.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_moge_depth")


def project_observations(points: torch.Tensor, poses: torch.Tensor, intrinsics: torch.Tensor, W: int, H: int,
                         max_after: int):
    """points f16 [N,K,3], poses f32 [N,4,4], intrinsics f32 [N,3,3] -> (uv f32 [N,N,K,2], valid bool [N,N,K])."""
    lib = _L.load()
    N, K = points.shape[:2]
    assert points.dtype == torch.float16 and points.is_contiguous()
    poses, intrinsics = poses.float().contiguous(), intrinsics.float().contiguous()
    uv = torch.zeros(N, N, K, 2, device=points.device, dtype=torch.float32)
    valid = torch.empty(N, N, K, device=points.device, dtype=torch.uint8)
    rc = lib.pi3_project_observations(points.data_ptr(), poses.data_ptr(), intrinsics.data_ptr(), N, K, W, H,
                                      max_after, uv.data_ptr(), valid.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_project_observations")
    return uv, valid.bool()


def ingest_frames(frames_u8: torch.Tensor, H1: int, W1: int, xb: torch.Tensor, xk: torch.Tensor, yb: torch.Tensor,
                  yk: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H0,W0,3] -> float32 [N,3,H1,W1]; bounds / coefs are int32 device tensors from image_io.resample_coeffs."""
    lib = _L.load()
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-1] == 3
    N, H0, W0 = frames_u8.shape[:3]
    for t in (xb, xk, yb, yk):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert xb.shape == (W1, 2) and yb.shape == (H1, 2) and xk.shape[0] == W1 and yk.shape[0] == H1
    tmp = torch.empty(N, H0, W1, 3, device=frames_u8.device, dtype=torch.uint8)
    dst = torch.empty(N, 3, H1, W1, device=frames_u8.device, dtype=torch.float32)
    rc = lib.pi3_ingest_frames(frames_u8.data_ptr(), N, H0, W0, H1, W1, xb.data_ptr(), xk.data_ptr(), xk.shape[1],
                               yb.data_ptr(), yk.data_ptr(), yk.shape[1], tmp.data_ptr(), dst.data_ptr(),
                               _L.stream_ptr())
    _L.check(rc, "pi3_ingest_frames")
    return dst


def undistort_maps(params16, model: int, H: int, W: int, device):
    """params16: 16 python floats (see include/pi3slam_hip.h) -> (map_x, map_y) f32 [H,W] on `device`."""
    import ctypes
    lib = _L.load()
    arr = (ctypes.c_double * 16)(*[float(v) for v in params16])
    mx = torch.empty(H, W, device=device, dtype=torch.float32)
    my = torch.empty(H, W, device=device, dtype=torch.float32)
    rc = lib.pi3_undistort_maps(ctypes.cast(arr, ctypes.c_void_p), int(model), H, W, mx.data_ptr(), my.data_ptr(),
                                _L.stream_ptr())
    _L.check(rc, "pi3_undistort_maps")
    return mx, my


def remap_bilinear_u8(frames_u8: torch.Tensor, map_x: torch.Tensor, map_y: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H0,W0,3] + f32 maps [H,W] -> float32 [N,3,H,W] (cv2.remap INTER_LINEAR, border 0, then / 255)."""
    lib = _L.load()
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-1] == 3
    assert map_x.dtype == torch.float32 and map_y.dtype == torch.float32 and map_x.shape == map_y.shape
    N, H0, W0 = frames_u8.shape[:3]
    H, W = map_x.shape
    dst = torch.empty(N, 3, H, W, device=frames_u8.device, dtype=torch.float32)
    rc = lib.pi3_remap_bilinear_u8(frames_u8.data_ptr(), N, H0, W0, map_x.contiguous().data_ptr(),
                                   map_y.contiguous().data_ptr(), H, W, dst.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_remap_bilinear_u8")
    return dst


# ----------------------------------------------------------------------------------------------- bundle adjustment
def bundle_adjust(points: torch.Tensor, poses: torch.Tensor, intr: torch.Tensor, uv: torch.Tensor, valid: torch.Tensor,
                  huber_width: float, max_iters: int, prior_R: Optional[torch.Tensor] = None,
                  prior_C: Optional[torch.Tensor] = None, prior_flag: Optional[torch.Tensor] = None,
                  sqrt_info_rot: float = 0.0, sqrt_info_pos: float = 0.0, homogeneous: bool = False,
                  inverse_depth: bool = False) -> torch.Tensor:
    """points f64 [N*K,3] and poses f64 [N,12] (R world->camera | centre) refined in place; intr f64 [N,4];
    uv f32 [N,N,K,2], valid u8 [N,N,K].  -> summary f64 [11] (device).  homogeneous: Theia's default point
    parametrization (pi3_bundle_adjust_homogeneous) instead of Euclidean steps; inverse_depth: one inverse depth per track
    along its reference keypoint's ray (pi3_bundle_adjust_inverse_depth; points are snapped onto those rays)."""
    assert not (homogeneous and inverse_depth)
    lib = _L.load()
    N, _, K = valid.shape
    for t in (points, poses, intr):
        assert t.dtype == torch.float64 and t.is_contiguous()
    assert uv.dtype == torch.float32 and uv.is_contiguous() and valid.dtype == torch.uint8 and valid.is_contiguous()
    assert tuple(points.shape) == (N * K, 3) and tuple(poses.shape) == (N, 12) and tuple(intr.shape) == (N, 4)
    uvT = uv.permute(0, 2, 1, 3).contiguous()          # [source][keypoint][target]: a track's cameras are contiguous
    validT = valid.permute(0, 2, 1).contiguous()
    n_ws = int(lib.pi3_ba_workspace_doubles(N, K))
    ws = torch.empty(n_ws, device=points.device, dtype=torch.float64)
    summary = torch.empty(11, device=points.device, dtype=torch.float64)
    if prior_flag is not None:
        assert prior_flag.dtype == torch.uint8 and prior_R.dtype == torch.float64 and prior_C.dtype == torch.float64
        prior_R, prior_C, prior_flag = prior_R.contiguous(), prior_C.contiguous(), prior_flag.contiguous()
    fn, fn_name = ((lib.pi3_bundle_adjust_inverse_depth, "pi3_bundle_adjust_inverse_depth") if inverse_depth else
                   (lib.pi3_bundle_adjust_homogeneous, "pi3_bundle_adjust_homogeneous") if homogeneous else
                   (lib.pi3_bundle_adjust, "pi3_bundle_adjust"))
    rc = fn(points.data_ptr(), poses.data_ptr(), intr.data_ptr(), uv.data_ptr(), valid.data_ptr(),
            uvT.data_ptr(), validT.data_ptr(), N, K, float(huber_width), int(max_iters),
            _L.ptr(prior_R), _L.ptr(prior_C), _L.ptr(prior_flag), float(sqrt_info_rot),
            float(sqrt_info_pos), summary.data_ptr(), ws.data_ptr(), n_ws, _L.stream_ptr())
    _L.check(rc, fn_name)
    return summary


def ba_outlier_tracks(points: torch.Tensor, poses: torch.Tensor, intr: torch.Tensor, uv: torch.Tensor,
                      valid: torch.Tensor, max_px: float, min_angle_deg: float) -> torch.Tensor:
    lib = _L.load()
    N, _, K = valid.shape
    est = torch.empty(N * K, device=points.device, dtype=torch.uint8)
    rc = lib.pi3_ba_outlier_tracks(points.data_ptr(), poses.data_ptr(), intr.data_ptr(), uv.data_ptr(), valid.data_ptr(),
                                   N, K, float(max_px), float(min_angle_deg), est.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_ba_outlier_tracks")
    return est.view(N, K).bool()


# ---------------------------------------------------------------------------------------------------- voxel map
VOXEL_SLOT_BYTES = 64       # key, W, U[3], C[3] as uint64 (csrc/voxel.hip)


def voxel_capacity(n_candidates: int) -> int:
    """Slots for n candidate points: the next power of two >= 2 n (the table is never more than half full)."""
    need = max(2 * int(n_candidates), 1)
    return 1 << (need - 1).bit_length()


def voxel_clear(table: torch.Tensor, stats: torch.Tensor) -> None:
    lib = _L.load()
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    assert stats.dtype == torch.int64 and stats.numel() >= 4
    _L.check(lib.pi3_voxel_clear(table.data_ptr(), table.numel() // 8, stats.data_ptr(), _L.stream_ptr()),
             "pi3_voxel_clear")


def voxel_fuse_pixels(table: torch.Tensor, stats: torch.Tensor, points: torch.Tensor, conf: Optional[torch.Tensor],
                      masks: Optional[torch.Tensor], imgs: Optional[torch.Tensor], conf_logit_thr: float,
                      inv_voxel: float) -> None:
    """points f32 (N,H,W,3), conf f32 logits (N,H,W[,1]), masks uint8/bool (N,H,W), imgs f32 (N,3,H,W)."""
    lib = _L.load()
    N, H, W = points.shape[:3]
    assert points.dtype == torch.float32 and points.is_contiguous() and points.shape[3] == 3
    assert table.dtype == torch.int64 and table.is_contiguous() and stats.dtype == torch.int64
    if conf is not None:
        assert conf.dtype == torch.float32 and conf.is_contiguous() and conf.numel() == N * H * W
    if masks is not None:
        assert masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous() and masks.numel() == N * H * W
    if imgs is not None:
        assert imgs.dtype == torch.float32 and imgs.is_contiguous() and tuple(imgs.shape) == (N, 3, H, W)
    rc = lib.pi3_voxel_fuse_pixels(table.data_ptr(), table.numel() // 8, points.data_ptr(), _L.ptr(conf),
                                   _L.ptr(masks), _L.ptr(imgs), N, H, W, float(conf_logit_thr), float(inv_voxel),
                                   stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_fuse_pixels")


def voxel_fuse_points(table: torch.Tensor, stats: torch.Tensor, points: torch.Tensor, colors: Optional[torch.Tensor],
                      weights: Optional[torch.Tensor], inv_voxel: float) -> None:
    """points f32 (n,3), colors uint8 (n,3), weights int32 (n,)."""
    lib = _L.load()
    assert points.dtype == torch.float32 and points.is_contiguous() and points.shape[-1] == 3
    n = points.numel() // 3
    if colors is not None:
        assert colors.dtype == torch.uint8 and colors.is_contiguous() and colors.numel() == 3 * n
    if weights is not None:
        assert weights.dtype == torch.int32 and weights.is_contiguous() and weights.numel() == n
    rc = lib.pi3_voxel_fuse_points(table.data_ptr(), table.numel() // 8, points.data_ptr(), _L.ptr(colors),
                                   _L.ptr(weights), n, float(inv_voxel), stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_fuse_points")


def voxel_rehash(src: torch.Tensor, dst: torch.Tensor, stats: torch.Tensor) -> None:
    lib = _L.load()
    assert src.dtype == torch.int64 and dst.dtype == torch.int64 and src.is_contiguous() and dst.is_contiguous()
    _L.check(lib.pi3_voxel_rehash(src.data_ptr(), src.numel() // 8, dst.data_ptr(), dst.numel() // 8, stats.data_ptr(),
                                  _L.stream_ptr()), "pi3_voxel_rehash")


def voxel_empty_outputs(rows: int, device):
    """Output buffers of voxel_extract: keys int64 (rows,), points f32 (rows,3), colors uint8 (rows,3), weights int32."""
    m = max(int(rows), 1)
    return (torch.empty(m, device=device, dtype=torch.int64), torch.empty(m, 3, device=device, dtype=torch.float32),
            torch.empty(m, 3, device=device, dtype=torch.uint8), torch.empty(m, device=device, dtype=torch.int32))


def voxel_extract(table: torch.Tensor, stats: torch.Tensor, voxel_size: float, max_out: int, out=None,
                  keep: Optional[torch.Tensor] = None):
    """-> device (keys int64, points f32 (,3), colors uint8 (,3), weights int32) with >= max_out rows (`out`, or fresh
    buffers), unordered; the number of valid entries lands in stats[2].  keep uint8 (capacity,): only the slots it
    marks (pi3_voxel_extract_kept)."""
    lib = _L.load()
    keys, pts, cols, w = out if out is not None else voxel_empty_outputs(max_out, table.device)
    assert keys.shape[0] >= max_out and pts.shape[0] >= max_out and cols.shape[0] >= max_out and w.shape[0] >= max_out
    if keep is None:
        rc = lib.pi3_voxel_extract(table.data_ptr(), table.numel() // 8, float(voxel_size), keys.data_ptr(),
                                   pts.data_ptr(), cols.data_ptr(), w.data_ptr(), int(max_out), stats.data_ptr(),
                                   _L.stream_ptr())
        _L.check(rc, "pi3_voxel_extract")
    else:
        _slot_array(keep, table, torch.uint8)
        rc = lib.pi3_voxel_extract_kept(table.data_ptr(), table.numel() // 8, float(voxel_size), keys.data_ptr(),
                                        pts.data_ptr(), cols.data_ptr(), w.data_ptr(), int(max_out), stats.data_ptr(),
                                        keep.data_ptr(), _L.stream_ptr())
        _L.check(rc, "pi3_voxel_extract_kept")
    return keys, pts, cols, w


# ---- cleaning the fused map (csrc/voxel_clean.hip): arrays with one entry per slot of the table
VOXEL_CLEAN_COUNTERS = ("voxels", "eligible", "after_support", "after_components", "components", "components_kept")


def _slot_array(t: torch.Tensor, table: torch.Tensor, dtype) -> None:
    assert t.dtype == dtype and t.is_contiguous() and t.device == table.device and t.numel() == table.numel() // 8


def voxel_support(table: torch.Tensor, min_weight: int, radius: int, min_support: int, keep: torch.Tensor,
                  support: Optional[torch.Tensor], counters: torch.Tensor, exclude: Optional[torch.Tensor] = None) -> None:
    """Stage A: keep uint8 (capacity,), support int32 (capacity,) or None, counters int64 (8,) (zeroed by the call).
    exclude uint8 (capacity,) (pi3_voxel_support_excluding): the slots it marks are neither eligible nor anybody's
    neighbour, and counters[6] counts the occupied ones among them."""
    lib = _L.load()
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    _slot_array(keep, table, torch.uint8)
    if support is not None:
        _slot_array(support, table, torch.int32)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 8
    if exclude is None:
        rc = lib.pi3_voxel_support(table.data_ptr(), table.numel() // 8, int(min_weight), int(radius), int(min_support),
                                   keep.data_ptr(), _L.ptr(support), counters.data_ptr(), _L.stream_ptr())
        _L.check(rc, "pi3_voxel_support")
    else:
        _slot_array(exclude, table, torch.uint8)
        rc = lib.pi3_voxel_support_excluding(table.data_ptr(), table.numel() // 8, int(min_weight), int(radius),
                                             int(min_support), keep.data_ptr(), _L.ptr(support), counters.data_ptr(),
                                             exclude.data_ptr(), _L.stream_ptr())
        _L.check(rc, "pi3_voxel_support_excluding")


def voxel_label_init(table: torch.Tensor, keep: torch.Tensor, label: torch.Tensor) -> None:
    lib = _L.load()
    _slot_array(keep, table, torch.uint8)
    _slot_array(label, table, torch.int64)
    _L.check(lib.pi3_voxel_label_init(table.data_ptr(), table.numel() // 8, keep.data_ptr(), label.data_ptr(),
                                      _L.stream_ptr()), "pi3_voxel_label_init")


def voxel_label_sweep(table: torch.Tensor, label: torch.Tensor, changed: torch.Tensor) -> None:
    """One sweep; changed: one int32 on the device (a view of one element is fine), zeroed by the caller."""
    lib = _L.load()
    _slot_array(label, table, torch.int64)
    assert changed.dtype == torch.int32 and changed.numel() == 1 and changed.device == table.device
    _L.check(lib.pi3_voxel_label_sweep(table.data_ptr(), table.numel() // 8, label.data_ptr(), changed.data_ptr(),
                                       _L.stream_ptr()), "pi3_voxel_label_sweep")


def voxel_component_sizes(table: torch.Tensor, label: torch.Tensor, size: torch.Tensor) -> None:
    lib = _L.load()
    _slot_array(label, table, torch.int64)
    _slot_array(size, table, torch.int32)
    _L.check(lib.pi3_voxel_component_sizes(table.data_ptr(), table.numel() // 8, label.data_ptr(), size.data_ptr(),
                                           _L.stream_ptr()), "pi3_voxel_component_sizes")


def voxel_component_filter(table: torch.Tensor, label: torch.Tensor, size: torch.Tensor, min_component: int,
                           keep: torch.Tensor, counters: torch.Tensor) -> None:
    lib = _L.load()
    _slot_array(label, table, torch.int64)
    _slot_array(size, table, torch.int32)
    _slot_array(keep, table, torch.uint8)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 8
    rc = lib.pi3_voxel_component_filter(table.data_ptr(), table.numel() // 8, label.data_ptr(), size.data_ptr(),
                                        int(min_component), keep.data_ptr(), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_component_filter")


def dense_consistency(points: torch.Tensor, local_points: torch.Tensor, conf: Optional[torch.Tensor],
                      masks: Optional[torch.Tensor], poses: torch.Tensor, fxfycxcy: torch.Tensor, conf_logit_thr: float,
                      radius: int, stride: int, min_views: int, rel_tol: float, want_counts: bool = False):
    """Multi-view depth consistency of one chunk (csrc/dense_filter.hip).  points / local_points f32 (N,H,W,3), conf f32
    logits (N,H,W[,1]), masks uint8/bool (N,H,W), poses f32 (N,4,4) cam->world, fxfycxcy f32 (N,4) ->
    (out_mask uint8 (N,H,W), counts uint8 (N,H,W,2) [agree, conflict] or None, stats int64 (2,) [candidates, kept])."""
    lib = _L.load()
    N, H, W = (int(x) for x in points.shape[:3])
    dev = points.device
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 4 and points.shape[3] == 3
    assert local_points.dtype == torch.float32 and local_points.is_contiguous() and local_points.shape == points.shape
    assert poses.dtype == torch.float32 and poses.is_contiguous() and tuple(poses.shape) == (N, 4, 4)
    assert fxfycxcy.dtype == torch.float32 and fxfycxcy.is_contiguous() and tuple(fxfycxcy.shape) == (N, 4)
    assert local_points.device == dev and poses.device == dev and fxfycxcy.device == dev
    if conf is not None:
        assert conf.dtype == torch.float32 and conf.is_contiguous() and conf.numel() == N * H * W and conf.device == dev
    if masks is not None:
        assert masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous() and masks.numel() == N * H * W
        assert masks.device == dev
    zplane = torch.empty(N, H, W, device=dev, dtype=torch.float32)
    out_mask = torch.empty(N, H, W, device=dev, dtype=torch.uint8)
    counts = torch.empty(N, H, W, 2, device=dev, dtype=torch.uint8) if want_counts else None
    stats = torch.zeros(2, device=dev, dtype=torch.int64)
    if N * H * W == 0:          # empty tensors have no address to pass
        return out_mask, counts, stats
    rc = lib.pi3_dense_consistency(points.data_ptr(), local_points.data_ptr(), _L.ptr(conf), _L.ptr(masks),
                                   poses.data_ptr(), fxfycxcy.data_ptr(), N, H, W, float(conf_logit_thr), int(radius),
                                   int(stride), int(min_views), float(rel_tol), zplane.data_ptr(), out_mask.data_ptr(),
                                   _L.ptr(counts), stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_dense_consistency")
    return out_mask, counts, stats


def depth_plane_shape(N: int, H: int, W: int, every: int, pixel_stride: int) -> Tuple[int, int, int]:
    """(Nk, H', W') of the depth keyframes of an (N,H,W) chunk: frames 0, every, 2 every, .. and every pixel_stride-th
    row and column, both starting at 0."""
    return (int(N) + int(every) - 1) // int(every), -(-int(H) // int(pixel_stride)), -(-int(W) // int(pixel_stride))


def dense_depth_planes(points: torch.Tensor, local_points: torch.Tensor, conf: Optional[torch.Tensor],
                       masks: Optional[torch.Tensor], conf_logit_thr: float, every: int, pixel_stride: int,
                       out: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None):
    """Depth keyframes of one chunk (csrc/dense_filter.hip: pi3_dense_depth_planes).  points / local_points f32
    (N,H,W,3), conf f32 logits (N,H,W[,1]) or None, masks uint8/bool (N,H,W) or None -> (depth fp16 (Nk,H',W') with the
    shape of depth_plane_shape: the local z of dense_consistency's candidates rounded to nearest even, 0 elsewhere and
    where it rounds to 0 or inf; count int64 (1,): the non-zero samples).  out: a contiguous fp16 buffer with at least
    Nk H' W' elements to write into (the result is a view of it); count: an int64 device tensor to write into."""
    lib = _L.load()
    N, H, W = (int(x) for x in points.shape[:3])
    dev = points.device
    every, pixel_stride = int(every), int(pixel_stride)
    assert every >= 1 and pixel_stride in (1, 2, 4)
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 4 and points.shape[3] == 3
    assert local_points.dtype == torch.float32 and local_points.is_contiguous() and local_points.shape == points.shape
    assert local_points.device == dev
    if conf is not None:
        assert conf.dtype == torch.float32 and conf.is_contiguous() and conf.numel() == N * H * W and conf.device == dev
    if masks is not None:
        assert masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous() and masks.numel() == N * H * W
        assert masks.device == dev
    shape = depth_plane_shape(N, H, W, every, pixel_stride)
    n_out = shape[0] * shape[1] * shape[2]
    if out is None:
        out = torch.empty(max(n_out, 1), device=dev, dtype=torch.float16)
    assert out.dtype == torch.float16 and out.is_contiguous() and out.numel() >= n_out and out.device == dev
    if count is None:
        count = torch.zeros(1, device=dev, dtype=torch.int64)
    assert count.dtype == torch.int64 and count.numel() >= 1 and count.device == dev
    depth = out.reshape(-1)[:n_out].view(shape)
    if N * H * W == 0:          # empty tensors have no address to pass
        count.zero_()
        return depth, count
    rc = lib.pi3_dense_depth_planes(points.data_ptr(), local_points.data_ptr(), _L.ptr(conf), _L.ptr(masks), N, H, W,
                                    float(conf_logit_thr), every, pixel_stride, out.data_ptr(), count.data_ptr(),
                                    _L.stream_ptr())
    _L.check(rc, "pi3_dense_depth_planes")
    return depth, count


# ---- carving the fused map with depth keyframes (csrc/voxel_carve.hip)
VOXEL_CARVE_COUNTERS = ("voxels", "carved", "unvoted")
CARVE_VIEW_DOUBLES = 20     # render.pack_cameras' row; [17] = the view's depth scale
CARVE_DEPTH_SCALE_AT = 17


def voxel_carve(table: torch.Tensor, voxel_size: float, views: torch.Tensor, planes: torch.Tensor, pixel_stride: int,
                rel_tol: float, margin: float, min_conflicts: int, carved: torch.Tensor,
                agree: Optional[torch.Tensor], conflict: Optional[torch.Tensor], counters: torch.Tensor) -> None:
    """Per slot of the table: X = the extraction's centroid (f64 -> fp32 -> f64); per view m (views f64 (M,20): rigid
    world->camera 3x4, fx fy cx cy, 0, [17] = depth scale s; planes fp16 (M,H',W')): xc = ((r00 x + r01 y) + r02 z) + t0,
    likewise yc, zc; no vote unless zc > 0 and finite; u = fx (xc / zc) + cx, v = fy (yc / zc) + cy; pu = rint(u / S),
    pv = rint(v / S), inside the plane; zo = s plane[m, pv, pu], no vote when 0 or not finite; r = zc - zo,
    lim = rel_tol zo + margin; |r| <= lim agrees, r < -lim conflicts.  carved uint8 (capacity,) = conflict >=
    min_conflicts and conflict > agree; agree / conflict int32 (capacity,) (the uint32 votes) or None; counters int64
    (4,) = occupied, carved, no view voted (zeroed by the call)."""
    lib = _L.load()
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    dev = table.device
    assert views.dtype == torch.float64 and views.is_contiguous() and views.ndim == 2
    assert views.shape[1] == CARVE_VIEW_DOUBLES and views.device == dev
    M = int(views.shape[0])
    assert planes.dtype == torch.float16 and planes.is_contiguous() and planes.ndim == 3 and planes.device == dev
    assert int(planes.shape[0]) == M and M < 1 << 31
    Hp, Wp = int(planes.shape[1]), int(planes.shape[2])
    _slot_array(carved, table, torch.uint8)
    for t in (agree, conflict):
        if t is not None:
            _slot_array(t, table, torch.int32)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    rc = lib.pi3_voxel_carve(table.data_ptr(), table.numel() // 8, float(voxel_size), views.data_ptr() if M else None, M,
                             planes.data_ptr() if M else None, Hp, Wp, int(pixel_stride), float(rel_tol), float(margin),
                             int(min_conflicts), carved.data_ptr(), _L.ptr(agree), _L.ptr(conflict), counters.data_ptr(),
                             _L.stream_ptr())
    _L.check(rc, "pi3_voxel_carve")


# ---- moving a chunk's cloud with the views that saw it (csrc/cloud_follow.hip)
CLOUD_FOLLOW_COUNTERS = ("dropped", "level1", "level2", "level3")
FOLLOW_MOVE_DOUBLES = 12    # D_m, 3x4 row-major


def cloud_follow_views(points: torch.Tensor, normals: Optional[torch.Tensor], views: torch.Tensor, moves: torch.Tensor,
                       planes: torch.Tensor, pixel_stride: int, rel_tol: float, margin: float, out_points: torch.Tensor,
                       out_normals: Optional[torch.Tensor], level: Optional[torch.Tensor],
                       support: Optional[torch.Tensor], counters: torch.Tensor) -> None:
    """Per point X of points f32 (P,3) (normals f32 (P,3) or None) and per view m in order (views f64 (M,20) as
    voxel_carve's, moves f64 (M,12) = D_m 3x4 row-major, planes fp16 (M,H',W')): Y = D_m X, Nn = the 3x3 part of D_m
    times the normal; every view adds to level 3; a view in whose plane the point projects (the carver's xc, yc, zc, u,
    v, pu, pv) adds with w = 1 / zc^2 to level 2; a view whose depth zo = views[m,17] plane[m,pv,pu] is non-zero, finite
    and has |zc - zo| <= rel_tol zo + margin adds with w to level 1.  out_points (may be points) = S_l / W_l of the first
    level that has a view (level 3: S3 / M), out_normals (may be normals) = N_l normalised (0 when it has no length);
    level uint8 (P,) or None; support int32 (P,) or None = the level-1 views; counters int64 (4,) =
    CLOUD_FOLLOW_COUNTERS (zeroed by the call).  A point that is not finite is copied, level 0, counted as dropped."""
    lib = _L.load()
    dev = points.device
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    P = int(points.shape[0])
    assert out_points.dtype == torch.float32 and out_points.is_contiguous() and out_points.shape == points.shape
    assert out_points.device == dev
    assert (normals is None) == (out_normals is None)
    for t in (normals, out_normals):
        if t is not None:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == points.shape and t.device == dev
    assert views.dtype == torch.float64 and views.is_contiguous() and views.ndim == 2
    assert views.shape[1] == CARVE_VIEW_DOUBLES and views.device == dev
    M = int(views.shape[0])
    assert moves.dtype == torch.float64 and moves.is_contiguous() and tuple(moves.shape) == (M, FOLLOW_MOVE_DOUBLES)
    assert moves.device == dev
    assert planes.dtype == torch.float16 and planes.is_contiguous() and planes.ndim == 3 and planes.device == dev
    assert int(planes.shape[0]) == M and 1 <= M < 1 << 31
    Hp, Wp = int(planes.shape[1]), int(planes.shape[2])
    if level is not None:
        assert level.dtype == torch.uint8 and level.is_contiguous() and level.numel() == P and level.device == dev
    if support is not None:
        assert support.dtype == torch.int32 and support.is_contiguous() and support.numel() == P and support.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    empty = P == 0              # empty tensors have no address to pass
    rc = lib.pi3_cloud_follow_views(None if empty else points.data_ptr(), None if empty else _L.ptr(normals), P,
                                    views.data_ptr(), moves.data_ptr(), M, planes.data_ptr(), Hp, Wp, int(pixel_stride),
                                    float(rel_tol), float(margin), None if empty else out_points.data_ptr(),
                                    None if empty else _L.ptr(out_normals), None if empty else _L.ptr(level),
                                    None if empty else _L.ptr(support), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_cloud_follow_views")


# ---- occupancy grid and clearance field of the dense map (csrc/occupancy.hip)
OCCUPANCY_UNKNOWN, OCCUPANCY_FREE, OCCUPANCY_OCCUPIED = 0, 1, 2
OCCUPANCY_MARK_COUNTERS = ("marked", "dropped", "outside")
OCCUPANCY_OBSERVE_COUNTERS = ("cells", "occupied", "free", "unknown", "unvoted", "camera_cells_freed")
EDT_MAX_RADIUS = 255
EDT_FAR = 0xFFFF


def _grid_state(state: torch.Tensor) -> Tuple[int, int, int]:
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.ndim == 3
    return int(state.shape[2]), int(state.shape[1]), int(state.shape[0])


def occupancy_mark(points: torch.Tensor, inv_cell: float, origin, state: torch.Tensor, counters: torch.Tensor) -> None:
    """state uint8 (nz,ny,nx) is zeroed, then every row of points f32 (P,3) goes through the voxel quantiser at inv_cell
    per axis (k = floor(p * inv_cell) in fp32) and the cell k - origin, when it is inside the grid, becomes 2 (occupied).
    origin: three integers (ox, oy, oz).  counters int64 (4,) = OCCUPANCY_MARK_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    nx, ny, nz = _grid_state(state)
    dev = state.device
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    assert points.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    ox, oy, oz = (int(v) for v in origin)
    if state.numel() == 0:      # empty tensors have no address to pass
        counters[:4] = 0
        return
    P = int(points.shape[0])
    rc = lib.pi3_occupancy_mark(points.data_ptr() if P else None, P, float(inv_cell), ox, oy, oz, nx, ny, nz,
                                state.data_ptr(), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_occupancy_mark")


def occupancy_observe(state: torch.Tensor, origin, cell: float, views: torch.Tensor, planes: torch.Tensor,
                      pixel_stride: int, rel_tol: float, margin: float, min_free_views: int,
                      free_votes: Optional[torch.Tensor], hit_votes: Optional[torch.Tensor],
                      counters: torch.Tensor) -> None:
    """Per cell of state uint8 (nz,ny,nx) that is not occupied (!= 2): the centre cell ((origin + i) + 0.5) per axis is
    projected into every view with voxel_carve's arithmetic (views f64 (M,20), planes fp16 (M,H',W')); r = zc - zo,
    lim = rel_tol zo + margin; r < -lim is a free vote, |r| <= lim a hit vote; the cell becomes 1 (free) when free >=
    min_free_views and free > hit, else 0 (unknown); after the vote an unknown cell that holds a view's camera centre
    (floor(-R^T t / cell)) becomes free as well.  free_votes / hit_votes int32 (nz,ny,nx) (the uint32 votes) or
    None; counters int64 (8,) = OCCUPANCY_OBSERVE_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    nx, ny, nz = _grid_state(state)
    dev = state.device
    assert views.dtype == torch.float64 and views.is_contiguous() and views.ndim == 2
    assert views.shape[1] == CARVE_VIEW_DOUBLES and views.device == dev
    M = int(views.shape[0])
    assert planes.dtype == torch.float16 and planes.is_contiguous() and planes.ndim == 3 and planes.device == dev
    assert int(planes.shape[0]) == M and M < 1 << 31
    Hp, Wp = int(planes.shape[1]), int(planes.shape[2])
    for t in (free_votes, hit_votes):
        if t is not None:
            assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == state.shape and t.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 8 and counters.device == dev
    ox, oy, oz = (int(v) for v in origin)
    if state.numel() == 0:      # empty tensors have no address to pass
        counters[:8] = 0
        return
    rc = lib.pi3_occupancy_observe(state.data_ptr(), nx, ny, nz, ox, oy, oz, float(cell), views.data_ptr() if M else None,
                                   M, planes.data_ptr() if M else None, Hp, Wp, int(pixel_stride), float(rel_tol),
                                   float(margin), int(min_free_views), _L.ptr(free_votes), _L.ptr(hit_votes),
                                   counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_occupancy_observe")


def grid_edt(state: torch.Tensor, radius: int, unknown_is_obstacle: bool, d2: torch.Tensor,
             workspace: torch.Tensor) -> None:
    """The exact squared Euclidean distance transform of state uint8 (nz,ny,nx), in cells, truncated at `radius` cells
    (1..EDT_MAX_RADIUS): d2 int16 (nz,ny,nx) (the uint16 values) = the squared distance to the nearest site (state 2,
    and state 0 when unknown_is_obstacle) when it is <= radius^2, else EDT_FAR.  workspace: int16, the same size, not
    d2 (the three passes ping-pong between the two)."""
    lib = _L.load()
    nx, ny, nz = _grid_state(state)
    dev = state.device
    for t in (d2, workspace):
        assert t.dtype == torch.int16 and t.is_contiguous() and t.numel() == state.numel() and t.device == dev
    assert d2.data_ptr() != workspace.data_ptr() or state.numel() == 0
    if state.numel() == 0:      # empty tensors have no address to pass
        return
    rc = lib.pi3_grid_edt(state.data_ptr(), nx, ny, nz, int(radius), 1 if unknown_is_obstacle else 0, d2.data_ptr(),
                          workspace.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_edt")


# ---- routes through the occupancy grid (csrc/grid_route.hip)
ROUTE_FAR = 0xFFFFFFFF
ROUTE_COSTS = (12, 17, 21)              # a move along one, two, three axes
ROUTE_MAX_CELLS = 1 << 27               # 21 (cells - 1) stays below ROUTE_FAR
ROUTE_INIT_COUNTERS = ("traversable", "sources_accepted", "sources_blocked", "sources_outside")


def _grid_field(field: torch.Tensor, walk: Optional[torch.Tensor] = None) -> Tuple[int, int, int]:
    """(nx, ny, nz) of a grid field of 32-bit words, int32 (nz,ny,nx): dist, with its walk uint8 (nz,ny,nx), or label."""
    assert field.dtype == torch.int32 and field.is_contiguous() and field.ndim == 3
    if walk is not None:
        assert _grid_state(walk) and walk.shape == field.shape and walk.device == field.device
    assert 0 < field.numel() <= ROUTE_MAX_CELLS, f"{field.numel()} cells: 1 .. 2^27"
    return int(field.shape[2]), int(field.shape[1]), int(field.shape[0])


def sweep_until_quiet(launch, device, bound: int, what: str, per_read: int) -> int:
    """Repeats a fixed-point sweep until one changes nothing -> the sweeps run, the quiet one included.  launch(flag)
    queues one sweep that sets the int32 (1,) `flag` when it changed something.  The kernels only launch; the loop is
    here: per_read sweeps, one read of their flags.  More than `bound` sweeps without a quiet one raise the RuntimeError
    `what`, a text with a place for {sweeps}."""
    changed = torch.empty(per_read, dtype=torch.int32, device=device)
    sweeps = 0
    while True:
        changed.zero_()
        for j in range(per_read):
            launch(changed[j:j + 1])
        flags = changed.tolist()
        if 0 in flags:
            return sweeps + flags.index(0) + 1
        sweeps += per_read
        if sweeps > bound:
            raise RuntimeError(what.format(sweeps=sweeps))


def sweep_many_until_quiet(launch, device, K: int, bound: int, what: str, per_read: int) -> List[int]:
    """sweep_until_quiet for K fields that settle at different times -> the sweeps run per field, the quiet one included.
    launch(active, flags) queues one sweep of the fields listed in active int32 (A,) (ascending field numbers) that sets
    flags[f] of the int32 (K,) `flags` when field f changed.  per_read launches are queued, each with its own row of K
    flags over the same list, and the rows are read once; a field leaves the list after the first launch in which it was
    listed and its flag stayed 0 (the launches queued behind that one in the same batch ran it again without effect and
    are not counted).  More than `bound` sweeps of a field without a quiet one raise the RuntimeError `what`, a text
    with a place for {sweeps}."""
    K = int(K)
    changed = torch.empty((per_read, K), dtype=torch.int32, device=device)
    sweeps = [0] * K
    listed = list(range(K))
    while listed:
        active = torch.tensor(listed, dtype=torch.int32, device=device)
        changed.zero_()
        for j in range(per_read):
            launch(active, changed[j])
        rows = changed.tolist()
        still = []
        for f in listed:
            quiet = next((j for j in range(per_read) if rows[j][f] == 0), None)
            if quiet is None:
                sweeps[f] += per_read
                if sweeps[f] > bound:
                    raise RuntimeError(what.format(sweeps=sweeps[f]))
                still.append(f)
            else:
                sweeps[f] += quiet + 1
        listed = still
    return sweeps


def grid_route_init(state: torch.Tensor, d2: Optional[torch.Tensor], min_d2: int, through_unknown: bool,
                    sources: torch.Tensor, walk: torch.Tensor, dist: torch.Tensor, counters: torch.Tensor) -> None:
    """walk uint8 (nz,ny,nx) = 1 where state uint8 (nz,ny,nx) is free (with through_unknown: not occupied) and, with
    d2 int16 (nz,ny,nx) (grid_edt's field, the uint16 values), d2 >= min_d2; dist int32 (nz,ny,nx) (the uint32 values)
    = ROUTE_FAR everywhere, then 0 at every entry of sources int64 (Ns,) (linear indices) that lies inside the grid on
    a traversable cell.  counters int64 (4,) = ROUTE_INIT_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist, walk)
    dev = state.device
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.shape == walk.shape and walk.device == dev
    if d2 is not None:
        assert d2.dtype == torch.int16 and d2.is_contiguous() and d2.shape == state.shape and d2.device == dev
    assert d2 is not None or int(min_d2) == 0, "min_d2 needs the clearance field d2"
    assert sources.dtype == torch.int64 and sources.is_contiguous() and sources.ndim == 1 and sources.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    Ns = int(sources.shape[0])
    rc = lib.pi3_grid_route_init(state.data_ptr(), _L.ptr(d2), int(min_d2), 1 if through_unknown else 0, nx, ny, nz,
                                 sources.data_ptr() if Ns else None, Ns, walk.data_ptr(), dist.data_ptr(),
                                 counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_init")


# ---- routes for a body that stands (csrc/grid_stand.hip)
STAND_MAX_HEIGHT = 254                  # cells: how far below a cell its support is looked for
STAND_NONE = 0                          # no verified support: an unknown cell or the grid's border came first
STAND_FAR = 255                         # nothing within STAND_MAX_HEIGHT cells
ROUTE_INIT_STAND_COUNTERS = ROUTE_INIT_COUNTERS + ("off_band",)


def grid_stand_height(state: torch.Tensor, up_axis: int, up_sign: int, through_unknown: bool,
                      height: torch.Tensor) -> None:
    """height uint8 (nz,ny,nx) of state uint8 (nz,ny,nx) for up = up_sign e_up_axis (up_axis 0, 1, 2 = x, y, z): j when
    the first cell among c - j up, j = 1 .. STAND_MAX_HEIGHT, that is outside the grid or not passable (state != 1;
    with through_unknown state == 2) is occupied, STAND_NONE when it is anything else, STAND_FAR when there is none."""
    lib = _L.load()
    assert _grid_state(state) and 0 < state.numel() <= ROUTE_MAX_CELLS, f"{state.numel()} cells: 1 .. 2^27"
    assert height.dtype == torch.uint8 and height.is_contiguous() and height.shape == state.shape
    assert height.device == state.device and height.data_ptr() != state.data_ptr()
    nz, ny, nx = (int(v) for v in state.shape)
    rc = lib.pi3_grid_stand_height(state.data_ptr(), nx, ny, nz, int(up_axis), int(up_sign), 1 if through_unknown else 0,
                                   height.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_stand_height")


def grid_route_init_stand(state: torch.Tensor, d2: Optional[torch.Tensor], min_d2: int, through_unknown: bool,
                          height: torch.Tensor, h_lo: int, h_hi: int, sources: torch.Tensor, walk: torch.Tensor,
                          dist: torch.Tensor, counters: torch.Tensor) -> None:
    """grid_route_init for a body that stands: walk also needs h_lo <= height <= h_hi on height uint8 (nz,ny,nx)
    (grid_stand_height's field), 1 <= h_lo <= h_hi <= STAND_MAX_HEIGHT.  counters int64 (5,) =
    ROUTE_INIT_STAND_COUNTERS (zeroed by the call): off_band counts the cells that only the band closed."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist, walk)
    dev = state.device
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.shape == walk.shape and walk.device == dev
    if d2 is not None:
        assert d2.dtype == torch.int16 and d2.is_contiguous() and d2.shape == state.shape and d2.device == dev
    assert d2 is not None or int(min_d2) == 0, "min_d2 needs the clearance field d2"
    assert height.dtype == torch.uint8 and height.is_contiguous() and height.shape == state.shape and height.device == dev
    assert sources.dtype == torch.int64 and sources.is_contiguous() and sources.ndim == 1 and sources.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 5 and counters.device == dev
    Ns = int(sources.shape[0])
    rc = lib.pi3_grid_route_init_stand(state.data_ptr(), _L.ptr(d2), int(min_d2), 1 if through_unknown else 0,
                                       height.data_ptr(), int(h_lo), int(h_hi), nx, ny, nz,
                                       sources.data_ptr() if Ns else None, Ns, walk.data_ptr(), dist.data_ptr(),
                                       counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_init_stand")


def grid_route_sweep(walk: torch.Tensor, dist: torch.Tensor, changed: torch.Tensor) -> None:
    """One relaxation sweep over dist int32 (nz,ny,nx) (tiles of 8 x 8 x 8 cells, each relaxed to its fixed point);
    changed int32 (1,) becomes 1 when a cell got lower (the caller zeroes it)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist, walk)
    assert changed.dtype == torch.int32 and changed.numel() == 1 and changed.device == walk.device
    rc = lib.pi3_grid_route_sweep(walk.data_ptr(), nx, ny, nz, dist.data_ptr(), changed.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_sweep")


def grid_route_trace(walk: torch.Tensor, dist: torch.Tensor, goal: int, path: torch.Tensor, length: torch.Tensor) -> None:
    """The cheapest way from the cell `goal` (a linear index inside the grid) back to a source over the settled dist:
    path int64 (cap,) gets the linear indices goal .. source, length int64 (1,) their number: 0 when there is no way,
    -needed when path is too short (it is then left untouched)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist, walk)
    dev = walk.device
    assert path.dtype == torch.int64 and path.is_contiguous() and path.ndim == 1 and path.numel() >= 1 and path.device == dev
    assert length.dtype == torch.int64 and length.numel() == 1 and length.device == dev
    assert 0 <= int(goal) < walk.numel(), f"goal {goal} outside the grid's {walk.numel()} cells"
    rc = lib.pi3_grid_route_trace(walk.data_ptr(), dist.data_ptr(), nx, ny, nz, int(goal), path.data_ptr(),
                                  int(path.numel()), length.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_trace")


ROUTE_FIELDS_COUNTERS = ("sources_accepted", "sources_blocked", "sources_outside")
ROUTE_MAX_FIELDS = 65535


def _grid_fields(dist: torch.Tensor, walk: torch.Tensor) -> Tuple[int, int, int, int]:
    """(nx, ny, nz, K) of K fields int32 (K,nz,ny,nx) (the uint32 values) over their walk uint8 (nz,ny,nx)."""
    assert dist.dtype == torch.int32 and dist.is_contiguous() and dist.ndim == 4
    assert _grid_state(walk) and walk.shape == dist.shape[1:] and walk.device == dist.device
    assert 0 < walk.numel() <= ROUTE_MAX_CELLS, f"{walk.numel()} cells: 1 .. 2^27"
    assert 1 <= int(dist.shape[0]) <= ROUTE_MAX_FIELDS, f"{dist.shape[0]} fields: 1 .. {ROUTE_MAX_FIELDS}"
    return int(dist.shape[3]), int(dist.shape[2]), int(dist.shape[1]), int(dist.shape[0])


def grid_route_fields_init(walk: torch.Tensor, sources: torch.Tensor, dist: torch.Tensor, counters: torch.Tensor) -> None:
    """dist int32 (K,nz,ny,nx) (the uint32 values) = ROUTE_FAR everywhere, then field f = 0 at sources[f] (int64 (K,),
    linear indices) when that lies inside the grid on a traversable cell of walk uint8 (nz,ny,nx); a field whose source
    is refused stays all far.  counters int64 (3,) = ROUTE_FIELDS_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    nx, ny, nz, K = _grid_fields(dist, walk)
    dev = walk.device
    assert sources.dtype == torch.int64 and sources.is_contiguous() and tuple(sources.shape) == (K,) and sources.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 3 and counters.device == dev
    rc = lib.pi3_grid_route_fields_init(walk.data_ptr(), nx, ny, nz, sources.data_ptr(), K, dist.data_ptr(),
                                        counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_fields_init")


def grid_route_sweep_many(walk: torch.Tensor, dist: torch.Tensor, active: torch.Tensor, group: int,
                          changed: torch.Tensor) -> None:
    """One relaxation sweep of the fields of dist int32 (K,nz,ny,nx) listed in active int32 (A,) (distinct field numbers,
    A <= K), a workgroup per tile and `group` listed fields; changed int32 (K,): entry f becomes 1 when a cell of field
    f got lower (the caller zeroes it).  Fields that are not listed, and their entries, are not touched."""
    lib = _L.load()
    nx, ny, nz, K = _grid_fields(dist, walk)
    dev = walk.device
    assert active.dtype == torch.int32 and active.is_contiguous() and active.ndim == 1 and active.device == dev
    A = int(active.numel())
    assert A <= K, f"{A} listed fields of {K}"
    assert int(group) >= 1, f"group {group}: >= 1"
    assert changed.dtype == torch.int32 and changed.is_contiguous() and tuple(changed.shape) == (K,) and changed.device == dev
    rc = lib.pi3_grid_route_sweep_many(walk.data_ptr(), nx, ny, nz, dist.data_ptr(), K, active.data_ptr() if A else None,
                                       A, int(group), changed.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_sweep_many")


def grid_route_trace_many(walk: torch.Tensor, dist: torch.Tensor, field_of: torch.Tensor, goal: torch.Tensor,
                          offset: torch.Tensor, path: torch.Tensor, length: torch.Tensor) -> None:
    """grid_route_trace for L legs at once: leg l walks over field field_of[l] (int32 (L,)) of the settled dist int32
    (K,nz,ny,nx) from goal[l] (int64 (L,)) into path[offset[l] : offset[l + 1]] (offset int64 (L + 1,), ascending within
    path int64 (P,): the caller's to keep); length int64 (L,) = the waypoints per leg, 0 when there is no way, -needed
    when the slot is too short (it is then left untouched).  All on the device."""
    lib = _L.load()
    nx, ny, nz, K = _grid_fields(dist, walk)
    dev = walk.device
    L = int(field_of.numel())
    assert field_of.dtype == torch.int32 and field_of.is_contiguous() and field_of.ndim == 1 and field_of.device == dev
    for t, n in ((goal, L), (offset, L + 1), (length, L)):
        assert t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == (n,) and t.device == dev
    assert path.dtype == torch.int64 and path.is_contiguous() and path.ndim == 1 and path.device == dev
    assert L == 0 or path.numel() >= 1
    rc = lib.pi3_grid_route_trace_many(walk.data_ptr(), dist.data_ptr(), nx, ny, nz, K,
                                       field_of.data_ptr() if L else None, goal.data_ptr() if L else None,
                                       offset.data_ptr() if L else None, path.data_ptr() if L else None,
                                       length.data_ptr() if L else None, L, _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_trace_many")


SIGHT_MAX_SPAN = 4096


def grid_sight_words(span: int) -> int:
    """The 64-bit words per row of grid_route_sight_paths' vis."""
    return (int(span) + 63) // 64


def grid_route_sight_paths(walk: torch.Tensor, cells: torch.Tensor, offsets: torch.Tensor, span: int,
                           vis: torch.Tensor) -> None:
    """Line of sight along ways (csrc/grid_sight.hip): way l is cells[offsets[l] : offsets[l + 1]] (cells int64 (P,)
    linear indices, offsets int64 (legs + 1,) ascending from 0 to P).  vis int64 (P, grid_sight_words(span)) (the uint64
    values): bit k of row p is set when p and p + 1 + k lie in the same way, k < span, and cells[p] sees cells[p + 1 + k]
    over walk uint8 (nz,ny,nx); every other bit is written 0.  span outside 1 .. SIGHT_MAX_SPAN is refused by the
    library.  All on the device."""
    lib = _L.load()
    nx, ny, nz = _grid_state(walk)
    dev = walk.device
    assert 0 < walk.numel() <= ROUTE_MAX_CELLS, f"{walk.numel()} cells: 1 .. 2^27"
    assert cells.dtype == torch.int64 and cells.is_contiguous() and cells.ndim == 1 and cells.device == dev
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.ndim == 1 and offsets.numel() >= 1
    assert offsets.device == dev
    P, legs = int(cells.numel()), int(offsets.numel()) - 1
    assert vis.dtype == torch.int64 and vis.is_contiguous() and vis.device == dev
    if 1 <= int(span) <= SIGHT_MAX_SPAN:                        # any other span launches nothing: the library says why
        W = grid_sight_words(span)
        assert tuple(vis.shape) == (P, W), f"vis {tuple(vis.shape)}: ({P}, {W})"
    some = P > 0 and legs > 0
    rc = lib.pi3_grid_route_sight_paths(walk.data_ptr(), nx, ny, nz, cells.data_ptr() if some else None, P,
                                        offsets.data_ptr() if some else None, legs, int(span),
                                        vis.data_ptr() if some else None, _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_sight_paths")


def grid_route_sight_pairs(walk: torch.Tensor, d2: Optional[torch.Tensor], a: torch.Tensor, b: torch.Tensor,
                           sees: torch.Tensor, touched: torch.Tensor, min_d2: torch.Tensor) -> None:
    """Line of sight between the cells a[i] and b[i] (int64 (N,) linear indices) over walk uint8 (nz,ny,nx): sees uint8
    (N,) = 1 when every cell the segment between the two centres touches is traversable, touched int32 (N,) = those
    cells' number (the whole segment is walked), min_d2 int16 (N,) (the uint16 values) = the smallest entry of d2 int16
    (nz,ny,nx) (grid_edt's field) over them, EDT_FAR without d2.  An end outside the grid gives 0, 0, EDT_FAR."""
    lib = _L.load()
    nx, ny, nz = _grid_state(walk)
    dev = walk.device
    assert 0 < walk.numel() <= ROUTE_MAX_CELLS, f"{walk.numel()} cells: 1 .. 2^27"
    if d2 is not None:
        assert d2.dtype == torch.int16 and d2.is_contiguous() and d2.shape == walk.shape and d2.device == dev
    N = int(a.numel())
    for t, dt in ((a, torch.int64), (b, torch.int64), (sees, torch.uint8), (touched, torch.int32), (min_d2, torch.int16)):
        assert t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (N,) and t.device == dev
    p = (lambda t: t.data_ptr() if N else None)
    rc = lib.pi3_grid_route_sight_pairs(walk.data_ptr(), _L.ptr(d2), nx, ny, nz, p(a), p(b), N, p(sees), p(touched),
                                        p(min_d2), _L.stream_ptr())
    _L.check(rc, "pi3_grid_route_sight_pairs")


# ---- frontiers of the occupancy grid (csrc/grid_frontier.hip)
FRONTIER_NONE = 0xFFFFFFFF              # the label of a cell that is no frontier cell
FRONTIER_MARK_COUNTERS = ("frontier_cells", "unknown_faces")
FRONTIER_STATS_COUNTERS = ("cells_reduced", "cells_without_root", "cells_reachable")
FRONTIER_STATS_FIELDS = ("cells", "unknown_faces", "sum_x", "sum_y", "sum_z", "min_x", "min_y", "min_z", "max_x",
                         "max_y", "max_z", "best")
FRONTIER_KEY_SHIFT = 27                 # best = (cost << 27) | cell as uint64, all ones when no cell is reachable


def grid_frontier_mark(state: torch.Tensor, label: torch.Tensor, counters: torch.Tensor) -> None:
    """label int32 (nz,ny,nx) (the uint32 values) = the cell's own linear index where state uint8 (nz,ny,nx) is free
    and one of the 6 face neighbours is unknown (outside the grid counts as unknown), else FRONTIER_NONE.  counters
    int64 (4,) = FRONTIER_MARK_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(label)
    dev = label.device
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.shape == label.shape and state.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    rc = lib.pi3_grid_frontier_mark(state.data_ptr(), nx, ny, nz, label.data_ptr(), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_frontier_mark")


def grid_frontier_sweep(label: torch.Tensor, changed: torch.Tensor) -> None:
    """One sweep of minimum-label propagation over the 26-connected labelled cells of label int32 (nz,ny,nx) (tiles of
    8 x 8 x 8 cells, each relaxed to its fixed point); changed int32 (1,) becomes 1 when a cell got lower (the caller
    zeroes it)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(label)
    assert changed.dtype == torch.int32 and changed.numel() == 1 and changed.device == label.device
    rc = lib.pi3_grid_frontier_sweep(nx, ny, nz, label.data_ptr(), changed.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_frontier_sweep")


def grid_frontier_roots(label: torch.Tensor, roots: torch.Tensor, count: torch.Tensor) -> None:
    """The cells with label[c] == c into roots int64 (cap,), in any order; count int64 (1,) = their number, also when
    it exceeds cap (the caller checks)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(label)
    dev = label.device
    assert roots.dtype == torch.int64 and roots.is_contiguous() and roots.ndim == 1 and roots.device == dev
    assert count.dtype == torch.int64 and count.numel() == 1 and count.device == dev
    cap = int(roots.numel())
    rc = lib.pi3_grid_frontier_roots(label.data_ptr(), nx, ny, nz, roots.data_ptr() if cap else None, cap,
                                     count.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_frontier_roots")


def grid_frontier_stats(state: torch.Tensor, label: torch.Tensor, dist: Optional[torch.Tensor],
                        roots_sorted: torch.Tensor, stats: torch.Tensor, counters: torch.Tensor) -> None:
    """stats int64 (K,12) = FRONTIER_STATS_FIELDS per cluster of the settled label int32 (nz,ny,nx): row k reduces the
    cells whose label is roots_sorted[k] (int64 (K,), ascending).  dist int32 (nz,ny,nx) (a settled route field, the
    uint32 values) or None: `best` is then all ones.  counters int64 (4,) = FRONTIER_STATS_COUNTERS (zeroed by the
    call)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(label)
    dev = label.device
    assert state.dtype == torch.uint8 and state.is_contiguous() and state.shape == label.shape and state.device == dev
    if dist is not None:
        assert dist.dtype == torch.int32 and dist.is_contiguous() and dist.shape == label.shape and dist.device == dev
    assert roots_sorted.dtype == torch.int64 and roots_sorted.is_contiguous() and roots_sorted.ndim == 1
    assert roots_sorted.device == dev
    K = int(roots_sorted.numel())
    assert stats.dtype == torch.int64 and stats.is_contiguous() and tuple(stats.shape) == (K, len(FRONTIER_STATS_FIELDS))
    assert stats.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    rc = lib.pi3_grid_frontier_stats(state.data_ptr(), label.data_ptr(), _L.ptr(dist), nx, ny, nz,
                                     roots_sorted.data_ptr() if K else None, K, stats.data_ptr() if K else None,
                                     counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_frontier_stats")


# ---- views of the occupancy grid (csrc/grid_view.hip)
VIEW_MAX_RANGE = 32                     # cells: the occupied bits of the (2 R + 1)^3 box live in LDS
VIEW_FAR_MAX_RANGE = 64                 # cells, the far form: the bits of one octant's (R + 1)^3 box per workgroup
VIEW_MAX_DEPTH = 255                    # unknown_depth: the unknown cells a ray may cross
VIEW_MAX_HEADINGS = 32
VIEW_MAX_AXIS = 1024                    # per component of a heading
VIEW_COUNTERS = ("candidates", "rays", "rays_blocked", "rays_visible")
VIEW_COS2_DEN = 1 << 20                 # cos^2 of half the field of view is passed as num / 2^20


def grid_view_candidates(dist: torch.Tensor, index_origin, stride: int, max_cost: int, cells: torch.Tensor,
                         count: torch.Tensor) -> None:
    """The cells of dist int32 (nz,ny,nx) (a settled route field, the uint32 values) with a finite dist <= max_cost whose
    absolute index index_origin + (x, y, z) is a multiple of stride on every axis, into cells int64 (cap,), in any
    order; count int64 (1,) = their number, also when it exceeds cap (the caller checks)."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist)
    dev = dist.device
    assert cells.dtype == torch.int64 and cells.is_contiguous() and cells.ndim == 1 and cells.device == dev
    assert count.dtype == torch.int64 and count.numel() == 1 and count.device == dev
    ox, oy, oz = (int(v) for v in index_origin)
    cap = int(cells.numel())
    rc = lib.pi3_grid_view_candidates(dist.data_ptr(), nx, ny, nz, ox, oy, oz, int(stride), int(max_cost),
                                      cells.data_ptr() if cap else None, cap, count.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_view_candidates")


def grid_view_candidates_stand(dist: torch.Tensor, height: torch.Tensor, index_origin, stride: int, max_cost: int,
                               up_axis: int, h_lo: int, cells: torch.Tensor, count: torch.Tensor) -> None:
    """grid_view_candidates for a standing planner (csrc/grid_stand.hip): on the two axes other than up_axis (0, 1, 2 =
    x, y, z) the absolute index is a multiple of stride; along it the lattice follows the floor, (height - h_lo) mod
    stride == 0 on height uint8 (nz,ny,nx) (grid_stand_height's field), 1 <= h_lo <= STAND_MAX_HEIGHT."""
    lib = _L.load()
    nx, ny, nz = _grid_field(dist)
    dev = dist.device
    assert height.dtype == torch.uint8 and height.is_contiguous() and height.shape == dist.shape and height.device == dev
    assert cells.dtype == torch.int64 and cells.is_contiguous() and cells.ndim == 1 and cells.device == dev
    assert count.dtype == torch.int64 and count.numel() == 1 and count.device == dev
    ox, oy, oz = (int(v) for v in index_origin)
    cap = int(cells.numel())
    rc = lib.pi3_grid_view_candidates_stand(dist.data_ptr(), height.data_ptr(), nx, ny, nz, ox, oy, oz, int(stride),
                                            int(max_cost), int(up_axis), int(h_lo), cells.data_ptr() if cap else None, cap,
                                            count.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_grid_view_candidates_stand")


def _view_entry(lib, name: str, view_range: int, far: bool):
    """The entry point `name`, or its far form (ranges up to VIEW_FAR_MAX_RANGE, the same bytes) when the range needs it
    or `far` asks for it -> (the function, its name)."""
    if far or int(view_range) > VIEW_MAX_RANGE:
        name += "_far"
    return getattr(lib, name), name


def _view_depth(unknown_depth) -> Optional[int]:
    """unknown_depth as the depth entry points take it: None (the transparent entry points) or an integer in
    0 .. VIEW_MAX_DEPTH."""
    if unknown_depth is None:
        return None
    assert not isinstance(unknown_depth, bool) and int(unknown_depth) == unknown_depth, \
        f"unknown_depth {unknown_depth!r}: None or an integer"
    assert 0 <= int(unknown_depth) <= VIEW_MAX_DEPTH, f"unknown_depth {unknown_depth}: 0 .. {VIEW_MAX_DEPTH}"
    return int(unknown_depth)


class ViewFrustum(NamedTuple):
    """The frustum form of the ray calls: frames (H,6) integers, row h = f (forward) then r (right), both
    non-zero, orthogonal, components within +-VIEW_MAX_FRAME; tan^2 of half the horizontal and the vertical field of
    view as fractions, 0 <= num <= VIEW_MAX_TAN2, 1 <= den <= VIEW_MAX_TAN2."""
    frames: object
    tan2_h_num: int
    tan2_h_den: int
    tan2_v_num: int
    tan2_v_den: int


VIEW_MAX_FRAME = 64                     # per component of a frame's f and r
VIEW_MAX_TAN2 = 1 << 20                 # the largest numerator and denominator of a tan^2 fraction


def _view_frustum(frustum: ViewFrustum, unknown_depth, view_range: int, far: bool):
    """A frustum call's arguments -> (the frames as a ctypes array, H, what stands between range and frames (depth,
    far), the four fraction terms).  The entry points check the frames' rules and name them."""
    fr = np.ascontiguousarray(frustum.frames, dtype=np.int64)
    assert fr.ndim == 2 and fr.shape[1] == 6 and 1 <= len(fr) <= VIEW_MAX_HEADINGS, \
        f"frames of shape {fr.shape}: (H, 6) with H in 1 .. {VIEW_MAX_HEADINGS}"
    assert int(np.abs(fr).max()) <= VIEW_MAX_FRAME, f"a frame's components lie within +-{VIEW_MAX_FRAME}"
    H = len(fr)
    depth = _view_depth(unknown_depth)
    form = (-1 if depth is None else depth, int(bool(far) or int(view_range) > VIEW_MAX_RANGE))
    return (C.c_int * (6 * H))(*[int(c) for c in fr.reshape(-1)]), H, form, tuple(int(v) for v in frustum[1:])


VIEW_MARK_COUNTERS = ("views", "rays", "rays_visible", "in_cone", "new")
VIEW_MAX_TAG = 32767                    # owner is int16


def grid_view_seen_words(cells: int) -> int:
    """The int32 words of a seen mask over `cells` cells: cell c is bit c & 31 of word c >> 5."""
    return (int(cells) + 31) >> 5


def _view_headings(headings):
    hd = [tuple(int(c) for c in a) for a in headings]
    H = len(hd)
    assert 1 <= H <= VIEW_MAX_HEADINGS, f"{H} headings: 1 .. {VIEW_MAX_HEADINGS}"
    assert all(len(a) == 3 and any(a) and max(abs(c) for c in a) <= VIEW_MAX_AXIS for a in hd), \
        f"a heading is no non-zero integer axis (x, y, z) within +-{VIEW_MAX_AXIS}"
    return (C.c_int * (3 * H))(*[c for a in hd for c in a]), H


def _view_seen(seen: torch.Tensor, state: torch.Tensor) -> None:
    assert seen.dtype == torch.int32 and seen.is_contiguous() and seen.ndim == 1 and seen.device == state.device
    assert int(seen.numel()) == grid_view_seen_words(state.numel()), \
        f"a mask of {seen.numel()} words for {state.numel()} cells: {grid_view_seen_words(state.numel())}"


def _view_grid(state: torch.Tensor, seen: Optional[torch.Tensor]):
    """What every ray call checks first: the grid and, where the call has one, its mask -> (nx, ny, nz)."""
    dims = _grid_state(state)
    assert 0 < state.numel() <= ROUTE_MAX_CELLS, f"{state.numel()} cells: 1 .. 2^27"
    if seen is not None:
        _view_seen(seen, state)
    return dims


def _view_gain(name: str, state, seen, candidates, view_range, headings, cos2_num, cos2_den, gain, visible, best,
               counters, far, unknown_depth=None, frustum=None) -> None:
    """grid_view_gain (seen None) and grid_view_gain_unseen: the entry points differ in the mask argument.  With an
    unknown_depth both go to pi3_grid_view_gain_depth, which takes the mask or NULL, the depth and the form; with a
    frustum to pi3_grid_view_gain_frustum, which takes those and the frames instead of the cones."""
    lib = _L.load()
    nx, ny, nz = _view_grid(state, seen)
    dev = state.device
    assert candidates.dtype == torch.int64 and candidates.is_contiguous() and candidates.ndim == 1
    assert candidates.device == dev
    V = int(candidates.numel())
    if frustum is None:
        flat, H = _view_headings(headings)
        shape = (int(cos2_num), int(cos2_den))
    else:
        flat, H, frustum_form, shape = _view_frustum(frustum, unknown_depth, view_range, far)
    assert gain.dtype == torch.int32 and gain.is_contiguous() and tuple(gain.shape) == (V, H) and gain.device == dev
    for t in (visible, best):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (V,) and t.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    depth = _view_depth(unknown_depth)
    if frustum is not None:
        entry, name = lib.pi3_grid_view_gain_frustum, "pi3_grid_view_gain_frustum"
        mask, form = (_L.ptr(seen),), frustum_form
    elif depth is None:
        entry, name = _view_entry(lib, name, view_range, far)
        mask, form = () if seen is None else (seen.data_ptr(),), ()
    else:
        entry, name = lib.pi3_grid_view_gain_depth, "pi3_grid_view_gain_depth"
        mask, form = (_L.ptr(seen),), (depth, int(bool(far) or int(view_range) > VIEW_MAX_RANGE))
    rc = entry(state.data_ptr(), nx, ny, nz, *mask, candidates.data_ptr() if V else None, V, int(view_range), *form,
               flat, H, *shape, gain.data_ptr() if V else None, visible.data_ptr() if V else None,
               best.data_ptr() if V else None, counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, name)


def grid_view_gain(state: torch.Tensor, candidates: torch.Tensor, view_range: int, headings, cos2_num: int,
                   cos2_den: int, gain: torch.Tensor, visible: torch.Tensor, best: torch.Tensor,
                   counters: torch.Tensor, far: bool = False, unknown_depth: Optional[int] = None,
                   frustum: Optional[ViewFrustum] = None) -> None:
    """Per entry of candidates int64 (V,) (linear indices into state uint8 (nz,ny,nx)): visible int32 (V,) (the uint32
    values) = the unknown cells within view_range cells that no occupied cell hides, gain int32 (V,H) = those in the
    cone of each of the H integer axes `headings` (H,3) (x, y, z) at cos^2 of the half angle cos2_num / cos2_den, best
    int32 (V,) = the smallest heading of the largest gain (-1 and zeros for a candidate outside the grid).  counters
    int64 (4,) = VIEW_COUNTERS (zeroed by the call).  A view_range above VIEW_MAX_RANGE, up to VIEW_FAR_MAX_RANGE, goes
    to the far entry point (the octant form of csrc/grid_view.hip); far=True sends any range there.  unknown_depth K in
    0 .. VIEW_MAX_DEPTH: a cell is visible only when at most K cells between it and the candidate are
    unknown as well; rays_blocked then counts every ray that did not arrive.  None: unknown cells are transparent.
    frustum (a ViewFrustum): heading h is the frustum of frames[h] instead of a cone, H = len(frames);
    headings, cos2_num and cos2_den are then not read."""
    _view_gain("pi3_grid_view_gain", state, None, candidates, view_range, headings, cos2_num, cos2_den, gain, visible,
               best, counters, far, unknown_depth, frustum)


def grid_view_gain_unseen(state: torch.Tensor, seen: torch.Tensor, candidates: torch.Tensor, view_range: int, headings,
                          cos2_num: int, cos2_den: int, gain: torch.Tensor, visible: torch.Tensor, best: torch.Tensor,
                          counters: torch.Tensor, far: bool = False, unknown_depth: Optional[int] = None,
                          frustum: Optional[ViewFrustum] = None) -> None:
    """grid_view_gain over the unknown cells whose bit of seen int32 (grid_view_seen_words(cells),) (the uint32 words) is
    clear; every output keeps its shape and meaning, and with an all-zero mask its bytes.  view_range, far,
    unknown_depth and frustum as there."""
    _view_gain("pi3_grid_view_gain_unseen", state, seen, candidates, view_range, headings, cos2_num, cos2_den, gain,
               visible, best, counters, far, unknown_depth, frustum)


def grid_view_mark(state: torch.Tensor, seen: torch.Tensor, cells: torch.Tensor, heading_of, view_range: int, headings,
                   cos2_num: int, cos2_den: int, counters: torch.Tensor, owner: Optional[torch.Tensor] = None,
                   tag: int = 0, far: bool = False, unknown_depth: Optional[int] = None,
                   frustum: Optional[ViewFrustum] = None) -> None:
    """Sets in seen int32 (grid_view_seen_words(cells),) the bit of every unknown cell within view_range cells of cells[i]
    (int64 (V,), linear indices on the device) that no occupied cell hides and that lies in the cone of heading
    heading_of[i] (V host integers in -1 .. H - 1; -1: in the cone of any heading).  owner int16 (nz,ny,nx), only with
    V == 1: the cells whose bit this call turned get `tag` (0 .. VIEW_MAX_TAG).  counters int64 (5,) =
    VIEW_MARK_COUNTERS (zeroed by the call).  view_range, far, unknown_depth and frustum as grid_view_gain's ("cone"
    then reads "frustum of the frame")."""
    lib = _L.load()
    nx, ny, nz = _view_grid(state, seen)
    dev = state.device
    assert cells.dtype == torch.int64 and cells.is_contiguous() and cells.ndim == 1 and cells.device == dev
    V = int(cells.numel())
    if frustum is None:
        flat, H = _view_headings(headings)
        shape = (int(cos2_num), int(cos2_den))
    else:
        flat, H, frustum_form, shape = _view_frustum(frustum, unknown_depth, view_range, far)
    hof = np.ascontiguousarray(heading_of, dtype=np.int32).reshape(-1)
    assert len(hof) == V and bool(((hof >= -1) & (hof < H)).all()), f"{V} rows need {V} headings in -1 .. {H - 1}"
    assert 0 <= int(tag) <= VIEW_MAX_TAG, f"tag {tag}: 0 .. {VIEW_MAX_TAG}"
    if owner is not None:
        assert owner.dtype == torch.int16 and owner.is_contiguous() and owner.shape == state.shape and owner.device == dev
        assert V == 1, f"an owner takes one row per call, got {V}"
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 5 and counters.device == dev
    depth = _view_depth(unknown_depth)
    if frustum is not None:
        entry, name, form = lib.pi3_grid_view_mark_frustum, "pi3_grid_view_mark_frustum", frustum_form
    elif depth is None:
        (entry, name), form = _view_entry(lib, "pi3_grid_view_mark", view_range, far), ()
    else:
        entry, name = lib.pi3_grid_view_mark_depth, "pi3_grid_view_mark_depth"
        form = (depth, int(bool(far) or int(view_range) > VIEW_MAX_RANGE))
    rc = entry(state.data_ptr(), nx, ny, nz, seen.data_ptr(), cells.data_ptr() if V else None,
               hof.ctypes.data_as(C.POINTER(C.c_int)) if V else None, V, int(view_range), *form, flat, H, *shape,
               _L.ptr(owner), int(tag), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, name)


# ---- nearest neighbours between two clouds (csrc/cloud_nn.hip)
CLOUD_INDEX_COUNTERS = ("dropped", "cells", "no_slot", "largest_cell")
CLOUD_NEAREST_COUNTERS = ("dropped", "matched", "beyond", "evaluations")
CLOUD_CELL_FACTOR = 1.25    # cell edge in units of max_dist: the 27 cells around a query then hold every candidate


def cloud_inv_cell(max_dist: float) -> float:
    """The fp32 inverse cell edge for a search radius: cells of CLOUD_CELL_FACTOR * max_dist."""
    md = float(max_dist)
    if not (md > 0.0 and math.isfinite(md)):
        raise ValueError(f"max_dist must be finite and positive, got {max_dist}")
    inv = C.c_float(1.0 / (CLOUD_CELL_FACTOR * md)).value          # rounded to fp32, as the kernels receive it
    if not (inv > 0.0 and math.isfinite(inv)):
        raise ValueError(f"max_dist {max_dist}: 1 / cell is not a positive finite float32")
    return inv


def cloud_index_build(points: torch.Tensor, inv_cell: float, table: torch.Tensor, cells: torch.Tensor,
                      counters: torch.Tensor) -> None:
    """points f32 (n,3) -> table int64 (8 capacity,) (64-byte slots: key, count, start, fill, cursor; capacity =
    voxel_capacity(n)) and cells int32 (n,4) = x y z bits + original index, grouped by cell; counters int64 (4,) =
    CLOUD_INDEX_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    dev = table.device
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    n = int(points.shape[0])
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0 and table.is_cuda
    assert cells.dtype == torch.int32 and cells.is_contiguous() and tuple(cells.shape) == (n, 4)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4
    assert points.device == dev and cells.device == dev and counters.device == dev
    rc = lib.pi3_cloud_index_build(points.data_ptr() if n else None, n, float(inv_cell), table.data_ptr(),
                                   table.numel() // 8, cells.data_ptr() if n else None, counters.data_ptr(),
                                   _L.stream_ptr())
    _L.check(rc, "pi3_cloud_index_build")


def cloud_nearest(table: torch.Tensor, cells: torch.Tensor, inv_cell: float, queries: torch.Tensor, max_dist: float,
                  d2: torch.Tensor, idx: torch.Tensor, counters: torch.Tensor) -> None:
    """queries f32 (m,3) against cloud_index_build's table and cells: d2 f64 (m,) = (dx dx + dy dy) + dz dz of the
    nearest indexed point within max_dist (inclusive; ties: the smallest original index), idx int32 (m,) its index;
    +inf / -1 without one; counters int64 (4,) = CLOUD_NEAREST_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    dev = table.device
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0 and table.is_cuda
    assert cells.dtype == torch.int32 and cells.is_contiguous() and cells.ndim == 2 and cells.shape[1] == 4
    assert queries.dtype == torch.float32 and queries.is_contiguous() and queries.ndim == 2 and queries.shape[1] == 3
    n, m = int(cells.shape[0]), int(queries.shape[0])
    assert d2.dtype == torch.float64 and d2.is_contiguous() and d2.numel() == m
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == m
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4
    assert all(t.device == dev for t in (cells, queries, d2, idx, counters))
    rc = lib.pi3_cloud_nearest(table.data_ptr(), table.numel() // 8, cells.data_ptr() if n else None, n, float(inv_cell),
                               queries.data_ptr() if m else None, m, float(max_dist), d2.data_ptr() if m else None,
                               idx.data_ptr() if m else None, counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_cloud_nearest")


# ---- nearest triangle of a mesh (csrc/mesh_nn.hip)
MESH_INDEX_COUNTERS = ("dropped", "cells", "no_slot", "largest_cell", "rows")
MESH_NEAREST_COUNTERS = ("dropped", "matched", "beyond", "evaluations")
MESH_MAX_ROWS = 2 ** 31 - 1


def _mesh_args(vertices: torch.Tensor, faces: torch.Tensor) -> Tuple[int, int]:
    assert vertices.dtype == torch.float32 and vertices.is_contiguous() and vertices.ndim == 2 and vertices.shape[1] == 3
    assert faces.dtype == torch.int32 and faces.is_contiguous() and faces.ndim == 2 and faces.shape[1] == 3
    assert vertices.is_cuda and faces.device == vertices.device
    return int(vertices.shape[0]), int(faces.shape[0])


def mesh_index_count(vertices: torch.Tensor, faces: torch.Tensor, inv_cell: float, table: torch.Tensor,
                     packed: torch.Tensor, max_rows: int, counters: torch.Tensor) -> None:
    """vertices f32 (V,3), faces int32 (F,3) -> table int64 (8 capacity,) cleared and, unless the row total exceeds
    max_rows, holding the rows per cell; packed f32 (F,12) = a, b, c, 2 spare, face index (-1 = dropped); counters
    int64 (8,) = MESH_INDEX_COUNTERS + 3 spare (zeroed by the call; 'largest_cell' comes from the fill)."""
    lib = _L.load()
    V, F = _mesh_args(vertices, faces)
    dev = vertices.device
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    assert packed.dtype == torch.float32 and packed.is_contiguous() and tuple(packed.shape) == (F, 12)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 8
    assert table.device == dev and packed.device == dev and counters.device == dev
    rc = lib.pi3_mesh_index_count(vertices.data_ptr() if V else None, V, faces.data_ptr() if F else None, F,
                                  float(inv_cell), table.data_ptr(), table.numel() // 8, packed.data_ptr() if F else None,
                                  int(max_rows), counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_mesh_index_count")


def mesh_index_fill(table: torch.Tensor, packed: torch.Tensor, inv_cell: float, rows: torch.Tensor,
                    counters: torch.Tensor) -> None:
    """After mesh_index_count with the same table, packed and inv_cell: rows int32 (counters['rows'],) = the face
    indices grouped by cell; counters (the count call's) gains 'largest_cell'."""
    lib = _L.load()
    dev = table.device
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0 and table.is_cuda
    assert packed.dtype == torch.float32 and packed.is_contiguous() and packed.ndim == 2 and packed.shape[1] == 12
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.ndim == 1
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 8
    assert packed.device == dev and rows.device == dev and counters.device == dev
    F, n = int(packed.shape[0]), int(rows.numel())
    rc = lib.pi3_mesh_index_fill(table.data_ptr(), table.numel() // 8, packed.data_ptr() if F else None, F,
                                 float(inv_cell), rows.data_ptr() if n else None, n, counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_mesh_index_fill")


def mesh_nearest(table: torch.Tensor, rows: torch.Tensor, packed: torch.Tensor, inv_cell: float, queries: torch.Tensor,
                 max_dist: float, d2: torch.Tensor, face: torch.Tensor, closest: torch.Tensor,
                 counters: torch.Tensor) -> None:
    """queries f32 (m,3) against the index of mesh_index_count / mesh_index_fill: d2 f64 (m,) to the nearest triangle
    within max_dist (inclusive; ties: the smallest face index), face int32 (m,), closest f32 (m,3) the point of that
    triangle; +inf / -1 / 0 without one; counters int64 (4,) = MESH_NEAREST_COUNTERS (zeroed by the call)."""
    lib = _L.load()
    dev = table.device
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0 and table.is_cuda
    assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.ndim == 1
    assert packed.dtype == torch.float32 and packed.is_contiguous() and packed.ndim == 2 and packed.shape[1] == 12
    assert queries.dtype == torch.float32 and queries.is_contiguous() and queries.ndim == 2 and queries.shape[1] == 3
    F, n, m = int(packed.shape[0]), int(rows.numel()), int(queries.shape[0])
    assert d2.dtype == torch.float64 and d2.is_contiguous() and d2.numel() == m
    assert face.dtype == torch.int32 and face.is_contiguous() and face.numel() == m
    assert closest.dtype == torch.float32 and closest.is_contiguous() and tuple(closest.shape) == (m, 3)
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4
    assert all(t.device == dev for t in (rows, packed, queries, d2, face, closest, counters))
    rc = lib.pi3_mesh_nearest(table.data_ptr(), table.numel() // 8, rows.data_ptr() if n else None, n,
                              packed.data_ptr() if F else None, F, float(inv_cell), queries.data_ptr() if m else None, m,
                              float(max_dist), d2.data_ptr() if m else None, face.data_ptr() if m else None,
                              closest.data_ptr() if m else None, counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_mesh_nearest")


# ---- area-weighted samples of a mesh's surface (csrc/mesh_sample.hip)
def mesh_sample_counts(vertices: torch.Tensor, faces: torch.Tensor, spacing: float, seed: int, counts: torch.Tensor,
                       counters: torch.Tensor) -> None:
    """counts int64 (F,) = samples per face at one per spacing^2 of area on average (0 for a dropped face); counters
    int64 (4,) = dropped faces + 3 spare (zeroed by the call)."""
    lib = _L.load()
    V, F = _mesh_args(vertices, faces)
    dev = vertices.device
    assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() == F and counts.device == dev
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4 and counters.device == dev
    rc = lib.pi3_mesh_sample_counts(vertices.data_ptr() if V else None, V, faces.data_ptr() if F else None, F,
                                    float(spacing), int(seed) & (2 ** 64 - 1), counts.data_ptr() if F else None,
                                    counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_mesh_sample_counts")


def mesh_sample_points(vertices: torch.Tensor, faces: torch.Tensor, offsets: torch.Tensor, seed: int,
                       points: torch.Tensor, face: torch.Tensor, normals: torch.Tensor) -> None:
    """offsets int64 (F+1,) = the exclusive prefix sums of mesh_sample_counts' counts -> points f32 (n,3), face int32
    (n,), normals f32 (n,3) with n = points.shape[0] = offsets[F]."""
    lib = _L.load()
    V, F = _mesh_args(vertices, faces)
    dev = vertices.device
    n = int(points.shape[0])
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.numel() == F + 1 and offsets.device == dev
    assert points.dtype == torch.float32 and points.is_contiguous() and tuple(points.shape) == (n, 3)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and tuple(normals.shape) == (n, 3)
    assert face.dtype == torch.int32 and face.is_contiguous() and face.numel() == n
    assert points.device == dev and normals.device == dev and face.device == dev
    rc = lib.pi3_mesh_sample_points(vertices.data_ptr() if V else None, V, faces.data_ptr(), F, offsets.data_ptr(), n,
                                    int(seed) & (2 ** 64 - 1), points.data_ptr() if n else None,
                                    face.data_ptr() if n else None, normals.data_ptr() if n else None, _L.stream_ptr())
    _L.check(rc, "pi3_mesh_sample_points")


# ---- the normal equations of one ICP step from a search's pairs (csrc/cloud_icp.hip)
CLOUD_ICP_COUNTERS = ("used", "unmatched", "trimmed", "normal_rejected")
CLOUD_ICP_SPAN = 4096       # queries per workgroup = per row of partials (kSpan of the kernel)
CLOUD_ICP_DOUBLES = 40      # A's upper triangle (28), b (7), r2, the sum of e.e, 3 spare


def cloud_icp_partial_rows(m: int) -> int:
    """Rows of CLOUD_ICP_DOUBLES doubles that cloud_pair_equations needs in `partials` for m queries."""
    return (max(int(m), 0) + CLOUD_ICP_SPAN - 1) // CLOUD_ICP_SPAN


def cloud_pair_equations(queries: torch.Tensor, points: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor,
                         trim_dist: float, centre, normals: Optional[torch.Tensor], normals_of: int, Rn,
                         partials: torch.Tensor, out: torch.Tensor, counters: torch.Tensor) -> None:
    """queries f32 (m,3) (the moved estimate, the rows cloud_nearest was given), points f32 (n,3) (the indexed cloud),
    idx int32 (m,), d2 f64 (m,) as cloud_nearest wrote them -> out f64 (40,) = A's upper triangle row-major (28), b (7),
    r2, the sum of e.e, 3 zeros, about `centre` (3 host floats) with parameters w (3), l, t (3); counters int64 (4,) =
    CLOUD_ICP_COUNTERS (zeroed by the call).  normals_of 0: point to point; 1: normals f32 (n,3), the target's; 2:
    normals f32 (m,3), the source's, rotated by Rn (9 host floats row-major, or None = identity).  partials f64
    (>= cloud_icp_partial_rows(m), 40): workspace.  Bitwise reproducible."""
    lib = _L.load()
    dev = out.device
    assert queries.dtype == torch.float32 and queries.is_contiguous() and queries.ndim == 2 and queries.shape[1] == 3
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    m, n = int(queries.shape[0]), int(points.shape[0])
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == m
    assert d2.dtype == torch.float64 and d2.is_contiguous() and d2.numel() == m
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= CLOUD_ICP_DOUBLES and out.is_cuda
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() % CLOUD_ICP_DOUBLES == 0
    assert all(t.device == dev for t in (queries, points, idx, d2, counters, partials))
    if normals_of in (1, 2):
        assert normals is not None and normals.dtype == torch.float32 and normals.is_contiguous() and normals.device == dev
        assert tuple(normals.shape) == ((n, 3) if normals_of == 1 else (m, 3)), (tuple(normals.shape), n, m, normals_of)
    c3 = (C.c_double * 3)(*torch.as_tensor(centre, dtype=torch.float64).reshape(3).tolist())
    r9 = None if Rn is None else (C.c_double * 9)(*torch.as_tensor(Rn, dtype=torch.float64).reshape(9).tolist())
    has_normals = normals_of in (1, 2) and normals.numel() > 0
    rc = lib.pi3_cloud_pair_equations(queries.data_ptr() if m else None, m, points.data_ptr() if n else None, n,
                                      idx.data_ptr() if m else None, d2.data_ptr() if m else None, float(trim_dist),
                                      C.cast(c3, C.c_void_p), normals.data_ptr() if has_normals else None,
                                      int(normals_of), None if r9 is None else C.cast(r9, C.c_void_p),
                                      partials.data_ptr() if partials.numel() else None,
                                      partials.numel() // CLOUD_ICP_DOUBLES, out.data_ptr(), counters.data_ptr(),
                                      _L.stream_ptr())
    _L.check(rc, "pi3_cloud_pair_equations")


# ---- loop closure: co-occupancy of the chunks' clouds (csrc/chunk_overlap.hip), the pose graph (csrc/pose_graph.hip)
CHUNK_OVERLAP_COUNTERS = ("dropped", "cells", "no_slot", "most_chunks")
CHUNK_OVERLAP_MAX_CHUNKS = 448      # seven 64-bit mask words per cell
POSE_GRAPH_OUT = ("final_cost", "initial_cost", "iterations", "accepted_steps", "lambda", "status")
POSE_GRAPH_STATUS = ("converged", "max_iterations", "factorisation_failed")


def chunk_cooccupancy(points: torch.Tensor, offsets: torch.Tensor, inv_cell: float, table: torch.Tensor,
                      counts: torch.Tensor, counters: torch.Tensor) -> None:
    """points f32 (P,3): all chunks' clouds in the world frame, chunk c the rows offsets[c] .. offsets[c+1]-1 (offsets
    int64 (C+1,) on the device) -> counts int64 (C,C): the cells (edge 1 / inv_cell) that chunks i and j both occupy,
    the diagonal the cells of chunk i; counters int64 (4,) = CHUNK_OVERLAP_COUNTERS.  table int64 (8 capacity,),
    capacity = voxel_capacity(P): workspace.  Everything is written by the call; exact integers."""
    lib = _L.load()
    dev = counts.device
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.ndim == 1 and offsets.numel() >= 1
    P, C = int(points.shape[0]), int(offsets.numel()) - 1
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    assert counts.dtype == torch.int64 and counts.is_contiguous() and tuple(counts.shape) == (C, C) and counts.is_cuda
    assert counters.dtype == torch.int64 and counters.is_contiguous() and counters.numel() >= 4
    assert all(t.device == dev for t in (points, offsets, table, counters))
    rc = lib.pi3_chunk_cooccupancy(points.data_ptr() if P else None, P, offsets.data_ptr(), C, float(inv_cell),
                                   table.data_ptr() if table.numel() else None, table.numel() // 8,
                                   counts.data_ptr() if C else None, counters.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_chunk_cooccupancy")


def pose_graph_workspace(n_nodes: int, n_edges: int) -> int:
    """Doubles of workspace pose_graph_sim3 needs for that many nodes and edges."""
    n = C.c_long(0)
    _L.check(_L.load(False).pi3_pose_graph_workspace(int(n_nodes), int(n_edges), C.byref(n)), "pi3_pose_graph_workspace")
    return int(n.value)


def pose_graph_sim3(nodes: torch.Tensor, centres: torch.Tensor, edges: torch.Tensor, Z: torch.Tensor,
                    edge_centres: torch.Tensor, info: torch.Tensor, fixed: torch.Tensor, max_iterations: int,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Levenberg-Marquardt on the Sim(3) pose graph, in place on nodes f64 (C,4,4) (include/pi3slam_hip.h states the
    model): centres f64 (C,3), edges int32 (E,2), Z f64 (E,4,4), edge_centres f64 (E,3), info f64 (E,28), fixed uint8
    (C,) -> out f64 (16,) on the device = POSE_GRAPH_OUT, ten zeros.  No synchronisation."""
    lib = _L.load()
    dev = nodes.device
    C, E = int(nodes.numel() // 16), int(edges.numel() // 2)
    assert nodes.dtype == torch.float64 and nodes.is_contiguous() and nodes.numel() == 16 * C and nodes.is_cuda
    assert centres.dtype == torch.float64 and centres.is_contiguous() and centres.numel() == 3 * C
    assert edges.dtype == torch.int32 and edges.is_contiguous() and edges.numel() == 2 * E
    assert Z.dtype == torch.float64 and Z.is_contiguous() and Z.numel() == 16 * E
    assert edge_centres.dtype == torch.float64 and edge_centres.is_contiguous() and edge_centres.numel() == 3 * E
    assert info.dtype == torch.float64 and info.is_contiguous() and info.numel() == 28 * E
    assert fixed.dtype == torch.uint8 and fixed.is_contiguous() and fixed.numel() == C
    assert all(t.device == dev for t in (centres, edges, Z, edge_centres, info, fixed))
    need = pose_graph_workspace(C, E)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    assert workspace.dtype == torch.float64 and workspace.is_contiguous() and workspace.device == dev
    out = torch.empty(16, dtype=torch.float64, device=dev)
    rc = lib.pi3_pose_graph_sim3(nodes.data_ptr(), centres.data_ptr(), C, edges.data_ptr() if E else None,
                                 Z.data_ptr() if E else None, edge_centres.data_ptr() if E else None,
                                 info.data_ptr() if E else None, E, fixed.data_ptr(), int(max_iterations),
                                 workspace.data_ptr(), workspace.numel(), out.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_pose_graph_sim3")
    return out


# ---------------------------------------------------------------------------------------------------- map renderer
RENDER_CAM_DOUBLES = 20     # world->camera 3x4 row-major, fx, fy, cx, cy, ortho flag, 3 spare (csrc/render.hip)


def render_splat(points: torch.Tensor, weights: Optional[torch.Tensor], cams: torch.Tensor, zbuf: torch.Tensor,
                 stats: torch.Tensor, H: int, W: int, voxel_size: float, splat_scale: float = 1.0, min_weight: int = 1,
                 near: float = 0.05, far: float = float("inf")) -> None:
    """points f32 (V,3), weights int32 (V,) or None, cams f64 (M,20) -> zbuf int64 (>= M H W words, the first M H W are
    cleared and written); stats int64 (4,) accumulates [0] voxels without a pixel and [1] radius clamps."""
    lib = _L.load()
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 2 and points.shape[1] == 3
    V = int(points.shape[0])
    if weights is not None:
        assert weights.dtype == torch.int32 and weights.is_contiguous() and weights.numel() == V
        assert weights.device == points.device
    assert cams.dtype == torch.float64 and cams.is_contiguous() and cams.ndim == 2 and cams.shape[1] == RENDER_CAM_DOUBLES
    M = int(cams.shape[0])
    assert zbuf.dtype == torch.int64 and zbuf.is_contiguous() and zbuf.numel() >= M * int(H) * int(W)
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 4
    assert cams.device == points.device and zbuf.device == points.device and stats.device == points.device
    rc = lib.pi3_render_splat(points.data_ptr(), _L.ptr(weights), V, cams.data_ptr(), M, int(H), int(W), float(voxel_size),
                              float(splat_scale), int(min_weight), float(near), float(far),
                              zbuf.data_ptr(), stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_render_splat")


def render_resolve(zbuf: torch.Tensor, colors: torch.Tensor, stats: torch.Tensor, M: int, H: int, W: int, out=None):
    """zbuf int64 (>= M H W) + colors uint8 (V,3) -> (depth f32 (M,H,W), color uint8 (M,H,W,3), index int32 (M,H,W)),
    `out` or fresh buffers; stats[2] accumulates the non-empty pixels."""
    lib = _L.load()
    M, H, W = int(M), int(H), int(W)
    assert zbuf.dtype == torch.int64 and zbuf.is_contiguous() and zbuf.numel() >= M * H * W
    assert colors.dtype == torch.uint8 and colors.is_contiguous() and colors.ndim == 2 and colors.shape[1] == 3
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 4
    assert colors.device == zbuf.device and stats.device == zbuf.device
    if out is None:
        out = (torch.empty(M, H, W, device=zbuf.device, dtype=torch.float32),
               torch.empty(M, H, W, 3, device=zbuf.device, dtype=torch.uint8),
               torch.empty(M, H, W, device=zbuf.device, dtype=torch.int32))
    depth, color, index = out
    assert depth.dtype == torch.float32 and depth.is_contiguous() and depth.numel() == M * H * W
    assert color.dtype == torch.uint8 and color.is_contiguous() and color.numel() == 3 * M * H * W
    assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == M * H * W
    assert depth.device == zbuf.device and color.device == zbuf.device and index.device == zbuf.device
    rc = lib.pi3_render_resolve(zbuf.data_ptr(), colors.data_ptr() if colors.numel() else None, int(colors.shape[0]), M, H,
                                W, depth.data_ptr(), color.data_ptr(), index.data_ptr(), stats.data_ptr(),
                                _L.stream_ptr())
    _L.check(rc, "pi3_render_resolve")
    return depth, color, index


# ------------------------------------------------------------------------------- normals of the voxel map, shading
VOXEL_NACC_WORDS = 4        # Nx, Ny, Nz, cnt as int64 per slot, parallel to the table (csrc/voxel_normals.hip)
VOXEL_NORMAL_COUNTERS = ("contributions", "skipped", "degenerate", "lost")


def _nacc_check(table: torch.Tensor, nacc: torch.Tensor, stats: torch.Tensor) -> None:
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() % 8 == 0
    assert nacc.dtype == torch.int64 and nacc.is_contiguous() and nacc.device == table.device
    assert nacc.numel() == VOXEL_NACC_WORDS * (table.numel() // 8), "nacc must have 4 int64 per slot of the table"
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 4 and stats.device == table.device


def voxel_fuse_pixel_normals(table: torch.Tensor, nacc: torch.Tensor, stats: torch.Tensor, points: torch.Tensor,
                             conf: Optional[torch.Tensor], masks: Optional[torch.Tensor], conf_logit_thr: float,
                             inv_voxel: float) -> None:
    """After voxel_fuse_pixels on the same points f32 (N,H,W,3), conf, masks: the pixels' normals into nacc int64
    (capacity,4); stats int64 (4,) accumulates VOXEL_NORMAL_COUNTERS."""
    lib = _L.load()
    _nacc_check(table, nacc, stats)
    N, H, W = points.shape[:3]
    assert points.dtype == torch.float32 and points.is_contiguous() and points.ndim == 4 and points.shape[3] == 3
    if conf is not None:
        assert conf.dtype == torch.float32 and conf.is_contiguous() and conf.numel() == N * H * W
    if masks is not None:
        assert masks.dtype in (torch.uint8, torch.bool) and masks.is_contiguous() and masks.numel() == N * H * W
    rc = lib.pi3_voxel_fuse_pixel_normals(table.data_ptr(), table.numel() // 8, nacc.data_ptr(), points.data_ptr(),
                                          _L.ptr(conf), _L.ptr(masks), N, H, W, float(conf_logit_thr), float(inv_voxel),
                                          stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_fuse_pixel_normals")


def voxel_fuse_point_normals(table: torch.Tensor, nacc: torch.Tensor, stats: torch.Tensor, points: torch.Tensor,
                             normals: torch.Tensor, nweights: torch.Tensor, rot9: torch.Tensor, inv_voxel: float) -> None:
    """After voxel_fuse_points on the same (world-frame) points f32 (n,3): normals f32 (n,3) in the cloud's frame,
    nweights int32 (n,), rot9 f64 (9,) on the device, the rotation into the world frame."""
    lib = _L.load()
    _nacc_check(table, nacc, stats)
    assert points.dtype == torch.float32 and points.is_contiguous() and points.shape[-1] == 3
    n = points.numel() // 3
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.numel() == 3 * n
    assert nweights.dtype == torch.int32 and nweights.is_contiguous() and nweights.numel() == n
    assert rot9.dtype == torch.float64 and rot9.is_contiguous() and rot9.numel() == 9
    assert normals.device == table.device and nweights.device == table.device and rot9.device == table.device
    if n == 0:          # empty tensors have no address to pass
        return
    rc = lib.pi3_voxel_fuse_point_normals(table.data_ptr(), table.numel() // 8, nacc.data_ptr(), points.data_ptr(),
                                          normals.data_ptr(), nweights.data_ptr(), rot9.data_ptr(), n, float(inv_voxel),
                                          stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_fuse_point_normals")


def voxel_empty_normal_outputs(rows: int, device):
    """Output buffers of voxel_extract_normals: keys int64 (rows,), normals f32 (rows,3), nweights int32 (rows,)."""
    m = max(int(rows), 1)
    return (torch.empty(m, device=device, dtype=torch.int64), torch.empty(m, 3, device=device, dtype=torch.float32),
            torch.empty(m, device=device, dtype=torch.int32))


def voxel_extract_normals(table: torch.Tensor, nacc: torch.Tensor, stats: torch.Tensor, max_out: int, out=None,
                          keep: Optional[torch.Tensor] = None):
    """-> device (keys int64, normals f32 (,3), nweights int32) with >= max_out rows (`out`, or fresh buffers),
    unordered.  stats int64 (4,), zeroed by the call: rows, rows that did not fit, rows with a non-zero normal, spare.
    keep uint8 (capacity,): only the slots it marks."""
    lib = _L.load()
    _nacc_check(table, nacc, stats)
    keys, nrm, nw = out if out is not None else voxel_empty_normal_outputs(max_out, table.device)
    assert keys.dtype == torch.int64 and nrm.dtype == torch.float32 and nw.dtype == torch.int32
    assert keys.is_contiguous() and nrm.is_contiguous() and nw.is_contiguous()
    assert keys.shape[0] >= max_out and nrm.numel() >= 3 * max_out and nw.shape[0] >= max_out
    if keep is not None:
        _slot_array(keep, table, torch.uint8)
    rc = lib.pi3_voxel_extract_normals(table.data_ptr(), table.numel() // 8, nacc.data_ptr(), _L.ptr(keep),
                                       keys.data_ptr(), nrm.data_ptr(), nw.data_ptr(), int(max_out), stats.data_ptr(),
                                       _L.stream_ptr())
    _L.check(rc, "pi3_voxel_extract_normals")
    return keys, nrm, nw


def render_shade(index: torch.Tensor, normals: torch.Tensor, cams: torch.Tensor, stats: torch.Tensor, out=None):
    """index int32 (M,H,W) of render_resolve, normals f32 (V,3) of the map, cams f64 (M,20) -> (normal_rgb uint8
    (M,H,W,3), shaded uint8 (M,H,W)), `out` or fresh buffers; stats int64 (>= 1) accumulates the shaded pixels in [0]."""
    lib = _L.load()
    assert index.dtype == torch.int32 and index.is_contiguous() and index.ndim == 3
    M, H, W = (int(x) for x in index.shape)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.ndim == 2 and normals.shape[1] == 3
    assert cams.dtype == torch.float64 and cams.is_contiguous() and tuple(cams.shape) == (M, RENDER_CAM_DOUBLES)
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 1
    assert normals.device == index.device and cams.device == index.device and stats.device == index.device
    if out is None:
        out = (torch.empty(M, H, W, 3, device=index.device, dtype=torch.uint8),
               torch.empty(M, H, W, device=index.device, dtype=torch.uint8))
    rgb, shaded = out
    assert rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.numel() == 3 * M * H * W
    assert shaded.dtype == torch.uint8 and shaded.is_contiguous() and shaded.numel() == M * H * W
    assert rgb.device == index.device and shaded.device == index.device
    rc = lib.pi3_render_shade(index.data_ptr(), normals.data_ptr() if normals.numel() else None, int(normals.shape[0]),
                              cams.data_ptr(), M, H, W, rgb.data_ptr(), shaded.data_ptr(), stats.data_ptr(),
                              _L.stream_ptr())
    _L.check(rc, "pi3_render_shade")
    return rgb, shaded


# ------------------------------------------------------------------------- surface mesh of the voxel map (voxel_mesh.hip)
VOXEL_MESH_VERT_WORDS = 8   # x y z nx ny nz (fp32 bits), rgb | flags << 24, spare: uint32 per slot of the cell table
VOXEL_MESH_CELL_BYTES = 8 + 4 * VOXEL_MESH_VERT_WORDS
VOXEL_MESH_COUNTERS = ("sources", "cells", "overflow", "vertices", "quads", "ambiguous_faces", "vertex_rows", "quad_rows",
                       "vertex_rows_unstored", "quad_rows_unstored")


def _mesh_check(table: torch.Tensor, nacc: torch.Tensor, keep: Optional[torch.Tensor], stats: torch.Tensor) -> None:
    _nacc_check(table, nacc, stats)
    assert stats.numel() >= 12
    if keep is not None:
        _slot_array(keep, table, torch.uint8)


def _mesh_cells_check(cells: torch.Tensor, device) -> int:
    cap = int(cells.numel())
    assert cells.dtype == torch.int64 and cells.is_contiguous() and cells.device == device
    assert cap > 0 and cap & (cap - 1) == 0, "the cell table's capacity must be a power of two"
    return cap


def voxel_mesh_cells(table: torch.Tensor, nacc: torch.Tensor, keep: Optional[torch.Tensor],
                     cells: Optional[torch.Tensor], stats: torch.Tensor) -> None:
    """The cell table of the mesh: cells int64 (cell_capacity,) is cleared and gets the keys of the 27 cells around every
    source voxel.  stats int64 (12,): [0] sources, [1] cells, [2] inserts that found no slot (the caller grows the table
    and calls again; nothing is written out of bounds).  cells None: only [0] is counted."""
    lib = _L.load()
    _mesh_check(table, nacc, keep, stats)
    ccap = _mesh_cells_check(cells, table.device) if cells is not None else 0
    rc = lib.pi3_voxel_mesh_cells(table.data_ptr(), table.numel() // 8, nacc.data_ptr(), _L.ptr(keep), _L.ptr(cells),
                                  ccap, stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_mesh_cells")


def voxel_mesh_vertices(table: torch.Tensor, nacc: torch.Tensor, keep: Optional[torch.Tensor], cells: torch.Tensor,
                        verts: torch.Tensor, voxel_size: float, stats: torch.Tensor) -> None:
    """One vertex per cell of voxel_mesh_cells' table with a sign change -> verts int32 (cell_capacity, 8); stats[3:6]
    = vertices, quads, ambiguous faces."""
    lib = _L.load()
    _mesh_check(table, nacc, keep, stats)
    ccap = _mesh_cells_check(cells, table.device)
    assert verts.dtype == torch.int32 and verts.is_contiguous() and verts.device == table.device
    assert verts.numel() == VOXEL_MESH_VERT_WORDS * ccap, "verts must have 8 int32 per slot of the cell table"
    rc = lib.pi3_voxel_mesh_vertices(table.data_ptr(), table.numel() // 8, nacc.data_ptr(), _L.ptr(keep),
                                     cells.data_ptr(), ccap, float(voxel_size), verts.data_ptr(), stats.data_ptr(),
                                     _L.stream_ptr())
    _L.check(rc, "pi3_voxel_mesh_vertices")


def voxel_mesh_extract(cells: torch.Tensor, verts: torch.Tensor, max_vertices: int, max_quads: int, stats: torch.Tensor):
    """-> device (vkeys int64 (V,), vxyz f32 (V,3), vnrm f32 (V,3), vrgb uint8 (V,3), qkeys int64 (Q,), qcodes int32 (Q,))
    with V = max_vertices and Q = max_quads rows, unordered; stats[6:10] = vertex rows, quad rows and the rows of either
    kind that did not fit."""
    lib = _L.load()
    ccap = _mesh_cells_check(cells, cells.device)
    assert verts.dtype == torch.int32 and verts.is_contiguous() and verts.device == cells.device
    assert verts.numel() == VOXEL_MESH_VERT_WORDS * ccap
    assert stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 12 and stats.device == cells.device
    V, Q, dev = max(int(max_vertices), 0), max(int(max_quads), 0), cells.device
    out = (torch.empty(V, device=dev, dtype=torch.int64), torch.empty(V, 3, device=dev, dtype=torch.float32),
           torch.empty(V, 3, device=dev, dtype=torch.float32), torch.empty(V, 3, device=dev, dtype=torch.uint8),
           torch.empty(Q, device=dev, dtype=torch.int64), torch.empty(Q, device=dev, dtype=torch.int32))
    ptr = [t.data_ptr() if t.numel() else None for t in out]
    rc = lib.pi3_voxel_mesh_extract(cells.data_ptr(), ccap, verts.data_ptr(), ptr[0], ptr[1], ptr[2], ptr[3], V, ptr[4],
                                    ptr[5], Q, stats.data_ptr(), _L.stream_ptr())
    _L.check(rc, "pi3_voxel_mesh_extract")
    return out


# ---------------------------------------------------------------------------------------------------- device guard
# Every wrapper launches on torch's CURRENT stream, i.e. on the current device.  A tensor that lives on another card
# (e.g. 'cuda:0' data in a rank bound to cuda:3) would hand that card's pointers to a kernel running elsewhere: fail
# loudly instead.  Checked on the first tensor argument of each call (all tensors of a call share a device by contract).
def _guarded(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        for a in args:
            if isinstance(a, torch.Tensor):
                if not a.is_cuda:
                    raise _L.Pi3HipError(f"{fn.__name__}: expected a device tensor, got {a.device}")
                if a.device.index != torch.cuda.current_device():
                    raise _L.Pi3HipError(
                        f"{fn.__name__}: tensor on {a.device} but the current device (and stream) is "
                        f"cuda:{torch.cuda.current_device()}; wrap the call in torch.cuda.device(t.device)")
                break
        return fn(*args, **kwargs)
    return wrapper


for _name, _fn in list(globals().items()):
    if isinstance(_fn, type(_guarded)) and getattr(_fn, "__module__", None) == __name__ and not _name.startswith("_") \
            and _name not in ("undistort_maps",):          # plain functions only (cuRoPE2D is a module class)
        globals()[_name] = _guarded(_fn)
del _name, _fn
