"""ctypes binding of the C-ABI kernel library (include/pi3slam_hip.h).

The library is the product: every arithmetic step of the hot path runs in it.  There is no CPU or eager-PyTorch
fallback — if the shared object is missing, fails to load, or no GPU is visible, the calls raise.
PyTorch is used only as the owner of device memory and streams: tensors are passed as raw device pointers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PI3_LIB_PATH: load another build of the same library (the AddressSanitizer host build of tests/test_asan_host.py)
LIB_PATH = os.environ.get("PI3_LIB_PATH") or os.path.join(_HERE, "libpi3slam_hip.so")

_vp, _i, _l, _f, _u64, _d = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_ulonglong, C.c_double

# name -> argtypes; every function returns int (0 = ok) except the two noted below.  Mirrors include/pi3slam_hip.h.
SIGNATURES = {
    "pi3_gemm": [_vp, _l, _vp, _l, _i, _i, _i, _i, _vp, _vp, _vp, _l, _vp, _l, _i, _i, _i, _i, _i, _vp, _l, _f, _i, _vp],
    "pi3_gemm_qkv": [_vp, _l, _vp, _l, _i, _i, _i, _vp, _vp, _l, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _i, _i, _vp],
    "pi3_attention": [_vp, _vp, _vp, _l, _l, _vp, _l, _l, _i, _i, _i, _i, _i, _vp, _i, _vp],
    "pi3_attention_path_counters": [_vp],
    "pi3_layernorm": [_vp, _l, _i, _i, _vp, _vp, _f, _vp, _l, _i, _i, _i, _vp, _vp],
    "pi3_qknorm_rope": [_vp, _l, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp],
    "pi3_rope_2d": [_vp, _vp, _i, _i, _i, _i, _l, _l, _l, _f, _f, _i, _vp],
    "pi3_cast_rows": [_vp, _l, _vp, _l, _l, _i, _i, _vp],
    "pi3_cast_rows_pad": [_vp, _l, _i, _vp, _l, _l, _i, _i, _vp],
    "pi3_patch_gather": [_vp, _i, _i, _i, _vp, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp],
    "pi3_resample_grid": [_vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp],
    "pi3_fill_tokens": [_vp, _i, _i, _i, _i, _i, _vp, _vp],
    "pi3_recipe_fill": [_vp, _l, _u64, _f, _f, _i, _vp],
    "pi3_unpatchify_points": [_vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "pi3_camera_tail": [_vp, _l, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "pi3_compute_masks": [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp],
    "pi3_masked_ratio_median": [_vp, _vp, _l, _vp, _l, _vp, _vp],
    "pi3_apply_scale": [_vp, _vp, _vp, _l, _vp, _i, _vp],
    "pi3_gather_keypoints": [_vp] * 6 + [_i] * 4 + [_vp] * 7,
    "pi3_focal_shift": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "pi3_conv3x3": [_vp, _l, _i, _i, _i, _i, _vp, _i, _vp, _vp, _l, _vp, _l, _i, _i, _i, _vp],
    "pi3_groupnorm_stats": [_vp, _l, _i, _i, _i, _i, _vp, _vp, _l, _vp],
    "pi3_groupnorm_apply": [_vp, _l, _i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _vp, _l, _i, _vp],
    "pi3_add_rows": [_vp, _l, _vp, _l, _l, _i, _vp],
    "pi3_convt_scatter": [_vp, _l, _i, _i, _i, _i, _i, _i, _vp, _l, _i, _vp],
    "pi3_uv_affine": [_vp, _l, _i, _i, _i, _i, _vp, _l, _i, _vp, _vp, _vp, _i, _vp],
    "pi3_resize_taps": [_vp, _l, _l, _l, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _l, _l, _l, _vp],
    "pi3_dense_vec": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "pi3_moge_remap": [_vp, _vp, _l, _i, _vp, _vp],
    "pi3_moge_depth": [_vp, _vp, _vp, _vp, _l, _vp, _vp],
    "pi3_sim3_match_keypoints": [_vp, _vp, _i, _i, _vp, _vp],
    "pi3_sim3_umeyama": [_vp] * 5 + [_i, _i, _vp, _i, _vp, _vp],
    "pi3_sim3_umeyama_weighted": [_vp] * 5 + [_i, _i, _vp, _i, _vp, _vp],
    "pi3_sim3_apply": [_vp, _vp, _l, _vp, _i, _vp],
    "pi3_sim3_compose_prefix": [_vp, _vp, _i, _vp],
    "pi3_project_observations": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "pi3_ingest_frames": [_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp],
    "pi3_undistort_maps": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "pi3_remap_bilinear_u8": [_vp, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp],
    "pi3_bundle_adjust": [_vp] * 7 + [_i, _i, _d, _i, _vp, _vp, _vp, _d, _d, _vp, _vp, _l, _vp],
    "pi3_bundle_adjust_homogeneous": [_vp] * 7 + [_i, _i, _d, _i, _vp, _vp, _vp, _d, _d, _vp, _vp, _l, _vp],
    "pi3_bundle_adjust_inverse_depth": [_vp] * 7 + [_i, _i, _d, _i, _vp, _vp, _vp, _d, _d, _vp, _vp, _l, _vp],
    "pi3_ba_outlier_tracks": [_vp] * 5 + [_i, _i, _d, _d, _vp, _vp],
    "pi3_voxel_clear": [_vp, _l, _vp, _vp],
    "pi3_voxel_fuse_pixels": [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp],
    "pi3_voxel_fuse_points": [_vp, _l, _vp, _vp, _vp, _l, _f, _vp, _vp],
    "pi3_voxel_rehash": [_vp, _l, _vp, _l, _vp, _vp],
    "pi3_voxel_extract": [_vp, _l, _d, _vp, _vp, _vp, _vp, _l, _vp, _vp],
    "pi3_voxel_extract_kept": [_vp, _l, _d, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp],
    "pi3_voxel_support": [_vp, _l, _u64, _i, _i, _vp, _vp, _vp, _vp],
    "pi3_voxel_support_excluding": [_vp, _l, _u64, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "pi3_voxel_label_init": [_vp, _l, _vp, _vp, _vp],
    "pi3_voxel_label_sweep": [_vp, _l, _vp, _vp, _vp],
    "pi3_voxel_component_sizes": [_vp, _l, _vp, _vp, _vp],
    "pi3_voxel_component_filter": [_vp, _l, _vp, _vp, _l, _vp, _vp, _vp],
    "pi3_dense_consistency": [_vp] * 6 + [_i, _i, _i, _f, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp],
    "pi3_dense_depth_planes": [_vp] * 4 + [_i, _i, _i, _f, _i, _i, _vp, _vp, _vp],
    "pi3_voxel_carve": [_vp, _l, _d, _vp, _i, _vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp],
    "pi3_cloud_follow_views": [_vp, _vp, _l, _vp, _vp, _i, _vp, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp],
    "pi3_cloud_index_build": [_vp, _l, _f, _vp, _l, _vp, _vp, _vp],
    "pi3_cloud_nearest": [_vp, _l, _vp, _l, _f, _vp, _l, _d, _vp, _vp, _vp, _vp],
    "pi3_cloud_pair_equations": [_vp, _l, _vp, _l, _vp, _vp, _d, _vp, _vp, _i, _vp, _vp, _l, _vp, _vp, _vp],
    "pi3_mesh_index_count": [_vp, _l, _vp, _l, _f, _vp, _l, _vp, _l, _vp, _vp],
    "pi3_mesh_index_fill": [_vp, _l, _vp, _l, _f, _vp, _l, _vp, _vp],
    "pi3_mesh_nearest": [_vp, _l, _vp, _l, _vp, _l, _f, _vp, _l, _d, _vp, _vp, _vp, _vp, _vp],
    "pi3_mesh_sample_counts": [_vp, _l, _vp, _l, _d, _u64, _vp, _vp, _vp],
    "pi3_mesh_sample_points": [_vp, _l, _vp, _l, _vp, _l, _u64, _vp, _vp, _vp, _vp],
    "pi3_render_splat": [_vp, _vp, _l, _vp, _i, _i, _i, _d, _d, _i, _d, _d, _vp, _vp, _vp],
    "pi3_render_resolve": [_vp, _vp, _l, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "pi3_voxel_fuse_pixel_normals": [_vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp],
    "pi3_voxel_fuse_point_normals": [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _f, _vp, _vp],
    "pi3_voxel_extract_normals": [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp],
    "pi3_render_shade": [_vp, _vp, _l, _vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "pi3_voxel_mesh_cells": [_vp, _l, _vp, _vp, _vp, _l, _vp, _vp],
    "pi3_voxel_mesh_vertices": [_vp, _l, _vp, _vp, _vp, _l, _d, _vp, _vp, _vp],
    "pi3_voxel_mesh_extract": [_vp, _l, _vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _l, _vp, _vp],
    "pi3_chunk_cooccupancy": [_vp, _l, _vp, _i, _f, _vp, _l, _vp, _vp, _vp],
    "pi3_occupancy_mark": [_vp, _l, _f] + [_i] * 6 + [_vp, _vp, _vp],
    "pi3_occupancy_observe": [_vp] + [_i] * 6 + [_d, _vp, _i, _vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp],
    "pi3_grid_edt": [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp],
    "pi3_grid_route_init": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _vp],
    "pi3_grid_route_sweep": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "pi3_grid_route_trace": [_vp, _vp, _i, _i, _i, _l, _vp, _l, _vp, _vp],
    "pi3_grid_route_fields_init": [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp],
    "pi3_grid_route_sweep_many": [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp],
    "pi3_grid_route_trace_many": [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp],
    "pi3_grid_route_sight_paths": [_vp, _i, _i, _i, _vp, _l, _vp, _i, _i, _vp, _vp],
    "pi3_grid_route_sight_pairs": [_vp, _vp, _i, _i, _i, _vp, _vp, _l, _vp, _vp, _vp, _vp],
    "pi3_grid_frontier_mark": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "pi3_grid_frontier_sweep": [_i, _i, _i, _vp, _vp, _vp],
    "pi3_grid_frontier_roots": [_vp, _i, _i, _i, _vp, _l, _vp, _vp],
    "pi3_grid_frontier_stats": [_vp, _vp, _vp, _i, _i, _i, _vp, _l, _vp, _vp, _vp],
    "pi3_grid_view_candidates": [_vp, _i, _i, _i, _i, _i, _i, _i, _l, _vp, _l, _vp, _vp],
    "pi3_grid_view_gain": [_vp, _i, _i, _i, _vp, _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _vp, _vp, _vp, _vp],
    "pi3_grid_view_gain_unseen": [_vp, _i, _i, _i, _vp, _vp, _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _vp, _vp, _vp, _vp],
    "pi3_grid_view_mark": [_vp, _i, _i, _i, _vp, _vp, C.POINTER(_i), _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _i, _vp,
                           _vp],
    "pi3_grid_view_gain_far": [_vp, _i, _i, _i, _vp, _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _vp, _vp, _vp, _vp],
    "pi3_grid_view_gain_unseen_far": [_vp, _i, _i, _i, _vp, _vp, _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _vp, _vp, _vp,
                                      _vp],
    "pi3_grid_view_mark_far": [_vp, _i, _i, _i, _vp, _vp, C.POINTER(_i), _l, _i, C.POINTER(_i), _i, _l, _l, _vp, _i, _vp,
                               _vp],
    "pi3_grid_view_gain_depth": [_vp, _i, _i, _i, _vp, _vp, _l, _i, _i, _i, C.POINTER(_i), _i, _l, _l, _vp, _vp, _vp, _vp,
                                 _vp],
    "pi3_grid_view_mark_depth": [_vp, _i, _i, _i, _vp, _vp, C.POINTER(_i), _l, _i, _i, _i, C.POINTER(_i), _i, _l, _l, _vp,
                                 _i, _vp, _vp],
    "pi3_grid_view_gain_frustum": [_vp, _i, _i, _i, _vp, _vp, _l, _i, _i, _i, C.POINTER(_i), _i, _l, _l, _l, _l, _vp, _vp,
                                   _vp, _vp, _vp],
    "pi3_grid_view_mark_frustum": [_vp, _i, _i, _i, _vp, _vp, C.POINTER(_i), _l, _i, _i, _i, C.POINTER(_i), _i, _l, _l, _l,
                                   _l, _vp, _i, _vp, _vp],
    "pi3_grid_stand_height": [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp],
    "pi3_grid_route_init_stand": [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _vp, _vp, _vp],
    "pi3_grid_view_candidates_stand": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _l, _i, _i, _vp, _l, _vp, _vp],
    "pi3_pose_graph_workspace": [_i, _i, C.POINTER(_l)],
    "pi3_pose_graph_sim3": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _l, _vp, _vp],
    "pi3_set_knob": [C.c_char_p, _l],
    "pi3_get_knob": [C.c_char_p, C.POINTER(_l)],
    "pi3_unset_knob": [C.c_char_p],
}


def set_knob(name: str, value: int) -> None:
    """Run-time A/B knob of the kernel library (speed only; tools/ interleave variants in one process with it)."""
    check(load(False).pi3_set_knob(name.encode(), int(value)), "pi3_set_knob")


def get_knob(name: str) -> Optional[int]:
    """The knob's value, or None when it is unset (the library then uses its default)."""
    v = _l(0)
    rc = load(False).pi3_get_knob(name.encode(), C.byref(v))
    if rc < 0:
        check(rc, "pi3_get_knob")
    return int(v.value) if rc == 1 else None


def restore_knob(name: str, previous: Optional[int]) -> None:
    """Put a knob back to what get_knob() returned before a temporary set_knob()."""
    if previous is None:
        check(load(False).pi3_unset_knob(name.encode()), "pi3_unset_knob")
    else:
        set_knob(name, previous)


def build_flavor() -> str:
    return load(False).pi3_build_flavor().decode()

_lib: Optional[C.CDLL] = None


class Pi3HipError(RuntimeError):
    pass


def load(require_gpu: bool = True) -> C.CDLL:
    """Load libpi3slam_hip.so (built by `__graft_entry__.build()` / `make -C pi3_slam_amd/csrc`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Pi3HipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "There is no CPU fallback for the hot path.")
        lib = C.CDLL(LIB_PATH)
        lib.pi3_last_error.restype = C.c_char_p
        lib.pi3_last_error.argtypes = []
        lib.pi3_abi_version.restype = _i
        if hasattr(lib, "pi3_build_flavor") or not os.environ.get("PI3_DEV_PARTIAL"):     # (an older build under PI3_DEV_PARTIAL)
            lib.pi3_build_flavor.restype = C.c_char_p
            lib.pi3_build_flavor.argtypes = []
        lib.pi3_device_count.restype = _i
        lib.pi3_groupnorm_ws_doubles.restype = _l
        lib.pi3_groupnorm_ws_doubles.argtypes = [_i, _i, _i]
        lib.pi3_ba_workspace_doubles.restype = _l
        lib.pi3_ba_workspace_doubles.argtypes = [_i, _i]
        for name, argt in SIGNATURES.items():
            if os.environ.get("PI3_DEV_PARTIAL") and not hasattr(lib, name):
                continue  # development builds of a subset of the kernels only
            fn = getattr(lib, name)  # AttributeError here == header/library mismatch: fail loudly
            fn.argtypes = argt
            fn.restype = _i
        _lib = lib
    if require_gpu and _lib.pi3_device_count() <= 0:
        raise Pi3HipError("no HIP device visible: the Pi3-SLAM hot path runs only on a GPU (gfx950)")
    return _lib


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise Pi3HipError("expected a device tensor")
    return t.data_ptr()


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load(False).pi3_last_error().decode("utf-8", "replace")
        raise Pi3HipError(f"{what or 'pi3 call'} failed (rc={rc}): {msg}")
