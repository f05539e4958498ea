"""Dense voxel map, the parts that need no GPU: the C ABI declares and exports the voxel entries, the configuration and
CLI carry the new options (off by default), and the numpy oracle's key / offset / merge arithmetic on hand-made cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import dense_map_ref as ref

VOXEL_ENTRIES = ("pi3_voxel_clear", "pi3_voxel_fuse_pixels", "pi3_voxel_fuse_points", "pi3_voxel_rehash",
                 "pi3_voxel_extract")


def test_header_declares_and_library_exports_voxel_entries(built_lib):
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    dll = ctypes.CDLL(built_lib)
    from pi3_slam_amd import lib
    for name in VOXEL_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(dll, name), name
        assert name in lib.SIGNATURES, name
    assert lib.load(require_gpu=False).pi3_abi_version() == 7


def test_voxel_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    """Argument checks run before any launch: NULL tables and non-power-of-two capacities come back as PI3_ERR_ARG."""
    from pi3_slam_amd import lib
    dll = lib.load(require_gpu=False)
    assert dll.pi3_voxel_clear(None, 1024, None, None) == -1
    assert dll.pi3_voxel_clear(ctypes.c_void_p(16), 1000, None, None) == -1
    assert dll.pi3_voxel_fuse_points(None, 1024, None, None, None, 0, 1.0, None, None) == -1
    assert dll.pi3_voxel_fuse_pixels(ctypes.c_void_p(16), 16, ctypes.c_void_p(16), None, None, None, 1, 4, 4, 0.0,
                                     1.0, ctypes.c_void_p(16), None) == -1      # capacity < 2 N H W
    assert dll.pi3_voxel_extract(ctypes.c_void_p(16), 64, 0.0, ctypes.c_void_p(16), ctypes.c_void_p(16),
                                 ctypes.c_void_p(16), ctypes.c_void_p(16), 1, ctypes.c_void_p(16), None) == -1
    assert b"pi3_voxel_extract" in dll.pi3_last_error()


def test_creator_config_dense_map_is_off_by_default(tmp_path):
    from pi3_slam_amd.chunk_creator import OfflineCreatorConfig
    cfg = OfflineCreatorConfig("recipe", str(tmp_path))
    assert cfg.dense_voxel_size is None
    assert cfg.dense_conf_threshold == 0.5


def test_cli_parses_dense_flags():
    from pi3_slam_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["create", "--images", "x", "--output", "o", "--dense-voxel-size", "0.02",
                      "--dense-conf-threshold", "0.7"])
    assert a.dense_voxel_size == 0.02 and a.dense_conf_threshold == 0.7
    a = p.parse_args(["create", "--images", "x", "--output", "o"])
    assert a.dense_voxel_size is None and a.dense_conf_threshold == 0.5
    a = p.parse_args(["online", "--output_path", "o", "--dense_voxel_size", "0.05", "--conf_threshold", "0.3"])
    assert a.dense_voxel_size == 0.05 and a.conf_threshold == 0.3
    assert p.parse_args(["online", "--output_path", "o"]).dense_voxel_size is None


def test_product_logit_threshold_matches_oracle():
    from pi3_slam_amd.dense_map import conf_logit_threshold, inverse_voxel
    for t in (0.0, 0.1, 0.5, 0.7, 0.999, 1.0):
        assert np.float32(conf_logit_threshold(t)) == ref.conf_logit(t)
    assert conf_logit_threshold(0.5) == 0.0
    assert inverse_voxel(0.02) == ref.inv_voxel(0.02)
    with pytest.raises(ValueError):
        inverse_voxel(0.0)


def _key(kx, ky, kz):
    return np.uint64(((kx + ref.BIAS) << 42) | ((ky + ref.BIAS) << 21) | (kz + ref.BIAS))


def test_oracle_keys_and_offsets_at_boundaries():
    # voxel 0.5: inv_v = 2 exactly, so s = 2 p is exact and the cases are easy to state
    p = np.array([[0.0, 0.0, 0.0],          # a voxel corner: k = 0, u = 0
                  [0.25, 0.49999997, 0.5],  # half a voxel; just below the boundary; exactly on it -> next voxel
                  [-0.25, -0.5, -1e-30],    # negative: floor; exactly -1 voxel; a tiny negative (s - k rounds to 1)
                  ], np.float32)
    ok, keys, u = ref.quantise(p, 2.0)
    assert ok.all()
    assert keys[0] == _key(0, 0, 0) and (u[0] == 0).all()
    assert keys[1] == _key(0, 0, 1)
    assert u[1, 0] == 1 << 23 and u[1, 1] == int(np.float32(0.99999994) * np.float32(2 ** 24)) and u[1, 2] == 0
    assert keys[2] == _key(-1, -1, -1)
    assert u[2, 0] == 1 << 23 and u[2, 1] == 0 and u[2, 2] == (1 << 24) - 1    # clamped, not 2^24


def test_oracle_range_and_non_finite_drops():
    lim = np.float32(2.0 ** 20)
    p = np.array([[lim - 1, 0, 0], [lim, 0, 0], [-lim, 0, 0], [-(lim - 1), 0, 0], [np.nan, 0, 0], [0, np.inf, 0],
                  [0, 0, -np.inf], [3e38, 0, 0]], np.float32)
    ok, keys, _ = ref.quantise(p, 1.0)
    assert ok.tolist() == [True, False, False, True, False, False, False, False]
    assert keys[0] == _key((1 << 20) - 1, 0, 0) and keys[3] == _key(-(1 << 20) + 1, 0, 0)
    out = ref.fuse_points(p, None, None, 1.0)
    assert out["dropped"] == 6 and len(out["keys"]) == 2
    assert out["keys"][0] < out["keys"][1]          # ascending key order: -2^20+1 before 2^20-1


def test_oracle_merge_weights_centroid_and_colour():
    # three points in one voxel (voxel 1.0): weights 1, 2, 5; colours chosen so the rounding of (C + W/2) / W shows
    p = np.array([[0.25, 0.5, 0.75], [0.5, 0.5, 0.5], [0.75, 0.25, 0.125], [2.5, 0.5, 0.5]], np.float32)
    c = np.array([[10, 0, 255], [11, 1, 255], [12, 2, 254], [7, 7, 7]], np.uint8)
    w = np.array([1, 2, 5, 0], np.int32)                 # w <= 0 is skipped, not dropped
    out = ref.fuse_points(p, c, w, 1.0)
    assert out["dropped"] == 0 and len(out["keys"]) == 1
    assert out["weights"][0] == 8
    expect = (1 * p[0] + 2 * p[1] + 5 * p[2]) / 8.0     # exact in binary: offsets are multiples of 1/8
    assert np.array_equal(out["points"][0], expect.astype(np.float32))
    ci = c.astype(np.int64)
    C = 1 * ci[0] + 2 * ci[1] + 5 * ci[2]
    assert out["colors"][0].tolist() == [(C[i] + 4) // 8 for i in range(3)]


def test_oracle_pixels_filter_and_colour_rule():
    N, H, W = 1, 2, 3
    pts = np.zeros((N, H, W, 3), np.float32)
    pts[..., 0] = np.arange(H * W, dtype=np.float32).reshape(1, H, W)      # one voxel per pixel at v = 1
    conf = np.array([[[5.0, -1.0, 0.0], [0.0001, 3.0, 3.0]]], np.float32)
    masks = np.array([[[1, 1, 1], [1, 0, 1]]], np.uint8)
    imgs = np.zeros((N, 3, H, W), np.float32)
    imgs[0, 0] = [[1.0, 0.5, 0.2], [1.5, -0.1, 0.99999]]
    pts[0, 1, 2, 1] = np.nan                                   # conf and mask pass, point not finite: dropped
    out = ref.fuse_pixels(pts, conf, masks, imgs, 0.5, 1.0)
    # conf > logit(0.5) = 0 is strict: pixel (0,2) with conf 0 is out; (1,1) masked; (1,2) dropped
    assert out["dropped"] == 1
    assert out["points"][:, 0].tolist() == [0.0, 3.0]
    assert out["colors"][:, 0].tolist() == [255, 255]          # 1.0 -> 255; 1.5 saturates
    assert int(np.float32(0.2) * np.float32(255)) == ref.colour_u8(np.float32(0.2))
    assert ref.colour_u8(np.float32(-0.1)) == 0 and ref.colour_u8(np.float32(0.99999)) == 254
    assert (out["weights"] == 1).all()


def test_oracle_is_order_independent():
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((5000, 3)) * 0.05).astype(np.float32)
    c = rng.integers(0, 256, (5000, 3), dtype=np.uint8)
    w = rng.integers(1, 50, 5000).astype(np.int32)
    a = ref.fuse_points(p, c, w, 0.01)
    perm = rng.permutation(5000)
    b = ref.fuse_points(p[perm], c[perm], w[perm], 0.01)
    for k in ("keys", "points", "colors", "weights"):
        assert np.array_equal(a[k], b[k]), k
    # two halves fused as two sets == one set
    d = ref.fuse_point_sets([(p[:2500], c[:2500], w[:2500]), (p[2500:], c[2500:], w[2500:])], 0.01)
    for k in ("keys", "points", "colors", "weights"):
        assert np.array_equal(a[k], d[k]), k


def test_product_does_not_import_the_dense_map_oracle():
    """tests/dense_map_ref.py is test infrastructure: nothing under pi3_slam_amd/ or tools/ may import it."""
    for sub in ("pi3_slam_amd", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith(".py"):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+(tests\.)?dense_map_ref\b", src, flags=re.M), f
