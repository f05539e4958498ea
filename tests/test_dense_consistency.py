"""Multi-view depth consistency filter, CPU side: the numpy oracle's properties on an analytic scene (cameras translating
along x with a small yaw in front of a tilted plane), ConsistencyFilter's validation and the command-line flags."""
import numpy as np
import pytest

import dense_consistency_ref as ref

N, H, W = 6, 24, 40
DEFAULTS = dict(radius=3, stride=2, min_views=2, rel_tol=0.03)


def _run(scene, **kw):
    p = dict(DEFAULTS, **kw)
    return ref.consistency(scene["points"], scene["local_points"], None, None, scene["poses"], scene["fxfycxcy"],
                           -np.inf, p["radius"], p["stride"], p["min_views"], p["rel_tol"])


@pytest.fixture(scope="module")
def exact():
    scene = ref.plane_scene(N, H, W)
    return scene, _run(scene)


def test_exact_data_keeps_every_pixel_seen_by_enough_neighbours(exact):
    scene, out = exact
    assert out["stats"][0] == N * H * W                       # every pixel is a candidate
    # a point that projects at least one pixel inside a neighbour lands on a pixel of it whatever the rounding does
    must = ref.inside_count(scene, DEFAULTS["radius"], DEFAULTS["stride"], margin=1.0) >= DEFAULTS["min_views"]
    assert must.sum() > 0.3 * N * H * W
    assert np.all(out["mask"][must] == 1)
    assert np.all(out["counts"][..., 1] == 0)                  # nothing looks through anything
    assert out["stats"][1] == out["mask"].sum() >= must.sum()
    # and nothing is kept without its agreeing views
    assert np.all(out["counts"][..., 0][out["mask"] == 1] >= DEFAULTS["min_views"])
    for mv in (1, 2):
        o = _run(scene, min_views=mv)
        m = ref.inside_count(scene, DEFAULTS["radius"], DEFAULTS["stride"], margin=1.0) >= mv
        assert np.all(o["mask"][m] == 1)


def test_pulled_rectangle_is_removed_with_conflicts_and_pushed_one_without(exact):
    scene0, base = exact
    rows, cols = slice(8, 16), slice(14, 26)
    scene = {k: v.copy() for k, v in scene0.items()}
    ref.scale_block(scene, 2, rows, cols, 0.5)                 # in front of the plane: the neighbours look through it
    ref.scale_block(scene, 3, rows, cols, 1.6)                 # behind the plane: occluded in every neighbour
    out = _run(scene)
    assert base["mask"][2, rows, cols].all() and base["mask"][3, rows, cols].all()      # kept while they were on the plane
    assert not out["mask"][2, rows, cols].any()
    assert np.all(out["counts"][2, rows, cols, 1] > 0)          # conflict in at least one neighbour
    assert np.all(out["counts"][2, rows, cols, 0] == 0)
    assert not out["mask"][3, rows, cols].any()
    assert np.all(out["counts"][3, rows, cols, 1] == 0) and np.all(out["counts"][3, rows, cols, 0] == 0)
    # the other frames lose at most the votes of the two damaged rectangles
    others = np.ones((N, H, W), bool)
    others[2, rows, cols] = others[3, rows, cols] = False
    assert out["mask"][others].sum() >= 0.8 * base["mask"][others].sum()


def test_single_frame_has_no_neighbours():
    scene = ref.plane_scene(1, H, W)
    for mv in (1, 2):
        out = _run(scene, min_views=mv)
        assert out["stats"][0] == H * W and out["stats"][1] == 0 and not out["mask"].any()


def test_candidates_follow_mask_confidence_and_finiteness():
    scene = ref.plane_scene(3, 8, 8)
    conf = np.full((3, 8, 8, 1), 1.0, np.float32)
    masks = np.ones((3, 8, 8), np.uint8)
    conf[0, 0, 0] = 0.0                       # not above the threshold (strict >)
    masks[0, 0, 1] = 0
    scene["points"][0, 0, 2, 1] = np.nan
    scene["local_points"][0, 0, 3, 2] = -1.0
    scene["local_points"][0, 0, 4, 2] = np.inf
    out = ref.consistency(scene["points"], scene["local_points"], conf, masks, scene["poses"], scene["fxfycxcy"], 0.0,
                          1, 1, 1, 0.03)
    assert not out["candidates"][0, 0, :5].any() and out["candidates"][0, 0, 5:].all()
    assert out["stats"][0] == 3 * 64 - 5
    assert not out["mask"][0, 0, :5].any() and not out["counts"][0, 0, :5].any()


def test_consistency_filter_validates_like_the_c_entry():
    from pi3_slam_amd.dense_map import ConsistencyFilter
    f = ConsistencyFilter()
    assert f.settings() == {"min_views": 2, "radius": 3, "stride": 2, "rel_tol": 0.03}
    assert ConsistencyFilter(min_views=32, radius=16).min_views == 32
    for bad in (dict(radius=0), dict(radius=17), dict(stride=0), dict(min_views=0), dict(min_views=7),
                dict(min_views=3, radius=1), dict(rel_tol=0.0), dict(rel_tol=-0.1), dict(rel_tol=float("inf")),
                dict(rel_tol=float("nan")), dict(min_views=1.5)):
        with pytest.raises(ValueError):
            ConsistencyFilter(**bad)


def test_creator_config_defaults_leave_the_filter_off():
    from pi3_slam_amd.chunk_creator import OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir="unused")
    assert cfg.dense_min_views is None
    assert (cfg.dense_view_radius, cfg.dense_view_stride, cfg.dense_depth_tolerance) == (3, 2, 0.03)


def test_cli_flags():
    from pi3_slam_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(["create", "--images", "i", "--output", "o"])
    assert a.dense_min_views is None
    assert (a.dense_view_radius, a.dense_view_stride, a.dense_depth_tolerance) == (3, 2, 0.03)
    a = p.parse_args(["create", "--images", "i", "--output", "o", "--dense-voxel-size", "0.02", "--dense-min-views", "3",
                      "--dense-view-radius", "4", "--dense-view-stride", "1", "--dense-depth-tolerance", "0.05"])
    assert (a.dense_min_views, a.dense_view_radius, a.dense_view_stride, a.dense_depth_tolerance) == (3, 4, 1, 0.05)
    a = p.parse_args(["online", "--image_dir", "i", "--output_path", "o"])
    assert a.dense_min_views is None
    a = p.parse_args(["online", "--image_dir", "i", "--output_path", "o", "--dense_voxel_size", "0.05",
                      "--dense_min_views", "1", "--dense_view_radius", "2", "--dense_view_stride", "3",
                      "--dense_depth_tolerance", "0.1"])
    assert (a.dense_min_views, a.dense_view_radius, a.dense_view_stride, a.dense_depth_tolerance) == (1, 2, 3, 0.1)
