"""CPU: host-side logic of the product (no kernels): chunk layout, grid keypoints, target size, recipe, taps,
boundary packing — against the oracle / reference vectors."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import post_ref
from pi3_slam_amd import recipe
from pi3_slam_amd.alignment import create_view_graph_matches
from pi3_slam_amd.engine import bicubic_aa_taps
from pi3_slam_amd.image_io import chunk_indices, target_size_for
from pi3_slam_amd.keypoints import GridKeypointExtractor, create_keypoint_extractor
from pi3_slam_amd.weights import Pi3Config, param_shapes


def test_chunk_layout_and_view_graph_match_reference_vectors():
    g = np.load(os.path.join(GOLDEN, "post_layout.npz"))
    for k in g.files:
        parts = k.split("_")
        if parts[0] == "chunks":
            n, cl, ov = map(int, parts[1:])
            assert np.array_equal(np.array(chunk_indices(n, cl, ov)).reshape(-1, 2), g[k]), k
        else:
            cl, ov = map(int, parts[1:])
            assert np.array_equal(np.array(create_view_graph_matches(cl, ov)).reshape(-1, 2), g[k]), k


def test_quirk_tail_chunk_of_overlap_frames_only():
    assert chunk_indices(32, 32, 8) == [(0, 32), (24, 32)]
    assert len(chunk_indices(1000, 100, 20)) == 13 and chunk_indices(1000, 100, 20)[-1] == (960, 1000)
    assert len(chunk_indices(4000, 100, 20)) == 50
    assert chunk_indices(1, 100, 20) == []                            # a single frame is dropped (< 2 frames)


@pytest.mark.parametrize("name,max_kp,seed,tag", [("post_a", 4096, None, "full"), ("post_a", 12, 1234, "sub"),
                                                  ("post_b", 4096, None, "full"), ("post_b", 12, 1234, "sub")])
def test_grid_keypoints_bit_exact(name, max_kp, seed, tag):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    N, H, W = g["shape"]
    ext = GridKeypointExtractor(max_num_keypoints=max_kp, seed=seed)
    kp = ext.extract(torch.zeros(int(N), 3, int(H), int(W)))["keypoints"]
    assert kp.dtype == torch.float32 and np.array_equal(kp.numpy(), g[f"kp_{tag}"])


def test_headline_chunk_keypoints_colours_and_layout_of_the_full_size_reference_run():
    """tests/golden/pi3_full.npz is the reference's own `_process_single_chunk` at the headline size (100 frames, 308 x
    406, K = 200; oracle/gen_golden_full.py).  What does not need the network, on the CPU: the extractor with the
    reference's RNG behaviour (seed=None: the global generator) reproduces all 100 per-frame random subsets of the
    234-point grid bit for bit; the oracle's colour sampler returns the stored colours; the chunk's schema is the one
    SURVEY.md §8(b) records."""
    from oracle.gen_golden import golden_images
    g = np.load(os.path.join(GOLDEN, "pi3_full.npz"))
    N, H, W, K = (int(v) for v in g["shape"])
    assert (N, H, W, K) == (100, 308, 406, 200)
    ext = create_keypoint_extractor("grid", K, device="cpu", seed=None)
    torch.manual_seed(int(g["seed"][0]))
    kp = ext.extract(torch.zeros(N, 3, H, W))["keypoints"]
    ref = torch.from_numpy(g["c_keypoints"]).view(torch.float16)
    assert torch.equal(kp.half().view(torch.int16), ref.view(torch.int16))
    assert len({tuple(map(tuple, kp[i].tolist())) for i in range(3)}) == 3          # the subsets differ per frame
    col = post_ref.keypoint_colors(golden_images("pi3_full", 1, N, H, W)[0], kp)
    assert torch.equal(torch.as_tensor(col).to(torch.float16).view(torch.int16),
                       torch.from_numpy(g["c_colors"]).view(torch.float16).view(torch.int16))
    schema = set(g["schema"].tolist())
    for want in ("points:float16:100x200x3", "local_points:float16:100x200x3", "conf:float16:100x200x1",
                 "masks:bool:100x200x1", "camera_poses:float32:100x4x4", "keypoints:float16:100x200x2",
                 "descriptors:float16:100x200x128", "scores:float16:100x200", "colors:float16:100x200x3",
                 "intrinsics:float32:100x3x3", "camera_params.focal:float32:1x100", "original_width:int",
                 "original_height:int", "image_paths:list", "_metrics:dict"):
        assert want in schema, (want, sorted(schema))
    # poses the reference returned are rigid
    P = torch.from_numpy(g["camera_poses"])[0].double()
    assert (P[:, :3, :3] @ P[:, :3, :3].transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-5


def test_keypoint_factory_and_north_star_grid():
    ext = create_keypoint_extractor("aliked", 200)      # falls back to grid like the reference when lightglue is absent
    assert isinstance(ext, GridKeypointExtractor)
    assert ext._calculate_grid_spacing(308, 406) == 22 and GridKeypointExtractor(400)._calculate_grid_spacing(308, 406) == 16
    out = ext.extract(torch.zeros(2, 3, 308, 406))
    assert out["keypoints"].shape == (2, 200, 2) and out["descriptors"].shape == (2, 200, 128)
    assert float(out["descriptors"].abs().sum()) == 0 and float(out["scores"].min()) == 1
    with pytest.raises(ValueError):
        create_keypoint_extractor("sift", 10)


def test_target_size_rule():
    assert target_size_for(640, 480, 127500) == (308, 406)
    assert target_size_for(512, 384, 127500) == (308, 406)
    assert target_size_for(256, 192, 127500) == (308, 406)
    assert target_size_for(752, 480, 127500) == (280, 448)


def test_recipe_is_deterministic_and_name_keyed():
    a = recipe.recipe_tensor("decoder.0.attn.qkv.weight", (7, 5), 0.0, 1.0)
    b = recipe.recipe_tensor("decoder.0.attn.qkv.weight", (7, 5), 0.0, 1.0)
    c = recipe.recipe_tensor("decoder.1.attn.qkv.weight", (7, 5), 0.0, 1.0)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a.dtype == np.float32 and np.abs(a).max() < 1.0
    assert recipe.fnv1a64("") == 0xCBF29CE484222325 and recipe.fnv1a64("a") == 0xAF63DC4C8601EC8C
    # chunked generation == one-shot generation
    u = recipe.recipe_unit(123, 1000)
    assert np.array_equal(u[100:200], recipe.recipe_unit(123, 100, 100))


def test_param_inventory_default_config():
    shapes = param_shapes(Pi3Config())
    assert len(shapes) == 1208
    assert sum(int(np.prod(s)) for s in shapes.values()) == 958696732      # measured on the reference
    for name, shape in shapes.items():
        recipe.recipe_params(name, shape)


def test_bicubic_antialias_taps_match_torch():
    torch.manual_seed(0)
    for (i, oh, ow) in [(37, 22, 29), (5, 2, 3), (37, 40, 45), (37, 20, 32)]:
        x = torch.randn(1, 3, i, i)
        ref = torch.nn.functional.interpolate(x, size=(oh, ow), mode="bicubic", antialias=True)[0]
        wy, wx = torch.from_numpy(bicubic_aa_taps(i, oh)), torch.from_numpy(bicubic_aa_taps(i, ow))
        mine = torch.einsum("yi,cij,xj->cyx", wy, x[0], wx)
        assert float((ref - mine).abs().max()) < 5e-6


def test_boundary_pack_roundtrip():
    from pi3_slam_amd.dist import pack_boundary, unpack_boundary
    N, K, ov = 7, 5, 3
    ch = dict(points=torch.randn(N, K, 3).half(), keypoints=(torch.rand(N, K, 2) * 300).half(),
              masks=torch.rand(N, K, 1) > 0.5, camera_poses=torch.randn(N, 4, 4))
    b = unpack_boundary(pack_boundary(ch, ov, K), ov, K)
    assert b["n_frames"] == N
    assert torch.equal(b["head"]["points"], ch["points"][:ov]) and torch.equal(b["tail"]["points"], ch["points"][-ov:])
    assert torch.equal(b["head"]["keypoints"], ch["keypoints"][:ov])
    assert torch.equal(b["tail"]["masks"], ch["masks"][-ov:]) and torch.equal(b["last_pose"], ch["camera_poses"][-1])


def test_match_keypoints_oracle():
    kp = (torch.rand(3, 6, 2) * 100).half().numpy()
    perm = np.array([2, 0, 5, 1, 4, 3])
    q = kp[:, perm].copy()
    q[1, 2] = [999.0, 999.0]
    idx = post_ref.match_keypoints(kp, q)
    assert np.array_equal(idx[0], perm) and idx[1, 2] == -1 and np.array_equal(idx[2], perm)


# ------------------------------------------------------------------------------------------- undistortion (§8f rank 4)
def _calib(name):
    import json
    return json.load(open(os.path.join(GOLDEN, "calib_" + name)))


def test_undistortion_camera_quirks_and_oracle_known_answers():
    """Host mirror of pi3/utils/camera.py + the undistorted-camera quirks, and known answers of the oracle restatement
    (pytheia / cv2 are absent: parity unpinned, see oracle/undistort_ref.py)."""
    from oracle import undistort_ref as U
    from pi3_slam_amd.undistortion import Camera, UndistortionMaps, undistorted_copy
    cal = _calib("euroc_cam0_calib.json")
    cam = Camera()
    cam.load_camera_calibration_json(cal, 1.0)
    assert (cam.image_width, cam.image_height, cam.model) == (752, 480, "PINHOLE_RADIAL_TANGENTIAL")
    und = undistorted_copy(cam)
    assert und.aspect_ratio == 1.0 and und.radial == [0.0] * 4 and und.tangential == [0.0, 0.0]
    assert und.principal_point == cam.principal_point == (367.215, 248.375)     # the re-centring is a no-op upstream
    p = UndistortionMaps(cam, device="cpu").params16()
    assert p[0] == p[5] == 458.654 and p[1] == 1.0 and abs(p[6] - 0.9970391624187296) < 1e-15 and p[10] == -0.28340811
    # zero distortion + unit aspect ratio: identity map, and the remap of an identity map is the crop itself
    cal0 = {**cal, "intrinsics": {**cal["intrinsics"], "aspect_ratio": 1.0, "radial_distortion_1": 0.0,
                                  "radial_distortion_2": 0.0, "tangential_distortion_1": 0.0,
                                  "tangential_distortion_2": 0.0}}
    mx, my = U.undistort_maps(cal0, (60, 90))
    assert np.array_equal(mx, np.tile(np.arange(90, dtype=np.float32), (60, 1)))
    assert np.array_equal(my, np.tile(np.arange(60, dtype=np.float32)[:, None], (1, 90)))
    img = np.random.default_rng(0).integers(0, 256, (480, 752, 3), dtype=np.uint8)
    assert np.array_equal(U.remap_bilinear_u8(img, mx, my), img[:60, :90])
    # remap known answers: half-pixel shift = rounded mean of two neighbours; 1/32-pixel quantisation; border taps read 0
    ramp = np.arange(12, dtype=np.uint8).reshape(1, 12, 1).repeat(3, 0).repeat(3, 2) * 20
    xs = np.array([[0.5, 3.5, 10.5, 11.0, 11.5, -0.5, -1.0, 2.0 + 1 / 64, 2.0 + 1 / 32]], np.float32)
    out = U.remap_bilinear_u8(ramp, xs, np.ones_like(xs))[0, :, 0]
    assert out.tolist() == [10, 70, 210, 220, 110, 0, 0, 40, 41]       # rint(1/64*32)=rint(0.5)=0 (half to even)
    # barrel distortion of EuRoC: image corners come from further inside the distorted image; centre is a fixed point
    mx, my = U.undistort_maps(cal, (480, 752))
    assert 60 < mx[0, 0] < 90 and 35 < my[0, 0] < 65 and abs(mx[248, 367] - 367.0) < 0.01
    # division model: x_u = x_d / (1 + k r_d^2) must invert the projection
    cd = _calib("cam_calib.json")
    mx, my = U.undistort_maps(cd, (540, 960))
    k, f, ar = cd["intrinsics"]["div_undist_distortion"], cd["intrinsics"]["focal_length"], cd["intrinsics"]["aspect_ratio"]
    cx, cy = cd["intrinsics"]["principal_pt_x"], cd["intrinsics"]["principal_pt_y"]
    xd, yd = mx.astype(np.float64) - cx, my.astype(np.float64) - cy
    den = 1.0 + k * (xd * xd + yd * yd)
    c, r = np.meshgrid(np.arange(960.0), np.arange(540.0))
    assert np.abs(xd / den - (c - cx)).max() < 2e-3 and np.abs(yd / den - ar * (r - cy)).max() < 2e-3


def test_cli_parsers_and_image_listing(tmp_path):
    """Flags and defaults of the reference CLIs (create_offline_chunks.py:44-62, reconstruct_offline.py:21-29)."""
    from pi3_slam_amd import cli
    a = cli.build_parser().parse_args(["create", "--images", "x", "--output", "y"])
    assert (a.chunk_length, a.overlap, a.device, a.metric_depth, a.keypoints, a.max_kp, a.kp_threshold,
            a.estimate_intrinsics, a.num_workers, a.skip_start, a.skip_end, a.cam_dist_path) == \
        (50, 5, "cuda", True, "grid", 200, 0.005, True, 4, 0, 0, None)
    assert cli.build_parser().parse_args(["create", "--images", "x", "--output", "y", "--no-metric-depth"]).metric_depth is False
    r = cli.build_parser().parse_args(["reconstruct", "--chunks", "c", "--output", "o"])
    assert (r.chunk_length, r.overlap, r.max_observations_per_track, r.save_per_chunk, r.use_inverse_depth) == \
        (None, None, 5, False, False)
    for n in ("b.jpg", "a.png", "c.png", "a.bmp", "z.txt"):
        (tmp_path / n).write_bytes(b"")
    got = [os.path.basename(p) for p in cli.list_images(str(tmp_path))]
    assert got == ["a.png", "c.png", "b.jpg", "a.bmp"]                       # grouped by extension, each group sorted
    lst = tmp_path / "list.txt"
    lst.write_text("p1.png\n\n p2.png \n")
    assert cli.list_images(str(lst)) == ["p1.png", "p2.png"]
    assert [os.path.basename(p) for p in cli.list_images(str(tmp_path / "*.png"))] == ["a.png", "c.png"]
    with pytest.raises(SystemExit):
        cli.main(["create", "--images", str(tmp_path / "nothing_*.png"), "--output", str(tmp_path / "o")])


def test_cli_online_parser_follows_the_reference_script(tmp_path):
    """Flags, types and defaults of pi3_slam_online_modular.py:117-183 (underscore names); the frame trimming of its
    load_image_paths; a video is refused with a reason (no decoder here)."""
    from pi3_slam_amd import cli
    a = cli.build_parser().parse_args(["online", "--image_dir", "d", "--output_path", "o"])
    assert (a.start_frame, a.end_frame, a.skip_start, a.skip_end, a.device, a.chunk_length, a.overlap, a.conf_threshold,
            a.cam_scale, a.estimate_camera_params, a.cam_dist_path, a.keypoint_type, a.max_num_keypoints,
            a.keypoint_detection_threshold, a.save_chunk_reconstructions, a.save_transformed_reconstructions,
            a.save_debug_reconstructions, a.save_debug_projections, a.max_observations_per_track, a.do_metric_depth,
            a.use_inverse_depth, a.viz_port, a.no_visualization, a.keep_viz_open, a.max_points, a.save_tum,
            a.tum_integer_timestamp) == \
        (0, None, 0, 0, "cuda", 30, 5, 0.5, 1.0, True, None, "grid", 200, 0.005, False, False, False, False, 6, True,
         False, 8080, False, False, 1000000, False, False)
    for i in range(7):
        (tmp_path / f"f{i}.png").write_bytes(b"")
    a = cli.build_parser().parse_args(["online", "--image_dir", str(tmp_path), "--output_path", "o", "--skip_start", "2",
                                       "--skip_end", "1"])
    assert [os.path.basename(p) for p in cli.online_image_paths(a)] == ["f2.png", "f3.png", "f4.png", "f5.png"]
    for argv in (["online", "--output_path", "o"],
                 ["online", "--image_dir", "d", "--video_path", "v.mp4", "--output_path", "o"],
                 ["online", "--video_path", "v.mp4", "--output_path", "o"],
                 ["online", "--image_dir", str(tmp_path), "--output_path", "o", "--skip_start", "7"]):
        with pytest.raises(SystemExit):
            cli.online_image_paths(cli.build_parser().parse_args(argv))


def test_in_order_drain_releases_chunks_in_chunk_order():
    """Reorder buffer of the chunk-parallel online path (reference: slam/online_reconstructor.py:852-920)."""
    import random
    from pi3_slam_amd.online import InOrderDrain
    rng = random.Random(0)
    order = list(range(23))
    rng.shuffle(order)
    d, got = InOrderDrain(), []
    for i in order:
        d.put(i, f"chunk{i}")
        for idx, item in d.pop_ready():
            assert item == f"chunk{idx}"
            got.append(idx)
        assert got == list(range(len(got)))            # never releases past a hole
    assert got == list(range(23)) and len(d) == 0 and d.next_index == 23
    with pytest.raises(ValueError):
        d.put(3, "again")


def test_use_inverse_depth_reaches_both_adjustments(tmp_path):
    """utils/chunk_reconstruction.py:186-187,199-204 / utils/reconstruction_alignment.py:147-152: --use-inverse-depth
    switches BOTH adjustments to one inverse-depth parameter per track.  The flag travels from the constructor into the
    settings of the per-chunk stage and, through align_and_refine_reconstructions, of the prior-constrained stage."""
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    r = OfflineReconstructor(str(tmp_path), str(tmp_path / "o"), device="cpu")
    assert r.use_inverse_depth is False and r.bundle_adjust is True
    r = OfflineReconstructor(str(tmp_path), str(tmp_path / "o2"), device="cpu", use_inverse_depth=True)
    assert r.use_inverse_depth is True
    args = r._ba_args({"keypoints": torch.zeros(2, 3, 2), "original_width": 10, "original_height": 8})
    assert args["settings"]["inverse_depth"] is True and args["settings"]["sanity_gate"] is True
    from pi3_slam_amd.bundle_adjust import AFTER_ALIGNMENT, PER_CHUNK
    assert PER_CHUNK["homogeneous_points"] and AFTER_ALIGNMENT["homogeneous_points"]        # the reference's default
    assert "inverse_depth" not in PER_CHUNK or PER_CHUNK["inverse_depth"] is False


def test_bundle_adjust_sanity_gate():
    """bundle_adjust.sanity_gate: a 'successful' adjustment is not taken over when fewer than three tracks survive the
    outlier test or a camera moved by more than the scene extent (pure host logic on the solver's outputs)."""
    import torch
    from pi3_slam_amd.bundle_adjust import sanity_gate
    g = torch.Generator().manual_seed(0)
    pts = torch.randn(40, 3, generator=g, dtype=torch.float64) + torch.tensor([0.0, 0.0, 5.0], dtype=torch.float64)
    rc = torch.zeros(4, 12, dtype=torch.float64)
    rc[:, 9:] = torch.randn(4, 3, generator=g, dtype=torch.float64) * 0.2
    est = torch.ones(4, 10, dtype=torch.bool)
    assert sanity_gate(pts, rc, pts, rc, est, None) is None
    few = torch.zeros(4, 10, dtype=torch.bool); few[0, :2] = True
    assert "tracks survived" in sanity_gate(pts, rc, pts, rc, few, None)
    # cumulative flag: tracks that took no part do not count as lost
    before = torch.zeros(4, 10, dtype=torch.bool); before[1, :5] = True
    assert sanity_gate(pts, rc, pts, rc, before.clone(), before) is None
    moved = rc.clone(); moved[2, 9:] += 100.0
    assert "scene extent" in sanity_gate(pts, rc, pts, moved, est, None)
    nan = rc.clone(); nan[1, 9] = float("nan")
    assert sanity_gate(pts, rc, pts, nan, est, None) is not None          # a NaN move is not '<= extent'


def test_chain_payload_carries_what_the_next_alignment_reads():
    """dist.chain_payload: the refined chunk handed to the next owner under torchrun with bundle adjustment on."""
    import torch
    from pi3_slam_amd.dist import CHAIN_KEYS, chain_payload
    ch = dict(points=torch.zeros(3, 4, 3), keypoints=torch.zeros(3, 4, 2).half(), masks=torch.ones(3, 4, 1, dtype=torch.bool),
              camera_poses=torch.eye(4).repeat(3, 1, 1), colors=torch.zeros(3, 4, 3), image_paths=[["a"], ["b"], ["c"]],
              _chunk_frame={"points": torch.zeros(3, 4, 3).half(), "camera_poses": torch.eye(4).repeat(3, 1, 1)},
              _sim3_global=torch.eye(4, dtype=torch.float64), _observations=("big", "device", "arrays"))
    pay = chain_payload(ch)
    assert set(pay) == {"points", "keypoints", "masks", "camera_poses", "_chunk_frame", "_sim3_global"} <= set(CHAIN_KEYS)
    assert pay["_chunk_frame"]["points"].dtype == torch.float16 and chain_payload(None) is None


def test_checkpoint_directory_config_json(tmp_path):
    """Pi3.from_pretrained(<dir>) hands `<dir>/config.json` to Pi3.__init__ (PyTorchModelHubMixin; pi3.py:17-21):
    pos_type sets the RoPE base, decoder sizes the reference cannot run are refused, no file = the defaults."""
    import json
    from pi3_slam_amd.weights import Pi3Config, config_from_checkpoint_dir
    assert config_from_checkpoint_dir(str(tmp_path)) == Pi3Config()
    (tmp_path / "config.json").write_text(json.dumps({"pos_type": "rope50", "decoder_size": "large"}))
    cfg = config_from_checkpoint_dir(str(tmp_path))
    assert cfg.rope_base == 50.0 and cfg.dec_depth == 36
    (tmp_path / "config.json").write_text(json.dumps({"decoder_size": "small"}))
    with pytest.raises(NotImplementedError):
        config_from_checkpoint_dir(str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps({"pos_type": None}))
    with pytest.raises(NotImplementedError):
        config_from_checkpoint_dir(str(tmp_path))


def test_ba_summary_and_keypoint_weights():
    """bundle_adjust.ba_summary counts what ran / was applied / was rejected by the sanity gate / failed (what
    OfflineReconstructor.refinement_summary reports); alignment.keypoint_weights is w = mask * sigmoid(conf) (SURVEY §7
    step 7) on the overlap views of a chunk dictionary."""
    from pi3_slam_amd.alignment import keypoint_weights
    from pi3_slam_amd.bundle_adjust import ba_summary
    infos = [{"success": True}, {"success": False, "rejected": "a camera moved 3 units"}, None, {"success": False},
             {"success": True}, {"success": False, "reason": "no keypoints"}]
    assert ba_summary(infos) == {"ran": 5, "applied": 2, "rejected_by_sanity_gate": 1, "failed": 2}
    assert ba_summary([]) == {"ran": 0, "applied": 0, "rejected_by_sanity_gate": 0, "failed": 0}
    g = torch.Generator().manual_seed(0)
    conf = torch.randn(5, 7, 1, generator=g).half()
    masks = torch.rand(5, 7, 1, generator=g) > 0.3
    w = keypoint_weights({"conf": conf, "masks": masks}, [4, 1])
    assert w.shape == (2, 7) and w.dtype == torch.float32
    want = torch.sigmoid(conf[[4, 1]].float().reshape(2, 7)) * masks[[4, 1]].reshape(2, 7).float()
    assert torch.equal(w, want) and (w[~masks[[4, 1]].reshape(2, 7)] == 0).all() and (w <= 1).all()


def test_hostmem_byte_movers_equal_the_aten_operators():
    """pi3_slam_amd/hostmem.py moves the consumer side's bytes with memcpy / calloc instead of ATen CPU operators (the
    OpenMP regions behind the one-off 85-110 ms host stalls of round 4): same values, dtypes, shapes, and fresh storage."""
    from pi3_slam_amd import hostmem
    g = torch.Generator().manual_seed(3)
    for t in (torch.randn(60, 200, 3, generator=g).half(), torch.randn(7, 5, generator=g), torch.rand(33, generator=g) > 0.5,
              torch.randint(0, 255, (40, 3), generator=g, dtype=torch.uint8), torch.randn(6, 4, 4, generator=g).double(),
              torch.zeros(0, 3)):
        c = hostmem.clone_host(t)
        assert c.dtype == t.dtype and c.shape == t.shape and torch.equal(c, t) and (t.numel() == 0 or c.data_ptr() != t.data_ptr())
    nc = torch.randn(8, 6, generator=g).t()                      # non-contiguous source
    assert torch.equal(hostmem.clone_host(nc), nc) and hostmem.clone_host(nc).is_contiguous()
    z = hostmem.zeros_host((3, 4, 128), torch.float16)
    assert z.dtype == torch.float16 and z.shape == (3, 4, 128) and float(z.abs().sum()) == 0
    z[0, 0, 0] = 1                                                # writable, owned
    o = hostmem.full_host((5, 7), 1.0, torch.float16)
    assert o.dtype == torch.float16 and torch.equal(o, torch.ones(5, 7, dtype=torch.float16))
    # byte copy between views of different dtype (how the packed D2H buffer is unpacked)
    src = torch.arange(24, dtype=torch.uint8)
    dst = torch.empty(6, dtype=torch.float32)
    hostmem.memcpy_into(dst, src)
    assert torch.equal(dst.view(torch.uint8), src)
    with pytest.raises(AssertionError):
        hostmem.memcpy_into(torch.empty(5, dtype=torch.float32), src)


def test_packed_results_round_trip():
    """chunk_creator.pack_results / unpack_results (one device buffer, one copy per chunk): offsets and length are
    16-byte aligned, the layout keeps the insertion order, every tensor comes back equal in storage of its own."""
    from pi3_slam_amd.chunk_creator import pack_results, unpack_results
    g = torch.Generator().manual_seed(11)
    out = {"_scale": torch.randn(2, generator=g), "cam.focal": torch.randn(1, 3, generator=g),
           "f64": torch.randn(33, generator=g).double(), "_dense_stats": torch.randint(-9, 9, (4,), generator=g),
           "masks": torch.randint(0, 255, (3, 5, 1), generator=g, dtype=torch.uint8),      # 15 bytes: padded
           "points": torch.randn(3, 5, 3, generator=g).half(), "strided": torch.randn(4, 6, generator=g)[:, ::2],
           "camera_poses": torch.randn(3, 4, 4, generator=g), "empty": torch.zeros(0, 3)}
    assert not out["strided"].is_contiguous() and out["strided"].shape == (4, 3)
    packed, layout = pack_results(out)
    assert packed.dtype == torch.uint8 and packed.ndim == 1 and packed.numel() % 16 == 0
    assert [e[0] for e in layout] == list(out)
    end = 0
    for k, dt, shape, off, nbytes in layout:
        assert off % 16 == 0 and off >= end and nbytes == out[k].numel() * out[k].element_size()
        end = off + nbytes
    assert end <= packed.numel() < end + 16 and packed.numel() == 688
    got = unpack_results(packed, layout)

    def same():
        assert list(got) == list(out)
        for k, t in out.items():
            assert got[k].dtype == t.dtype and got[k].shape == t.shape and torch.equal(got[k], t), k
    same()
    packed.fill_(0xA5)                          # the results do not alias the buffer (it goes back to a pool)
    same()


def test_overlap_block_takes_negative_view_indices_like_an_advanced_index():
    """A run of negative view indices that ends at -1 ([-20 .. -1]) is consecutive; as a slice it would read
    t[-20:0] = nothing.  The block must equal what the advanced index t[frames] returns."""
    from pi3_slam_amd.alignment import _and_estimated, _overlap_block
    g = torch.Generator().manual_seed(3)
    n, K = 30, 7
    chunk = dict(points=torch.randn(n, K, 3, generator=g).half(), keypoints=(torch.rand(n, K, 2, generator=g) * 200).half(),
                 masks=torch.rand(n, K, 1, generator=g) > 0.3, track_estimated=torch.rand(n, K, generator=g) > 0.2)
    for frames in (list(range(-20, 0)), list(range(-5, -1)), [3, 4, 5], [-1], [2, -3, 7]):
        blk = _overlap_block(chunk, frames, "cpu")
        idx = torch.tensor(frames)
        for k in ("points", "keypoints", "masks"):
            assert blk[k].shape[0] == len(frames) and torch.equal(blk[k], chunk[k][idx]), (frames, k)
        e = _and_estimated(None, chunk, frames, "cpu")
        assert torch.equal(e.bool(), chunk["track_estimated"][idx])


# ---------------------------------------------------------------------------------------------------------------
# MoGe tap builders (pi3_slam_amd/moge.py) against F.interpolate on an fp32 identity: every MoGe depth goes through them
# ---------------------------------------------------------------------------------------------------------------
_TAP_PAIRS = [(518, 140), (476, 644), (84, 112), (112, 84), (37, 14), (64, 16), (16, 64), (23, 23), (5, 3), (3, 5), (8, 2),
              (32, 8), (7, 1), (1, 4), (2, 1), (480, 308), (752, 406)]


def _taps_dense(sc, w, n_in):
    m = np.zeros((sc.shape[0], n_in), dtype=np.float64)
    for i, (s, n) in enumerate(sc):
        assert 0 <= s and n >= 1 and s + n <= n_in, (i, s, n)
        m[i, s:s + n] = w[i, :n]
        assert not w[i, n:].any()                                   # unused slots stay zero
    return m


def _interp_matrix(n_in, n_out, antialias):
    """[out, in] matrix of F.interpolate(bilinear, align_corners=False) along one axis, from an fp32 identity."""
    eye = torch.eye(n_in, dtype=torch.float32).view(1, n_in, 1, n_in)           # channel c = unit vector c along W
    out = torch.nn.functional.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=False, antialias=antialias)
    return out[0, :, 0, :].t().double().numpy()


@pytest.mark.parametrize("n_in,n_out", _TAP_PAIRS)
def test_linear_taps_antialias_equal_torchs_weights(n_in, n_out):
    """Same fp32 formula as ATen's antialias kernel: within 2^-22 (measured worst 1.5e-8)."""
    from pi3_slam_amd.moge import linear_taps
    sc, w = linear_taps(n_in, n_out, True)
    assert sc.dtype == np.int32 and w.dtype == np.float32 and sc.shape == (n_out, 2) and w.shape == (n_out, 8)
    assert sc[:, 1].max() <= 8
    m = _taps_dense(sc, w, n_in)
    assert np.abs(m.sum(1) - 1.0).max() <= 2.0 ** -22
    assert np.abs(m - _interp_matrix(n_in, n_out, True)).max() <= 2.0 ** -22


def test_linear_taps_antialias_refuses_a_support_beyond_the_table():
    from pi3_slam_amd.moge import linear_taps
    with pytest.raises(AssertionError, match="antialias support exceeds the tap table"):
        linear_taps(33, 8, True)


@pytest.mark.parametrize("n_in,n_out", _TAP_PAIRS)
def test_linear_taps_plain_equal_torchs_weights(n_in, n_out):
    """Without antialias the weight is the fraction of the fp32 source coordinate; torch's CPU kernel forms it in another
    order, so the two differ by up to the coordinate's rounding: one fp32 spacing at n_in (measured worst 3.05e-5 at
    752 -> 406, spacing 6.1e-5)."""
    from pi3_slam_amd.moge import linear_taps
    sc, w = linear_taps(n_in, n_out, False)
    assert set(np.unique(sc[:, 1])) <= {1, 2}
    m = _taps_dense(sc, w, n_in)
    assert np.abs(m - _interp_matrix(n_in, n_out, False)).max() <= float(np.spacing(np.float32(n_in)))


@pytest.mark.parametrize("M,n", [(37, 22), (37, 29), (37, 37), (16, 6), (16, 8), (37, 50), (37, 60)])
def test_bicubic_taps_dense_equal_torchs_scale_factor_path(M, n):
    """The DINOv2 position-embedding resample: F.interpolate(scale_factor=(n + 0.1) / M, mode='bicubic') along one axis;
    within 4e-6 (measured worst 2.3e-6)."""
    from pi3_slam_amd.moge import bicubic_taps_dense
    got = bicubic_taps_dense(M, n, M / (n + 0.1))
    eye = torch.eye(M, dtype=torch.float32).view(1, M, 1, M)                    # channel c = unit vector c along W
    out = torch.nn.functional.interpolate(eye, scale_factor=(1, (n + 0.1) / M), mode="bicubic")
    assert out.shape[-1] == n and got.shape == (n, M) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - out[0, :, 0, :].t().double().numpy()).max() <= 4e-6
