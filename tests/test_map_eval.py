"""CPU: the host side of map scoring (pi3_slam_amd/map_eval.py) and the brute-force oracle of its device search
(tests/cloud_nn_ref.py): the oracle against scipy's k-d tree, the statistics on hand-made arrays, the F-score identity on
planted data, the PLY reader on every layout export.py writes, the synthetic room's reference cloud, the command line."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_nn_ref as nnref            # noqa: E402

GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")


def oracle_search(ref, queries, max_dist):
    """compare_clouds' search hook, served by the oracle (host arrays in, the device search's dict out)."""
    out = nnref.nearest(np.asarray(ref.cpu()), np.asarray(queries.cpu()), max_dist)
    return dict(d2=out["d2"], idx=out["idx"].astype(np.int64), ref_dropped=out["ref_dropped"], counters=out["counters"])


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("n,m,max_dist", [(400, 300, 0.05), (2000, 1500, 0.1), (50, 700, 0.3), (1, 10, 2.0)])
def test_oracle_agrees_with_ckdtree(n, m, max_dist):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(n + m)
    p = rng.random((n, 3)).astype(np.float32)
    q = rng.random((m, 3)).astype(np.float32)
    q[: m // 10] = p[rng.integers(0, n, m // 10)]                   # exact hits
    got = nnref.nearest(p, q, max_dist)
    d, i = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=2 if n > 1 else 1, distance_upper_bound=max_dist)
    d, i = d.reshape(m, -1), i.reshape(m, -1)
    hit = np.isfinite(d[:, 0])
    assert 0 < hit.sum() and got["ref_dropped"] == 0
    assert got["counters"] == dict(dropped=0, matched=int(hit.sum()), beyond=int((~hit).sum()))
    assert np.array_equal(got["idx"] >= 0, hit) and np.all(np.isinf(got["d2"][~hit]))
    np.testing.assert_allclose(np.sqrt(got["d2"][hit]), d[hit, 0], rtol=1e-12, atol=0)
    unique = hit & ((d.shape[1] == 1) | (d[:, -1] > d[:, 0]))      # the second neighbour is farther (or beyond)
    assert unique.sum() > hit.sum() // 2
    assert np.array_equal(got["idx"][unique], i[unique, 0])


def test_oracle_tie_drop_and_empty_rules():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0.5, 0.5, 0]], np.float32)
    q = np.array([[0, 0, 0], [0.5, 0, 0], [np.inf, 0, 0], [9, 9, 9], [1e9, 0, 0]], np.float32)
    got = nnref.nearest(p, q, 0.5)
    assert got["idx"].tolist() == [0, 0, -1, -1, -1]                # duplicates and the equidistant pair: lowest index
    assert got["d2"].tolist() == [0.0, 0.25, np.inf, np.inf, np.inf]            # 0.5 away: inclusive
    assert got["ref_dropped"] == 1 and got["counters"] == dict(dropped=2, matched=2, beyond=1)
    none = nnref.nearest(np.zeros((0, 3), np.float32), q, 0.5)
    assert none["idx"].tolist() == [-1] * 5 and none["counters"] == dict(dropped=0, matched=0, beyond=5)
    assert nnref.nearest(p, np.zeros((0, 3), np.float32), 0.5)["d2"].shape == (0,)


# ------------------------------------------------------------------------------------------------ statistics
def test_distance_stats_on_hand_made_arrays():
    from pi3_slam_amd.map_eval import distance_stats, fscore, tau_key
    inf = np.inf
    a = distance_stats([inf, inf, inf], [0.1], 0.2)
    assert (a["points"], a["matched"], a["beyond"]) == (3, 0, 3) and a["within"] == {tau_key(0.1): 0.0}
    assert all(a[k] is None for k in ("mean", "median", "rmse", "p90", "max"))
    z = distance_stats(np.zeros(5), [0.0, 0.1], 0.2)
    assert (z["matched"], z["beyond"]) == (5, 0) and z["within"] == {tau_key(0.0): 1.0, tau_key(0.1): 1.0}
    assert all(z[k] == 0.0 for k in ("mean", "median", "rmse", "p90", "max"))
    m = distance_stats([0.1, 0.2, 0.3, inf], [0.2, 0.25, 0.4], 0.4)
    assert m["within"] == {tau_key(0.2): 0.5, tau_key(0.25): 0.5, tau_key(0.4): 0.75}           # tau == a distance: inclusive
    assert (m["matched"], m["beyond"], m["median"], m["max"]) == (3, 1, 0.2, 0.3)
    assert m["mean"] == pytest.approx(0.2) and m["rmse"] == pytest.approx(np.sqrt(0.14 / 3))
    assert m["p90"] == pytest.approx(0.28)
    e = distance_stats(np.zeros(0), [0.1], 0.1)
    assert e["points"] == 0 and e["within"] == {tau_key(0.1): 0.0} and e["mean"] is None
    with pytest.raises(ValueError, match="max_dist"):
        distance_stats([0.1], [0.1, 0.3], 0.2)
    with pytest.raises(ValueError, match="NaN"):
        distance_stats([np.nan], [0.1], 0.2)
    assert fscore(0.0, 0.0) == 0.0 and fscore(1.0, 1.0) == 1.0 and fscore(0.5, 1.0) == pytest.approx(2 / 3)
    json.dumps(m)                                                    # plain floats, ints, None and string keys


def planted(V=600, K=37, max_dist=0.1, seed=5):
    """A reference cloud in the unit box and the estimate = that cloud + K points at least 2 max_dist from all of it."""
    rng = np.random.default_rng(seed)
    ref = rng.random((V, 3)).astype(np.float32)
    far = (rng.random((K, 3)) * np.array([1.0, 1.0, 0.5]) + np.array([0.0, 0.0, 1.0 + 2.0 * max_dist + 1e-3])).astype(np.float32)
    return ref, np.concatenate([ref[: V // 2], far, ref[V // 2:]]), far


def test_fscore_identity_on_planted_data():
    from pi3_slam_amd.map_eval import compare_clouds, tau_key
    V, K, md = 600, 37, 0.1
    ref, est, far = planted(V, K, md)
    gap = np.sqrt(nnref.nearest(ref, far, 10.0)["d2"])
    assert gap.min() >= 2 * md
    res = compare_clouds(est, ref, [0.0, 0.05], max_dist=md, device="cpu", _nearest=oracle_search)
    for t in (0.0, 0.05):
        k = tau_key(t)
        assert res["precision"][k] == V / (V + K) and res["recall"][k] == 1.0
        assert res["fscore"][k] == 2 * (V / (V + K)) / (V / (V + K) + 1.0)
    assert res["accuracy"]["beyond"] == K and res["accuracy"]["matched"] == V and res["completeness"]["beyond"] == 0
    assert res["accuracy"]["max"] == 0.0 and res["dropped"] == {"estimate": 0, "reference": 0}
    assert res["points"] == dict(estimate=V + K, reference=V, estimate_used=V + K, reference_used=V)
    assert res["settings"]["max_dist"] == md and res["settings"]["thresholds"] == [0.0, 0.05]
    assert np.isinf(res["_distances"]["estimate"]).sum() == K and res["_distances"]["reference"].shape == (V,)
    # max_dist defaults to twice the largest threshold; a threshold above max_dist is refused
    assert compare_clouds(est, ref, [0.02, 0.05], device="cpu", _nearest=oracle_search)["settings"]["max_dist"] == 0.1
    with pytest.raises(ValueError, match="max_dist"):
        compare_clouds(est, ref, [0.2], max_dist=0.1, device="cpu", _nearest=oracle_search)


def test_error_colors_ramp():
    from pi3_slam_amd.map_eval import error_colors
    c = error_colors([0.0, 0.05, 0.1, 0.2, np.inf, 0.025], 0.1)
    assert c.dtype == np.uint8 and c.tolist() == [[0, 255, 0], [255, 255, 0], [255, 0, 0], [255, 0, 0], [255, 0, 255],
                                                  [128, 255, 0]]


# ------------------------------------------------------------------------------------------------ PLY
def test_read_ply_points_round_trips(tmp_path):
    from pi3_slam_amd.export import write_mesh_ply, write_ply, write_ply_normals
    from pi3_slam_amd.map_eval import read_ply_points
    rng = np.random.default_rng(2)
    pts = (rng.standard_normal((257, 3)) * 3).astype(np.float32)
    nrm = rng.standard_normal((257, 3)).astype(np.float32)
    col = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    faces = rng.integers(0, 257, (90, 3)).astype(np.int32)
    write_ply(pts, col, str(tmp_path / "a.ply"))
    write_ply_normals(pts, nrm, col, str(tmp_path / "b.ply"))
    write_mesh_ply(pts, nrm, col, faces, str(tmp_path / "c.ply"))
    for name in ("a.ply", "b.ply", "c.ply"):
        p, c = read_ply_points(str(tmp_path / name))
        assert p.dtype == np.float32 and p.tobytes() == pts.tobytes() and c.tobytes() == col.tobytes(), name
    write_ply(pts[:0], col[:0], str(tmp_path / "empty.ply"))
    p, c = read_ply_points(str(tmp_path / "empty.ply"))
    assert p.shape == (0, 3) and c.shape == (0, 3)
    # ascii, properties in another order, a comment, colours missing, a face element behind
    with open(tmp_path / "d.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float z\nproperty float x\n"
                "property int label\nproperty float y\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                "3 1 7 2\n6 4 8 5\n-0.5 1e-3 9 2.5e2\n3 0 1 2\n")
    p, c = read_ply_points(str(tmp_path / "d.ply"))
    assert c is None and p.tolist() == np.array([[1, 2, 3], [4, 5, 6], [1e-3, 2.5e2, -0.5]], np.float32).tolist()
    # double precision, an element of known size before the vertices
    rec = np.empty(4, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    xyz = rng.standard_normal((4, 3))
    rec["x"], rec["y"], rec["z"] = xyz.T
    rec["red"], rec["green"], rec["blue"] = col[:4].T
    with open(tmp_path / "e.ply", "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement camera 2\nproperty float fx\nproperty uchar id\n"
                b"element vertex 4\nproperty double x\nproperty double y\nproperty double z\nproperty uchar red\n"
                b"property uchar green\nproperty uchar blue\nend_header\n")
        f.write(b"\x01" * 10 + rec.tobytes())
    p, c = read_ply_points(str(tmp_path / "e.ply"))
    assert p.tobytes() == xyz.astype(np.float32).tobytes() and c.tobytes() == col[:4].tobytes()
    # refusals name what was found
    with open(tmp_path / "f.ply", "wb") as f:
        f.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                b"property float z\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        read_ply_points(str(tmp_path / "f.ply"))
    with open(tmp_path / "g.ply", "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty int x\nproperty float y\nproperty float z\n"
                b"end_header\n1 2 3\n")
    with pytest.raises(ValueError, match="x must be float or double, found i4"):
        read_ply_points(str(tmp_path / "g.ply"))
    with open(tmp_path / "h.ply", "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError, match="no vertex element.*face"):
        read_ply_points(str(tmp_path / "h.ply"))
    with open(tmp_path / "i.ply", "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
                b"property float z\nend_header\n" + b"\x00" * 30)
    with pytest.raises(ValueError, match="30 bytes found"):
        read_ply_points(str(tmp_path / "i.ply"))
    with open(tmp_path / "j.txt", "wb") as f:
        f.write(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply_points(str(tmp_path / "j.txt"))


# ------------------------------------------------------------------------------------------------ the reference cloud
def test_reference_cloud_lies_on_the_room_and_leaves_sphere_zero_out():
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, H=36, W=48, chunk_length=12, overlap=4, n_frames=24, noise=dict(ss.NOISE_NONE))
    cloud = seq.reference_cloud()
    assert cloud.dtype.is_floating_point and tuple(cloud.shape)[1] == 3 and str(cloud.dtype) == "torch.float32"
    X = cloud.numpy().astype(np.float64)
    wall = np.min(np.concatenate([np.abs(X - seq.lo), np.abs(X - seq.hi)], 1), 1)
    sph = [np.abs(np.linalg.norm(X - ctr, axis=1) - r) for ctr, r in seq.spheres]
    others = np.min(np.stack(sph[1:]), 0)
    on_room = np.minimum(wall, others) <= 1e-5
    assert on_room.all(), float(np.minimum(wall, others).max())
    # none on sphere 0 (a point of a wall or of another sphere may touch it only where the surfaces meet)
    assert not ((sph[0] <= 1e-5) & (np.minimum(wall, others) > 1e-5)).any()
    assert (sph[0] > 1e-5).all()
    full = 24 * 36 * 48
    assert 0.5 * full < len(X) <= full
    # the camera sees sphere 0 somewhere in the full sequence at this size, so leaving it out removes rays
    sub = seq.reference_cloud(frame_step=5, pixel_stride=3)
    assert len(sub) <= 5 * 12 * 16 and len(sub) > 0
    inside = ((X >= seq.lo - 1e-5) & (X <= seq.hi + 1e-5)).all(1)
    assert inside.all()


def test_reference_cloud_drops_exactly_the_low_confidence_rays():
    import torch
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, H=24, W=32, chunk_length=12, overlap=4, n_frames=180, noise=dict(ss.NOISE_NONE))
    v, u = torch.meshgrid(torch.arange(24), torch.arange(32), indexing="ij")
    uv = torch.stack([u.reshape(-1), v.reshape(-1)], -1)
    # count the sphere-0 rays through _cast directly
    P = torch.as_tensor(seq.poses_gt, dtype=torch.float64)
    d_cam = torch.stack([(uv[:, 0] - seq.cx) / seq.fx, (uv[:, 1] - seq.cy) / seq.fy, torch.ones(len(uv))], -1).double()
    d_w = torch.einsum("nij,pj->npi", P[:, :3, :3], d_cam)
    _, flag = seq._cast(P[:, None, :3, 3], d_w)
    low = int(flag.sum())
    assert low > 0                                                    # the sequence does look at sphere 0
    assert len(seq.reference_cloud()) == 180 * 24 * 32 - low


# ------------------------------------------------------------------------------------------------ command line
def _write_tum(path, stamps, pos):
    with open(path, "w") as f:
        f.write("# timestamp tx ty tz qx qy qz qw\n")
        for s, p in zip(stamps, pos):
            f.write(f"{s} {p[0]:.9f} {p[1]:.9f} {p[2]:.9f} 0 0 0 1\n")


def test_cli_parsing_and_trajectory_alignment(tmp_path):
    from scipy.spatial.transform import Rotation
    from pi3_slam_amd import cli, map_eval
    a = cli.build_parser().parse_args(["evaluate-map", "--estimate", "e.ply", "--reference", "r.ply", "--thresholds", "0.02",
                                       "0.05"])
    assert a.command == "evaluate-map" and a.thresholds == [0.02, 0.05] and a.max_dist is None and a.voxel_size is None
    assert a.transform is None and a.error_ply is None and not a.json and a.device == "cuda"
    assert cli.evaluate_map_transform(a) is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["evaluate-map", "--estimate", "e.ply", "--reference", "r.ply"])
    # a known similarity between two trajectories: est = the reference seen through the inverse of (c, R, t)
    rng = np.random.default_rng(3)
    ref_pos = rng.standard_normal((30, 3))
    R = Rotation.from_rotvec([0.3, -0.8, 0.5]).as_matrix()
    c, t = 1.7, np.array([0.4, -2.0, 1.1])
    est_pos = (ref_pos - t) @ R / c                                   # ref = c R est + t
    _write_tum(tmp_path / "ref.tum", range(30), ref_pos)
    _write_tum(tmp_path / "est.tum", range(2, 27), est_pos[2:27])     # the shorter one: association by stamp
    M = map_eval.trajectory_alignment(str(tmp_path / "est.tum"), str(tmp_path / "ref.tum"))
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = c * R, t
    np.testing.assert_allclose(M, want, atol=1e-7)
    full = ["evaluate-map", "--estimate", "e.ply", "--reference", "r.ply", "--thresholds", "0.1", "--max-dist", "0.3",
            "--voxel-size", "0.02", "--estimate-trajectory", str(tmp_path / "est.tum"), "--reference-trajectory",
            str(tmp_path / "ref.tum"), "--error-ply", "err.ply", "--json"]
    b = cli.build_parser().parse_args(full)
    assert (b.max_dist, b.voxel_size, b.error_ply, b.json) == (0.3, 0.02, "err.ply", True)
    np.testing.assert_allclose(cli.evaluate_map_transform(b), want, atol=1e-7)
    np.savetxt(tmp_path / "T.txt", want)
    b = cli.build_parser().parse_args(full[:7] + ["--transform", str(tmp_path / "T.txt")])
    assert np.array_equal(cli.evaluate_map_transform(b), want)
    for argv in (full + ["--transform", str(tmp_path / "T.txt")], full[:7] + ["--estimate-trajectory", "x.tum"]):
        with pytest.raises(SystemExit):
            cli.evaluate_map_transform(cli.build_parser().parse_args(argv))
    # the same functions as tools/eval_ape.py: its APE of the pair is zero after the alignment
    import eval_ape
    assert eval_ape.ape(str(tmp_path / "ref.tum"), str(tmp_path / "est.tum"))["rmse"] < 1e-7


def test_table_lists_both_directions_and_every_threshold():
    from pi3_slam_amd.map_eval import compare_clouds, format_table, public
    ref, est, _ = planted()
    res = compare_clouds(est, ref, [0.02, 0.05], device="cpu", _nearest=oracle_search)
    text = format_table(res)
    assert "accuracy" in text and "completeness" in text and "0.02" in text and "0.05" in text and "fscore" in text
    assert "_distances" not in public(res) and json.loads(json.dumps(public(res))) == public(res)

