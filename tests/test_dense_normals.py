"""Surface normals of the dense map without a GPU: the numpy oracle (tests/dense_normals_ref.py, the arithmetic the
kernels of csrc/voxel_normals.hip reproduce byte for byte) against analytic geometry, with bounds derived below; the
C-ABI argument checks of the four entry points; the option's config and CLI flags; the PLY writer.

Error terms shared by the geometry tests (angles in radians, small enough that sin x ~ x is not used: asin is taken):

  e_p   the points are fp32.  A coordinate c is off by at most 2^-24 |c|, a point by 2^-24 |P|, a difference of two
        points by eta = 2^-23 Pmax.  For n = b x a and a unit vector u, (b x a) x u = a (b.u) - b (a.u), so a change of
        a, b by at most eta turns the direction of n by at most asin((eta / |a| + eta / |b|) / sin(theta)), theta the
        angle between a and b.  e_p takes the smallest |a|, |b| and sin(theta) over the contributing pixels.
  e_q   a pixel adds rint(32768 n / |n|): every component is off by at most 1/2, the vector by sqrt(3)/2, relative to the
        length 32768: e_q = sqrt(3) / 65536.  The mean of vectors that each lie within angle A of u and carry an
        error vector of at most e_q lies within A + asin(e_q / cos A) of u (the sum's component along u is at least
        K cos A, the summed errors at most K e_q).
  e_o   the output is fp32: each component of the unit normal is off by at most 2^-24, the vector by sqrt(3) 2^-24."""
import ctypes as C
import dataclasses
import math
import os

import numpy as np
import pytest

import dense_map_ref as dm
import dense_normals_ref as ref

E_Q = math.sqrt(3.0) / 65536.0
E_O = math.sqrt(3.0) * 2.0 ** -24


def _rays(H, W, f):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([(x - (W - 1) / 2) / f, (y - (H - 1) / 2) / f, np.ones((H, W))], -1)     # x right, y down, z forward


def _differences(P, contributes):
    """a, b of the contributing pixels from the fp32 points, in f64."""
    f, y, x = np.nonzero(contributes)
    P = P.astype(np.float64)
    return P[f, y, x + 1] - P[f, y, x - 1], P[f, y + 1, x] - P[f, y - 1, x], (f, y, x)


def _e_p(P, contributes):
    a, b, _ = _differences(P, contributes)
    la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    sin_t = np.linalg.norm(np.cross(b, a), axis=1) / (la * lb)
    eta = 2.0 ** -23 * float(np.abs(P[np.isfinite(P)]).max()) * math.sqrt(3.0)
    return math.asin(min(1.0, (eta / la.min() + eta / lb.min()) / sin_t.min())), float(sin_t.min())


def _voxel_rows(P, conf_thr, v):
    """The oracle's stage 1 of maps without conf / masks -> (cloud, normal rows, the per-pixel part)."""
    cloud = dm.fuse_pixels(P, None, None, None, conf_thr, v)
    part = ref.pixel_normals(P, None, None, conf_thr, dm.inv_voxel(v))
    rows = ref.extract(cloud["keys"], ref.accumulate([part]))
    return cloud, rows, part


def _angle(n, u):
    c = np.sum(n.astype(np.float64) * u, axis=1) / (np.linalg.norm(n.astype(np.float64), axis=1) * np.linalg.norm(u, axis=1))
    return np.arccos(np.clip(c, -1.0, 1.0))


@pytest.mark.parametrize("normal", [(0.0, 0.0, -1.0), (0.35, -0.25, -0.9)], ids=["fronto-parallel", "tilted"])
def test_plane_normals_are_the_planes_and_face_the_camera(normal):
    """Every pixel of a plane has the plane's normal m exactly, up to e_p; so every voxel's normal lies within
    A + asin(e_q / cos A) + e_o of m with A = e_p (module docstring), and faces the camera: n . (P - C) < 0."""
    H, W, f, v = 24, 32, 40.0, 0.05
    m = np.asarray(normal) / np.linalg.norm(normal)
    C0 = np.array([0.2, -0.1, 0.3])
    rays = _rays(H, W, f)
    t = (m @ (np.array([0.0, 0.0, 2.5]) - C0)) / (rays @ m)              # the plane through (0, 0, 2.5)
    P = (C0 + rays * t[..., None]).astype(np.float32)[None]
    cloud, rows, part = _voxel_rows(P, 0.5, v)
    assert part["stats"].tolist() == [(H - 2) * (W - 2), 2 * H + 2 * W - 4, 0, 0]
    e_p, _ = _e_p(P, part["contributes"])
    bound = e_p + math.asin(E_Q / math.cos(e_p)) + E_O
    has = rows["normals"].any(1)
    assert has.sum() > 100 and bound < 2e-4
    ang = _angle(rows["normals"][has], np.broadcast_to(m, (int(has.sum()), 3)))
    assert ang.max() <= bound, (ang.max(), bound)
    assert np.all(np.sum(rows["normals"][has] * (cloud["points"][has].astype(np.float64) - C0), axis=1) < 0)
    assert np.all(np.abs(np.linalg.norm(rows["normals"][has].astype(np.float64), axis=1) - 1.0) <= 1e-6)


def _look(direction):
    z = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)          # columns: the camera's axes in the world, det +1


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
def test_sphere_normals_against_the_analytic_normal_at_the_centroid(inside):
    """A sphere of radius r around c, seen by six cameras along +-x, +-y, +-z (from the centre when inside, from 3 r
    away looking at the centre when outside), so all eight sign patterns of (nx, ny, nz) occur.  The camera-facing
    analytic normal at a point X is u(X) = -+(X - c) / |X - c| (inward inside, outward outside).

    Bound on the angle between a voxel's normal and u(G), G its centroid:
      voxel term   every pixel point P of the voxel and G lie in the voxel's box, |P - G| <= sqrt(3) v (+ fp32 rounding
                   of G, 2^-23 |G|); |P - c| = r, and a displacement d of a vector of length r turns it by at most
                   asin(d / r): u(P) is within asin(sqrt(3) v / r) of u(G);
      chord term   a = R - L and b = D - U are chords: (R - L) . (R + L - 2 c) = |R - c|^2 - |L - c|^2 = 0, so a is
                   perpendicular to the radius through its midpoint M_a, which is within s (the largest distance of a
                   contributing pixel to one of its four neighbours) of P, hence within asin(s / r) of u(P): |a . u(P)|
                   <= |a| s / r, likewise b.  With |(b x a) x u| <= |a| |b . u| + |b| |a . u| and |b x a| = |a| |b|
                   sin(theta): the pixel's normal is within asin(2 (s / r) / sin(theta_min)) of u(P);
      e_p, e_q, e_o as in the module docstring, with A = voxel + chord + e_p.
    The sign is part of the bound (< pi / 2)."""
    r, v, H, W, f = 1.0, 0.04, 32, 32, 40.0
    c = np.array([0.3, -0.2, 0.5])
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    rays, P, M = _rays(H, W, f), [], []
    for d in dirs:
        R = _look(d)
        w = rays @ R.T                                                   # ray directions in the world, unnormalised
        wn = w / np.linalg.norm(w, axis=-1, keepdims=True)
        if inside:
            X = c + r * wn                                               # from the centre every ray meets the sphere at r
            ok = np.ones((H, W), bool)
        else:
            eye = c - 3.0 * r * R[:, 2]
            bq = np.sum(wn * (eye - c), -1)
            disc = bq * bq - (np.sum((eye - c) ** 2) - r * r)
            ok = disc > 0.25 * r * r                                     # the central cap only: no grazing chords
            X = eye + wn * (-bq - np.sqrt(np.where(ok, disc, 0.0)))[..., None]
        P.append(X.astype(np.float32))
        M.append(ok.astype(np.uint8))
    P, M = np.stack(P), np.stack(M)
    inv_v = dm.inv_voxel(v)
    cloud = dm.fuse_pixels(P, None, M, None, 0.5, v)
    part = ref.pixel_normals(P, None, M, 0.5, inv_v)
    rows = ref.extract(cloud["keys"], ref.accumulate([part]))
    assert part["stats"][0] > 1500 and part["stats"][2] == 0
    a, b, (fi, yi, xi) = _differences(P, part["contributes"])
    P64 = P.astype(np.float64)
    s = max(float(np.linalg.norm(P64[fi, yi, xi] - P64[fi, yi + dy, xi + dx], axis=1).max())
            for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)))
    e_p, sin_t = _e_p(P, part["contributes"])
    has = rows["normals"].any(1)
    G = cloud["points"][has].astype(np.float64)
    voxel = math.asin((math.sqrt(3.0) * v + 2.0 ** -23 * float(np.abs(G).max()) * math.sqrt(3.0)) / r)
    chord = math.asin(2.0 * (s / r) / sin_t)
    A = voxel + chord + e_p
    bound = A + math.asin(E_Q / math.cos(A)) + E_O
    assert bound < math.pi / 2
    u = (G - c) / np.linalg.norm(G - c, axis=1, keepdims=True) * (-1.0 if inside else 1.0)
    ang = _angle(rows["normals"][has], u)
    print(f"{'inside' if inside else 'outside'}: {int(has.sum())} voxels, largest angle {ang.max():.4f} rad, bound "
          f"{bound:.4f} (voxel {voxel:.4f}, chord {chord:.4f}, e_p {e_p:.2e})")
    assert has.sum() > 800 and ang.max() <= bound
    signs = {tuple(np.sign(n).astype(int)) for n in rows["normals"][has] if np.all(n != 0)}
    assert len(signs) == 8


def test_zero_normal_voxels_are_exactly_those_without_a_full_neighbourhood():
    """An exact condition, computed here pixel by pixel from the inputs (no array shifts, none of the oracle's helpers
    but the key quantisation): a voxel has a zero normal iff none of its candidate pixels is an interior pixel whose four
    neighbours are candidates.  (The surface is smooth and seen from one side: no degenerate cross product, no
    cancellation; both are asserted.)"""
    rng = np.random.default_rng(4)
    N, H, W, thr, v = 3, 16, 24, 0.6, 0.02
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    P = np.empty((N, H, W, 3), np.float32)
    for f in range(N):
        z = 2.0 + 0.2 * np.sin(0.3 * x + f) * np.cos(0.25 * y)
        P[f] = np.stack([(x - W / 2) * z / 70.0 + 0.1 * f, (y - H / 2) * z / 70.0, z], -1)
    conf = rng.normal(1.5, 1.0, (N, H, W)).astype(np.float32)
    masks = (rng.random((N, H, W)) < 0.9).astype(np.uint8)
    P.reshape(-1, 3)[rng.choice(N * H * W, 6, replace=False), 0] = [np.nan, np.inf, 3.0e5, -np.inf, np.nan, -3.0e5]
    cloud = dm.fuse_pixels(P, conf, masks, None, thr, v)
    part = ref.pixel_normals(P, conf, masks, thr, dm.inv_voxel(v))
    rows = ref.extract(cloud["keys"], ref.accumulate([part]))
    assert part["stats"][2] == 0
    ok, keys, _ = dm.quantise(P.reshape(-1, 3), dm.inv_voxel(v))
    ok, keys = ok.reshape(N, H, W), keys.reshape(N, H, W)
    logit = dm.conf_logit(thr)
    cand = lambda f, i, j: bool(masks[f, i, j]) and bool(conf[f, i, j] > logit) and bool(ok[f, i, j])      # noqa: E731
    occupied, with_normal = set(), set()
    for f in range(N):
        for i in range(H):
            for j in range(W):
                if not cand(f, i, j):
                    continue
                occupied.add(int(keys[f, i, j]))
                if 1 <= i <= H - 2 and 1 <= j <= W - 2 and cand(f, i, j - 1) and cand(f, i, j + 1) \
                        and cand(f, i - 1, j) and cand(f, i + 1, j):
                    with_normal.add(int(keys[f, i, j]))
    assert occupied == {int(k) for k in cloud["keys"]}
    zero = {int(k) for k, n in zip(rows["keys"], rows["normals"]) if not n.any()}
    assert zero == occupied - with_normal
    assert len(zero) > 20 and len(with_normal) > 100
    assert all(w == 0 for k, w in zip(rows["keys"], rows["normal_weights"]) if int(k) in zero)
    assert int(rows["normal_weights"].sum()) == int(part["stats"][0])


def test_oracle_point_normals_cancel_and_shade_values():
    """Stage 2 and the shading by hand: opposite normals of equal weight give (0,0,0) with their weights kept; a normal
    facing the camera is white in `shaded`, one facing away black, and normal_rgb is (n + 1) * 127.5 rounded to even."""
    pts = np.array([[0.01, 0.01, 0.01], [0.012, 0.01, 0.01], [0.5, 0.5, 0.5]], np.float32)
    nr = np.array([[0.0, 0.6, 0.8], [0.0, -0.6, -0.8], [0.0, 0.0, -1.0]], np.float32)
    part = ref.point_normals(pts, nr, np.array([2, 2, 5], np.int32), np.eye(3).reshape(9), dm.inv_voxel(0.05))
    acc = ref.accumulate([part])
    rows = ref.extract(acc["keys"], acc)
    assert rows["normals"].tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0]] and rows["normal_weights"].tolist() == [4, 5]
    cams = np.zeros((1, 20))
    cams[0, [0, 5, 10]] = 1.0
    index = np.array([[[0, 1, 2, -1, 7]]], np.int32)
    normals = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.6, 0.0, -0.8]], np.float32)
    out = ref.shade(index, normals, cams)
    assert out["shaded"].tolist() == [[[255, 0, 204, 0, 0]]] and out["pixels"] == 3
    assert out["normal"][0, 0].tolist() == [[128, 128, 0], [128, 128, 255], [204, 128, 25], [0, 0, 0], [0, 0, 0]]


# --------------------------------------------------------------------------------------------------- product, no GPU
def test_entry_points_are_declared_bound_and_check_their_arguments(built_lib):
    from conftest import ROOT
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    names = ("pi3_voxel_fuse_pixel_normals", "pi3_voxel_fuse_point_normals", "pi3_voxel_extract_normals",
             "pi3_render_shade")
    for name in names:
        assert name + "(" in text and name in lib.SIGNATURES, name
    dll = lib.load(require_gpu=False)
    assert dll.pi3_abi_version() == 7
    buf = (C.c_ulonglong * 64)()                 # a host address: every call below must be refused before any launch
    p = C.addressof(buf)
    inf = float("inf")
    bad = {
        "pi3_voxel_fuse_pixel_normals": [
            (None, 64, p, p, None, None, 1, 3, 3, 0.0, 50.0, p, None),         # no table
            (p, 48, p, p, None, None, 1, 3, 3, 0.0, 50.0, p, None),            # capacity not a power of two
            (p, 64, None, p, None, None, 1, 3, 3, 0.0, 50.0, p, None),         # no nacc
            (p, 64, p, None, None, None, 1, 3, 3, 0.0, 50.0, p, None),         # no points
            (p, 64, p, p, None, None, 1, 3, 3, 0.0, 50.0, None, None),         # no stats
            (p, 64, p, p, None, None, 1, 0, 3, 0.0, 50.0, p, None),            # H = 0
            (p, 16, p, p, None, None, 1, 3, 3, 0.0, 50.0, p, None),            # capacity < 2 N H W
            (p, 64, p, p, None, None, 1, 3, 3, 0.0, 0.0, p, None),             # inv_voxel = 0
            (p, 64, p, p, None, None, 1, 3, 3, 0.0, inf, p, None)],
        "pi3_voxel_fuse_point_normals": [
            (None, 64, p, p, p, p, p, 4, 50.0, p, None),
            (p, 63, p, p, p, p, p, 4, 50.0, p, None),
            (p, 64, None, p, p, p, p, 4, 50.0, p, None),
            (p, 64, p, p, None, p, p, 4, 50.0, p, None),                       # no normals
            (p, 64, p, p, p, None, p, 4, 50.0, p, None),                       # no nweights
            (p, 64, p, p, p, p, None, 4, 50.0, p, None),                       # no rotation
            (p, 64, p, p, p, p, p, -1, 50.0, p, None),
            (p, 4, p, p, p, p, p, 4, 50.0, p, None),                           # capacity < 2 n
            (p, 64, p, p, p, p, p, 4, -1.0, p, None)],
        "pi3_voxel_extract_normals": [
            (None, 64, p, None, p, p, p, 8, p, None),
            (p, 0, p, None, p, p, p, 8, p, None),
            (p, 64, None, None, p, p, p, 8, p, None),
            (p, 64, p, None, None, p, p, 8, p, None),
            (p, 64, p, None, p, None, p, 8, p, None),
            (p, 64, p, None, p, p, None, 8, p, None),
            (p, 64, p, None, p, p, p, -1, p, None),
            (p, 64, p, None, p, p, p, 8, None, None)],
        "pi3_render_shade": [
            (None, p, 4, p, 1, 2, 2, p, p, p, None),
            (p, None, 4, p, 1, 2, 2, p, p, p, None),                           # V > 0 without normals
            (p, p, -1, p, 1, 2, 2, p, p, p, None),
            (p, p, 1 << 31, p, 1, 2, 2, p, p, p, None),
            (p, p, 4, None, 1, 2, 2, p, p, p, None),
            (p, p, 4, p, 0, 2, 2, p, p, p, None),
            (p, p, 4, p, 1, 2, 0, p, p, p, None),
            (p, p, 4, p, 1, 2, 2, None, p, p, None),
            (p, p, 4, p, 1, 2, 2, p, None, p, None),
            (p, p, 4, p, 1, 2, 2, p, p, None, None)],
    }
    for name, cases in bad.items():
        fn = getattr(dll, name)
        for args in cases:
            assert len(args) == len(lib.SIGNATURES[name])
            assert fn(*args) < 0, (name, args)
            assert name.encode() in dll.pi3_last_error()
    # empty inputs are fine and launch nothing
    assert dll.pi3_voxel_fuse_pixel_normals(p, 64, p, None, None, None, 0, 3, 3, 0.0, 50.0, p, None) == 0
    assert dll.pi3_voxel_fuse_point_normals(p, 64, p, None, None, None, p, 0, 50.0, p, None) == 0


def test_makefile_compiles_the_normals_without_contraction():
    from conftest import ROOT
    import subprocess
    csrc = os.path.join(ROOT, "pi3_slam_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "voxel_normals.hip" in mk.split("SRCS =")[1].split("\n")[0]
    rule = [blk for blk in mk.replace("\\\n", " ").split("\n") if "-ffp-contract=off" in blk and not blk.startswith("#")]
    assert len(rule) == 1
    # what make itself would run (a dry run: nothing is compiled): the object of every build, =off after =fast
    objs = [f"{d}/{s}.o" for d in ("build", "build_asan", "build_dev") for s in ("voxel_normals", "dense_filter")]
    said = subprocess.run(["make", "-C", csrc, "-n", "-B"] + objs, check=True, capture_output=True, text=True).stdout
    for o in objs:
        cmd = [ln for ln in said.split("\n") if ln.rstrip().endswith(f"-o {o}")]
        assert len(cmd) == 1 and cmd[0].rfind("-ffp-contract=off") > cmd[0].rfind("-ffp-contract=fast") >= 0, (o, cmd)
    plain = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/voxel.o"], check=True, capture_output=True, text=True)
    assert "-ffp-contract=off" not in plain.stdout and "-ffp-contract=fast" in plain.stdout


def test_option_in_config_cli_and_online_signature(capsys):
    import inspect
    from pi3_slam_amd import cli
    from pi3_slam_amd.chunk_creator import OfflineCreatorConfig
    from pi3_slam_amd.dense_map import ChunkCloudBuilder
    from pi3_slam_amd.online import Pi3SLAMOnline
    assert OfflineCreatorConfig(model_path="recipe", output_dir="x").dense_normals is False
    assert inspect.signature(Pi3SLAMOnline.__init__).parameters["dense_normals"].default is False
    ps = cli.build_parser()
    a = ps.parse_args(["create", "--images", "i", "--output", "o", "--dense-voxel-size", "0.02", "--dense-normals"])
    assert a.dense_normals is True
    assert ps.parse_args(["create", "--images", "i", "--output", "o"]).dense_normals is False
    assert ps.parse_args(["online", "--output_path", "o", "--dense_normals"]).dense_normals is True
    assert ps.parse_args(["online", "--output_path", "o"]).dense_normals is False
    assert not hasattr(ps.parse_args(["reconstruct", "--chunks", "c", "--output", "o"]), "dense_normals")
    # without a voxel size the option warns and builds nothing, as dense_min_views does
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir="x", dense_normals=True)
    assert ChunkCloudBuilder.from_config(cfg, "cpu") is None
    assert "dense_normals has no effect without dense_voxel_size" in capsys.readouterr().out
    assert ChunkCloudBuilder.from_config(OfflineCreatorConfig(model_path="recipe", output_dir="x"), "cpu") is None
    assert capsys.readouterr().out == ""


def test_write_ply_normals_header_and_round_trip(tmp_path):
    from pi3_slam_amd.export import DenseMap, write_dense_points, write_ply, write_ply_normals
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(7, 3)).astype(np.float32)
    nr = rng.normal(size=(7, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    path = str(tmp_path / "n.ply")
    write_ply_normals(pts, nr, rgb, path)
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    assert head.decode().split("\n") == [
        "ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y",
        "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
        "property uchar green", "property uchar blue", ""]
    assert len(body) == 7 * 27
    rec = np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    assert rec["xyz"].tobytes() == pts.tobytes() and rec["n"].tobytes() == nr.tobytes() and rec["rgb"].tobytes() == rgb.tobytes()
    with pytest.raises(ValueError):
        write_ply_normals(pts, nr[:3], rgb, path)
    # write_dense_points: the old file without normals, byte for byte; the new layout with them
    dense = DenseMap(pts, rgb, np.ones(7, np.int32), 0.02)
    write_dense_points(dense, str(tmp_path / "a.ply"))
    write_ply(pts, rgb, str(tmp_path / "b.ply"))
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    write_dense_points(dataclasses.replace(dense, normals=nr), str(tmp_path / "c.ply"))
    assert open(tmp_path / "c.ply", "rb").read() == data
