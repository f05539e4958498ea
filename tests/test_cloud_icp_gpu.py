"""The ICP reduction on the GPU (csrc/cloud_icp.hip through ops.cloud_pair_equations) against the numpy oracle
(tests/cloud_icp_ref.py) under the bound two differently ordered f64 sums can differ by, then map_eval.icp_refine and
compare_clouds(icp=...) on the planted room against what the oracle's own ICP reaches there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_icp_ref as iref            # noqa: E402
import test_cloud_icp as cpu            # noqa: E402  (the oracle's runs on the room and the limits they must meet)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPAN = iref.SPAN
U = 2.0 ** -52
ROT30 = np.array([[np.cos(np.pi / 6), -np.sin(np.pi / 6), 0.0], [np.sin(np.pi / 6), np.cos(np.pi / 6), 0.0], [0.0, 0.0, 1.0]])
# every normals_of mode; mode 2 with Rn NULL and with a 30 degree rotation
VARIANTS = [(0, None), (1, None), (2, None), (2, ROT30)]


def run_kernel(q, pts, idx, d2, trim, centre, normals, mode, Rn, out_fill=None):
    """-> (out f64 (40,), counters dict) of one call; the workspace is filled with NaN first (it must not matter)."""
    from pi3_slam_amd import ops
    m = len(q)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)        # noqa: E731
    partials = torch.full((ops.cloud_icp_partial_rows(m), 40), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((40,), 7.0 if out_fill is None else out_fill, dtype=torch.float64, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    nt = None if normals is None else t(normals, np.float32).reshape(-1, 3)
    ops.cloud_pair_equations(t(q, np.float32).reshape(-1, 3), t(pts, np.float32).reshape(-1, 3), t(idx, np.int32),
                             t(d2, np.float64), trim, centre, nt, mode, Rn, partials, out, counters)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dict(zip(ops.CLOUD_ICP_COUNTERS, counters.tolist()))


def check(q, pts, idx, d2, trim, centre, normals=None, mode=0, Rn=None, say=""):
    """One call against the oracle: every one of the 37 sums within (pairs + 64) 2^-52 majorant (two f64 sums of
    `pairs` terms in different orders, each term a handful of rounded operations), the counters equal, the spare
    doubles zero.  -> (out, oracle)."""
    got, cnt = run_kernel(q, pts, idx, d2, trim, centre, normals, mode, Rn)
    exp = iref.pair_equations(q, pts, idx, d2, trim, centre, normals, mode, Rn)
    pairs = exp["counters"]["used"]
    bound = (pairs + 64) * U * exp["majorant"]
    diff = np.abs(got[:37] - exp["sums"])
    worst = float(np.max(np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))))
    print(f"{say} mode {mode}{' Rn' if Rn is not None else ''} m={len(q)} pairs={pairs}: worst |device - oracle| / bound = {worst:.3g}")
    assert cnt == exp["counters"], (cnt, exp["counters"])
    assert np.isfinite(got).all() and got[37:].tolist() == [0.0, 0.0, 0.0]
    assert np.all(diff <= bound), (np.flatnonzero(diff > bound), diff, bound)
    return got, exp


def searched(pts, q, max_dist):
    """idx int32 and d2 f64 exactly as pi3_cloud_nearest writes them."""
    from pi3_slam_amd.map_eval import CloudIndex
    index = CloudIndex(pts, max_dist, DEV)
    qt = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV).reshape(-1, 3)
    d2 = torch.empty(len(q), dtype=torch.float64, device=DEV)
    idx = torch.empty(len(q), dtype=torch.int32, device=DEV)
    index.nearest_into(qt, d2, idx, torch.zeros(4, dtype=torch.int64, device=DEV))
    return idx.cpu().numpy(), d2.cpu().numpy()


def cloud_pair(n, m, seed, shift=(0.0, 0.0, 0.0), spread=0.02):
    """n indexed points in a unit cube (+ shift), m queries near random ones of them (a tenth far away), normals for
    both: random directions and lengths."""
    rng = np.random.default_rng(seed)
    shift = np.asarray(shift, np.float64)
    pts = (rng.random((n, 3)) + shift).astype(np.float32)
    q = pts[rng.integers(0, n, m)].astype(np.float64) + spread * rng.standard_normal((m, 3))
    q[rng.random(m) < 0.1] += 5.0
    npts = (rng.standard_normal((n, 3)) * rng.uniform(0.1, 3.0, (n, 1))).astype(np.float32)
    nq = (rng.standard_normal((m, 3)) * rng.uniform(0.1, 3.0, (m, 1))).astype(np.float32)
    return pts, q.astype(np.float32), npts, nq


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 5])
def test_agreement_with_the_oracle_at_every_size(m):
    n, md = 500, 0.1
    pts, q, npts, nq = cloud_pair(n, m, 100 + m)
    idx, d2 = searched(pts, q, md)
    trim = 0.04                                                                        # some matched pairs are trimmed
    centre = [0.4, 0.6, 0.5]
    for mode, Rn in VARIANTS:
        got, exp = check(q, pts, idx, d2, trim, centre, (None, npts, nq)[mode], mode, Rn, say="sizes")
        c = exp["counters"]
        assert sum(c.values()) == m
        if m >= 63:
            assert c["used"] > m // 4 and c["unmatched"] > 0 and c["trimmed"] > 0
        if m == 0:
            assert not got.any()


def test_every_query_unmatched():
    pts, q, npts, nq = cloud_pair(500, 700, 1)
    idx, d2 = np.full(700, -1, np.int32), np.full(700, np.inf)
    for mode, Rn in VARIANTS:
        got, cnt = run_kernel(q, pts, idx, d2, 0.1, [0, 0, 0], (None, npts, nq)[mode], mode, Rn)
        assert not got.any() and cnt == dict(used=0, unmatched=700, trimmed=0, normal_rejected=0)
    # an index past the cloud is unmatched too, never read
    idx[::2] = 500
    got, cnt = run_kernel(q, pts, idx, np.zeros(700), 0.1, [0, 0, 0], npts, 1, None)
    assert not got.any() and cnt["unmatched"] == 700


def test_all_queries_matched_to_one_row():
    pts, q, npts, nq = cloud_pair(500, 1000, 2)
    q = (pts[7].astype(np.float64) + 0.01 * np.random.default_rng(3).standard_normal((1000, 3))).astype(np.float32)
    idx = np.full(1000, 7, np.int32)
    dq = q.astype(np.float64) - pts[7].astype(np.float64)
    d2 = (dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2]
    for mode, Rn in VARIANTS:
        got, exp = check(q, pts, idx, d2, 1.0, pts[7].astype(np.float64), (None, npts, nq)[mode], mode, Rn, say="one row")
        assert exp["counters"]["used"] == 1000


def test_trim_distance_is_inclusive_to_the_ulp():
    a, b, R = 3.0 / 128.0, 4.0 / 128.0, 5.0 / 128.0                                    # 3-4-5: every square and sum exact
    pts = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    q = np.array([[a, b, 0], [1 + a / 2, 1, 1], [2, 2 - 2 * b, 2]], np.float32)
    idx, d2 = searched(pts, q, 0.1)
    assert idx.tolist() == [0, 1, 2] and d2[0] == R * R and d2[1] < d2[0] < d2[2]
    nrm = np.ones((3, 3), np.float32)
    for mode, Rn in VARIANTS:
        _, exp = check(q, pts, idx, d2, R, [0, 0, 0], nrm if mode else None, mode, Rn, say="trim at d")
        assert exp["counters"] == dict(used=2, unmatched=0, trimmed=1, normal_rejected=0)
        _, exp = check(q, pts, idx, d2, float(np.nextafter(R, 0.0)), [0, 0, 0], nrm if mode else None, mode, Rn, say="an ulp below")
        assert exp["counters"] == dict(used=1, unmatched=0, trimmed=2, normal_rejected=0)
    _, exp = check(q, pts, idx, d2, 0.0, [0, 0, 0], say="trim 0")
    assert exp["counters"]["used"] == 0


def test_bad_normals_are_rejected_and_counted():
    pts, q, npts, nq = cloud_pair(500, 900, 5, spread=0.005)
    idx, d2 = searched(pts, q, 0.1)
    bad = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [-0.0, 0.0, 0.0], [np.nan] * 3], np.float32)
    npts[::5] = bad[np.arange(len(npts[::5])) % len(bad)]
    nq[::7] = bad[np.arange(len(nq[::7])) % len(bad)]
    for mode, Rn in VARIANTS[1:]:
        got, exp = check(q, pts, idx, d2, 0.1, [0.5, 0.5, 0.5], (None, npts, nq)[mode], mode, Rn, say="bad normals")
        assert exp["counters"]["normal_rejected"] > 50 and exp["counters"]["used"] > 400
        assert not np.isnan(got).any()
    tiny = np.full((900, 3), 1e-40, np.float32)                                      # subnormal, but not zero: a direction
    _, exp = check(q, pts, idx, d2, 0.1, [0.5, 0.5, 0.5], tiny, 2, None, say="tiny normals")
    assert exp["counters"]["normal_rejected"] == 0


def test_far_from_the_origin_with_the_centre_there():
    """Coordinates near 9 000 m: the sums are about `centre`, so the bound still holds; it would not if x were p."""
    shift = np.array([9000.0, -9000.0, 4000.0])
    pts, q, npts, nq = cloud_pair(500, 2 * SPAN + 77, 6, shift=shift, spread=0.01)
    idx, d2 = searched(pts, q, 0.1)
    centre = shift + 0.5
    for mode, Rn in VARIANTS:
        got, exp = check(q, pts, idx, d2, 0.1, centre, (None, npts, nq)[mode], mode, Rn, say="9000 m")
        assert exp["counters"]["used"] > SPAN
        about_origin = iref.pair_equations(q, pts, idx, d2, 0.1, [0, 0, 0], (None, npts, nq)[mode], mode, Rn)
        bound = (exp["counters"]["used"] + 64) * U * exp["majorant"]
        assert np.abs(about_origin["sums"][:28] - got[:28]).max() > 1e6 * bound[:28].max()          # the centre matters


def test_two_calls_give_the_same_bits():
    m = 3 * SPAN + 5
    pts, q, npts, nq = cloud_pair(500, m, 7)
    idx, d2 = searched(pts, q, 0.1)
    for mode, Rn in VARIANTS:
        a, ca = run_kernel(q, pts, idx, d2, 0.05, [0.5, 0.5, 0.5], (None, npts, nq)[mode], mode, Rn)
        b, cb = run_kernel(q, pts, idx, d2, 0.05, [0.5, 0.5, 0.5], (None, npts, nq)[mode], mode, Rn, out_fill=-3.0)
        assert a.tobytes() == b.tobytes() and ca == cb and a[:37].any()


def test_argument_errors_launch_nothing_on_the_device():
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    pts, q, npts, nq = cloud_pair(500, 300, 8)
    idx, d2 = searched(pts, q, 0.1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)        # noqa: E731
    qt, pt, it, dt_, nt = t(q, np.float32), t(pts, np.float32), t(idx, np.int32), t(d2, np.float64), t(nq, np.float32)
    partials = torch.full((1, 40), 3.0, dtype=torch.float64, device=DEV)
    out = torch.full((40,), 5.0, dtype=torch.float64, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    for kw in (dict(trim_dist=-1.0), dict(trim_dist=float("nan")), dict(trim_dist=float("inf")), dict(normals_of=3),
               dict(normals_of=-1), dict(centre=[0.0, float("nan"), 0.0]), dict(normals_of=2, Rn=np.full((3, 3), np.inf))):
        a = dict(trim_dist=0.1, centre=[0.0, 0.0, 0.0], normals_of=0, Rn=None)
        a.update(kw)
        with pytest.raises(L.Pi3HipError, match="pi3_cloud_pair_equations"):
            if a["normals_of"] in (0, 1, 2):
                ops.cloud_pair_equations(qt, pt, it, dt_, a["trim_dist"], a["centre"], nt if a["normals_of"] else None,
                                         a["normals_of"], a["Rn"], partials, out, counters)
            else:                                                                      # past the wrapper's own asserts
                c3 = (C.c_double * 3)(0.0, 0.0, 0.0)
                rc = L.load().pi3_cloud_pair_equations(qt.data_ptr(), 300, pt.data_ptr(), 500, it.data_ptr(), dt_.data_ptr(),
                                                       0.1, C.cast(c3, C.c_void_p), nt.data_ptr(), a["normals_of"], None,
                                                       partials.data_ptr(), 1, out.data_ptr(), counters.data_ptr(),
                                                       L.stream_ptr())
                L.check(rc, "pi3_cloud_pair_equations")
    with pytest.raises(L.Pi3HipError, match="rows"):                                   # a workspace one row short
        big = torch.zeros((SPAN + 1, 3), dtype=torch.float32, device=DEV)
        ops.cloud_pair_equations(big, pt, torch.zeros(SPAN + 1, dtype=torch.int32, device=DEV),
                                 torch.zeros(SPAN + 1, dtype=torch.float64, device=DEV), 0.1, [0, 0, 0], None, 0, None,
                                 partials, out, counters)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and counters.tolist() == [11] * 4 and bool((partials == 3.0).all())
    ops.cloud_pair_equations(qt, pt, it, dt_, 0.1, [0.0, 0.0, 0.0], None, 0, None, partials, out, counters)
    torch.cuda.synchronize()
    assert counters.tolist()[0] > 200 and sum(counters.tolist()) == 300 and float(out[22]) == counters.tolist()[0]


# ------------------------------------------------------------------------------------------------ icp_refine
@pytest.fixture(scope="module")
def rooms():
    return {scale: iref.planted_room(scale=scale) for scale in (1.0, 1.02)}


@pytest.mark.parametrize("mode", ["point", "plane"])
def test_identity_is_found_in_one_iteration_exactly(rooms, mode):
    from pi3_slam_amd.map_eval import icp_refine
    room = rooms[1.0]
    est = room["ref"][::3]
    kw = dict(ref_normals=room["ref_normals"]) if mode == "plane" else {}
    res = icp_refine(est, room["ref"], mode=mode, max_dist=0.25, init=np.eye(4), device=DEV, **kw)
    assert res["status"] == "converged" and res["iterations"] == 1
    assert np.array_equal(res["transform"], np.eye(4)) and np.array_equal(res["increment"], np.eye(4))
    h = res["history"][0]
    assert h["pairs"] == len(est) and h["rms"] == 0.0 and h["point_rms"] == 0.0 and h["step"] == 0.0


@pytest.mark.parametrize("scale", [1.0, 1.02])
@pytest.mark.parametrize("mode,source_normals", [("plane", False), ("plane", True), ("point", False)])
def test_recovery_of_the_planted_motion(rooms, mode, source_normals, scale):
    """The device's ICP ends within twice the oracle's own final error plus 0.001 deg / 0.01 mm of the truth (the factor
    two: the device sees fp32-rounded moved points, the oracle does not).  source_normals: only the estimate's normals
    are given (normals_of = 2); the bound fails if Rn is not applied."""
    from pi3_slam_amd.map_eval import icp_refine
    room = rooms[scale]
    oracle = cpu.oracle_run(mode, scale, source_normals)
    kw = {}
    if mode == "plane":
        kw = dict(est_normals=room["est_normals"]) if source_normals else dict(ref_normals=room["ref_normals"])
    res = icp_refine(room["est"], room["ref"], mode=mode, with_scale=scale != 1.0, max_dist=cpu.MAX_DIST,
                     iterations=cpu.ORACLE_ITERATIONS[mode], device=DEV, **kw)
    err = iref.alignment_error(res["transform"], room["truth"])
    print(f"{mode}{' (source normals)' if source_normals else ''} scale {scale}: device {res['status']} after "
          f"{res['iterations']}: {err}; oracle {oracle['status']} after {oracle['iterations']}: {oracle['error']}")
    assert np.isfinite(res["transform"]).all()
    assert err["rotation_deg"] <= 2.0 * oracle["error"]["rotation_deg"] + cpu.DEVICE_SLACK[0]
    assert err["centre_m"] <= 2.0 * oracle["error"]["centre_m"] + cpu.DEVICE_SLACK[1]
    if scale == 1.0:
        assert abs(np.cbrt(np.linalg.det(res["transform"][:3, :3])) - 1.0) < 1e-12          # rigid stays rigid
    np.testing.assert_allclose(res["increment"], res["transform"], rtol=0, atol=0)            # init = None
    if mode == "plane":
        assert res["status"] == "converged" and res["iterations"] <= 15
    else:
        rms = [h["point_rms"] for h in res["history"]]
        assert all(b <= a + 1e-9 for a, b in zip(rms, rms[1:])), rms
    for h in res["history"]:
        assert sum(h["counters"].values()) == len(room["est"]) and h["pairs"] == h["counters"]["used"]


def test_init_is_composed_and_the_increment_reported(rooms):
    from pi3_slam_amd.map_eval import icp_refine
    room = rooms[1.0]
    init = iref.increment(np.array([0.01, 0.0, -0.01, 0.0, 0.02, 0.0, 0.01]), np.zeros(3))
    res = icp_refine(room["est"], room["ref"], mode="plane", ref_normals=room["ref_normals"], max_dist=0.25, init=init, device=DEV)
    oracle = cpu.oracle_run("plane", 1.0, False)
    err = iref.alignment_error(res["transform"], room["truth"])
    assert res["status"] == "converged"
    assert err["rotation_deg"] <= 2.0 * oracle["error"]["rotation_deg"] + cpu.DEVICE_SLACK[0]
    assert err["centre_m"] <= 2.0 * oracle["error"]["centre_m"] + cpu.DEVICE_SLACK[1]
    np.testing.assert_allclose(res["increment"] @ init, res["transform"], rtol=0, atol=1e-12)


def test_refusals():
    from pi3_slam_amd.map_eval import icp_refine
    rng = np.random.default_rng(11)
    plane = np.c_[rng.random((3000, 2)) * [4.0, 3.0], np.zeros(3000)].astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (3000, 1))
    init = iref.increment(np.array([0.0, 0.0, 0.0, 0.0, 0.01, 0.0, 0.02]), np.zeros(3))
    res = icp_refine(plane[::2], plane, mode="plane", ref_normals=up, max_dist=0.25, init=init, device=DEV)
    assert res["status"] == "degenerate" and res["iterations"] == 1
    assert np.array_equal(res["transform"], init) and np.isfinite(res["increment"]).all()
    assert res["history"][0]["pairs"] == 1500 and res["history"][0]["step"] is None
    line = np.c_[np.linspace(0, 4, 2000), np.zeros((2000, 2))].astype(np.float32)
    res = icp_refine(line[::2] + np.float32([0, 0.01, 0]), line, mode="point", max_dist=0.25, device=DEV)
    assert res["status"] == "degenerate" and np.array_equal(res["transform"], np.eye(4))
    far = plane[::2] + np.float32([0, 0, 10.0])
    res = icp_refine(far, plane, mode="point", max_dist=0.25, device=DEV)
    assert res["status"] == "too_few_pairs" and np.array_equal(res["transform"], np.eye(4))
    assert res["history"][0]["pairs"] == 0 and res["history"][0]["rms"] is None
    with pytest.raises(ValueError, match="normals"):
        icp_refine(far, plane, mode="plane", max_dist=0.25, device=DEV)


# ------------------------------------------------------------------------------------------------ compare_clouds
KEYS_WITHOUT_ICP = ["points", "dropped", "accuracy", "completeness", "precision", "recall", "fscore", "search", "settings",
                    "_distances", "_points"]


@pytest.mark.parametrize("voxel_size,which", [(None, "ref_normals"), (0.05, "est_normals")])
def test_compare_clouds_scores_the_moved_room_as_the_unmoved_one(rooms, voxel_size, which):
    from pi3_slam_amd.map_eval import compare_clouds, public, tau_key
    room = rooms[1.0]
    k = tau_key(0.02)
    kw = dict(max_dist=0.25, voxel_size=voxel_size, device=DEV)
    plain = compare_clouds(room["est"], room["ref"], [0.02], **kw)
    unmoved = compare_clouds(room["est_unmoved"], room["ref"], [0.02], **kw)
    refined = compare_clouds(room["est"], room["ref"], [0.02], icp={"mode": "plane", which: room[which]}, **kw)
    print({name: (r["precision"][k], r["recall"][k]) for name, r in (("plain", plain), ("unmoved", unmoved), ("refined", refined))},
          refined["icp"]["status"], refined["icp"]["iterations"])
    assert list(plain) == KEYS_WITHOUT_ICP and "icp" not in plain
    assert list(refined) == KEYS_WITHOUT_ICP[:-2] + ["icp"] + KEYS_WITHOUT_ICP[-2:]
    assert refined["icp"]["status"] == "converged"
    for score in ("precision", "recall"):
        assert refined[score][k] > plain[score][k]
        assert abs(refined[score][k] - unmoved[score][k]) <= 0.01
    M = np.array(refined["settings"]["transform"])
    assert np.array_equal(M, np.array(refined["icp"]["transform"])) and np.array_equal(M, np.array(refined["icp"]["increment"]))
    oracle = cpu.oracle_run("plane", 1.0, which == "est_normals")
    err = iref.alignment_error(M, room["truth"])
    if voxel_size is None:
        assert err["centre_m"] <= 2.0 * oracle["error"]["centre_m"] + cpu.DEVICE_SLACK[1]
    else:
        assert err["centre_m"] < 2e-3 and err["rotation_deg"] < 0.05                 # another cloud: the resampled one
    # the reported matrix, given back as `transform` without icp, reproduces the scores
    again = compare_clouds(room["est"], room["ref"], [0.02], transform=M, **kw)
    a, b = public(refined), public(again)
    a.pop("icp")
    assert a == b and again["_distances"]["estimate"].tobytes() == refined["_distances"]["estimate"].tobytes()
    # icp=None is the call without the argument
    assert public(compare_clouds(room["est"], room["ref"], [0.02], icp=None, **kw)) == public(plain)


def test_compare_clouds_refines_on_top_of_a_transform(rooms):
    """A coarse `transform` first (as the trajectory pair would give), the estimate's normals in the estimate's own
    frame: the refinement must rotate them by the transform AND its own increments."""
    from pi3_slam_amd.map_eval import compare_clouds, tau_key
    room = rooms[1.02]
    coarse = iref.increment(np.array([0.0, 0.0, np.deg2rad(-40.0), 0.0, 0.0, 0.0, 0.0]), np.zeros(3))
    spun = room["est"].astype(np.float64) @ coarse[:3, :3]                             # coarse^-1 est
    spun_n = room["est_normals"].astype(np.float64) @ coarse[:3, :3]
    res = compare_clouds(spun.astype(np.float32), room["ref"], [0.02], max_dist=0.25, transform=coarse, device=DEV,
                         icp=dict(mode="plane", est_normals=spun_n.astype(np.float32), with_scale=True))
    err = iref.alignment_error(np.array(res["settings"]["transform"]) @ np.linalg.inv(coarse), room["truth"])
    print(res["icp"]["status"], res["icp"]["iterations"], err)
    oracle = cpu.oracle_run("plane", 1.02, True)
    assert res["icp"]["status"] == "converged"
    assert err["rotation_deg"] <= 2.0 * oracle["error"]["rotation_deg"] + cpu.DEVICE_SLACK[0] + 1e-4   # + the fp32 detour
    assert err["centre_m"] <= 2.0 * oracle["error"]["centre_m"] + cpu.DEVICE_SLACK[1] + 1e-5
    np.testing.assert_allclose(np.array(res["icp"]["increment"]) @ coarse, np.array(res["icp"]["transform"]), atol=1e-12)
