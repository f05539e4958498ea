"""CPU: the host side of the ICP refinement of evaluate-map (map_eval.icp_refine's increment, the PLY reader with
normals, the command line, the table's line), the entry point's argument checks (they return before anything touches a
GPU), and the oracle (tests/cloud_icp_ref.py): its Jacobian against finite differences and what its own ICP reaches on
the planted room, which is where the GPU tests take their bounds from."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import cloud_icp_ref as iref            # noqa: E402

# what the oracle's ICP must reach on the planted room (degrees, metres); the GPU tests allow the device twice the
# oracle's own error plus DEVICE_SLACK
ORACLE_LIMITS = {"plane": (0.02, 0.2e-3), "point": (0.1, 1.0e-3)}
ORACLE_ITERATIONS = {"plane": 30, "point": 40}
DEVICE_SLACK = (0.001, 0.01e-3)
MAX_DIST = 0.25
_oracle_runs = {}


def oracle_run(mode, scale, source_normals=False):
    """The oracle's ICP on the planted room, computed once per variant and shared (never modified by a test)."""
    key = (mode, scale, source_normals)
    if key not in _oracle_runs:
        room = iref.planted_room(scale=scale)
        kw = {}
        if mode == "plane":
            kw = dict(est_normals=room["est_normals"]) if source_normals else dict(ref_normals=room["ref_normals"])
        res = iref.icp(room["est"], room["ref"], mode, with_scale=scale != 1.0, max_dist=MAX_DIST,
                       iterations=ORACLE_ITERATIONS[mode], **kw)
        res["error"] = iref.alignment_error(res["transform"], room["truth"])
        _oracle_runs[key] = res
    return _oracle_runs[key]


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_jacobian_is_the_derivative_of_the_motion():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 3))
    J = iref.jacobians(x)
    h = 1e-6
    for a in range(7):
        step = np.zeros(7)
        step[a] = h
        moved = np.exp(step[3]) * x @ Rotation.from_rotvec(step[:3]).as_matrix().T + step[4:]
        np.testing.assert_allclose((moved - x) / h, J[:, :, a], atol=5e-6)
    # and the increment is that motion about the centre
    c = np.array([0.3, -2.0, 1.0])
    D = iref.increment(np.array([0.01, -0.02, 0.03, 0.05, 0.1, 0.2, -0.3]), c)
    p = rng.standard_normal((4, 3)) + c
    lin = p + np.cross([0.01, -0.02, 0.03], p - c) + 0.05 * (p - c) + [0.1, 0.2, -0.3]
    np.testing.assert_allclose(p @ D[:3, :3].T + D[:3, 3], lin, atol=5e-3)


def test_oracle_majorant_and_counters():
    rng = np.random.default_rng(4)
    pts = rng.random((50, 3)).astype(np.float32)
    q = (pts[:40] + 0.01 * rng.standard_normal((40, 3))).astype(np.float32)
    idx = np.arange(40)
    idx[:3] = -1
    idx[3] = 50
    d2 = np.full(40, 1e-4)
    d2[4:6] = 1.0
    nrm = rng.standard_normal((50, 3)).astype(np.float32)
    nrm[7], nrm[8], nrm[9] = 0.0, np.nan, np.inf
    for mode, normals in ((0, None), (1, nrm), (2, nrm[:40])):
        eq = iref.pair_equations(q, pts, idx, d2, 0.1, [0.5, 0.5, 0.5], normals, mode, None)
        rej = 3 if mode else 0
        assert eq["counters"] == dict(used=34 - rej, unmatched=4, trimmed=2, normal_rejected=rej)
        assert np.all(np.abs(eq["sums"]) <= eq["majorant"] * (1 + 1e-12)) and np.isfinite(eq["sums"]).all()
        assert eq["sums"][35] <= eq["sums"][36] * (1 + 1e-12)                       # (n.e)^2 <= e.e
    assert iref.pair_equations(q, pts, np.full(40, -1), d2, 0.1, [0, 0, 0])["sums"].tolist() == [0.0] * 37


@pytest.mark.parametrize("scale", [1.0, 1.02])
@pytest.mark.parametrize("mode,source_normals", [("plane", False), ("plane", True), ("point", False)])
def test_oracle_icp_reaches_its_limits_on_the_planted_room(mode, source_normals, scale):
    """The bound of the GPU recovery tests comes from here: the oracle's ICP (numpy f64, scipy's k-d tree) on the
    committed generator and seed reaches <= 0.02 deg / 0.2 mm in plane mode and <= 0.1 deg / 1 mm in point mode, the
    latter within 40 iterations."""
    res = oracle_run(mode, scale, source_normals)
    err = res["error"]
    print(mode, "source normals" if source_normals else "", scale, res["status"], res["iterations"], err)
    deg, metres = ORACLE_LIMITS[mode]
    assert err["rotation_deg"] <= deg and err["centre_m"] <= metres
    assert res["iterations"] <= ORACLE_ITERATIONS[mode]
    if mode == "plane":
        assert res["status"] == "converged" and res["iterations"] <= 15
    if scale != 1.0:
        assert err["scale"] < 5e-4


def test_room_generator():
    room = iref.planted_room()
    assert room["ref"].shape == (20000, 3) and room["est"].shape == (10000, 3)
    assert room["ref"].dtype == room["est"].dtype == room["est_normals"].dtype == np.float32
    lo, hi = -iref.ROOM / 2, iref.ROOM / 2
    ref, n = room["ref"].astype(np.float64), room["ref_normals"].astype(np.float64)
    assert np.all(ref >= lo - 1e-6) and np.all(ref <= hi + 1e-6)
    assert np.all(np.abs(n).sum(1) == 1.0)                                          # axis-aligned unit normals
    inward = ref + 0.01 * n                                                         # a step along the normal stays inside
    assert np.all(inward > lo) and np.all(inward < hi)
    cab = lo + iref.CABINET
    assert not np.any(np.all(inward < cab, axis=1))                                 # ... and outside the cabinet
    on_cabinet = np.any(np.isclose(ref, cab) & (n > 0), axis=1) & np.all(ref <= cab + 1e-6, axis=1)
    assert 300 < on_cabinet.sum() < 2000                                            # 3.4 m^2 of 58 m^2
    # the estimate is the unmoved sample taken back through the truth
    T = room["truth"]
    back = room["est"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    np.testing.assert_allclose(back, room["est_unmoved"], atol=2e-6)
    nb = room["est_normals"].astype(np.float64) @ T[:3, :3].T
    assert np.allclose(np.abs(nb).max(1), 1.0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ the increment
def test_increment_composition():
    from pi3_slam_amd.map_eval import sim3_increment, unpack_equations
    c = np.array([1.5, -0.25, 9000.0])
    assert np.array_equal(sim3_increment(np.zeros(7), c), np.eye(4))
    assert np.array_equal(sim3_increment(-np.zeros(7), c), np.eye(4))
    rng = np.random.default_rng(1)
    for _ in range(5):
        x = rng.standard_normal(7) * [0.3, 0.3, 0.3, 0.1, 1, 1, 1]
        D = sim3_increment(x, c)
        np.testing.assert_allclose(D[:3, :3] @ c + D[:3, 3], c + x[4:], rtol=0, atol=1e-11)     # centre -> centre + t
        assert np.linalg.det(D[:3, :3]) == pytest.approx(np.exp(3 * x[3]), rel=1e-12)
        R = D[:3, :3] / np.exp(x[3])
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
        np.testing.assert_allclose(D, iref.increment(x, c), atol=1e-11)                         # scipy's exponential
        assert D[3].tolist() == [0, 0, 0, 1]
    A, b, r2, ee = unpack_equations(np.arange(40.0))
    assert np.array_equal(A, A.T) and A[0].tolist() == [0, 1, 2, 3, 4, 5, 6] and A[1, 1:].tolist() == [7, 8, 9, 10, 11, 12]
    assert A[6, 6] == 27 and b.tolist() == list(range(28, 35)) and (r2, ee) == (35.0, 36.0)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_errors_return_before_any_launch(built_lib):
    """Bad arguments come back with an error code and a message and touch no pointer (these are not device pointers)."""
    from pi3_slam_amd import lib as L
    from pi3_slam_amd import ops
    lib = L.load(require_gpu=False)
    centre, rn = (C.c_double * 3)(0, 0, 0), (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    inf, nan = float("inf"), float("nan")

    def call(m=100, n=50, trim=0.1, mode=0, rows=1, centre_=centre, rn_=None, **null):
        a = dict(queries=64, points=64, idx=64, d2=64, normals=64, partials=64, out=64, counters=64)
        a.update({k: None for k in null})
        return lib.pi3_cloud_pair_equations(a["queries"], m, a["points"], n, a["idx"], a["d2"], trim,
                                            None if centre_ is None else C.cast(centre_, C.c_void_p), a["normals"], mode,
                                            None if rn_ is None else C.cast(rn_, C.c_void_p), a["partials"], rows, a["out"],
                                            a["counters"], None)

    bad = [dict(m=-1), dict(n=-1), dict(n=1 << 31), dict(mode=-1), dict(mode=3), dict(trim=-0.1), dict(trim=inf),
           dict(trim=nan), dict(rows=-1), dict(centre_=None), dict(centre_=(C.c_double * 3)(0, nan, 0)),
           dict(centre_=(C.c_double * 3)(inf, 0, 0)), dict(queries=1), dict(points=1), dict(idx=1), dict(d2=1),
           dict(partials=1), dict(out=1), dict(counters=1), dict(mode=1, normals=1), dict(mode=2, normals=1),
           dict(mode=2, rn_=(C.c_double * 9)(1, 0, 0, 0, nan, 0, 0, 0, 1))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"pi3_cloud_pair_equations" in lib.pi3_last_error()
    # the workspace: one row per span of queries
    assert ops.CLOUD_ICP_SPAN == iref.SPAN
    assert [ops.cloud_icp_partial_rows(m) for m in (0, 1, iref.SPAN, iref.SPAN + 1, 3 * iref.SPAN + 5)] == [0, 1, 1, 2, 4]
    for m in (1, iref.SPAN, iref.SPAN + 1, 3 * iref.SPAN + 5):
        assert call(m=m, rows=ops.cloud_icp_partial_rows(m) - 1) == -3, m
        assert b"rows" in lib.pi3_last_error()
    assert call(mode=2, rn_=rn, m=iref.SPAN + 1, rows=1) == -3            # a good Rn passes the argument check


# ------------------------------------------------------------------------------------------------ PLY with normals
def _write_ply(path, pts, colors=None, normals=None, ascii_=False, double=False):
    props, cols = [], []
    ft = "double" if double else "float"
    for k, a in enumerate("xyz"):
        props.append((a, ft))
        cols.append(pts[:, k])
    if normals is not None:
        for k, a in enumerate(("nx", "ny", "nz")):
            props.append((a, ft))
            cols.append(normals[:, k])
    if colors is not None:
        for k, a in enumerate(("red", "green", "blue")):
            props.append((a, "uchar"))
            cols.append(colors[:, k])
    head = "ply\nformat " + ("ascii" if ascii_ else "binary_little_endian") + f" 1.0\nelement vertex {len(pts)}\n"
    head += "".join(f"property {t} {a}\n" for a, t in props) + "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if ascii_:
            for i in range(len(pts)):
                f.write((" ".join(repr(float(c[i])) if t != "uchar" else str(int(c[i])) for c, (_, t) in zip(cols, props))
                         + "\n").encode())
        else:
            dt = np.dtype([(a, {"float": "<f4", "double": "<f8", "uchar": "u1"}[t]) for a, t in props])
            rec = np.zeros(len(pts), dt)
            for c, (a, _) in zip(cols, props):
                rec[a] = c
            f.write(rec.tobytes())


@pytest.mark.parametrize("ascii_", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("double", [False, True])
def test_read_ply_vertices_round_trip(tmp_path, ascii_, with_normals, double):
    from pi3_slam_amd.map_eval import read_ply_points, read_ply_vertices
    rng = np.random.default_rng(8)
    pts = rng.standard_normal((37, 3)).astype(np.float32)
    nrm = rng.standard_normal((37, 3)).astype(np.float32) if with_normals else None
    col = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    path = str(tmp_path / "cloud.ply")
    _write_ply(path, pts, col, nrm, ascii_, double)
    v = read_ply_vertices(path)
    assert sorted(v) == ["colors", "normals", "points"]
    assert v["points"].dtype == np.float32 and v["points"].tobytes() == pts.tobytes()
    assert v["colors"].tobytes() == col.tobytes()
    if with_normals:
        assert v["normals"].dtype == np.float32 and v["normals"].tobytes() == nrm.tobytes()
    else:
        assert v["normals"] is None
    p2, c2 = read_ply_points(path)                                  # unchanged: the same two arrays
    assert p2.tobytes() == pts.tobytes() and c2.tobytes() == col.tobytes()
    _write_ply(path, pts, None, nrm, ascii_, double)
    assert read_ply_vertices(path)["colors"] is None and read_ply_points(path)[1] is None


def test_read_ply_vertices_reads_what_the_exporter_writes(tmp_path):
    """dense_points.ply with nx ny nz (export.write_ply_normals) comes back with them; without (write_ply), None."""
    from pi3_slam_amd import export
    from pi3_slam_amd.map_eval import read_ply_vertices
    rng = np.random.default_rng(9)
    pts, col = rng.standard_normal((20, 3)).astype(np.float32), rng.integers(0, 256, (20, 3)).astype(np.uint8)
    nrm = rng.standard_normal((20, 3)).astype(np.float32)
    path = str(tmp_path / "dense_points.ply")
    export.write_ply_normals(pts, nrm, col, path)
    v = read_ply_vertices(path)
    assert v["points"].tobytes() == pts.tobytes() and v["normals"].tobytes() == nrm.tobytes()
    assert v["colors"].tobytes() == col.tobytes()
    export.write_ply(pts, col, path)
    assert read_ply_vertices(path)["normals"] is None


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["evaluate-map", "--estimate", "e.ply", "--reference", "r.ply", "--thresholds", "0.02"]


def test_cli_parses_the_icp_flags():
    from pi3_slam_amd import cli
    a = cli.build_parser().parse_args(BASE)
    assert (a.icp, a.icp_scale, a.icp_iterations, a.icp_max_dist, a.save_transform) == (None, False, 30, None, None)
    a = cli.build_parser().parse_args(BASE + ["--icp", "plane", "--icp-scale", "--icp-iterations", "12", "--icp-max-dist",
                                              "0.3", "--save-transform", "T.txt"])
    assert (a.icp, a.icp_scale, a.icp_iterations, a.icp_max_dist, a.save_transform) == ("plane", True, 12, 0.3, "T.txt")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(BASE + ["--icp", "surface"])
    pts = np.zeros((4, 3), np.float32)
    bare, normal = dict(points=pts, colors=None, normals=None), dict(points=pts, colors=None, normals=pts + 1)
    assert cli.evaluate_map_icp(cli.build_parser().parse_args(BASE), bare, bare) is None
    a = cli.build_parser().parse_args(BASE + ["--icp", "point", "--icp-max-dist", "0.3"])
    assert cli.evaluate_map_icp(a, normal, normal) == dict(mode="point", with_scale=False, iterations=30, max_dist=0.3)
    a = cli.build_parser().parse_args(BASE + ["--icp", "plane", "--icp-scale"])
    got = cli.evaluate_map_icp(a, normal, bare)                     # no normals in the reference: the estimate's
    assert got["est_normals"] is normal["normals"] and "ref_normals" not in got and got["with_scale"] is True
    got = cli.evaluate_map_icp(a, normal, normal)                   # both: the reference's
    assert got["ref_normals"] is normal["normals"] and "est_normals" not in got
    with pytest.raises(SystemExit, match="nx ny nz"):
        cli.evaluate_map_icp(a, bare, bare)
    with pytest.raises(SystemExit, match="--icp-scale needs --icp"):
        cli.evaluate_map_icp(cli.build_parser().parse_args(BASE + ["--icp-scale"]), bare, bare)


def test_cli_refuses_icp_scale_without_icp_before_reading_anything():
    from pi3_slam_amd import cli
    with pytest.raises(SystemExit, match="--icp-scale needs --icp"):
        cli.main(BASE + ["--icp-scale"])                            # e.ply does not exist: the refusal comes first


def _fake_result(transform):
    k = repr(0.02)
    st = dict(points=3, matched=3, beyond=0, mean=0.0, median=0.0, rmse=0.0, p90=0.0, max=0.0, within={k: 1.0})
    return {"points": dict(estimate=3, reference=3, estimate_used=3, reference_used=3), "dropped": dict(estimate=0, reference=0),
            "accuracy": st, "completeness": st, "precision": {k: 1.0}, "recall": {k: 1.0}, "fscore": {k: 1.0}, "search": {},
            "settings": dict(thresholds=[0.02], max_dist=0.04, voxel_size=None, transform=transform, cell=0.05)}


@pytest.mark.parametrize("given", [False, True])
def test_cli_save_transform_without_icp_writes_the_input_transform(tmp_path, monkeypatch, capsys, given):
    """--save-transform is allowed without --icp: it writes the matrix that was applied (the identity without one), in
    the form --transform reads, digit for digit.  The search itself is stubbed: this is about the command line."""
    from pi3_slam_amd import cli, map_eval
    rng = np.random.default_rng(2)
    M = np.eye(4)
    M[:3] = rng.standard_normal((3, 4)) / 3.0
    src, out = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    np.savetxt(src, M, fmt="%.17g")
    seen = {}

    def fake_compare(est, ref, thresholds, **kw):
        seen.update(kw)
        t = kw.get("transform")
        return _fake_result(None if t is None else [[float(x) for x in row] for row in np.asarray(t)])

    pts = np.zeros((3, 3), np.float32)
    monkeypatch.setattr(map_eval, "read_ply_vertices", lambda path: dict(points=pts, colors=None, normals=None))
    monkeypatch.setattr(map_eval, "compare_clouds", fake_compare)
    cli.main(BASE + ["--save-transform", out] + (["--transform", src] if given else []))
    assert "icp" not in seen                                        # without --icp the call is the one it was
    assert np.array_equal(map_eval.read_transform(out), M if given else np.eye(4))
    assert "fscore" in capsys.readouterr().out


def test_write_transform_reads_back_to_the_same_doubles(tmp_path):
    from pi3_slam_amd.map_eval import read_transform, write_transform
    rng = np.random.default_rng(6)
    M = rng.standard_normal((4, 4)) * np.array([1e-9, 1.0, 1e5, 1e12])
    path = str(tmp_path / "T.txt")
    write_transform(path, M)
    assert read_transform(path).tobytes() == M.tobytes()
    assert len(open(path).read().split()) == 16 and len(open(path).read().strip().splitlines()) == 4


# ------------------------------------------------------------------------------------------------ the table
def test_table_gains_one_line_when_icp_ran():
    from pi3_slam_amd.map_eval import format_icp_line, format_table
    res = _fake_result(None)
    plain = format_table(res)
    assert "icp" not in plain
    hist = [dict(pairs=900, counters={}, rms=0.0312, point_rms=0.05, step=0.1),
            dict(pairs=950, counters={}, rms=0.00021, point_rms=0.03, step=1e-8)]
    res["icp"] = dict(status="converged", iterations=2, history=hist, transform=np.eye(4).tolist(), increment=np.eye(4).tolist())
    table = format_table(res)
    assert table.startswith(plain) and table[len(plain):] == "\n\n" + format_icp_line(res["icp"])
    assert table.splitlines()[-1] == "icp: converged after 2 iterations, 950 pairs, rms 0.03120 -> 0.00021"
    few = dict(status="too_few_pairs", iterations=1, history=[dict(pairs=0, counters={}, rms=None, point_rms=None, step=None)])
    assert format_icp_line(few) == "icp: too_few_pairs after 1 iterations, 0 pairs, rms - -> -"


def test_icp_refine_refuses_plane_mode_without_normals_and_unknown_modes():
    """Raised before anything is sent to a device."""
    from pi3_slam_amd.map_eval import icp_refine
    pts = np.zeros((20, 3), np.float32)
    with pytest.raises(ValueError, match="normals"):
        icp_refine(pts, pts, mode="plane", max_dist=0.1)
    with pytest.raises(ValueError, match="mode"):
        icp_refine(pts, pts, mode="surface", max_dist=0.1)
