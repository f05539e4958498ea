"""Views through a camera on the CPU: the oracle's frustum rule against fractions.Fraction, its invariances,
view_planner.view_frames and the poses, the planner's and the command line's validation, and the argument checks of the
built library's _frustum entry points (no GPU: a refused call launches nothing).

Why int64 holds the rule (grid_view_frustum_ref.py states it, csrc/grid_view_ray.h's view_frames_ok likewise): with
|o|^2 <= 2^12, |f|^2 and |r|^2 <= 12288 and every fraction term <= 2^20, each side of each test is at most 2^12 * 12288 *
12288 * 2^20 = 2.25 * 2^58 < 2^63.  test_the_64_bit_bound evaluates the figure and reaches it with a frame and an offset
at the bounds."""
import ctypes
import itertools
import json
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grid_view_frustum_ref as fref        # noqa: E402
import grid_view_ref as vref                # noqa: E402

BIG = 1 << 20
FRAMES = [(1, 0, 0, 0, 1, 0), (0, 0, -1, 1, 0, 0), (1, 1, 0, 1, -1, 0), (1, 2, 2, 2, 1, -2), (3, -4, 12, 4, 3, 0),
          (64, 64, 64, 64, -64, 0), (0, 37, 64, 64, 0, 0), (-16, 13, 16, 16, 0, 16)]
FRACTIONS = [(0, 1), (1, 1), (BIG, 1), (1, BIG), (1829, 4096), (3, 7)]


def _brute(offs, frame, th, tv):
    """The rule in rationals: o.f > 0, tan^2 of the angle to either side <= the fraction."""
    f, r = frame[:3], frame[3:]
    u = (f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0])
    f2, r2 = sum(c * c for c in f), sum(c * c for c in r)
    out = []
    for o in offs.tolist():
        df, dr, du = (sum(a * b for a, b in zip(o, v)) for v in (f, r, u))
        if df <= 0:
            out.append(False)
            continue
        # tan^2 of the horizontal angle is (o.r / |r|)^2 / (o.f / |f|)^2, of the vertical one (o.u / |u|)^2 / (same)
        tan2_h = Fraction(dr * dr * f2, df * df * r2)
        tan2_v = Fraction(du * du * f2, df * df * f2 * r2)
        out.append(tan2_h <= Fraction(*th) and tan2_v <= Fraction(*tv))
    return np.array(out, bool)


def test_the_rule_against_fractions():
    ball = vref.ball_offsets(6)
    inside = 0
    for frame in FRAMES:
        assert fref.frame_ok(frame)
        for th, tv in itertools.product(FRACTIONS, FRACTIONS):
            got = fref.in_frustum(ball, frame, th, tv)
            assert got.tobytes() == _brute(ball, frame, th, tv).tobytes(), (frame, th, tv)
            inside += int(got.sum())
    assert inside > 10000
    # a fraction of 0 leaves the plane through f, both of them the ray along f
    assert fref.in_frustum(ball, FRAMES[0], (0, 1), (0, 1)).sum() == 6
    assert fref.in_frustum(ball, FRAMES[0], (0, 1), (BIG, 1)).sum() > 6
    # 2^20 / 1 on both sides is the open half space up to the last cell's slope: o.f > 0 within the ball of 64
    far = vref.ball_offsets(8)
    for frame in FRAMES[:5]:
        assert (fref.in_frustum(far, frame, (BIG, 1), (BIG, 1)) == (far @ np.array(frame[:3]) > 0)).all()


def test_the_64_bit_bound():
    bound = (1 << 12) * 12288 * 12288 * (1 << 20)
    assert bound == 9 * (1 << 56) and bound < (1 << 63)         # 2.25 * 2^58
    frame, o = (64, 64, 64, 64, -64, 0), np.array([[36, 37, 37], [45, -45, 0], [-26, -26, 52]], np.int64)
    f, r = np.array(frame[:3]), np.array(frame[3:])
    u = fref.cross(f, r)
    assert int(np.abs(u).max()) <= 8192 and int(u @ u) == int(f @ f) * int(r @ r) == 12288 * 8192
    assert max(int((x * x).sum()) for x in o) <= 64 * 64
    for th, tv in (((BIG, 1), (BIG, 1)), ((1, BIG), (1, BIG)), ((BIG, BIG), (0, BIG))):
        assert fref.in_frustum(o, frame, th, tv).tobytes() == _brute(o, frame, th, tv).tobytes()
    # the largest terms themselves, in Python integers
    most_f = max((int(x @ f) ** 2) for x in o)
    assert most_f * BIG * int(r @ r) < (1 << 63) and (64 * 64 * int(u @ u)) * BIG <= bound


def test_invariances():
    ball = vref.ball_offsets(6)
    for frame in FRAMES:
        f, r = np.array(frame[:3]), np.array(frame[3:])
        for th, tv in (((1, 1), (1829, 4096)), ((3, 7), (BIG, 1)), ((1, BIG), (2, 3))):
            base = fref.in_frustum(ball, frame, th, tv).tobytes()
            if int(np.abs(f).max()) <= 32:
                assert fref.in_frustum(ball, np.concatenate([2 * f, r]), th, tv).tobytes() == base
            if int(np.abs(r).max()) <= 21:
                assert fref.in_frustum(ball, np.concatenate([f, 3 * r]), th, tv).tobytes() == base
            assert fref.in_frustum(ball, np.concatenate([f, -r]), th, tv).tobytes() == base
            up = fref.cross(r, f)
            up //= math.gcd(*(int(abs(c)) for c in up))
            if int(np.abs(up).max()) <= 64:                     # the camera turned a quarter: the fractions change places
                assert fref.in_frustum(ball, np.concatenate([f, up]), tv, th).tobytes() == base
    assert sum(int(np.abs(fref.cross(fr[3:], fr[:3]) // math.gcd(*(abs(int(c)) for c in fref.cross(fr[3:], fr[:3])))).max()) <= 64
               for fr in FRAMES) >= 6


def test_faces_are_inclusive():
    ball = vref.ball_offsets(6)
    got = fref.in_frustum(ball, (1, 0, 0, 0, 1, 0), (1, 1), (1, 1))
    x, y, z = ball.T
    assert (got == ((x > 0) & (np.abs(y) <= x) & (np.abs(z) <= x))).all()
    assert got[(np.abs(y) == x) & (np.abs(z) == x) & (x > 0)].all() and got.sum() > 100


# ------------------------------------------------------------------------------------------------ frames and poses
def test_view_frames():
    from pi3_slam_amd.view_planner import view_frames
    four = view_frames(4)
    assert four.dtype == np.int64 and four.tolist() == [[0, 0, 1, 1, 0, 0], [-1, 0, 0, 0, 0, 1], [0, 0, -1, -1, 0, 0],
                                                        [1, 0, 0, 0, 0, -1]]
    eight = view_frames(8)
    assert eight[:, :3].tolist() == [[0, 0, 1], [-1, 0, 1], [-1, 0, 0], [-1, 0, -1], [0, 0, -1], [1, 0, -1], [1, 0, 0],
                                     [1, 0, 1]]
    assert eight[::2].tolist() == four.tolist()
    assert view_frames(4, up=(0, 0, 1))[:, :3].tolist() == [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]]
    for args in ((8, (-30, 0, 30)), (10, (-45.0, 10.0, 60.0), (1, 0, 0)), (5, (89.0, -89.0, 0, 33.3, 7, -61), (0, 0, -1)),
                 (32, (12.5,), (0, 1, 0)), (1, (0,), (-1, 0, 0)), (4, (0,), (0, -1, 0), True)):
        fr = view_frames(*args)
        assert fr.tobytes() == view_frames(*args).tobytes() and fr.shape == (args[0] * len(args[1]), 6)
        assert all(fref.frame_ok(row) for row in fr) and int(np.abs(fr).max()) <= 64
        assert len({tuple(row[:3]) for row in fr.tolist()}) == len(fr)
        up = np.array(args[2] if len(args) > 2 else (0, -1, 0))
        err = fref.frame_error(fr, args[0], args[1], up)
        print(args, float(err.max()))
        assert float(err.max()) < 1.0
        if len(args) < 4:
            assert (fr[:, 3:] @ up == 0).all() and (fr[:, 3:] == np.cross(fr[:, :3], up)).all()     # r is horizontal
    # the rows: pitch by pitch as given, yaw ascending
    fr = view_frames(4, (30, -30))
    assert (fr[:4, 1] < 0).all() and (fr[4:, 1] > 0).all()      # pitch is towards up, and up is -y
    # portrait: right is up, the same f
    tall = view_frames(8, portrait=True)
    assert tall[:, :3].tolist() == eight[:, :3].tolist() and (tall[:, 3:] == [0, -1, 0]).all()


def test_view_frames_refusals():
    from pi3_slam_amd.view_planner import view_frames
    for pitch in (90, -90, 89.9):
        with pytest.raises(ValueError, match="looks along up"):
            view_frames(4, (0, pitch))
    with pytest.raises(ValueError, match="frames 0 and 4 look the same way"):
        view_frames(4, (10, 10))
    with pytest.raises(ValueError, match="look the same way"):
        view_frames(4, (10, 10.01))
    for n, pitches in ((33, (0,)), (8, (0, 10, 20, 30, 40)), (4, ())):
        with pytest.raises(ValueError, match=r"frames: 1 \.\. 32"):
            view_frames(n, pitches)
    for n in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="yaw_steps must be an integer >= 1"):
            view_frames(n)
    for up in ((0, 0, 0), (1, 1, 0), (0, 2, 0), (0, -1), "up", (0.5, 0, 0)):
        with pytest.raises(ValueError, match="up must be one of the six signed axes"):
            view_frames(4, up=up)
    with pytest.raises(ValueError, match="every pitch must lie in -90 .. 90"):
        view_frames(4, (120,))
    with pytest.raises(ValueError, match=r"portrait: the frame at pitch 20, yaw 1 of 7 has the right .* outside \+-64"):
        view_frames(7, (20,), portrait=True)


def test_poses_are_rotations():
    from pi3_slam_amd.view_planner import view_frames, view_pose
    for args in ((8, (-30, 0, 30)), (10, (-45.0, 10.0, 60.0), (1, 0, 0)), (4, (0,), (0, -1, 0), True)):
        for row in view_frames(*args):
            pose = view_pose(row, (1.5, -2.0, 0.25))
            Rm = pose[:3, :3]
            assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rm) - 1.0) < 1e-12
            assert pose[3].tolist() == [0, 0, 0, 1] and pose[:3, 3].tolist() == [1.5, -2.0, 0.25]
            f = row[:3] / np.linalg.norm(row[:3])
            assert np.abs(Rm[:, 2] - f).max() < 1e-15 and np.abs(Rm[:, 0] - row[3:] / np.linalg.norm(row[3:])).max() < 1e-15
    # under the default up a level view is the identity turned about y: yaw 0 is the identity itself, down stays +y
    level = [view_pose(row, (0, 0, 0))[:3, :3] for row in view_frames(8)]
    assert level[0].tolist() == np.eye(3).tolist()
    for n, Rm in enumerate(level):
        a = 2 * math.pi * n / 8
        turn = np.array([[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]])
        assert np.abs(Rm - turn).max() < 1e-12


# ------------------------------------------------------------------------------------------------ the host side
def test_planner_validation_and_settings():
    from pi3_slam_amd import ops
    from pi3_slam_amd.view_planner import ViewPlanner, view_frames, view_headings
    assert (ops.VIEW_MAX_FRAME, ops.VIEW_MAX_TAN2) == (64, 1 << 20)
    plain = ViewPlanner(0, 1.0)
    assert plain.fov_deg == 90.0 and "frustum" not in plain.settings() and plain.frames is None
    assert plain.settings() == ViewPlanner(0, 1.0, 90).settings() == ViewPlanner(0, 1.0, frustum=None, yaw_steps=3).settings()
    (hd, num, den), kw = plain.shape_args()
    assert hd.tolist() == view_headings().tolist() and (num, den) == vref.cos2(90) and kw == {}
    p = ViewPlanner(0, 1.0, frustum=(90, 67.5), pitches_deg=(-30, 0, 30), unknown_depth=2, far=True)
    st = p.settings()
    fr = st["frustum"]
    assert p.frames.tobytes() == view_frames(8, (-30, 0, 30)).tobytes() and st["unknown_depth"] == 2 and st["far"] is True
    assert fr["tan2_h"] == [4096, 4096] == list(fref.tan2(90)) and fr["tan2_v"] == list(fref.tan2(67.5)) == [1829, 4096]
    assert (fr["hfov_deg"], fr["vfov_deg"], fr["yaw_steps"], fr["pitches_deg"], fr["up"], fr["portrait"]) == (
        90.0, 67.5, 8, [-30.0, 0.0, 30.0], [0, -1, 0], False)
    assert len(fr["realised"]) == 24 and max(r["error_deg"] for r in fr["realised"]) < 1.0
    assert [round(r["yaw_deg"]) for r in fr["realised"][:8]] == [0, 45, 90, 135, 180, 225, 270, 315]
    assert all(abs(r["pitch_deg"] - q) < 0.2 for r, q in zip(fr["realised"][::8], (-30, 0, 30)))
    k = fr["intrinsics"]
    assert (k["W"], k["H"], k["cx"], k["cy"]) == (640, 428, 320.0, 214.0) and abs(k["fx"] - 320.0) < 1e-9
    assert abs(k["fy"] - 214.0 / math.tan(math.radians(67.5 / 2))) < 1e-9
    assert st["fov_deg"] is None and st["cos2_num"] is None
    assert {a: b for a, b in st.items() if a not in ("frustum", "fov_deg", "cos2_num", "cos2_den")} == {
        a: b for a, b in ViewPlanner(0, 1.0, unknown_depth=2, far=True).settings().items()
        if a not in ("fov_deg", "cos2_num", "cos2_den")}
    json.dumps(st)
    (hd, num, den), kw = p.shape_args()
    assert hd.tolist() == p.frames[:, :3].tolist() and num is None and kw["frustum"][1:] == (4096, 4096, 1829, 4096)
    # portrait: the angles change places, and so does the image
    tall = ViewPlanner(0, 1.0, frustum=(90, 67.5), portrait=True, image_width=480).settings()["frustum"]
    assert tall["tan2_h"] == [1829, 4096] and tall["tan2_v"] == [4096, 4096] and tall["portrait"] is True
    assert (tall["intrinsics"]["W"], tall["intrinsics"]["H"]) == (480, round(480 / math.tan(math.radians(67.5 / 2))))
    # the largest fraction stays inside 2^20
    assert fref.tan2(170)[0] == 535126 < (1 << 20) and fref.tan2(2)[0] == 1
    for bad, text in (((1.9, 60), "must lie in"), ((90, 170.5), "must lie in"), ((90,), "must be"), ("wide", "must be"),
                      (90, "must be"), ((90, float("nan")), "must lie in")):
        with pytest.raises(ValueError, match=f"frustum {text}|angle of the frustum {text}"):
            ViewPlanner(0, 1.0, frustum=bad)
    with pytest.raises(ValueError, match="a frustum has its own two angles: leave fov_deg out"):
        ViewPlanner(0, 1.0, 90, frustum=(90, 60))
    for kw, text in ((dict(yaw_steps=33), r"frames: 1 \.\. 32"), (dict(pitches_deg=(90,)), "looks along up"),
                     (dict(up=(0, 1, 1)), "six signed axes"), (dict(portrait=1), "portrait must be True or False"),
                     (dict(image_width=0), "image_width must be an integer >= 1")):
        with pytest.raises(ValueError, match=text):
            ViewPlanner(0, 1.0, frustum=(90, 60), **kw)


def test_flags_parse_and_the_help_says_what_they_are():
    from pi3_slam_amd import cli
    base = ["views", "--occupancy", "o.npz", "--output", "d", "--start", "1", "2", "3"]
    a = cli.build_parser().parse_args(base)
    assert a.frustum is None and a.fov == 90.0 and not hasattr(a, "fov_given") and (a.yaw_steps, a.pitch, a.up, a.portrait, a.view_image_width) == (
        8, [0.0], [0, -1, 0], False, 640)
    a = cli.build_parser().parse_args(base + ["--frustum", "90", "67.5", "--yaw-steps", "8", "--pitch", "-30", "0", "30",
                                              "--up", "0", "0", "1", "--portrait", "--view-image-width", "320", "--far",
                                              "--unknown-depth", "2", "--cover", "--tour", "--taut"])
    assert a.frustum == [90.0, 67.5] and a.pitch == [-30.0, 0.0, 30.0] and a.up == [0, 0, 1] and a.portrait
    assert a.view_image_width == 320 and a.far and a.unknown_depth == 2 and a.cover and a.tour and a.taut
    text = " ".join(cli.build_parser()._subparsers._group_actions[0].choices["views"].format_help().split())
    assert "--frustum HFOV VFOV" in text and "A convention, not a measurement" in text and "--view-image-width W" in text
    assert "[--frustum HFOV VFOV [--yaw-steps 8] [--pitch DEG ...] [--up 0 -1 0] [--portrait]" in cli.__doc__
    for other in ("route", "frontiers"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args([other, "--frustum", "90", "60"])


def test_ops_refuses_frames_it_cannot_pass():
    from pi3_slam_amd import ops
    for frames in (np.zeros((0, 6)), np.zeros((33, 6)), np.zeros((2, 3)), [[65, 0, 0, 0, 1, 0]]):
        with pytest.raises(AssertionError):
            ops._view_frustum(ops.ViewFrustum(frames, 1, 1, 1, 1), None, 8, False)
    flat, H, form, shape = ops._view_frustum(ops.ViewFrustum([[1, 0, 0, 0, 1, 0]] * 2, 1, 2, 3, 4), None, 33, False)
    assert list(flat) == [1, 0, 0, 0, 1, 0] * 2 and H == 2 and form == (-1, 1) and shape == (1, 2, 3, 4)
    assert ops._view_frustum(ops.ViewFrustum([[1, 0, 0, 0, 1, 0]], 1, 2, 3, 4), 7, 8, False)[2] == (7, 0)


def test_signatures_and_header_agree():
    from pi3_slam_amd import lib
    text = open(os.path.join(ROOT, "include", "pi3slam_hip.h")).read()
    for name, base in (("pi3_grid_view_gain_frustum", "pi3_grid_view_gain_depth"),
                       ("pi3_grid_view_mark_frustum", "pi3_grid_view_mark_depth")):
        args = [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % name, text).group(1).split(",")]
        old = [a.split()[-1].lstrip("*") for a in re.search(r"int %s\(([^;]*)\);" % base, text).group(1).split(",")]
        assert len(args) == len(lib.SIGNATURES[name]) == len(old) + 2
        at = args.index("frames")
        assert args[at:at + 6] == ["frames", "H", "tan2_h_num", "tan2_h_den", "tan2_v_num", "tan2_v_den"]
        assert args[:at] == old[:at] and args[at + 6:] == old[at + 4:] and old[at:at + 4] == ["headings", "H", "cos2_num",
                                                                                              "cos2_den"]
        sig, was = lib.SIGNATURES[name], lib.SIGNATURES[base]
        assert sig[:at + 2] == was[:at + 2] and sig[at + 2:at + 6] == [ctypes.c_long] * 4 and sig[at + 6:] == was[at + 4:]


def test_the_library_has_the_symbols_and_refuses_bad_arguments_without_a_gpu():
    from pi3_slam_amd import lib as L
    lib = L.load(require_gpu=False)
    assert lib.pi3_abi_version() == 7
    G, M = lib.pi3_grid_view_gain_frustum, lib.pi3_grid_view_mark_frustum
    # never dereferenced: a refused call returns before anything is launched or read on the host side but the frames
    p = 4096
    ints = lambda *a: (ctypes.c_int * len(a))(*a)               # noqa: E731
    good, two = ints(1, 0, 0, 0, 1, 0, 0, 37, 64, 64, 0, 0), ints(0, -1)
    gain = lambda **k: G(k.get("state", p), 5, 4, 3, k.get("seen", None), p, 2, k.get("range", 4), k.get("depth", -1),  # noqa: E731
                         k.get("far", 0), k.get("frames", good), k.get("H", 2), *k.get("tan2", (1, 1, 1829, 4096)), p, p,
                         p, k.get("counters", p), None)
    mark = lambda **k: M(k.get("state", p), 5, 4, 3, k.get("seen", p), p, k.get("rows", two), 2, k.get("range", 4),  # noqa: E731
                         k.get("depth", -1), k.get("far", 0), k.get("frames", good), k.get("H", 2),
                         *k.get("tan2", (1, 1, 1829, 4096)), None, k.get("tag", 0), k.get("counters", p), None)
    big = 1 << 20
    cases = [dict(state=None), dict(counters=None), dict(frames=None), dict(depth=-2), dict(depth=256), dict(range=0),
             dict(range=33, far=0), dict(range=65, far=1), dict(H=0), dict(H=33),
             dict(frames=ints(1, 0, 0, 1, 1, 0, 0, 37, 64, 64, 0, 0)),          # f.r != 0
             dict(frames=ints(1, 0, 0, 0, 1, 0, 0, 0, 0, 64, 0, 0)),            # a zero f
             dict(frames=ints(1, 0, 0, 0, 1, 0, 0, 37, 64, 0, 0, 0)),           # a zero r
             dict(frames=ints(65, 0, 0, 0, 1, 0, 0, 37, 64, 64, 0, 0)),         # a component of f outside +-64
             dict(frames=ints(1, 0, 0, 0, -65, 0, 0, 37, 64, 64, 0, 0)),        # of r
             dict(tan2=(-1, 1, 1, 1)), dict(tan2=(big + 1, 1, 1, 1)), dict(tan2=(1, 0, 1, 1)), dict(tan2=(1, big + 1, 1, 1)),
             dict(tan2=(1, 1, -1, 1)), dict(tan2=(1, 1, big + 1, 1)), dict(tan2=(1, 1, 1, 0)), dict(tan2=(1, 1, 1, big + 1))]
    for call, name in ((gain, b"pi3_grid_view_gain_frustum:"), (mark, b"pi3_grid_view_mark_frustum:")):
        for case in cases:
            assert call(**case) == -1, case
            err = lib.pi3_last_error()
            assert err.startswith(name), (case, err)
            assert (b" depth=%d (-1: transparent, else 0 .. 255)" % case.get("depth", -1)) in err, (case, err)
            assert (b"range=%d (1 .. %d)" % (case.get("range", 4), 64 if case.get("far") else 32)) in err, (case, err)
            assert (b"H=%d (1 .. 32; every frame f then r: both non-zero, f.r = 0, components within +-64"
                    % case.get("H", 2)) in err, (case, err)
            t = case.get("tan2", (1, 1, 1829, 4096))
            assert (b"tan2_h=%d/%d tan2_v=%d/%d (0 <= num <= 2^20, 1 <= den <= 2^20)" % t) in err, (case, err)
            assert b"null pointer" in err and b"cos2" not in err and b"2^63" not in err, (case, err)
    assert mark(seen=None) == -1 and mark(tag=32768) == -1 and b"tag=32768 (0 .. 32767)" in lib.pi3_last_error()
    assert mark(rows=ints(0, 2)) == -1 and b"every row's heading in -1 .. H - 1" in lib.pi3_last_error()
    assert mark(rows=ints(-2, 0)) == -1
    # the fractions at their bounds and both forms of the depth pass the checks: V = 0 would launch nothing, but zeroing
    # the counters needs a device, so only the refusals are exercised here
