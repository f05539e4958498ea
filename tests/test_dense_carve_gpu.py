"""Carving the fused dense map with depth keyframes on the GPU, byte for byte against the numpy oracles: the depth planes
(csrc/dense_filter.hip: pi3_dense_depth_planes, tests/dense_carve_ref.py), the carve kernel (csrc/voxel_carve.hip), the
cleaner with excluded voxels (csrc/voxel_clean.hip: pi3_voxel_support_excluding, tests/dense_clean_ref.py), and creator
-> reconstruct on the chess-room sequence with a planted floater."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dense_carve_ref as ref           # noqa: E402
import dense_clean_ref as clean_ref     # noqa: E402
import dense_consistency_ref as cref    # noqa: E402
import dense_map_ref as mref            # noqa: E402
import test_dense_carve as cpu          # noqa: E402  (the scenes and the gauged chunks of the CPU tests)
import test_dense_clean_gpu as clean_gpu               # noqa: E402  (the random boxes of the cleaning tests)
import test_dense_consistency_gpu as cons_gpu          # noqa: E402  (the damaged scenes, the creator helpers)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = cons_gpu.THR
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
REL_TOL = 0.03


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. depth planes
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("shape", [(1, 8, 8), (5, 24, 40), (16, 77, 101)], ids=lambda s: "%dx%dx%d" % s)
def test_depth_planes_match_oracle_byte_for_byte(shape, stride, every):
    from pi3_slam_amd import ops
    s = cons_gpu.damaged_scene(*shape)
    thr = mref.conf_logit(THR)
    N, H, W = shape
    for conf, masks in ((s["conf"], s["masks"]), (None, None)):
        exp, n = ref.depth_planes(s["points"], s["local_points"], conf, masks, thr, every, stride)
        out = torch.full((exp.size + 7,), 9.0, dtype=torch.float16, device=DEV)          # a larger buffer: a view of it
        got, cnt = ops.dense_depth_planes(_dev(s["points"]), _dev(s["local_points"]), _dev(conf), _dev(masks), float(thr),
                                          every, stride, out=out)
        again, cnt2 = ops.dense_depth_planes(_dev(s["points"]), _dev(s["local_points"]), _dev(conf), _dev(masks),
                                             float(thr), every, stride)
        print(f"{shape} S={stride} K={every} conf/masks {'on' if conf is not None else 'off'}: planes {exp.shape}, "
              f"{n} of {exp.size} samples non-zero; kernel {int(cnt)}")
        assert tuple(got.shape) == exp.shape == (-(-N // every), -(-H // stride), -(-W // stride))
        assert got.dtype == torch.float16 and got.data_ptr() == out.data_ptr()
        assert got.cpu().numpy().tobytes() == exp.tobytes() == again.cpu().numpy().tobytes()
        assert int(cnt) == n == int(cnt2)
        assert bool((out[exp.size:] == 9.0).all())                                       # nothing past the planes
        if N >= 5 and conf is not None:     # the scene exercises holes and samples
            assert 0 < n < exp.size


def test_depth_planes_round_like_the_oracle_at_the_fp16_edges():
    from pi3_slam_amd import ops
    z = np.array([2049.0, 2051.0, 70000.0, 65519.0, 65520.0, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 1.0,
                  6.1e-5, 1e-3], np.float32)
    lp = np.zeros((1, 1, len(z), 3), np.float32)
    lp[..., 2] = z
    pts = np.ones_like(lp)
    exp, n = ref.depth_planes(pts, lp, None, None, 0.0, 1, 1)
    got, cnt = ops.dense_depth_planes(_dev(pts), _dev(lp), None, None, 0.0, 1, 1)
    assert got.cpu().numpy().tobytes() == exp.tobytes() and int(cnt) == n
    assert exp.astype(np.float64).reshape(-1)[:5].tolist() == [2048.0, 2052.0, 0.0, 65504.0, 0.0]


# ------------------------------------------------------------------------------------------------ 2. carve kernel
def _slots(fz):
    keys = fz.table.view(-1, 8)[:, 0].cpu().numpy().view(np.uint64)
    occ = keys != NONE
    return keys, occ, np.argsort(keys[occ])


def _carve_device(fz, views, planes, stride, margin, min_conflicts, rel_tol=REL_TOL):
    from pi3_slam_amd import ops
    cap = fz.capacity
    carved = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    agree = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    conflict = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    ops.voxel_carve(fz.table, fz.voxel_size, _dev(views), _dev(planes), stride, rel_tol, margin, min_conflicts, carved,
                    agree, conflict, counters)
    return carved.cpu().numpy(), agree.cpu().numpy().view(np.uint32), conflict.cpu().numpy().view(np.uint32), \
        counters.cpu().numpy()


def _check_carve(fz, views, planes, stride, margin, min_conflicts):
    """The kernel on the fuser's table against the oracle on its extracted rows; -> the oracle's result."""
    rows = fz.extract()
    exp = ref.carve(rows["points"], views, planes, stride, REL_TOL, margin, min_conflicts)
    keys, occ, order = _slots(fz)
    assert np.array_equal(keys[occ][order], rows["keys"].view(np.uint64))
    got = _carve_device(fz, views, planes, stride, margin, min_conflicts)
    again = _carve_device(fz, views, planes, stride, margin, min_conflicts)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    carved, agree, conflict, counters = got
    assert carved[occ][order].tobytes() == exp["carved"].astype(np.uint8).tobytes()
    assert agree[occ][order].tobytes() == exp["agree"].tobytes()
    assert conflict[occ][order].tobytes() == exp["conflict"].tobytes()
    assert not carved[~occ].any() and not agree[~occ].any() and not conflict[~occ].any()
    st = exp["stats"]
    assert counters.tolist() == [st["voxels"], st["carved"], st["unvoted"], 0]
    return exp


def _fused_scene(s, voxel, reserve=0):
    from pi3_slam_amd.dense_map import VoxelFuser
    fz = VoxelFuser(voxel, DEV)
    if reserve:
        fz.reserve(reserve)
    fz.fuse_pixels(_dev(s["points"]), None, None, None, 0.5)
    return fz


@pytest.mark.parametrize("cfg", cpu.CONFIGS, ids=lambda c: "%dx%dx%d_v%g_S%d_K%d" % c)
def test_carve_matches_oracle_byte_for_byte(cfg):
    N, H, W, voxel, S, K = cfg
    s, m, dist = cpu.floater_scene(N, H, W, voxel)
    fz = _fused_scene(s, voxel)
    views, planes = cpu.scene_views(s, S, K)
    for mc in (1, 3):
        exp = _check_carve(fz, views, planes, S, voxel, mc)
        print(f"{cfg} min_conflicts {mc}: {exp['stats']}, views {len(views)}, capacity {fz.capacity}")
        assert exp["carved"][dist > 0.5].all() and not exp["carved"][dist <= 0.5].any() and exp["stats"]["carved"] > 0
    # the same map in a nearly empty table: other slots, other probe chains, the same answer per voxel
    sparse = _fused_scene(s, voxel, reserve=16 * N * H * W)
    assert sparse.capacity >= 8 * fz.capacity
    again = _check_carve(sparse, views, planes, S, voxel, 3)
    for k in ("carved", "agree", "conflict"):
        assert again[k].tobytes() == exp[k].tobytes()
    # no views at all: nothing is carved, nobody votes
    none = _carve_device(fz, np.zeros((0, 20)), np.zeros((0,) + planes.shape[1:], np.float16), S, voxel, 1)
    assert not none[0].any() and none[3].tolist() == [len(dist), 0, len(dist), 0]


def test_carve_in_a_table_exactly_half_full():
    from pi3_slam_amd.dense_map import VoxelFuser
    N, H, W, voxel, S, K = cpu.CONFIGS[3]
    s, m, dist = cpu.floater_scene(N, H, W, voxel)
    # 8 192 of the map's voxels, the floaters among them, as points of their own: capacity 2 n, every point a new voxel
    pick = np.r_[np.flatnonzero(dist > 0.5), np.flatnonzero(dist <= 0.5)][:8192]
    pts = m["points"][pick]
    ok, keys, _ = mref.quantise(pts, mref.inv_voxel(voxel))
    assert ok.all() and len(np.unique(keys)) == 8192
    fz = VoxelFuser(voxel, DEV)
    fz.fuse_points(_dev(pts), None, None)
    _, occ, _ = _slots(fz)
    assert fz.capacity == 16384 and int(occ.sum()) == 8192
    views, planes = cpu.scene_views(s, S, K)
    exp = _check_carve(fz, views, planes, S, voxel, 2)
    assert exp["stats"]["carved"] == int((dist > 0.5).sum()) == 336


def test_two_chunks_one_in_a_scaled_gauge_through_map_carver(capsys):
    from pi3_slam_amd.dense_map import MapCarver
    N, H, W, voxel, S, K = cpu.CONFIGS[3]
    s, m, dist = cpu.floater_scene(N, H, W, voxel)
    fz = _fused_scene(s, voxel)
    chunks = [cpu._gauged_chunk(s, S, K, 1.0), cpu._gauged_chunk(s, S, K, 1.7), {"camera_poses": torch.eye(4)[None]}]
    views, planes, stride = MapCarver.chunk_views(chunks)
    M = len(range(0, N, K))
    assert len(views) == 2 * M
    carver = MapCarver(3)
    carved = carver.apply(fz, chunks, arrays=True)
    exp = ref.carve(fz.extract()["points"], views, planes.numpy(), stride, REL_TOL, MapCarver.MARGIN_VOXELS * voxel, 3)
    _, occ, order = _slots(fz)
    assert carved.cpu().numpy()[occ][order].tobytes() == exp["carved"].astype(np.uint8).tobytes()
    for k in ("agree", "conflict"):
        assert carver.last_arrays[k].cpu().numpy().view(np.uint32)[occ][order].tobytes() == exp[k].tobytes()
    assert carver.last_stats == dict(views=2 * M, **exp["stats"])
    assert exp["carved"][dist > 0.5].all() and not exp["carved"][dist <= 0.5].any()
    # both chunks vote: twice the votes of one chunk alone, up to the fp16 rounding of the scaled planes
    one = ref.carve(fz.extract()["points"], views[:M], planes.numpy()[:M], stride, REL_TOL, voxel, 3)
    assert exp["conflict"].sum() > 1.9 * one["conflict"].sum() and exp["agree"].sum() > 1.9 * one["agree"].sum()
    plain = MapCarver(3)
    assert torch.equal(plain.apply(fz, chunks), carved) and plain.last_arrays is None
    assert plain.last_stats == carver.last_stats
    # no planes: one notice, nothing carved
    capsys.readouterr()
    assert MapCarver(3).apply(fz, [chunks[2]]) is None
    assert capsys.readouterr().out.count("No depth keyframes") == 1


def test_carve_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    N, H, W, voxel, S, K = cpu.CONFIGS[5]
    s, m, dist = cpu.floater_scene(N, H, W, voxel)
    fz = _fused_scene(s, voxel)
    views, planes = cpu.scene_views(s, S, K)
    v, p = _dev(views), _dev(planes)
    cap = fz.capacity
    carved = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    counters = torch.full((4,), 11, dtype=torch.int64, device=DEV)
    inf, nan = float("inf"), float("nan")

    def call(capacity=cap, vsize=voxel, M=len(views), Hp=planes.shape[1], Wp=planes.shape[2], stride=S, tol=0.03,
             margin=voxel, mc=1, **null):
        a = dict(table=fz.table.data_ptr(), views=v.data_ptr(), planes=p.data_ptr(), carved=carved.data_ptr(),
                 counters=counters.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_voxel_carve(a["table"], capacity, vsize, a["views"], M, a["planes"], Hp, Wp, stride, tol, margin, mc,
                                   a["carved"], None, None, a["counters"], L.stream_ptr())

    bad = [dict(capacity=cap - 1), dict(capacity=0), dict(vsize=0.0), dict(vsize=nan), dict(M=-1), dict(Hp=0), dict(Wp=-3),
           dict(stride=0), dict(stride=3), dict(stride=8), dict(tol=0.0), dict(tol=-1.0), dict(tol=inf), dict(tol=nan),
           dict(margin=-1e-9), dict(margin=inf), dict(margin=nan), dict(mc=0), dict(mc=-2), dict(table=1), dict(views=1),
           dict(planes=1), dict(carved=1), dict(counters=1)]
    for kw in bad:
        lib.pi3_set_knob(b"no_such_knob", 0)
        before = lib.pi3_last_error()
        assert call(**kw) == -1, kw
        msg = lib.pi3_last_error()
        assert msg and msg != before and b"pi3_voxel_carve" in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((carved == 7).all()) and counters.tolist() == [11] * 4
    assert call() == 0
    torch.cuda.synchronize()
    assert counters.tolist()[0] == len(dist) and not bool((carved == 7).any())
    # the planes entry point
    pts, lp = _dev(s["points"]), _dev(s["local_points"])
    depth = torch.full((N * H * W,), 9.0, dtype=torch.float16, device=DEV)
    count = torch.full((1,), 11, dtype=torch.int64, device=DEV)

    def planes_call(n=N, h=H, w=W, every=1, stride=1, **null):
        a = dict(points=pts.data_ptr(), local=lp.data_ptr(), depth=depth.data_ptr(), count=count.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_dense_depth_planes(a["points"], a["local"], None, None, n, h, w, 0.0, every, stride, a["depth"],
                                          a["count"], L.stream_ptr())

    for kw in [dict(n=-1), dict(h=0), dict(w=0), dict(every=0), dict(every=-1), dict(stride=0), dict(stride=3), dict(stride=5),
               dict(points=1), dict(local=1), dict(depth=1), dict(count=1)]:
        assert planes_call(**kw) == -1, kw
        assert b"pi3_dense_depth_planes" in lib.pi3_last_error()
    torch.cuda.synchronize()
    assert bool((depth == 9.0).all()) and count.tolist() == [11]
    assert planes_call(n=0) == 0                      # an empty chunk zeroes the count and launches nothing
    torch.cuda.synchronize()
    assert bool((depth == 9.0).all()) and count.tolist() == [0]
    assert planes_call() == 0
    torch.cuda.synchronize()
    assert count.tolist()[0] > 0 and not bool((depth == 9.0).any())


# ------------------------------------------------------------------------------------------------ 3. cleaner + exclude
TODAY = {"voxels", "eligible", "after_support", "after_components", "components", "components_kept", "sweeps"}


@pytest.mark.parametrize("R", [1, 2])
def test_cleaner_with_excluded_voxels_matches_reference(R):
    from pi3_slam_amd.dense_map import MapCleaner
    idx, w = clean_gpu._random_points()
    fz = clean_gpu._fused(idx, w)
    keys, W = clean_gpu._voxels(idx, w)
    slot_keys, occ, order = _slots(fz)
    assert np.array_equal(slot_keys[occ][order], keys)
    rng = np.random.default_rng(11)
    mask = (rng.random(fz.capacity) < 0.25).astype(np.uint8)          # a quarter of ALL slots: empty ones do not count
    mask[rng.random(fz.capacity) < 0.01] = 200                        # any non-zero byte excludes
    excluded = mask[occ][order] != 0                                  # per voxel, in key order
    assert 0 < int(excluded.sum()) < len(keys) and mask[~occ].any()
    exclude = torch.from_numpy(mask).to(DEV)
    full = fz.extract()
    pairs = ((4, 0), (0, 20), (3, 10), (0, 0)) if R == 1 else ((20, 0), (0, 20), (16, 10))
    for min_weight in (1, 3):
        for min_support, min_component in pairs:
            c = MapCleaner(min_weight, min_support, R, min_component)
            keep = c.apply(fz, arrays=True, exclude=exclude)
            exp = clean_ref.clean(keys[~excluded], W[~excluded], **c.settings())
            arr = {k: t.cpu().numpy() for k, t in c.last_arrays.items()}
            got = {"support": arr["support"][occ][order], "label": arr["label"].view(np.uint64)[occ][order],
                   "size": arr["size"].view(np.uint32)[occ][order], "keep": keep.cpu().numpy()[occ][order]}
            want = {"support": exp["support"], "label": exp["label"], "size": exp["root_size"],
                    "keep": exp["keep"].astype(np.uint8)}
            for k in got:
                assert got[k].dtype == want[k].dtype, k
                assert got[k][~excluded].tobytes() == want[k].tobytes(), (k, min_weight, min_support, min_component)
            # an excluded voxel is nothing: not eligible, no label, no size, not kept
            assert np.all(got["support"][excluded] == -1) and np.all(got["label"][excluded] == NONE)
            assert np.all(got["size"][excluded] == 0) and not got["keep"][excluded].any()
            assert not keep.cpu().numpy()[~occ].any()
            st = dict(c.last_stats)
            assert set(st) == TODAY | {"carved"}
            st.pop("sweeps")
            assert st.pop("carved") == int(excluded.sum())
            assert st.pop("voxels") == len(keys) == exp["stats"]["voxels"] + int(excluded.sum())
            assert st == {k: v for k, v in exp["stats"].items() if k != "voxels"}
            print(f"R={R} {c.summary()}; {int(excluded.sum())} excluded")
            if min_support:
                assert 0 < st["after_support"] < st["eligible"]
            rows = fz.extract(keep)
            sel = np.zeros(len(keys), bool)
            sel[~excluded] = exp["keep"]
            for k in clean_gpu.ROWS:
                assert rows[k].tobytes() == full[k][sel].tobytes(), k
            # without the test's arrays: the same mask; with an all-zero mask: the plain cleaner's result
            plain = MapCleaner(**c.settings())
            assert torch.equal(plain.apply(fz, exclude=exclude), keep) and plain.last_stats["carved"] == int(excluded.sum())
    zero = torch.zeros(fz.capacity, dtype=torch.uint8, device=DEV)
    a, b = MapCleaner(2, 4, R, 10), MapCleaner(2, 4, R, 10)
    assert torch.equal(a.apply(fz, exclude=zero), b.apply(fz))
    # (not `sweeps`: a sweep reads what the previous one wrote "or something newer", so two runs may settle in 5 and in 6)
    sa, sb = ({k: v for k, v in c.last_stats.items() if k not in ("carved", "sweeps")} for c in (a, b))
    assert sa == sb and set(a.last_stats) == set(b.last_stats) | {"carved"} and a.last_stats["carved"] == 0
    assert a.last_stats["sweeps"] > 0 and b.last_stats["sweeps"] > 0


def test_cleaner_without_exclude_reports_what_it_reports_today():
    from pi3_slam_amd.dense_map import MapCleaner
    idx, w = clean_gpu._random_points(6000, 26, seed=3)
    fz = clean_gpu._fused(idx, w)
    for c in (MapCleaner(2, 5, 1, 25), MapCleaner(min_support=3), MapCleaner()):
        c.apply(fz)
        assert set(c.last_stats) == TODAY
        c.apply(fz, arrays=True, exclude=None)
        assert set(c.last_stats) == TODAY


def test_support_excluding_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    idx, w = clean_gpu._random_points(2000, 20, seed=2)
    fz = clean_gpu._fused(idx, w)
    cap = fz.capacity
    keep = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    excl = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    counters = torch.full((8,), 11, dtype=torch.int64, device=DEV)

    def call(capacity=cap, radius=1, ms=0, **null):
        a = dict(table=fz.table.data_ptr(), keep=keep.data_ptr(), counters=counters.data_ptr(), exclude=excl.data_ptr())
        a.update({k: None for k in null})
        return lib.pi3_voxel_support_excluding(a["table"], capacity, 1, radius, ms, a["keep"], None, a["counters"],
                                               a["exclude"], L.stream_ptr())

    for kw in [dict(capacity=cap + 1), dict(radius=0), dict(radius=3), dict(ms=-1), dict(ms=27), dict(radius=2, ms=125),
               dict(table=1), dict(keep=1), dict(counters=1), dict(exclude=1)]:
        assert call(**kw) == -1, kw
        assert b"pi3_voxel_support_excluding" in lib.pi3_last_error()
    torch.cuda.synchronize()
    assert bool((keep == 7).all()) and counters.tolist() == [11] * 8
    assert call() == 0
    torch.cuda.synchronize()
    assert counters.tolist()[0] == counters.tolist()[2] == int(keep.sum()) and counters.tolist()[6] == 0


# ------------------------------------------------------------------------------------------------ 4. end to end
GT = os.path.join(ROOT, "tests", "golden", "gt_7scenes_chess.txt")
VOXEL, CONF_THR, MIN_CONFLICTS = 0.02, 0.7, 3
EVERY, STRIDE = 2, 2
FLOATER_FRAMES, FLOATER_ROWS, FLOATER_COLS = tuple(range(20, 45, 2)), slice(120, 160), slice(180, 220)
FILTER = dict(min_views=2, radius=3, stride=2, rel_tol=REL_TOL)         # the in-chunk consistency filter's defaults


class CarveFloaterEngine:
    """SceneEngine whose chunk 0 carries a confident floater that its neighbouring frames agree on: in every even frame
    from 20 to 44 a 40 x 40 block of local_points is pulled to half its depth, its world points follow through the
    frame's pose, its logits are set high.  Every frame of the run has at least as many neighbours (i +- 2, 4, 6) with
    the floater as without, so the in-chunk consistency filter at its defaults keeps it."""

    def __init__(self, seq):
        import synth_sequence as ss
        self.inner = ss.SceneEngine(seq)

    def flops(self, *a):
        return self.inner.flops(*a)

    def __call__(self, imgs, **kw):
        out = self.inner(imgs, **kw)
        if int(round(float(imgs[0, 0, 0, 0, 0]) * 1024.0)) == 0:           # chunk 0 starts at frame 0
            for f in FLOATER_FRAMES:
                lp = out["local_points"][0, f, FLOATER_ROWS, FLOATER_COLS] * 0.5
                pose = out["camera_poses"][0, f]
                out["local_points"][0, f, FLOATER_ROWS, FLOATER_COLS] = lp
                out["points"][0, f, FLOATER_ROWS, FLOATER_COLS] = (lp[..., None, :] * pose[:3, :3]).sum(-1) + pose[:3, 3]
                out["conf"][0, f, FLOATER_ROWS, FLOATER_COLS] = 8.0
        return out


def _creator(seq, out_dir, **kw):
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    kw.setdefault("keypoint_type", "grid")
    kw.setdefault("estimate_camera_params", True)
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, max_num_keypoints=seq.max_kp, num_loader_workers=0, **kw)
    cr = OfflineChunkCreator(cfg, model=CarveFloaterEngine(seq))
    cr.target_size = (seq.H, seq.W)
    return cr


def _create(seq, out_dir, chunks, write=True, **kw):
    cr = _creator(seq, out_dir, **kw)
    done = list(cr.process_chunks(cons_gpu._items(seq, cr.device, chunks)))
    if write:
        _, manifest, _ = cr.write_chunks(iter(done))
        cr.write_run_metadata(manifest)
    return [ch for _, ch in done]


def _reconstruct(chunk_dir, out_dir, **kw):
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    rec = OfflineReconstructor(chunk_dir=chunk_dir, output_dir=out_dir, bundle_adjust=False, **kw)
    rec.run()
    return rec


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _same(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if torch.is_tensor(x):
        return x.dtype == y.dtype and torch.equal(x, y)
    return x == y


# The CPU oracles alone, before any device run (the same scene and floater through the engine above on the CPU, masks
# from oracle/post_ref.compute_masks, the consistency oracle with the filter's defaults, the scene's true intrinsics and
# gauges in place of the estimated intrinsics and the alignment; 110 keyframes of 3 chunks, min_conflicts 1, 3 and 5
# alike): the filter keeps 921 to 1 406 of the block's 1 444 masked pixels in each of its 13 frames, so the floater
# reaches the map: of its 215 205 voxels 740 lie more than 10 cm from every wall and sphere.  The oracle carves 745,
# among them all 740 (none left), and keeps every one of the 6 144 on-surface voxels (centroid within 1 mm of a
# surface): retention 1.0000.  The floor is 0.05 below; it only guards against a scene change that silently empties
# the map.  (A block in frames 30, 32 and 34 only does not survive the filter: the frames 6 away contradict it.)
# On the device the result equals the oracle's on the device's own maps, filter mask and alignment (214 978 voxels, 751
# far ones, 752 carved, none left, 1.0000 of 6 055 on an MI355X).
RETENTION_ORACLE = 1.0
RETENTION_FLOOR = RETENTION_ORACLE - 0.05


def test_creator_reconstruct_carved_map_matches_oracle(tmp_path, capsys):
    """Three creator runs over the three chunks (100, 100 and 20 frames) of the 180-frame chess-room scene, three
    reconstructions, and on the host the planes' oracle for two chunks and the carve oracle over 110 keyframes."""
    import synth_sequence as ss
    from pi3_slam_amd.dense_map import MapCarver
    from pi3_slam_amd.export import write_ply
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), n_frames=180)
    all_chunks = tuple(range(len(seq.chunks)))
    assert all_chunks == (0, 1, 2)
    dense = dict(dense_voxel_size=VOXEL, dense_conf_threshold=CONF_THR, dense_min_views=FILTER["min_views"])
    off = _create(seq, str(tmp_path / "off"), all_chunks, **dense)
    on = _create(seq, str(tmp_path / "on"), all_chunks, dense_depth_every=EVERY, dense_depth_stride=STRIDE, **dense)
    maps = _create(seq, str(tmp_path / "maps"), (0, 2), write=False, keypoint_type="none")

    # stage 1: without the option nothing new; with it only dense_depth and its metric
    for a, b in zip(off, on):
        assert "dense_depth" not in a and "dense_depth_samples" not in a["_metrics"]
        assert set(b) - set(a) == {"dense_depth"} and set(a) <= set(b)
        assert set(b["_metrics"]) - set(a["_metrics"]) == {"dense_depth_samples"} and set(a["_metrics"]) <= set(b["_metrics"])
        for k in a:
            if k != "_metrics":
                assert _same(a[k], b[k]), k
        assert a["_metrics"]["dense_voxels"] == b["_metrics"]["dense_voxels"]
    for c, m in zip((0, 2), maps):
        b = on[c]
        pts, lp, conf, masks = (m[k].numpy() for k in ("points", "local_points", "conf", "masks"))
        cam = b["camera_params"]
        K = torch.stack([cam[k][0] for k in ("fx", "fy", "cx", "cy")], 1)
        # the planes run on the mask fuse_pixels used: the filter's, not the creator's
        flt = cref.consistency(pts, lp, conf, masks, b["camera_poses"].numpy(), K.numpy().astype(np.float32),
                               mref.conf_logit(CONF_THR), FILTER["radius"], FILTER["stride"], FILTER["min_views"],
                               FILTER["rel_tol"])
        used = masks.astype(bool) & flt["mask"].astype(bool)
        exp, n = ref.depth_planes(pts, lp, conf, used, mref.conf_logit(CONF_THR), EVERY, STRIDE)
        unfiltered, n_unfiltered = ref.depth_planes(pts, lp, conf, masks, mref.conf_logit(CONF_THR), EVERY, STRIDE)
        assert n < n_unfiltered and exp.tobytes() != unfiltered.tobytes()
        assert b["dense_cloud"]["consistency"] == FILTER
        assert b["_metrics"]["dense_consistent"] == int(flt["stats"][1])
        dd = b["dense_depth"]
        N = len(pts)
        assert dd["depth"].dtype == torch.float16 and dd["depth"].numpy().tobytes() == exp.tobytes()
        assert tuple(dd["depth"].shape) == (-(-N // EVERY), -(-seq.H // STRIDE), -(-seq.W // STRIDE))
        assert b["_metrics"]["dense_depth_samples"] == n > exp.size // 2
        assert dd["frames"].dtype == torch.int32 and dd["frames"].tolist() == list(range(0, N, EVERY))
        assert (dd["pixel_stride"], dd["height"], dd["width"]) == (STRIDE, seq.H, seq.W)
        assert dd["fxfycxcy"].dtype == torch.float32 and torch.equal(dd["fxfycxcy"], K[::EVERY])
        if c == 0:
            # the floater survives stage 1: the filter keeps most of the block in every one of its frames
            for f in FLOATER_FRAMES:
                assert int(flt["mask"][f, FLOATER_ROWS, FLOATER_COLS].sum()) > 500, f
            # and it is in the planes of its frames: half the depth of the last keyframe before the run
            blk = (slice(FLOATER_ROWS.start // STRIDE, FLOATER_ROWS.stop // STRIDE),
                   slice(FLOATER_COLS.start // STRIDE, FLOATER_COLS.stop // STRIDE))
            first = FLOATER_FRAMES[0] // EVERY
            a0, a1 = exp[(first - 1,) + blk].astype(np.float64), exp[(first,) + blk].astype(np.float64)
            both = (a0 > 0) & (a1 > 0)
            assert both.sum() > 100 and 0.45 < np.median(a1[both] / a0[both]) < 0.55

    # stage 2: without the carve option the output is what it is without the planes
    capsys.readouterr()
    _reconstruct(str(tmp_path / "off"), str(tmp_path / "rec_off"))
    rec_plain = _reconstruct(str(tmp_path / "on"), str(tmp_path / "rec_plain"))
    said = capsys.readouterr().out
    assert "Dense map carved" not in said
    t_off, t_plain = _tree(tmp_path / "rec_off"), _tree(tmp_path / "rec_plain")
    assert set(t_off) == set(t_plain) and "dense_points.ply" in t_off
    assert all(t_off[k] == t_plain[k] for k in t_off)
    rec = _reconstruct(str(tmp_path / "on"), str(tmp_path / "rec_carved"), dense_carve_min_conflicts=MIN_CONFLICTS)
    said = capsys.readouterr().out
    line = [ln for ln in said.splitlines() if "Dense map carved:" in ln]
    assert len(line) == 1 and "Dense map cleaned" not in said
    t_carved = _tree(tmp_path / "rec_carved")
    assert set(t_carved) == set(t_plain)
    assert all(t_carved[k] == t_plain[k] for k in t_plain if k != "dense_points.ply")

    chunks = rec.reconstructions
    assert all("dense_depth" in d for d in chunks)
    world = cons_gpu._oracle_world(chunks, VOXEL)
    views, planes, stride = MapCarver.chunk_views(chunks)
    assert len(views) == 50 + 50 + 10 and stride == STRIDE
    exp = ref.carve(world["points"], views, planes.numpy(), stride, REL_TOL, MapCarver.MARGIN_VOXELS * VOXEL, MIN_CONFLICTS)
    st = rec.dense_carver.last_stats
    assert st == dict(views=len(views), **exp["stats"])
    assert all(str(st[k]) in line[0] for k in ("views", "carved", "voxels", "unvoted"))
    keepv = ~exp["carved"]
    write_ply(world["points"], np.asarray(world["colors"], np.uint8), str(tmp_path / "oracle_plain.ply"))
    write_ply(world["points"][keepv], np.asarray(world["colors"][keepv], np.uint8), str(tmp_path / "oracle_carved.ply"))
    assert t_plain["dense_points.ply"] == open(tmp_path / "oracle_plain.ply", "rb").read()
    assert t_carved["dense_points.ply"] == open(tmp_path / "oracle_carved.ply", "rb").read()

    # geometry, in metres through chunk 0's gauge (the world frame is chunk 0's frame)
    _, d = cons_gpu.surface_distance(world["points"], seq, 0)
    far, on_surface = d > 0.10, d <= 1e-3
    retention = float(keepv[on_surface].mean())
    print(f"fused map {len(d)} voxels, {len(views)} keyframes: {int(far.sum())} voxels more than 10 cm from every surface, "
          f"{int((far & keepv).sum())} after carving; {exp['stats']['carved']} carved, {exp['stats']['unvoted']} without a "
          f"vote; retention of the {int(on_surface.sum())} on-surface voxels {retention:.4f}")
    assert int(far.sum()) >= 50                   # not vacuous: the floater is in the uncarved map
    assert int((far & keepv).sum()) == 0          # none left
    assert retention >= RETENTION_FLOOR

    # the online facade hands its carver to the same fusion
    from pi3_slam_amd.online import Pi3SLAMOnline
    slam = Pi3SLAMOnline.__new__(Pi3SLAMOnline)
    slam.chunk_reconstructions, slam.device, slam.dense_cleaner = chunks, torch.device(DEV), None
    slam.dense_carver = MapCarver.from_options(MIN_CONFLICTS)
    assert slam.save_dense_map(str(tmp_path / "online.ply")) == int(keepv.sum())
    assert open(tmp_path / "online.ply", "rb").read() == t_carved["dense_points.ply"]


def test_without_intrinsics_no_depth_planes_and_one_warning(tmp_path, capsys):
    import synth_sequence as ss
    seq = ss.SyntheticSequence(GT, noise=dict(ss.NOISE_BF16), n_frames=180)
    dense = dict(dense_voxel_size=VOXEL, dense_conf_threshold=CONF_THR, estimate_camera_params=False)
    plain = _create(seq, str(tmp_path / "plain"), (2,), write=False, **dense)[0]
    capsys.readouterr()
    got = _create(seq, str(tmp_path / "depth"), (2, 2), write=False, dense_depth_every=EVERY, **dense)     # two chunks, one run
    assert capsys.readouterr().out.count("dense depth keyframes: no intrinsics") == 1
    for ch in got:
        assert "dense_depth" not in ch and "dense_depth_samples" not in ch["_metrics"] and "camera_params" not in ch
        assert _same(ch["dense_cloud"], plain["dense_cloud"]) and len(ch["dense_cloud"]["points"]) > 1000
