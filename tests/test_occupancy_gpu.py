"""The occupancy grid and the clearance field on the GPU (csrc/occupancy.hip), byte for byte against the numpy oracle
(tests/occupancy_ref.py): the mark, observe and distance-transform kernels, the box room's invariants, and creator ->
reconstruct -> occupancy.npz on a two-chunk sequence.  Every output is filled with a poison value before each call."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import occupancy_ref as ref                 # noqa: E402
import test_dense_follow_gpu as follow_gpu  # noqa: E402  (the creator / reconstructor helpers of the follow tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON8, POISON16, POISON32, POISON64 = 7, 0x5A5A, -5, 11


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. mark
def _mark_device(points, cell, origin, dims):
    from pi3_slam_amd import ops
    nx, ny, nz = dims
    state = torch.full((nz, ny, nx), POISON8, dtype=torch.uint8, device=DEV)
    counters = torch.full((4,), POISON64, dtype=torch.int64, device=DEV)
    ops.occupancy_mark(_dev(points), float(ref.inv_cell(cell)), origin, state, counters)
    return state.cpu().numpy(), counters.cpu().numpy()


@pytest.mark.parametrize("cell", [0.1, 0.25])
def test_mark_matches_oracle_byte_for_byte(cell):
    origin, dims = (-7, -3, -2), (23, 9, 5)
    rng = np.random.default_rng(1)
    lo, hi = np.array(origin) * cell, (np.array(origin) + dims) * cell
    inside = rng.uniform(lo, hi, (120, 3))
    around = rng.uniform(lo - 1.0, hi + 1.0, (40, 3))                   # many outside the grid, negative coordinates
    edges = np.array([[i * cell, j * cell, k * cell] for i, j, k in
                      [(0, 0, 0), (-7, -3, -2), (16, 6, 3), (15, 5, 2), (-1, -1, -1), (1, 1, 1), (-8, 0, 0), (3, -3, 3)]])
    big = float(1 << 20) * cell
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [big, 0, 0], [0, -1.5 * big, 0], [0, 0, 2 * big],
                    [-big, 0.1, 0.1], [np.nan, np.nan, np.nan]])
    pts = np.concatenate([inside, around, edges, odd, inside[:24]]).astype(np.float32)           # the last: duplicates
    assert len(pts) == 200
    exp = ref.mark(pts, cell, origin, dims)
    st = exp["stats"]
    assert st["dropped"] >= 7 and st["outside"] >= 10 and st["marked"] >= 130
    assert st["marked"] > int((exp["state"] == 2).sum())                # several points share a cell
    got = _mark_device(pts, cell, origin, dims)
    again = _mark_device(pts, cell, origin, dims)
    print(f"cell {cell}: {st}, {int((exp['state'] == 2).sum())} cells occupied")
    assert got[0].tobytes() == exp["state"].tobytes() == again[0].tobytes()
    assert got[1].tolist() == [st["marked"], st["dropped"], st["outside"], 0] == again[1].tolist()
    none = _mark_device(np.zeros((0, 3), np.float32), cell, origin, dims)                        # no points: all unknown
    assert not none[0].any() and none[1].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 2. observe
CELL = 0.125            # exact in binary: the centres and the edge view below are exact


def _observe_device(state, cell, origin, views, planes, stride, rel_tol, margin, mfv):
    from pi3_slam_amd import ops
    st = _dev(state)
    free = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    hit = torch.full(st.shape, POISON32, dtype=torch.int32, device=DEV)
    counters = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    ops.occupancy_observe(st, origin, cell, _dev(np.asarray(views, np.float64).reshape(-1, 20)), _dev(planes), stride,
                          rel_tol, margin, mfv, free, hit, counters)
    return st.cpu().numpy(), free.cpu().numpy().view(np.uint32), hit.cpu().numpy().view(np.uint32), counters.cpu().numpy()


def _check_observe(state, cell, origin, views, planes, stride, rel_tol, margin, mfv):
    exp = ref.observe(state, cell, origin, views, planes, stride, rel_tol, margin, mfv)
    got = _observe_device(state, cell, origin, views, planes, stride, rel_tol, margin, mfv)
    again = _observe_device(state, cell, origin, views, planes, stride, rel_tol, margin, mfv)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    assert got[0].tobytes() == exp["state"].tobytes()
    assert got[1].tobytes() == exp["free"].tobytes() and got[2].tobytes() == exp["hit"].tobytes()
    s = exp["stats"]
    assert got[3].tolist() == [s["cells"], s["occupied"], s["free"], s["unknown"], s["unvoted"],
                               s["camera_cells_freed"], 0, 0]
    return exp


def _observe_scene(dims, M, S, seed):
    """A grid of CELL-sized cells with its low z face at z = 0, some occupied cells, and M views 12 x 16 samples at
    stride S from z < 0 looking along +z with random depths around the grid: view 0 (M >= 3) is the edge view, whose
    projections of the iz = 0 row of centres land on whole sample columns up to and just past W' - 1; view 2 stands
    behind the grid's far side, looking away from it."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    origin = (-(nx // 2), -(ny // 2), 0)
    Hp, Wp = 12, 16
    poses = np.tile(np.eye(4), (M, 1, 1))
    K = np.zeros((M, 4))
    for m in range(M):
        poses[m, :3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), -rng.uniform(1.5, 2.5)]
        a = rng.uniform(-0.15, 0.15)
        poses[m, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        f = rng.uniform(5.0, 9.0) * S
        K[m] = [f, f, S * (Wp - 1) / 2.0, S * (Hp - 1) / 2.0]
    edge_u = None
    if M >= 3:
        # edge view: zc = 2 exactly for the centres with z = CELL / 2; u = 4 S x + cx runs over the plane in half
        # columns (every second one a tie of rint) and reaches S (W' - 1) seven cells short of the grid's high x face
        poses[0] = np.eye(4)
        poses[0, :3, 3] = [0.0, 0.0, CELL / 2 - 2.0]
        x = CELL * (np.arange(nx) + origin[0] + 0.5)
        f = 8.0 * S
        cx = S * (Wp - 1) - f * (x[nx - 8] / 2.0)
        K[0] = [f, f, cx, S * (Hp - 1) / 2.0]
        edge_u = f * (x / 2.0) + cx
        poses[2] = np.eye(4)
        poses[2, :3, 3] = [0.0, 0.0, CELL * nz + 5.0]                 # the whole grid has zc < 0
    views = ref.carve_ref.pack_views(poses, K, 1.0)
    views[:, ref.SCALE_AT] = rng.uniform(0.8, 1.25, M)
    z = rng.uniform(1.2, 3.2, (M, Hp, Wp))
    kind = rng.random((M, Hp, Wp))
    z[kind < 0.06] = 0.0
    z[(kind >= 0.06) & (kind < 0.09)] = np.inf
    z[(kind >= 0.09) & (kind < 0.12)] = np.nan
    z[(kind >= 0.12) & (kind < 0.14)] = 70000.0                        # rounds to inf in fp16
    with np.errstate(over="ignore"):
        planes = z.astype(np.float16)
    state = np.full((nz, ny, nx), POISON8, np.uint8)                   # only 2 means anything on the way in
    state[rng.random((nz, ny, nx)) < 0.1] = 2
    return origin, views, planes, state, edge_u


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("M", [0, 1, 3, 65])
@pytest.mark.parametrize("dims", [(37, 5, 3), (64, 1, 1), (65, 7, 2)], ids=lambda d: "%dx%dx%d" % d)
def test_observe_matches_oracle_byte_for_byte(dims, M, S):
    origin, views, planes, state, edge_u = _observe_scene(dims, M, S, 1000 * M + 10 * S + dims[0])
    margin = CELL
    for mfv in (1, 2, 4):
        exp = _check_observe(state, CELL, origin, views, planes, S, 0.03, margin, mfv)
        open_ = exp["state"] != 2
        assert exp["stats"]["occupied"] == int((state == 2).sum())
        if M == 0:
            assert exp["stats"]["free"] == 0 and exp["stats"]["unvoted"] == exp["stats"]["cells"] - exp["stats"]["occupied"]
        if M == 65 and dims[1] > 1:             # the thresholds are exercised: ties and one vote short
            tie = open_ & (exp["free"] == exp["hit"]) & (exp["free"] >= mfv)
            short = open_ & (exp["free"] == mfv - 1) & (exp["free"] > exp["hit"])
            assert tie.any() and not (exp["state"][tie] == 1).any()
            assert (short.any() or mfv == 1 or dims[0] < 65) and not (exp["state"][short] == 1).any()
            assert 0 < exp["stats"]["free"] < exp["stats"]["cells"] and exp["hit"].any()
    if edge_u is not None and dims[0] >= 37:    # the edge view reaches W' - 1 exactly and goes past it
        last = S * (planes.shape[2] - 1)
        assert (edge_u == last).any() and (edge_u == last + S / 2).any() and (edge_u > last + S).any()
        one = ref.observe(state, CELL, origin, views[:1], planes[:1], S, 0.03, margin, 1)
        seen, occ = one["seen"][0, dims[1] // 2], state[0, dims[1] // 2] == 2
        assert (seen[edge_u == last] | occ[edge_u == last]).all() and not seen[edge_u > last].any()
        assert (seen[edge_u < last] > 0).sum() >= 4
        behind = ref.observe(state, CELL, origin, views[2:3], planes[2:3], S, 0.03, margin, 1)
        assert not behind["seen"].any()


def test_the_cells_the_cameras_stand_in_become_free():
    """Views inside the grid looking at nothing (empty planes: nobody votes): two share a cell, one stands in an
    occupied cell, one outside the grid, one at a cell boundary, one not finite."""
    dims, origin = (9, 6, 4), (-4, -3, 0)
    centres = np.array([[0.06, 0.06, 0.06], [0.07, 0.01, 0.12], [-0.3, 0.2, 0.3], [0.31, -0.26, 0.45], [5.0, 0.0, 0.1],
                        [0.25, 0.125, 0.375], [-0.5, -0.375, 0.0], [np.nan, 0.0, 0.1]])
    poses = np.tile(np.eye(4), (len(centres), 1, 1))
    a = 0.3
    poses[:, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    poses[:, :3, 3] = centres
    views = ref.carve_ref.pack_views(poses, np.tile([8.0, 8.0, 3.5, 2.5], (len(centres), 1)))
    planes = np.zeros((len(centres), 6, 8), np.float16)
    state = np.full(dims[::-1], POISON8, np.uint8)
    cells = ref.centre_cells(views[:7], CELL) - np.asarray(origin)
    state[cells[3, 2], cells[3, 1], cells[3, 0]] = 2
    exp = _check_observe(state, CELL, origin, views, planes, 1, 0.03, CELL, 2)
    assert (cells[0] == cells[1]).all() and exp["stats"]["camera_cells_freed"] == 4 == exp["stats"]["free"]
    assert exp["stats"]["unvoted"] == exp["stats"]["cells"] - 1 and not exp["free"].any()
    assert [int(exp["state"][c[2], c[1], c[0]]) for c in cells[[0, 2, 3, 5, 6]]] == [1, 1, 2, 1, 1]


def _edt_device(state, R, unknown, d2=None, work=None):
    from pi3_slam_amd import ops
    st = _dev(state)
    if d2 is None:
        d2 = torch.full(st.shape, POISON16, dtype=torch.int16, device=DEV)
        work = torch.full(st.shape, POISON16, dtype=torch.int16, device=DEV)
    ops.grid_edt(st, R, unknown, d2, work)
    return d2, work


def test_box_room_on_the_device_meets_the_five_invariants():
    r = ref.box_room()
    m = ref.mark(r["points"], r["cell"], r["origin"], r["dims"])
    got = _mark_device(r["points"], r["cell"], r["origin"], r["dims"])
    assert got[0].tobytes() == m["state"].tobytes() and got[1].tolist()[:3] == [12 * 48 * 64, 0, 0]
    exp = _check_observe(got[0], r["cell"], r["origin"], r["views"], r["planes"], 1, r["rel_tol"], r["margin"],
                         r["min_free_views"])
    state, free, hit, _ = _observe_device(got[0], r["cell"], r["origin"], r["views"], r["planes"], 1, r["rel_tol"],
                                          r["margin"], r["min_free_views"])
    d2 = _edt_device(state, 20, False)[0].cpu().numpy().view(np.uint16)
    assert d2.tobytes() == ref.edt_ref(exp["state"], 20).tobytes()
    inv = ref.room_invariants(r, state, free, hit, exp["seen"], ref.clearance(d2, r["cell"]))
    print(exp["stats"], inv)
    assert inv["free_outside"] == 0
    assert inv["deep_seen"] > 5000 and inv["deep_seen_not_free"] == 0
    assert inv["cameras"] == 12 and inv["cameras_not_free"] == 0
    assert inv["occupied_deep"] == 0
    assert inv["clearance_short"] == 0


# ------------------------------------------------------------------------------------------------ 3. distance transform
def _edt_states(shape, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2, shape).astype(np.uint8)
    corner = base.copy()
    corner[0, 0, 0] = 2
    far_corner = np.ones(shape, np.uint8)
    far_corner[-1, -1, -1] = 2
    rand = base.copy()
    rand[rng.random(shape) < 0.02] = 2
    return {"none": np.ones(shape, np.uint8), "all": np.full(shape, 2, np.uint8), "corner": corner,
            "far_corner": far_corner, "random": rand}


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 300), (300, 2, 3), (3, 300, 2), (65, 67, 66)],
                         ids=lambda d: "%dx%dx%d" % d)
def test_edt_matches_oracle_byte_for_byte(dims):
    nx, ny, nz = dims
    radii = (1, 2, 7) + ((255,) if max(dims) == 300 else ())
    for name, state in _edt_states((nz, ny, nx), nx + ny + nz).items():
        for R in radii:
            for unknown in (False, True):
                exp = ref.edt_ref(state, R, unknown)
                d2, work = _edt_device(state, R, unknown)
                first = d2.cpu().numpy().view(np.uint16)
                assert first.tobytes() == exp.tobytes(), (name, R, unknown)
                _edt_device(state, R, unknown, d2, work)                      # again into the same buffers
                assert d2.cpu().numpy().view(np.uint16).tobytes() == exp.tobytes(), (name, R, unknown, "second call")
                if name == "none" and not unknown:
                    assert (exp == ref.FAR).all()
                if name == "all":
                    assert not exp.any()
    sites = int((exp != ref.FAR).sum())
    print(f"{dims}: radii {radii}, last case {sites} of {exp.size} cells within R")


def test_argument_errors_launch_nothing():
    from pi3_slam_amd import lib as L
    lib = L.load()
    state = torch.full((3, 4, 5), POISON8, dtype=torch.uint8, device=DEV)
    d2 = torch.full((3, 4, 5), POISON16, dtype=torch.int16, device=DEV)
    work = torch.full((3, 4, 5), POISON16, dtype=torch.int16, device=DEV)
    counters = torch.full((8,), POISON64, dtype=torch.int64, device=DEV)
    pts = torch.zeros((6, 3), dtype=torch.float32, device=DEV)
    views = torch.zeros((2, 20), dtype=torch.float64, device=DEV)
    planes = torch.ones((2, 4, 4), dtype=torch.float16, device=DEV)
    sp = L.stream_ptr()
    calls = [lambda: lib.pi3_occupancy_mark(pts.data_ptr(), 6, 0.0, 0, 0, 0, 5, 4, 3, state.data_ptr(), counters.data_ptr(), sp),
             lambda: lib.pi3_occupancy_mark(pts.data_ptr(), 6, 8.0, 0, 0, 0, 5, 0, 3, state.data_ptr(), counters.data_ptr(), sp),
             lambda: lib.pi3_occupancy_mark(None, 6, 8.0, 0, 0, 0, 5, 4, 3, state.data_ptr(), counters.data_ptr(), sp),
             lambda: lib.pi3_occupancy_observe(state.data_ptr(), 5, 4, 3, 0, 0, 0, 0.1, views.data_ptr(), 2, planes.data_ptr(),
                                               4, 4, 3, 0.03, 0.1, 2, None, None, counters.data_ptr(), sp),
             lambda: lib.pi3_occupancy_observe(state.data_ptr(), 5, 4, 3, 0, 0, 0, 0.1, views.data_ptr(), 2, planes.data_ptr(),
                                               4, 4, 1, 0.03, 0.1, 0, None, None, counters.data_ptr(), sp),
             lambda: lib.pi3_occupancy_observe(state.data_ptr(), 5, 4, 3, 0, 0, 0, 0.1, None, 2, planes.data_ptr(),
                                               4, 4, 1, 0.03, 0.1, 2, None, None, counters.data_ptr(), sp),
             lambda: lib.pi3_grid_edt(state.data_ptr(), 5, 4, 3, 0, 0, d2.data_ptr(), work.data_ptr(), sp),
             lambda: lib.pi3_grid_edt(state.data_ptr(), 5, 4, 3, 256, 0, d2.data_ptr(), work.data_ptr(), sp),
             lambda: lib.pi3_grid_edt(state.data_ptr(), 5, 4, 3, 3, 0, d2.data_ptr(), d2.data_ptr(), sp)]
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"pi3_occupancy_" in lib.pi3_last_error() or b"pi3_grid_edt" in lib.pi3_last_error()
    torch.cuda.synchronize()
    assert bool((state == POISON8).all()) and bool((d2 == POISON16).all()) and bool((work == POISON16).all())
    assert counters.tolist() == [POISON64] * 8


# ------------------------------------------------------------------------------------------------ 4. end to end
SCENE = dict(follow_gpu.SCENE, n_frames=50)         # two chunks: frames 0..39 and 30..49
OCC_CELL, OCC_CLEARANCE = 0.1, 0.5


@pytest.fixture(scope="module")
def reconstructed(tmp_path_factory):
    import synth_sequence as ss
    tmp = tmp_path_factory.mktemp("occupancy")
    seq = ss.SyntheticSequence(follow_gpu.GT, noise=dict(ss.NOISE_NONE), **SCENE)
    assert len(seq.chunks) == 2
    follow_gpu._create(seq, str(tmp / "chunks"))
    runs = {"on": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "on"), bundle_adjust=False,
                                          occupancy_cell=OCC_CELL, occupancy_clearance=OCC_CLEARANCE),
            "off": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "off"), bundle_adjust=False),
            "others": follow_gpu._reconstruct(str(tmp / "chunks"), str(tmp / "others"), bundle_adjust=False,
                                              occupancy_clearance=OCC_CLEARANCE, occupancy_min_free_views=3)}
    return tmp, runs


def _oracle_grid(points, chunks, stage):
    from pi3_slam_amd.dense_map import MapCarver
    views, planes, stride = MapCarver.chunk_views(chunks)
    origin, dims = stage.bounds(points, views)
    m = ref.mark(points, stage.cell, origin, dims)
    o = ref.observe(m["state"], stage.cell, origin, views, planes.numpy(), stride, stage.rel_tol,
                    stage.MARGIN_CELLS * stage.cell, stage.min_free_views)
    d2 = ref.edt_ref(o["state"], stage.radius, stage.unknown_is_obstacle) if stage.radius is not None else None
    return views, origin, m, o, d2


def _same_as_oracle(z, points, chunks, stage):
    views, origin, m, o, d2 = _oracle_grid(points, chunks, stage)
    assert z["state"].tobytes() == o["state"].tobytes() and z["state"].shape == o["state"].shape
    assert z["index_origin"].tolist() == origin.tolist() and float(z["cell"]) == stage.cell
    assert z["origin"].tolist() == (stage.cell * origin.astype(np.float64)).tolist()
    assert z["clearance"].tobytes() == ref.clearance(d2, stage.cell).tobytes()
    counts = __import__("json").loads(str(z["counts"]))
    assert counts == dict(views=len(views), **m["stats"], **o["stats"])
    return views, origin, o


def test_reconstruct_writes_the_oracles_grid(reconstructed):
    from pi3_slam_amd.dense_map import fuse_chunks
    tmp, runs = reconstructed
    rec = runs["on"]
    chunks = rec.reconstructions
    assert len(chunks) == 2 and all("dense_depth" in c for c in chunks)
    dense = fuse_chunks(chunks, DEV)
    assert dense.occupancy is None and dense.occupancy_error is None
    with np.load(tmp / "on" / "occupancy.npz") as z:
        views, origin, o = _same_as_oracle(z, dense.points, chunks, rec.dense_occupancy)
        state, clear = z["state"], z["clearance"]
    st = o["stats"]
    print(f"{state.shape[::-1]} cells of {OCC_CELL} from {len(views)} views: {st}")
    assert rec.dense_occupancy.last_stats["free"] == st["free"] > 0 and st["occupied"] > 0       # not vacuous
    # every camera looked at the room from verified free space
    cams = ref.centre_cells(views, OCC_CELL) - origin
    at = (cams[:, 2], cams[:, 1], cams[:, 0])
    print(f"camera cells: {int((state[at] == 1).sum())} of {len(cams)} free, clearance {clear[at].min():.3f} .. "
          f"{clear[at].max():.3f}")
    assert (state[at] == 1).all() and (clear[at] > 0).all()


def test_flags_off_change_nothing(reconstructed):
    tmp, runs = reconstructed
    on, off, others = (follow_gpu._tree(tmp / k) for k in ("on", "off", "others"))
    assert set(on) - set(off) == {"occupancy.npz"} and set(off) <= set(on) and "dense_points.ply" in off
    assert all(on[k] == off[k] for k in off)
    assert set(others) == set(off) and all(others[k] == off[k] for k in off)      # the other flags alone ask for nothing
    assert runs["off"].dense_occupancy is None and runs["others"].dense_occupancy is None


def test_online_facade_saves_the_same_grid_of_one_chunk(reconstructed, tmp_path, capsys):
    from pi3_slam_amd.dense_map import MapOccupancy, fuse_chunks
    from pi3_slam_amd.online import Pi3SLAMOnline
    tmp, runs = reconstructed
    chunks = runs["on"].reconstructions[:1]
    slam = Pi3SLAMOnline.__new__(Pi3SLAMOnline)
    slam.chunk_reconstructions, slam.device, slam.dense_cleaner = chunks, torch.device(DEV), None
    with pytest.raises(RuntimeError, match="occupancy_cell"):
        slam.save_occupancy(str(tmp_path / "none.npz"))
    slam.dense_occupancy = MapOccupancy.from_options(OCC_CELL, clearance=OCC_CLEARANCE, unknown_is_obstacle=True)
    n_free = slam.save_occupancy(str(tmp_path / "occupancy.npz"))
    with np.load(tmp_path / "occupancy.npz") as z:
        _, _, o = _same_as_oracle(z, fuse_chunks(chunks, DEV).points, chunks, slam.dense_occupancy)
        assert np.isfinite(z["clearance"][z["state"] == 1]).any()
    assert n_free == o["stats"]["free"] > 0
    # chunks without depth keyframes: one notice, no file, no error
    bare = [{k: v for k, v in c.items() if k != "dense_depth"} for c in chunks]
    slam.chunk_reconstructions = bare
    capsys.readouterr()
    assert slam.save_occupancy(str(tmp_path / "bare.npz")) is None
    assert capsys.readouterr().out.count("No depth keyframes") == 1 and not os.path.exists(tmp_path / "bare.npz")
