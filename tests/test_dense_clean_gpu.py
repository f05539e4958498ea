"""The dense map's cleaning filters on the GPU (csrc/voxel_clean.hip, dense_map.MapCleaner) against the numpy reference
(tests/dense_clean_ref.py), byte for byte: support counts, labels, component sizes, the keep mask, the counters and the
extracted rows.  Voxels are fused through VoxelFuser.fuse_points at voxel centres with a power-of-two voxel size, so a
voxel index is exactly what the test wrote."""
import os

import numpy as np
import pytest
import torch

import dense_clean_ref as ref
import dense_map_ref as map_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = 0.25
ROWS = ("keys", "points", "colors", "weights")
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _colours(idx):
    """A colour that depends on the voxel only (so that any fusing order gives the same sums)."""
    i = np.asarray(idx, np.int64)
    return np.stack([(i[:, 0] * 7 + 3) % 256, (i[:, 1] * 13 + 5) % 256, (i[:, 2] * 29 + 11) % 256], 1).astype(np.uint8)


def _fuse(fz, idx, w):
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    pts = ((idx.astype(np.float64) + 0.5) * V).astype(np.float32)            # exact: |idx| < 2^20, V = 2^-2
    fz.fuse_points(torch.from_numpy(pts).to(DEV), torch.from_numpy(_colours(idx)).to(DEV),
                   torch.from_numpy(np.asarray(w, np.int32)).to(DEV).contiguous())


def _fused(idx, w):
    from pi3_slam_amd.dense_map import VoxelFuser
    fz = VoxelFuser(V, DEV)
    _fuse(fz, idx, w)
    return fz


def _voxels(idx, w):
    """The test's own account of the table: unique keys (ascending) and summed weights."""
    keys, inv = np.unique(ref.pack(idx), return_inverse=True)
    W = np.zeros(len(keys), np.uint64)
    np.add.at(W, inv.reshape(-1), np.asarray(w, np.uint64))
    return keys, W


def _check(fz, cleaner, keys, W, full=None):
    """Run the cleaner on the fuser's table and compare every per-slot array, the counters and the extracted rows with
    the reference over (keys ascending, W).  -> (reference result, device stats, extracted rows)."""
    keep = cleaner.apply(fz, arrays=True)
    exp = ref.clean(keys, W, **cleaner.settings())
    slot_keys = fz.table.view(-1, 8)[:, 0].cpu().numpy().view(np.uint64)
    occ = slot_keys != NONE
    order = np.argsort(slot_keys[occ])
    assert np.array_equal(slot_keys[occ][order], keys)
    arr = {k: t.cpu().numpy() for k, t in cleaner.last_arrays.items()}
    got = {"support": arr["support"], "label": arr["label"].view(np.uint64), "size": arr["size"].view(np.uint32),
           "keep": keep.cpu().numpy()}
    want = {"support": exp["support"], "label": exp["label"], "size": exp["root_size"],
            "keep": exp["keep"].astype(np.uint8)}
    for k in got:
        assert got[k].dtype == want[k].dtype, k
        assert got[k][occ][order].tobytes() == want[k].tobytes(), k
    # the device keeps a component's size at the slot of the voxel that gives the label: per voxel, through the label
    slot_of = dict(zip(slot_keys[occ].tolist(), np.flatnonzero(occ).tolist()))
    per_voxel = [int(got["size"][slot_of[int(l)]]) if l != NONE else 0 for l in exp["label"]]
    assert per_voxel == exp["size"].tolist()
    # a slot without a voxel carries the neutral value of every array
    assert np.all(got["support"][~occ] == -1) and np.all(got["label"][~occ] == NONE)
    assert np.all(got["size"][~occ] == 0) and np.all(got["keep"][~occ] == 0)
    st = dict(cleaner.last_stats)
    sweeps = st.pop("sweeps")
    assert st == exp["stats"], (st, exp["stats"])
    assert 1 <= sweeps <= exp["stats"]["after_support"] + 1 + cleaner.SWEEPS_PER_READ
    full = fz.extract() if full is None else full
    rows = fz.extract(keep)
    assert full["keys"].view(np.uint64).tobytes() == keys.tobytes()
    sel = exp["keep"]
    assert fz.last_stats["voxels"] == int(sel.sum()) == len(rows["keys"])
    for k in ROWS:
        assert rows[k].tobytes() == full[k][sel].tobytes(), k
    return exp, dict(cleaner.last_stats), rows


# ------------------------------------------------------------------------------------------------ 1. designed scene
TOP = (1 << 20) - 1


def _designed_scene():
    """-> {name: idx}, weight-3 objects with >= 3 empty cells between them, and weight-1 voxels that must not count."""
    s = {}
    s["slab"] = [(x, y, 0) for x in range(-6, 6) for y in range(-6, 6)]          # straddles the origin
    s["isolated"] = [(20, 0, 0)]
    s["pair"] = [(20, 10, 0), (21, 10, 0)]
    s["blob"] = [(30 + a, b, c) for a in range(3) for b in range(3) for c in range(3)]
    s["chain"] = [(40 + i, i, i) for i in range(5)]                               # touching by corners only
    s["edge_x"] = [(TOP, 0, 0), (TOP - 1, 1, 0)]
    s["edge_z"] = [(0, 0, -TOP), (0, 1, -TOP + 1)]
    s["bridge_ends"] = [(60, 0, 0), (62, 0, 0)]
    light = {"bridge": [(61, 0, 0)], "beside_isolated": [(20, 1, 0)], "on_slab": [(0, 0, 1), (-6, -6, 1)]}
    return {k: np.array(v, np.int64) for k, v in s.items()}, {k: np.array(v, np.int64) for k, v in light.items()}


def test_designed_scene_with_hand_derived_answers():
    from pi3_slam_amd.dense_map import MapCleaner
    heavy, light = _designed_scene()
    idx = np.concatenate(list(heavy.values()) + list(light.values()))
    w = np.concatenate([np.full(sum(len(v) for v in heavy.values()), 3), np.full(sum(len(v) for v in light.values()), 1)])
    rng = np.random.default_rng(0)
    p = rng.permutation(len(idx))
    fz = _fused(idx[p], w[p])
    keys, W = _voxels(idx, w)
    full = fz.extract()
    exp_rows = map_ref.fuse_points(((idx + 0.5) * V).astype(np.float32), _colours(idx), w.astype(np.int32), V)
    for k in ROWS:                                            # the table itself, against the map's own oracle
        assert full[k].tobytes() == exp_rows[k].tobytes(), k

    exp, st, _ = _check(fz, MapCleaner(min_weight=3), keys, W, full)
    at = {int(k): i for i, k in enumerate(keys)}

    def of(name, what, src=heavy):
        return [int(exp[what][at[int(k)]]) for k in ref.pack(src[name])]

    slab = heavy["slab"]
    on_rim = ((slab[:, 0] == -6) | (slab[:, 0] == 5)).astype(int) + ((slab[:, 1] == -6) | (slab[:, 1] == 5)).astype(int)
    assert of("slab", "support") == [{0: 8, 1: 5, 2: 3}[r] for r in on_rim]       # weight-1 voxels on it do not count
    assert of("isolated", "support") == [0] and of("pair", "support") == [1, 1]
    blob = heavy["blob"] - np.array([31, 1, 1])
    assert of("blob", "support") == [{0: 26, 1: 17, 2: 11, 3: 7}[int(n)] for n in np.abs(blob).sum(1)]
    assert of("chain", "support") == [1, 2, 2, 2, 1]
    assert of("edge_x", "support") == [1, 1] and of("edge_z", "support") == [1, 1]   # nothing wrapped, nothing lost
    assert of("bridge_ends", "support") == [0, 0]
    for name in light:
        assert set(of(name, "support", light)) == {-1} and not any(of(name, "keep", light))
    sizes = {"slab": 144, "isolated": 1, "pair": 2, "blob": 27, "chain": 5, "edge_x": 2, "edge_z": 2}
    for name, n in sizes.items():
        assert set(of(name, "size")) == {n}, name
        assert set(of(name, "label")) == {int(ref.pack(heavy[name]).min())}, name
    assert of("bridge_ends", "size") == [1, 1]                # the weight-1 voxel between them is no bridge
    assert st["voxels"] == len(keys) and st["eligible"] == st["after_support"] == len(keys) - 4
    assert st["components"] == 9 and st["components_kept"] == 9

    # the filters: support >= 1 drops the isolated voxel and the bridge ends, components >= 3 the pairs
    exp, st, rows = _check(fz, MapCleaner(min_weight=3, min_support=1, min_component=3), keys, W, full)
    assert (st["after_support"], st["after_components"], st["components"], st["components_kept"]) == (
        len(keys) - 4 - 3, 144 + 27 + 5, 6, 3)
    assert len(rows["keys"]) == 176
    # every voxel eligible: the weight-1 voxel bridges its ends into one component of 3, the slab gains two voxels
    exp, st, _ = _check(fz, MapCleaner(min_support=1, min_component=3), keys, W, full)
    assert of("bridge_ends", "size") == [3, 3] and set(of("slab", "size")) == {146} and of("isolated", "support") == [1]
    # radius 2
    exp, _, _ = _check(fz, MapCleaner(min_weight=3, support_radius=2, min_support=10), keys, W, full)
    assert max(of("slab", "support")) == 24 and min(of("slab", "support")) == 8 and set(of("blob", "support")) == {26}
    assert of("chain", "support") == [2, 3, 4, 3, 2] and of("bridge_ends", "support") == [1, 1]
    assert of("edge_x", "support") == [1, 1] and of("edge_z", "support") == [1, 1]


# ------------------------------------------------------------------------------------------------ 2. random
def _random_points(n=20000, box=40, seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(-box // 2, box // 2, (n, 3)), rng.integers(1, 6, n)


@pytest.mark.parametrize("min_weight", [1, 3])
@pytest.mark.parametrize("R", [1, 2])
def test_random_points_at_the_minimum_capacity(R, min_weight):
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import MapCleaner
    idx, w = _random_points()
    fz = _fused(idx, w)
    assert fz.capacity == ops.voxel_capacity(len(idx)) == 65536       # the capacity rule's minimum: probe chains occur
    keys, W = _voxels(idx, w)
    assert 15000 < len(keys) < len(idx)
    full = fz.extract()
    # each stage alone, both, neither; (40, 30) at radius 2 leaves few survivors, none at min_weight 3
    pairs = ((4, 0), (0, 20), (6, 30), (0, 0)) if R == 1 else ((30, 0), (0, 20), (28, 10), (40, 30))
    for min_support, min_component in pairs:
        c = MapCleaner(min_weight, min_support, R, min_component)
        _, st, _ = _check(fz, c, keys, W, full)
        print(f"R={R} {c.summary()}; {st['components']} components, {st['components_kept']} kept, {st['sweeps']} sweeps")
        if min_weight == 3:
            assert st["eligible"] < st["voxels"]
        if min_support and min_support < 40:
            assert 0 < st["after_support"] < st["eligible"]
        if min_component:
            assert st["components_kept"] < st["components"] or st["components"] == 0
        # what a caller gets without the test's arrays: the same mask and counters
        keep = c.apply(fz, arrays=True)
        plain = MapCleaner(**c.settings())
        assert torch.equal(plain.apply(fz), keep)
        if min_component > 1:
            assert {k: v for k, v in plain.last_stats.items() if k != "sweeps"} == {
                k: v for k, v in c.last_stats.items() if k != "sweeps"}
        else:
            assert plain.last_stats["components"] is None and plain.last_stats["sweeps"] == 0
            assert plain.last_stats["after_components"] == plain.last_stats["after_support"] == st["after_support"]


# ------------------------------------------------------------------------------------------------ 3. layout
def test_result_does_not_depend_on_the_table_layout():
    from pi3_slam_amd.dense_map import MapCleaner, VoxelFuser
    idx, w = _random_points(6000, 26, seed=3)
    keys, W = _voxels(idx, w)
    a = _fused(idx, w)
    p = np.random.default_rng(1).permutation(len(idx))
    b = _fused(idx[p], w[p])                                  # another claim order: other probe chains
    c = VoxelFuser(V, DEV)                                    # grown by reserve: rehashed into a larger table
    _fuse(c, idx[:500], w[:500])
    cap0 = c.capacity
    _fuse(c, idx[500:], w[500:])
    assert c.capacity > cap0 and c.capacity >= a.capacity
    d = VoxelFuser(V, DEV)
    d.reserve(8 * len(idx))                                   # a sparser table
    _fuse(d, idx, w)
    assert d.capacity > a.capacity
    outs = []
    for fz in (a, a, b, c, d):                                # `a` twice: two runs give the same bytes
        cl = MapCleaner(min_weight=2, min_support=5, min_component=25)
        _, st, rows = _check(fz, cl, keys, W)
        st.pop("sweeps")
        outs.append((st, {k: rows[k].tobytes() for k in ROWS}))
    assert 0 < outs[0][0]["after_components"] < outs[0][0]["after_support"] < outs[0][0]["eligible"] < len(keys)
    for o in outs[1:]:
        assert o == outs[0]


# ------------------------------------------------------------------------------------------------ 4. serpentine
def _serpentine(n, width=64):
    """A one-voxel-wide path folded in the plane z = 0: rows of `width` at y = 0, 2, 4, .. joined at alternating ends."""
    out, y, x, step = [], 0, 0, 1
    while len(out) < n:
        out.append((x, y, 0))
        if (x == width - 1 and step == 1) or (x == 0 and step == -1 and len(out) > 1):
            if len(out) < n:
                out.append((x, y + 1, 0))
            y, step = y + 2, -step
        else:
            x += step
    return np.array(out[:n], np.int64)


def test_serpentine_one_long_component():
    from pi3_slam_amd.dense_map import MapCleaner
    path = _serpentine(4096)
    assert len(np.unique(ref.pack(path))) == 4096
    other = np.array([(i, 0, 10) for i in range(50)], np.int64)
    idx = np.concatenate([path, other])
    w = np.ones(len(idx), np.int64)
    fz = _fused(idx, w)
    keys, W = _voxels(idx, w)
    cl = MapCleaner(min_component=100)
    exp, st, rows = _check(fz, cl, keys, W)
    is_path = np.isin(keys, ref.pack(path))
    assert np.all(exp["label"][is_path] == ref.pack(path).min()) and np.all(exp["size"][is_path] == 4096)
    assert np.all(exp["label"][~is_path] == ref.pack(other).min()) and np.all(exp["size"][~is_path] == 50)
    assert exp["support"][is_path].max() <= 4                # one voxel wide: a path, not a sheet
    assert np.array_equal(exp["keep"], is_path) and len(rows["keys"]) == 4096
    assert (st["components"], st["components_kept"], st["after_components"]) == (2, 1, 4096)
    # neighbour propagation alone needs about the path's length in sweeps; the host loop's bound is all that is asserted
    print(f"serpentine of 4096 voxels: {st['sweeps']} labelling sweeps")
    assert st["sweeps"] <= 4096 + 50 + 1 + cl.SWEEPS_PER_READ


# ------------------------------------------------------------------------------------------------ 5. end to end
def _scene_chunks(scene):
    chunks = []
    for c, (idx, w, cols, t) in enumerate(scene["chunks"]):
        G = torch.eye(4, dtype=torch.float64)
        G[:3, 3] = torch.from_numpy(t.astype(np.float64) * V)
        poses = torch.eye(4).repeat(2, 1, 1)
        poses[:, 0, 3] = torch.tensor([-2.0 + 1.5 * c, -1.25 + 1.5 * c])          # over the floor patch, at y = 0
        chunks.append({"dense_cloud": {"points": torch.from_numpy(((idx + 0.5) * V).astype(np.float32)),
                                       "colors": torch.from_numpy(cols), "weights": torch.from_numpy(w),
                                       "voxel_size": V, "conf_threshold": 0.5},
                       "_sim3_global": None if c == 0 else G, "camera_poses": poses,
                       "image_paths": [f"frame_{2 * c:03d}.png", f"frame_{2 * c + 1:03d}.png"]})
    return chunks


def _oracle_world(chunks):
    """The map's oracle over every chunk cloud moved by the product's sim3_apply (as tests/test_dense_map_gpu.py)."""
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import chunk_transform
    sets = []
    for d in chunks:
        cl = d["dense_cloud"]
        pts = cl["points"].to(DEV, torch.float32).contiguous().clone()
        ops.sim3_apply(chunk_transform(d).reshape(16).to(DEV).contiguous(), pts, None)
        sets.append((pts.cpu().numpy(), cl["colors"].numpy(), cl["weights"].numpy()))
    return map_ref.fuse_point_sets(sets, V)


def _ply(points, colors, path):
    from pi3_slam_amd.export import write_ply
    write_ply(points, np.asarray(colors, np.uint8), str(path))
    return open(path, "rb").read()


def _green(png):
    from PIL import Image
    im = np.asarray(Image.open(png).convert("RGB")).astype(int)
    return int(np.sum((im[..., 1] > 200) & (im[..., 0] < 50) & (im[..., 2] < 50)))


def test_end_to_end_cleaned_ply_and_renders(tmp_path, capsys):
    from pi3_slam_amd import export
    from pi3_slam_amd.dense_map import MapCleaner, fuse_chunks
    scene = ref.planted_scene()
    chunks = _scene_chunks(scene)
    world = _oracle_world(chunks)
    keys, W = ref.scene_world_voxels(scene)
    assert world["keys"].tobytes() == keys.tobytes() and np.array_equal(world["weights"].astype(np.uint64), W)

    # flags off: what the parent's code path writes (the same call without a cleaner)
    for name in ("off", "off2"):
        (tmp_path / name).mkdir()
    export.write_outputs(chunks, str(tmp_path / "off"), DEV, render_overview=True)
    export.write_outputs(chunks, str(tmp_path / "off2"), DEV, None, True, 1, 1.0)          # the parent's positional form
    off = open(tmp_path / "off" / "dense_points.ply", "rb").read()
    assert off == _ply(world["points"], world["colors"], tmp_path / "oracle_off.ply")
    assert off == open(tmp_path / "off2" / "dense_points.ply", "rb").read()
    assert open(tmp_path / "off" / "renders" / "overview.png", "rb").read() == \
        open(tmp_path / "off2" / "renders" / "overview.png", "rb").read()
    fused = fuse_chunks(chunks, DEV, voxel_size=V)
    assert fused.points.tobytes() == world["points"].tobytes()
    assert fused.weights.tobytes() == world["weights"].tobytes()
    assert _green(tmp_path / "off" / "renders" / "overview.png") > 0        # the strays show in the uncleaned map
    capsys.readouterr()

    # flags on
    (tmp_path / "on").mkdir()
    cleaner = MapCleaner.from_options(min_support=4, min_component=50)
    export.write_outputs(chunks, str(tmp_path / "on"), DEV, render_overview=True, dense_cleaner=cleaner)
    said = capsys.readouterr().out
    exp = ref.clean(keys, W, min_support=4, min_component=50)
    sel = exp["keep"]
    assert open(tmp_path / "on" / "dense_points.ply", "rb").read() == _ply(world["points"][sel], world["colors"][sel],
                                                                           tmp_path / "oracle_on.ply")
    st = {k: v for k, v in cleaner.last_stats.items() if k != "sweeps"}
    assert st == exp["stats"]
    line = [ln for ln in said.splitlines() if "Dense map cleaned:" in ln]
    assert len(line) == 1 and all(str(st[k]) in line[0] for k in ("voxels", "eligible", "after_support", "after_components"))
    kept = set(keys[sel].tolist())
    assert not kept & set(ref.pack(scene["strays"]).tolist())
    plane = scene["plane"]
    inner = plane[(np.abs(plane[:, 0] + 0.5) < 11) & (np.abs(plane[:, 2] + 0.5) < 11)]
    assert set(ref.pack(inner).tolist()) <= kept and len(kept) == 24 * 24 - 4
    assert _green(tmp_path / "on" / "renders" / "overview.png") == 0         # the renders draw the cleaned map
    assert os.path.exists(tmp_path / "on" / "renders" / "cameras.json")


def test_reconstruct_options_reach_write_outputs(tmp_path, monkeypatch):
    """OfflineReconstructor(dense_min_support=..) and Pi3SLAMOnline's save_dense_map hand their cleaner on."""
    from pi3_slam_amd import export
    from pi3_slam_amd.online import Pi3SLAMOnline
    scene = ref.planted_scene()
    chunks = _scene_chunks(scene)
    keys, W = ref.scene_world_voxels(scene)
    slam = Pi3SLAMOnline.__new__(Pi3SLAMOnline)               # the export methods need the chunks and the cleaner only
    slam.chunk_reconstructions, slam.device = chunks, torch.device(DEV)
    from pi3_slam_amd.dense_map import MapCleaner
    slam.dense_cleaner = MapCleaner.from_options(min_support=4, min_component=50)
    assert slam.save_dense_map(str(tmp_path / "online.ply")) == 24 * 24 - 4
    slam.save_renders(str(tmp_path / "renders"), every=None, overview=True)
    assert _green(tmp_path / "renders" / "overview.png") == 0
    slam.dense_cleaner = None
    assert slam.save_dense_map(str(tmp_path / "online_all.ply")) == len(keys)


# ------------------------------------------------------------------------------------------------ 6. masked extract
def test_extract_kept_with_all_ones_equals_extract():
    from pi3_slam_amd import ops
    from pi3_slam_amd.dense_map import sort_by_key
    idx, w = _random_points(6000, 26, seed=5)
    fz = _fused(idx, w)
    n = fz.bound
    a = ops.voxel_extract(fz.table, fz.stats, V, n)
    va = int(fz.stats[2].item())
    b = ops.voxel_extract(fz.table, fz.stats, V, n, keep=torch.ones(fz.capacity, dtype=torch.uint8, device=DEV))
    vb = int(fz.stats[2].item())
    assert va == vb == len(_voxels(idx, w)[0])
    sa = sort_by_key(*(t[:va].cpu().numpy() for t in a))
    sb = sort_by_key(*(t[:vb].cpu().numpy() for t in b))
    for k in ROWS:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    none = ops.voxel_extract(fz.table, fz.stats, V, n, keep=torch.zeros(fz.capacity, dtype=torch.uint8, device=DEV))
    assert int(fz.stats[2].item()) == 0 and int(fz.stats[3].item()) == 0 and len(none) == 4
