"""CPU: the numpy reference of the dense map's cleaning filters (tests/dense_clean_ref.py) against scipy.ndimage, an
independent implementation; MapCleaner's validation; the command line's flags and how they are handed through."""
import numpy as np
import pytest

import dense_clean_ref as ref


def _random_grid(seed, n=24, fill=0.3):
    rng = np.random.default_rng(seed)
    occ = rng.random((n, n, n)) < fill
    w = rng.integers(1, 6, (n, n, n))
    idx = np.argwhere(occ)
    perm = rng.permutation(len(idx))                  # the reference must not rely on the order of its input
    idx = idx[perm]
    return occ, w, idx, w[idx[:, 0], idx[:, 1], idx[:, 2]]


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("min_weight", [1, 3])
def test_reference_support_equals_scipy_correlate(R, min_weight):
    from scipy import ndimage
    occ, w, idx, wv = _random_grid(10 * R + min_weight)
    # the grid straddles the origin: indices -12 .. 11
    out = ref.clean(ref.pack(idx - 12), wv, min_weight=min_weight, support_radius=R)
    elig = occ & (w >= min_weight)
    k = 2 * R + 1
    exp = ndimage.correlate(elig.astype(np.int32), np.ones((k, k, k), np.int32), mode="constant", cval=0) - elig
    got = np.full(occ.shape, -1, np.int32)
    got[idx[:, 0], idx[:, 1], idx[:, 2]] = out["support"]
    assert np.array_equal(got[elig], exp[elig]) and np.all(got[~elig] == -1)
    assert np.array_equal(out["eligible"], elig[idx[:, 0], idx[:, 1], idx[:, 2]])
    assert out["stats"]["eligible"] == int(elig.sum()) and out["stats"]["voxels"] == len(idx)
    assert got[elig].max() > 3 * R and got[elig].min() < got[elig].max()


@pytest.mark.parametrize("min_weight,min_support,fill", [(1, 0, 0.3), (3, 0, 0.3), (1, 9, 0.3), (2, 3, 0.12)])
def test_reference_components_equal_scipy_label(min_weight, min_support, fill):
    from scipy import ndimage
    occ, w, idx, wv = _random_grid(100 + min_weight + min_support, fill=fill)
    out = ref.clean(ref.pack(idx - 12), wv, min_weight=min_weight, min_support=min_support, min_component=5)
    elig = occ & (w >= min_weight)
    sup = ndimage.correlate(elig.astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant", cval=0) - elig
    surv = elig & (sup >= min_support)
    lab, ncomp = ndimage.label(surv, structure=np.ones((3, 3, 3), int))
    sizes = np.bincount(lab.ravel())
    at = (idx[:, 0], idx[:, 1], idx[:, 2])
    assert np.array_equal(out["survivor"], surv[at])
    assert np.array_equal(out["size"][out["survivor"]], sizes[lab[at]][out["survivor"]])
    assert np.all(out["size"][~out["survivor"]] == 0) and np.all(out["label"][~out["survivor"]] == ref.NONE)
    # the same partition: one of our labels per scipy label and the other way round, and a label is the smallest key
    s = out["survivor"]
    pairs = np.unique(np.stack([out["label"][s], lab[at][s].astype(np.uint64)], 1), axis=0)
    assert len(pairs) == ncomp == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == out["stats"]["components"]
    keys = ref.pack(idx - 12)
    for l in np.unique(out["label"][s])[:50]:
        assert l == keys[s & (out["label"] == l)].min()
    assert np.array_equal(out["keep"], s & (out["size"] >= 5))
    assert out["stats"]["components_kept"] == int((sizes[1:] >= 5).sum())
    assert 0 < out["stats"]["after_components"] < out["stats"]["after_support"] or ncomp == 1


def test_reference_range_edge_has_no_wrapped_neighbours():
    top = (1 << 20) - 1
    idx = np.array([[top, 0, 0], [top - 1, 0, 0], [0, 0, -top], [0, 1, -top + 1],
                    [-top, top, 5], [-top, -top, 5]])          # the last two are neighbours only if y wraps
    out = ref.clean(ref.pack(idx), np.ones(len(idx)), min_support=1)
    assert out["support"].tolist() == [1, 1, 1, 1, 0, 0]
    assert out["keep"].tolist() == [True, True, True, True, False, False]
    assert np.array_equal(ref.unpack(ref.pack(idx)), idx)


def test_map_cleaner_validation():
    from pi3_slam_amd.dense_map import MapCleaner
    c = MapCleaner()
    assert c.settings() == {"min_weight": 1, "min_support": 0, "support_radius": 1, "min_component": 0}
    assert MapCleaner(2, 26, 1, 50).min_support == 26 and MapCleaner(1, 124, 2).min_support == 124
    assert MapCleaner(min_support=4.0).min_support == 4 and isinstance(MapCleaner(min_support=4.0).min_support, int)
    for kw, match in ((dict(support_radius=3), "support_radius"), (dict(support_radius=0), "support_radius"),
                      (dict(min_support=27), "min_support"), (dict(min_support=125, support_radius=2), "min_support"),
                      (dict(min_weight=-1), "min_weight"), (dict(min_support=-1), "min_support"),
                      (dict(min_component=-5), "min_component"), (dict(min_weight=1.5), "min_weight"),
                      (dict(min_component="3"), "min_component"), (dict(min_support=True), "min_support"),
                      (dict(min_component=1 << 32), "min_component")):
        with pytest.raises(ValueError, match=match):
            MapCleaner(**kw)


def test_defaults_construct_no_cleaner():
    from pi3_slam_amd.dense_map import MapCleaner
    assert MapCleaner.from_options() is None
    assert MapCleaner.from_options(support_radius=2) is None
    c = MapCleaner.from_options(min_support=4, min_component=50)
    assert c.settings() == {"min_weight": 1, "min_support": 4, "support_radius": 1, "min_component": 50}
    assert MapCleaner.from_options(min_weight=3, support_radius=2).settings() == {
        "min_weight": 3, "min_support": 0, "support_radius": 2, "min_component": 0}


def test_reconstruct_flags_reach_the_reconstructor(tmp_path, monkeypatch):
    from pi3_slam_amd import cli, reconstructor
    seen = {}

    class Fake:
        def __init__(self, **kw):
            seen.update(kw)

        def run(self):
            seen["ran"] = True

    monkeypatch.setattr(reconstructor, "OfflineReconstructor", Fake)
    base = ["reconstruct", "--chunks", str(tmp_path), "--output", str(tmp_path / "out")]
    cli.main(base)
    assert seen["ran"] and seen["dense_min_weight"] is None and seen["dense_min_support"] is None
    assert seen["dense_support_radius"] == 1 and seen["dense_min_component"] is None
    cli.main(base + ["--dense-min-weight", "2", "--dense-min-support", "4", "--dense-support-radius", "2",
                     "--dense-min-component", "50"])
    assert (seen["dense_min_weight"], seen["dense_min_support"], seen["dense_support_radius"],
            seen["dense_min_component"]) == (2, 4, 2, 50)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--dense-support-radius", "3"])


def test_offline_reconstructor_builds_the_cleaner_only_when_asked(tmp_path):
    from pi3_slam_amd.reconstructor import OfflineReconstructor
    kw = dict(chunk_dir=str(tmp_path), output_dir=str(tmp_path / "o"), device="cpu")
    assert OfflineReconstructor(**kw).dense_cleaner is None
    c = OfflineReconstructor(dense_min_support=4, dense_min_component=50, **kw).dense_cleaner
    assert c.settings() == {"min_weight": 1, "min_support": 4, "support_radius": 1, "min_component": 50}
    with pytest.raises(ValueError, match="min_support"):
        OfflineReconstructor(dense_min_support=30, **kw)


def test_online_flags_reach_the_facade(tmp_path, monkeypatch):
    from pi3_slam_amd import cli, online
    seen = {}

    class Stop(Exception):
        pass

    class Fake:
        def __init__(self, **kw):
            seen.update(kw)
            raise Stop

    monkeypatch.setattr(online, "Pi3SLAMOnline", Fake)
    (tmp_path / "a.png").write_bytes(b"")
    base = ["online", "--image_dir", str(tmp_path), "--output_path", str(tmp_path / "out")]
    with pytest.raises(Stop):
        cli.main(base)
    assert all(seen[k] is None for k in ("dense_min_weight", "dense_min_support", "dense_min_component"))
    assert seen["dense_support_radius"] == 1
    with pytest.raises(Stop):
        cli.main(base + ["--dense_min_weight", "3", "--dense_min_support", "5", "--dense_support_radius", "2",
                         "--dense_min_component", "80"])
    assert (seen["dense_min_weight"], seen["dense_min_support"], seen["dense_support_radius"],
            seen["dense_min_component"]) == (3, 5, 2, 80)


def test_help_texts_call_their_examples_starting_points():
    from pi3_slam_amd import cli
    for table in (cli.DENSE_MAP_FLAGS, cli.ONLINE_DENSE_FLAGS):     # the cleaner's three thresholds and the carver's
        helps = {f: kw["help"] for f, kw in table if "min" in f and "dense" in f and "views" not in f}
        assert len(helps) == 4 and sum("carve" in f for f in helps) == 1
        assert all("starting point" in h and "not a measured optimum" in h for h in helps.values())


def test_planted_scene_is_cleaned_by_the_reference_alone():
    """The end-to-end GPU test's scene: with its flags (min_support 4, min_component 50) the reference drops every
    planted stray and keeps ALL floor voxels that have their full neighbourhood; a minimum weight alone cannot."""
    scene = ref.planted_scene()
    keys, W = ref.scene_world_voxels(scene)
    assert len(keys) == 24 * 24 + len(scene["strays"])
    out = ref.clean(keys, W, min_support=4, min_component=50)
    kept = set(keys[out["keep"]].tolist())
    assert not kept & set(ref.pack(scene["strays"]).tolist())
    plane = scene["plane"]
    inner = plane[(np.abs(plane[:, 0] + 0.5) < 11) & (np.abs(plane[:, 2] + 0.5) < 11)]
    assert len(inner) == 22 * 22 and set(ref.pack(inner).tolist()) <= kept
    assert len(kept) == 24 * 24 - 4                       # the four corners have 3 neighbours
    # stage A alone leaves the blob (7 neighbours each), stage B alone leaves nothing out but it; weight 2 leaves a stray
    a = ref.clean(keys, W, min_support=4)
    assert a["stats"]["after_support"] == 24 * 24 - 4 + 8
    w2 = ref.clean(keys, W, min_weight=2)
    assert set(keys[w2["keep"]].tolist()) & set(ref.pack(scene["strays"]).tolist())
