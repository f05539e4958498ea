"""pi3_slam_amd/export.py: the stage-2 output writers as free functions over chunk dicts (host only, no kernel)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

N_VIEWS, N_KP, W, H = 6, 8, 64, 48


def _chunk(seed: int, names) -> dict:
    from scipy.spatial.transform import Rotation
    g = torch.Generator().manual_seed(seed)
    poses = torch.eye(4).repeat(N_VIEWS, 1, 1)
    poses[:, :3, :3] = torch.from_numpy(Rotation.random(N_VIEWS, random_state=seed).as_matrix()).float()
    poses[:, :3, 3] = torch.randn(N_VIEWS, 3, generator=g)
    K = torch.tensor([[50.0, 0.0, W // 2], [0.0, 50.0, H // 2], [0.0, 0.0, 1.0]]).repeat(N_VIEWS, 1, 1)
    return {"points": torch.randn(N_VIEWS, N_KP, 3, generator=g).half(), "colors": torch.rand(N_VIEWS, N_KP, 3, generator=g),
            "keypoints": torch.rand(N_VIEWS, N_KP, 2, generator=g).half(), "masks": torch.ones(N_VIEWS, N_KP, 1, dtype=torch.bool),
            "conf": torch.randn(N_VIEWS, N_KP, 1, generator=g), "camera_poses": poses, "image_paths": names, "intrinsics": K,
            "original_width": W, "original_height": H, "camera_params": {"fx": torch.full((N_VIEWS,), 50.0)},
            "_chunk_frame": {"points": torch.zeros(1), "camera_poses": torch.zeros(1)}}


@pytest.fixture(scope="module")
def chunks():
    """Two chunks of 6 views x 8 keypoints; the last two views of the first are the first two of the second.  The names
    come in the three forms a DataLoader leaves them in: str, 1-list, 1-tuple."""
    a = ["/d/f0.png", ["/d/f1.png"], ("/d/f2.png",), "/d/f3.png", ["/d/f4.png"], ("/d/f5.png",)]
    b = [("/e/f4.png",), "f5.png", ["/d/f6.png"], ("/d/f7.png",), "/d/f8.png", ["/d/f9.png"]]
    return [_chunk(1, a), _chunk(2, b)]


def test_views_walk_and_first_occurrence(chunks, tmp_path):
    from pi3_slam_amd import export
    every, unique = list(export.all_views(chunks)), list(export.unique_views(chunks))
    assert [v.name for v in every] == [f"f{i}.png" for i in (0, 1, 2, 3, 4, 5, 4, 5, 6, 7, 8, 9)]
    assert [v.index for v in every] == list(range(6)) * 2 and every[6].chunk is chunks[1]
    assert [v.name for v in unique] == [f"f{i}.png" for i in range(10)]
    for v, i in ((unique[4], 4), (unique[5], 5)):           # the shared names keep the FIRST chunk's pose
        assert v.chunk is chunks[0] and np.array_equal(v.pose, chunks[0]["camera_poses"][i].double().numpy())
    assert not np.array_equal(unique[4].pose, chunks[1]["camera_poses"][0].double().numpy())
    export.write_outputs(chunks, str(tmp_path), device="cpu")
    tum = [ln for ln in open(tmp_path / "trajectory_tum.txt").read().splitlines() if not ln.startswith("#")]
    assert len(tum) == 10 and [ln.split()[0] for ln in tum] == [str(i) for i in range(10)]
    x4 = [float(t) for t in tum[4].split()[1:4]]
    assert np.allclose(x4, chunks[0]["camera_poses"][4, :3, 3].numpy(), atol=1e-6, rtol=0)
    header = open(tmp_path / "final_camera_poses.ply", "rb").read(200)
    assert b"element vertex 12\n" in header                 # every view, duplicates included
    assert b"element vertex %d\n" % (2 * N_VIEWS * N_KP) in open(tmp_path / "final_points.ply", "rb").read(200)


def test_collect_keys_are_sufficient_for_every_output(chunks, tmp_path):
    from pi3_slam_amd import export
    from pi3_slam_amd.dist import COLLECT_KEYS
    assert {"intrinsics", "original_width", "original_height", "camera_poses", "image_paths"} <= set(COLLECT_KEYS)
    cut = [{k: d[k] for k in COLLECT_KEYS if k in d} for d in chunks]
    assert all(set(c) < set(d) for c, d in zip(cut, chunks))             # the cut did drop something
    os.makedirs(tmp_path / "full"), os.makedirs(tmp_path / "cut")
    export.write_outputs(chunks, str(tmp_path / "full"), device="cpu")
    export.write_outputs(cut, str(tmp_path / "cut"), device="cpu")
    for name in ("final_points.ply", "final_camera_poses.ply", "trajectory_tum.txt"):
        full = open(tmp_path / "full" / name, "rb").read()
        assert len(full) > 100 and full == open(tmp_path / "cut" / name, "rb").read(), name
    assert sorted(os.listdir(tmp_path / "cut")) == sorted(os.listdir(tmp_path / "full")) == sorted(
        ["final_points.ply", "final_camera_poses.ply", "trajectory_tum.txt"])       # no dense cloud: no map, no renders
    va, vb = export.render_views(chunks), export.render_views(cut)
    assert len(va) == len(vb) == 10
    for a, b in zip(va, vb):
        assert a["name"] == b["name"] and (a["H"], a["W"]) == (b["H"], b["W"]) == (H, W)
        assert np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["K"], b["K"])
        assert a["K"][0, 2] == W // 2 - 0.5 and a["K"][1, 2] == H // 2 - 0.5        # index coordinates


def test_online_facade_does_not_build_a_reconstructor():
    import pi3_slam_amd.export
    import pi3_slam_amd.online
    online = inspect.getsource(pi3_slam_amd.online)
    assert "__new__" not in online and "_exporter" not in online
    src = inspect.getsource(pi3_slam_amd.export)
    assert not re.search(r"^\s*(from|import)\s+[\w.]*\b(reconstructor|online)\b", src, flags=re.M)
    assert not re.search(r"^\s*from\s+\S+\s+import\s.*\b(reconstructor|online)\b", src, flags=re.M)
