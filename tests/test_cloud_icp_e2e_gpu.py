"""creator -> reconstruct -> evaluate-map --icp plane on the small synthetic room: the alignment by the trajectory pair,
then refined on the geometry.  The reference cloud has no normals, so the refinement uses dense_points.ply's own
(normals_of = 2).  The scores are printed, not bounded (DESIGN.md 7d records them)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import test_dense_carve_gpu as carve_gpu                # noqa: E402  (_reconstruct)
import test_dense_consistency_gpu as cons_gpu           # noqa: E402  (_items)
import test_map_eval_gpu as eval_gpu                    # noqa: E402  (the shape of its end-to-end test)

pytestmark = pytest.mark.gpu
DEV = eval_gpu.DEV


def _create_with_normals(seq, out_dir):
    """test_map_eval_gpu._create with --dense-normals: dense_points.ply then carries nx ny nz."""
    import synth_sequence as ss
    from pi3_slam_amd.chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    cfg = OfflineCreatorConfig(model_path="recipe", output_dir=out_dir, chunk_length=seq.chunk_length, overlap=seq.overlap,
                               device=DEV, do_metric_depth=False, keypoint_type="grid", max_num_keypoints=seq.max_kp,
                               estimate_camera_params=True, num_loader_workers=0, dense_voxel_size=eval_gpu.VOXEL,
                               dense_normals=True)
    cr = OfflineChunkCreator(cfg, model=ss.SceneEngine(seq))
    cr.target_size = (seq.H, seq.W)
    _, manifest, _ = cr.write_chunks(cr.process_chunks(cons_gpu._items(seq, cr.device, range(len(seq.chunks)))))
    cr.write_run_metadata(manifest)


def _finite(x):
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_finite(v) for v in x)
    return x is None or isinstance(x, (str, bool)) or np.isfinite(x)


@pytest.mark.parametrize("noise", ["NOISE_NONE", "NOISE_BF16"])
def test_evaluate_map_with_icp_end_to_end(noise, tmp_path, capsys):
    import synth_sequence as ss
    from pi3_slam_amd import cli, map_eval
    from pi3_slam_amd.export import write_ply
    seq = ss.SyntheticSequence(eval_gpu.GT, H=eval_gpu.H, W=eval_gpu.W, chunk_length=eval_gpu.CHUNK, overlap=eval_gpu.OVERLAP,
                               n_frames=eval_gpu.FRAMES, max_kp=100, noise=dict(getattr(ss, noise)))
    _create_with_normals(seq, str(tmp_path / "chunks"))
    carve_gpu._reconstruct(str(tmp_path / "chunks"), str(tmp_path / "rec"))
    est_ply, est_tum = str(tmp_path / "rec" / "dense_points.ply"), str(tmp_path / "rec" / "trajectory_tum.txt")
    ref_ply, saved = str(tmp_path / "reference.ply"), str(tmp_path / "refined.txt")
    cloud = seq.reference_cloud().numpy()
    write_ply(cloud, np.full((len(cloud), 3), 200, np.uint8), ref_ply)
    assert map_eval.read_ply_vertices(est_ply)["normals"] is not None and map_eval.read_ply_vertices(ref_ply)["normals"] is None
    base = ["evaluate-map", "--estimate", est_ply, "--reference", ref_ply, "--thresholds"] + [str(t) for t in eval_gpu.THRESHOLDS] + \
           ["--max-dist", str(eval_gpu.MAX_DIST), "--voxel-size", str(eval_gpu.EVAL_VOXEL), "--device", DEV]
    pair = ["--estimate-trajectory", est_tum, "--reference-trajectory", eval_gpu.GT]
    capsys.readouterr()

    def said(argv):
        cli.main(argv + ["--json"])
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == 1
        return json.loads(lines[0])

    plain = said(base + pair)
    refined = said(base + pair + ["--icp", "plane", "--save-transform", saved])
    assert "icp" not in plain and refined["icp"]["status"] in ("converged", "max_iterations")
    assert _finite(refined) and np.isfinite(np.array(refined["icp"]["transform"])).all()
    assert refined["settings"]["transform"] == refined["icp"]["transform"]
    assert np.array_equal(map_eval.read_transform(saved), np.array(refined["icp"]["transform"]))
    again = said(base + ["--transform", saved])                                       # the saved matrix, no --icp
    for k in ("points", "dropped", "accuracy", "completeness", "precision", "recall", "fscore", "settings"):
        assert again[k] == refined[k], k
    cli.main(base + pair + ["--icp", "plane"])
    table = capsys.readouterr().out
    assert table.strip().splitlines()[-1].startswith(f"icp: {refined['icp']['status']} after")
    for name, res in (("trajectory pair", plain), ("+ --icp plane", refined)):
        print(f"{noise} / {name}: " + ", ".join(f"F @ {t} = {res['fscore'][map_eval.tau_key(t)]:.4f}" for t in eval_gpu.THRESHOLDS)
              + f", accuracy {res['accuracy']['mean']}, completeness {res['completeness']['mean']}")
    print(table)
