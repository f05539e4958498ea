"""Command line of the MI355X path.  Sub-commands that take the flags of the reference's two offline scripts
(create_offline_chunks.py:44-62, reconstruct_offline.py:21-29) and of its online script
(pi3_slam_online_modular.py:117-183, without the viser window), declared as tables below, plus this build's own:

  python -m pi3_slam_amd.cli create --images /data/seq --output /data/seq_chunks --chunk-length 100 --overlap 20 \\
         --model-path /ckpt/pi3 [--moge-model-path model.pt] [--cam-dist-path calib.json] [--device-resize] [--hip-graph]
  python -m pi3_slam_amd.cli reconstruct --chunks /data/seq_chunks --output /data/seq_chunks/reconstruction

  python -m pi3_slam_amd.cli online --image_dir /data/seq --output_path /data/seq_result --chunk_length 100 --overlap 20 \
         --model_path /ckpt/pi3 --save_tum [--cam_dist_path calib.json] [--use_inverse_depth]
  python -m pi3_slam_amd.cli route --occupancy OUT/occupancy.npz --output DIR --from-trajectory OUT/trajectory_tum.txt \\
         [--goal X Y Z [--taut [--taut-span 256]]] [--radius 0.2]
  python -m pi3_slam_amd.cli frontiers --occupancy OUT/occupancy.npz --output DIR --from-trajectory OUT/trajectory_tum.txt \\
         [--radius 0.2] [--min-cells 20] [--route-to 0 [--taut]]
  python -m pi3_slam_amd.cli views --occupancy OUT/occupancy.npz --output DIR --from-trajectory OUT/trajectory_tum.txt \\
         [--radius 0.2] [--range 1.0 [--far]] [--unknown-depth K] [--fov 90] [--stride 4] [--count 10] [--route-to 0] \\
         [--frustum HFOV VFOV [--yaw-steps 8] [--pitch DEG ...] [--up 0 -1 0] [--portrait] [--view-image-width 640]] \\
         [--cover [--cover-until 0.9]] [--tour [--tour-from X Y Z]] [--taut [--taut-span 256]]

Under `python -m torch.distributed.run --nproc-per-node G -m pi3_slam_amd.cli ...` every stage shards over the G GPUs.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

# (flag, kwargs) - names, types and defaults follow the reference scripts; REQ marks what has a personal default path there
REQ = dict(required=True)
CREATE_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--images", dict(REQ, help="folder of images, glob pattern, or text file with one path per line")),
    ("--output", dict(REQ, help="output directory (chunks/, chunks_manifest.json, chunk_metadata.json)")),
    ("--model-path", dict(default="recipe", help="local Pi3 checkpoint; 'recipe' = synthetic weights (no network)")),
    ("--chunk-length", dict(type=int, default=50)),
    ("--overlap", dict(type=int, default=5)),
    ("--device", dict(default="cuda")),
    ("--cam-dist-path", dict(default=None, help="camera calibration JSON: undistort the frames first")),
    ("--keypoints", dict(default="grid", choices=("aliked", "grid", "none"))),
    ("--max-kp", dict(type=int, default=200)),
    ("--kp-threshold", dict(type=float, default=0.005)),
    ("--num-workers", dict(type=int, default=4)),
    ("--skip-start", dict(type=int, default=0, help="frames to drop at the beginning")),
    ("--skip-end", dict(type=int, default=0, help="frames to drop at the end")),
    # this build's additions
    ("--moge-model-path", dict(default=None, help="local MoGe-2 model.pt; 'recipe' = synthetic weights")),
    ("--keypoint-seed", dict(type=int, default=0, help="seed of the grid subsampling, -1 = unseeded")),
)
CREATE_SWITCHES = (("--device-resize", "Resize + ToTensor on the GPU (loader workers decode only)"),
                   ("--hip-graph", "replay the per-chunk forward as one captured hipGraph"),
                   ("--reuse-overlap-encoder", "overlap frames take their encoder output from the previous chunk "
                                               "(bit-identical; single-GPU streams)"))
# The dense map's flags, declared once, spelled with hyphens.  The chunk stage (dense_map.ChunkCloudBuilder) belongs to
# `create`, the map stage (dense_map.fuse_chunks: MapCarver, MapCleaner, MapMesher) to `reconstruct`; `online` runs both
# and takes both tables through underscored().
SWITCH = dict(action="store_true")
DENSE_CHUNK_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--dense-voxel-size", dict(type=float, default=None, help="also fuse each chunk's dense pointmap into voxels of this "
                                                               "edge length (metres): chunk['dense_cloud']")),
    ("--dense-conf-threshold", dict(type=float, default=0.5, help="pixels with sigmoid(conf) above this enter the dense map")),
    ("--dense-min-views", dict(type=int, default=None, help="with --dense-voxel-size: keep a pixel only when this many "
                                                            "neighbouring frames of its chunk agree with its depth")),
    ("--dense-view-radius", dict(type=int, default=3, help="neighbours i +- s * stride, s = 1..radius (1..16)")),
    ("--dense-view-stride", dict(type=int, default=2, help="frame step between the neighbours")),
    ("--dense-depth-tolerance", dict(type=float, default=0.03, help="relative depth difference that still agrees")),
    ("--dense-depth-every", dict(type=int, default=None, help="with --dense-voxel-size: every chunk keeps the depth of "
                                                              "every K-th frame (chunk['dense_depth'], fp16) so that "
                                                              "--dense-carve-min-conflicts can carve the fused map with "
                                                              "the views of every chunk")),
    ("--dense-depth-stride", dict(type=int, default=2, choices=(1, 2, 4), help="those depth planes keep every S-th row "
                                                                               "and column")),
    ("--dense-normals", dict(SWITCH, help="with --dense-voxel-size: every voxel of the dense cloud also gets a surface "
                                          "normal facing the cameras that saw it (dense_points.ply with nx ny nz, "
                                          "normal / shaded images under renders/)")),
)
DENSE_MAP_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--dense-min-weight", dict(type=int, default=None, help="dense map: drop voxels whose fused weight is below N "
                                                             "(from dense_points.ply and the renders; e.g. 2 as a "
                                                             "starting point, not a measured optimum)")),
    ("--dense-min-support", dict(type=int, default=None, help="dense map: drop voxels with fewer than N occupied cells "
                                                              "among their neighbours (26 at radius 1; e.g. 4 as a "
                                                              "starting point, not a measured optimum)")),
    ("--dense-support-radius", dict(type=int, default=1, choices=(1, 2), help="neighbourhood of --dense-min-support "
                                                                               "in voxels: 26 or 124 cells")),
    ("--dense-min-component", dict(type=int, default=None, help="dense map: then drop 26-connected components of fewer "
                                                                "than N voxels (e.g. 50 as a starting point, not a "
                                                                "measured optimum)")),
    ("--dense-carve-min-conflicts", dict(type=int, default=None, help="dense map: first drop the voxels that at least N "
                                                                      "depth keyframes of any chunk looked through, "
                                                                      "and more than agree with them (needs chunks "
                                                                      "created with --dense-depth-every; use with "
                                                                      "--no-bundle-adjust; e.g. 3 as a starting point, "
                                                                      "not a measured optimum)")),
    ("--dense-carve-tolerance", dict(type=float, default=0.03, help="relative depth difference (plus one voxel size) "
                                                                    "within which a keyframe agrees with a voxel")),
    ("--dense-mesh", dict(SWITCH, help="write dense_mesh.ply: a triangle mesh of the fused dense map (surface nets on its "
                                       "voxel lattice; the chunks must have been created with --dense-voxel-size and "
                                       "--dense-normals)")),
    # the occupancy grid (dense_map.MapOccupancy); the defaults are starting points, not measured optima
    ("--occupancy-cell", dict(type=float, default=None, help="write occupancy.npz: the occupied / free / unknown grid of "
                              "cells of this edge length (metres) around the dense map; a cell is free when enough depth "
                              "keyframes looked through it (needs chunks created with --dense-voxel-size and "
                              "--dense-depth-every; the keyframes sit where their chunk's similarity puts them: with "
                              "bundle adjustment on use --map-follow-poses, or --no-bundle-adjust)")),
    ("--occupancy-min-free-views", dict(type=int, default=2, help="keyframes that must have looked through a cell, and "
                                        "more than measured a surface in it (2 is a starting point, not a measured "
                                        "optimum)")),
    ("--occupancy-tolerance", dict(type=float, default=0.03, help="relative depth difference (plus one cell) within "
                                   "which a keyframe measured a surface in a cell (a starting point, not a measured "
                                   "optimum)")),
    ("--occupancy-clearance", dict(type=float, default=None, help="also the clearance field: the exact distance "
                                   "(metres) from every cell to the nearest occupied cell, up to this many metres "
                                   "(inf beyond; at most 255 cells)")),
    ("--occupancy-unknown-obstacle", dict(SWITCH, help="unknown cells are obstacles of the clearance field too")),
    ("--occupancy-max-cells", dict(type=int, default=1 << 27, help="refuse a grid of more cells than this (the message "
                                   "names the cell size that fits)")),
)


def option_names(table: Sequence[Tuple[str, Dict]]) -> Tuple[str, ...]:
    """The attributes a flag table's arguments parse into: --dense-min-views or --dense_min_views -> dense_min_views."""
    return tuple(flag[2:].replace("-", "_") for flag, _ in table)


def underscored(table: Sequence[Tuple[str, Dict]]) -> Tuple[Tuple[str, Dict], ...]:
    """A flag table in `online`'s spelling: --dense-min-views -> --dense_min_views, in the flags themselves and wherever
    a help text names one."""
    def respell(flag: str) -> str:
        return "--" + flag[2:].replace("-", "_")

    def respell_text(text: str) -> str:
        return re.sub(r"--[a-z]+(?:-[a-z]+)+", lambda m: respell(m.group(0)), text)
    return tuple((respell(flag), dict(kw, help=respell_text(kw["help"]))) for flag, kw in table)


RECON_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--chunks", dict(REQ, help="directory holding chunks/chunk_*.pt and chunk_metadata.json")),
    ("--output", dict(REQ, help="directory for trajectory_tum.txt and the ply files")),
    ("--chunk-length", dict(type=int, default=None)),
    ("--overlap", dict(type=int, default=None)),
    ("--max-observations-per-track", dict(type=int, default=5)),
    ("--device", dict(default="cuda")),
    # this build's additions
    ("--render-every", dict(type=int, default=None, help="write renders/depth_<frame>.png (16 bit, millimetres) and "
                                                         "color_<frame>.png of the dense map for every N-th view")),
    ("--render-min-weight", dict(type=int, default=1, help="voxels below this fused weight are not drawn")),
    ("--render-splat-scale", dict(type=float, default=1.0, help="half-width of a drawn voxel in voxel sizes")),
    ("--map-follow-tolerance", dict(type=float, default=0.03, help="with --map-follow-poses: relative depth difference "
                                                                   "(plus one voxel size) within which a keyframe saw a "
                                                                   "point of its chunk's cloud")),
)
MAP_FOLLOW_SWITCH = ("--map-follow-poses", "the dense map follows the bundle-adjusted poses: every point of a chunk's cloud "
                                           "moves with the depth keyframes of its chunk that saw it, each from the pose it "
                                           "was created with to its final pose (needs chunks created with "
                                           "--dense-depth-every; chunks without keyframes keep their similarity)")
# loop closure (loop_closure.close_loops); the defaults are starting points, not measured optima
LOOP_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--loop-min-gap", dict(type=int, default=2, help="with --loop-closure: chunks i and j are a candidate from j - i >= this")),
    ("--loop-min-overlap", dict(type=float, default=0.3, help="cells both chunks occupy / cells of the smaller one, at least")),
    ("--loop-max-edges", dict(type=int, default=3, help="loop edges per chunk, the best overlaps first")),
    ("--loop-max-dist", dict(type=float, default=0.1, help="ICP search radius in world units: the drift a loop may close")),
    ("--loop-max-rms", dict(type=float, default=0.03, help="an edge is accepted up to this ICP rms (world units)")),
    ("--loop-min-pair-fraction", dict(type=float, default=0.2, help="and from this share of the smaller cloud in ICP pairs")),
    ("--loop-cell", dict(type=float, default=0.16, help="edge of the co-occupancy cells (world units)")),
)
LOOP_SWITCH = ("--loop-closure", "close loops before the outputs are written: chunks that see the same surface (co-occupancy "
                                 "of their dense clouds) are aligned by ICP and a Sim(3) pose graph spreads the chain's "
                                 "error over the loops (needs chunks created with --dense-voxel-size; writes "
                                 "loop_closure.json)")
RECON_SWITCHES = (("--save-per-chunk", "per-chunk ply files as well"),
                  ("--render-overview", "write renders/overview.png: the dense map from above with the trajectory in red"),
                  ("--use-inverse-depth", "one inverse depth per track along its reference keypoint's ray in both bundle "
                                         "adjustments (utils/chunk_reconstruction.py:187-204; pi3_bundle_adjust_inverse_depth)"),
                  ("--save-observations", "also write the projected track observations"),
                  ("--no-bundle-adjust", "closed-form Sim(3) chain only: skip the per-chunk and the prior-constrained "
                                         "bundle adjustment (utils/chunk_reconstruction.py:188-219, "
                                         "utils/reconstruction_alignment.py:107-171)"),
                  ("--no-ba-sanity-gate", "apply every bundle adjustment that ends without a numerical failure, as the "
                                          "reference does (default: keep the input when fewer than 3 tracks survive or a "
                                          "camera moved by more than the scene extent)"),
                  MAP_FOLLOW_SWITCH, LOOP_SWITCH)


# pi3_slam_online_modular.py:117-183: same names (underscores), types and defaults; the reference's personal default paths
# become required arguments, the three viser flags are accepted and ignored (no window in this build)
ONLINE_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--image_dir", dict(default=None, help="directory containing images")),
    ("--video_path", dict(default=None, help="video file (not supported here: no decoder in this image)")),
    ("--start_frame", dict(type=int, default=0)),
    ("--end_frame", dict(type=int, default=None)),
    ("--skip_start", dict(type=int, default=0, help="frames to drop at the beginning")),
    ("--skip_end", dict(type=int, default=0, help="frames to drop at the end")),
    ("--model_path", dict(default="recipe", help="local Pi3 checkpoint; 'recipe' = synthetic weights (no network)")),
    ("--device", dict(default="cuda")),
    ("--chunk_length", dict(type=int, default=30)),
    ("--overlap", dict(type=int, default=5)),
    ("--conf_threshold", dict(type=float, default=0.5)),
    ("--cam_scale", dict(type=float, default=1.0)),
    ("--cam_dist_path", dict(default=None, help="camera calibration JSON: undistort the frames first")),
    ("--keypoint_type", dict(default="grid")),
    ("--max_num_keypoints", dict(type=int, default=200)),
    ("--keypoint_detection_threshold", dict(type=float, default=0.005)),
    ("--max_observations_per_track", dict(type=int, default=6)),
    ("--viz_port", dict(type=int, default=8080, help="ignored: no visualisation window in this build")),
    ("--output_path", dict(REQ, help="directory (or .ply file) for trajectory.ply / trajectory.tum")),
    ("--max_points", dict(type=int, default=1000000)),
    # this build's additions
    ("--moge_model_path", dict(default=None, help="local MoGe-2 model.pt; 'recipe' = synthetic weights")),
    ("--num_workers", dict(type=int, default=4, help="decode threads")),
    ("--dense_voxel_size", dict(type=float, default=None, help="write dense_points.ply: the dense maps filtered by "
                                                               "--conf_threshold, fused into voxels of this size (metres)")),
    ("--render_every", dict(type=int, default=None, help="with --dense_voxel_size: renders/ with depth and colour images "
                                                         "of the dense map for every N-th view and an overview")),
)
# both dense stages; --dense_voxel_size has its text above (here it writes dense_points.ply) and --conf_threshold is the
# pixel test's threshold
ONLINE_DENSE_FLAGS = underscored([row for row in tuple(DENSE_CHUNK_FLAGS) + tuple(DENSE_MAP_FLAGS)
                                  if row[0] not in ("--dense-voxel-size", "--dense-conf-threshold")])
# the two map-follow options of reconstruct, respelled
ONLINE_FOLLOW_FLAGS = underscored([row for row in RECON_FLAGS if row[0] == "--map-follow-tolerance"])
ONLINE_FOLLOW_SWITCH = underscored([(MAP_FOLLOW_SWITCH[0], dict(help=MAP_FOLLOW_SWITCH[1]))])[0]
ONLINE_SWITCHES = (("--save_chunk_reconstructions", "save each chunk reconstruction to disk"),
                   ("--save_transformed_reconstructions", "save transformed reconstructions as PLY files"),
                   ("--save_debug_reconstructions", "accepted for compatibility"),
                   ("--save_debug_projections", "accepted for compatibility"),
                   ("--use_inverse_depth", "inverse-depth parametrization in both bundle adjustments"),
                   ("--no_visualization", "accepted for compatibility (there is never a window)"),
                   ("--keep_viz_open", "accepted for compatibility"),
                   ("--save_tum", "save the trajectory in TUM format"),
                   ("--tum_integer_timestamp", "integer timestamps in the TUM file (7-Scenes)"),
                   ("--no_bundle_adjust", "closed-form Sim(3) chain only"),
                   ("--no_hip_graph", "plain kernel launches instead of the captured per-chunk graph"),
                   ("--reuse_overlap_encoder", "overlap frames take their encoder output from the previous chunk"),
                   (ONLINE_FOLLOW_SWITCH[0], ONLINE_FOLLOW_SWITCH[1]["help"]))

# evaluate-map: this build's own sub-command (map_eval.py), no counterpart in the reference
EVAL_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--estimate", dict(REQ, help="the map to score: dense_points.ply, or dense_mesh.ply (its vertices; its surface "
                                  "with --mesh-surface)")),
    ("--reference", dict(REQ, help="the reference cloud or mesh (PLY)")),
    ("--thresholds", dict(REQ, type=float, nargs="+", help="distances at which precision / recall / F-score are taken")),
    ("--max-dist", dict(type=float, default=None, help="search radius; farther points count as beyond "
                                                       "(default: twice the largest threshold)")),
    ("--voxel-size", dict(type=float, default=None, help="first resample both clouds to one point per voxel of this "
                                                         "size, so dense regions do not outweigh sparse ones")),
    ("--transform", dict(default=None, help="text file with a 4x4 similarity (16 numbers, row-major) applied to the "
                                            "estimate")),
    ("--estimate-trajectory", dict(default=None, help="TUM trajectory of the estimate: with --reference-trajectory the "
                                                      "estimate is aligned as `tools/eval_ape.py` aligns it (Sim(3) "
                                                      "Umeyama over associated stamps)")),
    ("--reference-trajectory", dict(default=None, help="TUM trajectory of the reference")),
    ("--error-ply", dict(default=None, help="write the (resampled, transformed) estimate coloured by its distance to "
                                            "the reference: green 0, red max-dist, magenta beyond (with --mesh-surface "
                                            "and a mesh estimate: its surface samples)")),
    ("--icp", dict(default=None, choices=("point", "plane"), help="refine the alignment by ICP on the (resampled) clouds "
                   "before scoring: point to point, or point to plane (the reference's nx ny nz when its PLY has them, "
                   "otherwise the estimate's); default: off")),
    ("--icp-iterations", dict(type=int, default=30, help="with --icp: the iteration limit")),
    ("--icp-max-dist", dict(type=float, default=None, help="with --icp: pairs farther apart take no part "
                                                           "(default: the search's --max-dist)")),
    ("--save-transform", dict(default=None, help="write the similarity that was applied to the estimate (after --icp: "
                                                 "the refined one) in the form --transform reads")),
    ("--mesh-sample-spacing", dict(type=float, default=None, help="with --mesh-surface: one surface sample per this "
                                   "length squared of area (default: --voxel-size, otherwise half the smallest threshold)")),
    ("--mesh-sample-seed", dict(type=int, default=0, help="with --mesh-surface: the seed of the surface samples")),
    ("--device", dict(default="cuda")),
)
EVAL_SWITCHES = (("--json", "print the result as one JSON line instead of the table"),
                 ("--icp-scale", "with --icp: refine the scale too (a similarity instead of a rigid motion)"),
                 ("--mesh-surface", "score every input that has faces by its surface: area-weighted samples as queries, "
                                    "exact point-to-triangle distance as target (default: by its vertices)"))


# --taut on route, frontiers --route-to and views --route-to / --tour: the way pulled straight by line of sight
TAUT_FLAG = ("--taut-span", dict(type=int, default=256, metavar="N",
                                 help="with --taut: two consecutive vertices of the taut way lie at most N trace cells "
                                      "apart, 1 .. 4096 (default 256: a first guess that no measurement has tuned)"))
TAUT_SWITCH = ("--taut", "also every way pulled taut: the shortest polyline over cells of the way's own trace whose "
                         "consecutive vertices see each other (route.json's and tour.json's taut_* keys, route_taut.ply)")


def check_taut(a: argparse.Namespace, name: str, needs: str, given: bool) -> None:
    if a.taut and not given:
        raise SystemExit(f"{name}: --taut needs {needs}")
    if a.taut and not 1 <= a.taut_span <= 4096:
        raise SystemExit(f"{name}: --taut-span is 1 .. 4096 trace cells, got {a.taut_span}")


def taut_text(taut) -> str:
    text = f"; taut {taut.length_m:.3f} m over {len(taut.waypoints)} vertices"
    if taut.min_clearance_m is not None:
        text += f", clearance >= {taut.min_clearance_m:.3f} m"
    return text


# a body that stands (grid_route.GridRouter's stand and up): route, frontiers and views
STAND_FLAG = ("--stand", dict(type=float, nargs=2, default=None, metavar=("LO", "HI"),
                              help="plan for a body that stands: a cell is traversable only when it also lies LO .. HI "
                                   "metres (ceil(LO / cell) .. floor(HI / cell) cells, centre to centre) above an occupied "
                                   "cell along --up, with nothing but passable cells in between; the carrying height of the "
                                   "camera (default: none, a sphere that flies)"))
UP_FLAG = ("--up", dict(type=int, nargs=3, default=[0, -1, 0], metavar=("X", "Y", "Z"),
                        help="with --stand: the world's up, one of the six signed axes.  A convention, not a measurement: "
                             "the world is the first camera's frame, whose y points down (default 0 -1 0)"))


def stand_text(counts: Dict, settings: Dict) -> str:
    """The summary line's part about the band; nothing without --stand."""
    band = settings.get("stand_cells")
    return "" if band is None else f"; standing {band[0]} .. {band[1]} cells above a floor ({counts['off_band']} cells off the band)"


# route: this build's own sub-command (grid_route.py) on the occupancy.npz of reconstruct or online
ROUTE_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--occupancy", dict(REQ, help="occupancy.npz of `reconstruct` or `online` (--occupancy-cell)")),
    ("--output", dict(REQ, help="directory for route.npz and, with --goal, route.json and route.ply")),
    ("--start", dict(type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="the source: one world point")),
    ("--from-trajectory", dict(default=None, help="the sources: the position of every pose of this TUM trajectory "
                                                  "(poses on cells that are not traversable are skipped and counted)")),
    ("--goal", dict(type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="also the shortest safe way to this "
                                                                                   "world point")),
    ("--radius", dict(type=float, default=0.0, help="the body's radius in metres: only cells with at least this "
                                                    "clearance are traversable (default 0: every free cell)")),
    STAND_FLAG,
    UP_FLAG,
    TAUT_FLAG,
    ("--device", dict(default="cuda")),
)
ROUTE_SWITCHES = (TAUT_SWITCH, ("--through-unknown", "unknown cells are traversable too, and no obstacles of the clearance "
                                        "(default: only verified free space, kept away from unknown space)"),
                  ("--approach-unknown", "only free cells are traversable, but --radius is kept from occupied cells alone: "
                                         "the body may come up to the edge of unknown space, as a goal of `frontiers` "
                                         "needs (not with --through-unknown)"))


# frontiers: this build's own sub-command (frontier.py) on the same file
FRONTIER_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--occupancy", dict(REQ, help="occupancy.npz of `reconstruct` or `online` (--occupancy-cell)")),
    ("--output", dict(REQ, help="directory for frontiers.json, frontiers.npz and frontiers.ply and, with --route-to, "
                                "route.json, route.ply and route.npz")),
    ("--start", dict(type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="rank the clusters by the route "
                                                                                    "from this world point")),
    ("--from-trajectory", dict(default=None, help="rank the clusters by the route from the nearest pose of this TUM "
                                                  "trajectory (poses on cells that are not traversable are skipped and "
                                                  "counted); without a source the clusters are ordered by size")),
    ("--radius", dict(type=float, default=0.0, help="the body's radius in metres for that route, kept from occupied "
                                                    "cells only (default 0: every free cell)")),
    ("--min-cells", dict(type=int, default=1, help="drop clusters of fewer frontier cells (default 1: none; a few tens "
                                                   "hide single-cell holes of the vote: a starting point, not a "
                                                   "measured optimum)")),
    ("--route-to", dict(type=int, default=None, metavar="RANK", help="also the way to the goal of the cluster of this "
                                                                     "rank (0 = the nearest), as `route` writes it")),
    STAND_FLAG,
    UP_FLAG,
    TAUT_FLAG,
    ("--device", dict(default="cuda")),
)


# views: this build's own sub-command (view_planner.py) on the same file
class _Given(argparse.Action):
    """Stores the value and notes that the flag was given (`<dest>_given`): a default cannot tell."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


VIEW_FLAGS: Sequence[Tuple[str, Dict]] = (
    ("--occupancy", dict(REQ, help="occupancy.npz of `reconstruct` or `online` (--occupancy-cell)")),
    ("--output", dict(REQ, help="directory for views.json, views.npz and views.ply and, with --route-to, route.json, "
                                "route.ply and route.npz, with --tour, tour.json, tour.npz and tour.ply")),
    ("--start", dict(type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="the source: one world point")),
    ("--from-trajectory", dict(default=None, help="the sources: the position of every pose of this TUM trajectory "
                                                  "(poses on cells that are not traversable are skipped and counted)")),
    ("--radius", dict(type=float, default=0.0, help="the body's radius in metres for the route, kept from occupied "
                                                    "cells only (default 0: every free cell)")),
    ("--range", dict(type=float, default=1.0, help="how far a view sees, in metres; at most 32 occupancy cells, 64 with --far "
                                                   "(default 1.0: a starting point, not a measured optimum)")),
    ("--unknown-depth", dict(type=int, default=None, metavar="K",
                             help="a ray ends once more than K unknown cells, 0 .. 255, lie between the pose and its "
                                  "target, so a view counts the first layers of a block of unknown space and not the "
                                  "whole block (default: none, unknown cells are transparent; whatever K you pick is where "
                                  "to start, no measured optimum, and 110 or more is the transparent rule)")),
    ("--fov", dict(type=float, default=90.0, action=_Given, help="the full opening angle of the viewing cone in degrees, in (0, 180] "
                                                  "(default 90: a starting point, not a measured optimum; not with "
                                                  "--frustum)")),
    ("--frustum", dict(type=float, nargs=2, default=None, metavar=("HFOV", "VFOV"),
                       help="views through the camera that will be carried instead of cones: its horizontal and vertical "
                            "field of view in degrees, each in [2, 170] (90 67.5 is a 4:3 frame).  The headings are "
                            "--yaw-steps yaws at every --pitch; every view gets a frame and a 4x4 camera-to-world pose, "
                            "and the settings the intrinsics that go with it (default: none, 26 cones of --fov)")),
    ("--yaw-steps", dict(type=int, default=8, metavar="N", help="with --frustum: the yaws per pitch, 360 / N degrees apart "
                                                                 "(default 8; N times the pitches is at most 32)")),
    ("--pitch", dict(type=float, nargs="+", default=[0.0], metavar="DEG",
                     help="with --frustum: the pitches in degrees, towards --up (default 0)")),
    ("--up", dict(type=int, nargs=3, default=[0, -1, 0], metavar=("X", "Y", "Z"),
                  help="with --frustum or --stand: the world's up, one of the six signed axes.  A convention, not a "
                       "measurement: the world is the first camera's frame, whose y points down (default 0 -1 0)")),
    STAND_FLAG,
    ("--view-image-width", dict(type=int, default=640, metavar="W",
                                help="with --frustum: the width in pixels of the intrinsics written to the settings; the "
                                     "height follows from the two angles (default 640)")),
    ("--stride", dict(type=int, default=4, help="every stride-th reachable cell per axis is a candidate pose (default "
                                                "4: a starting point, not a measured optimum)")),
    ("--count", dict(type=int, default=10, help="the views to keep at most (default 10)")),
    ("--separation", dict(type=float, default=None, help="no two kept views are nearer than this, in metres (default: "
                                                         "half of --range)")),
    ("--max-distance", dict(type=float, default=None, help="leave out poses farther than this by route, in metres "
                                                           "(default: none)")),
    ("--min-gain", dict(type=int, default=1, help="drop poses whose best heading sees fewer unknown cells (default 1)")),
    ("--route-to", dict(type=int, default=None, metavar="RANK", help="also the way to the view of this rank (0 = the "
                                                                     "best), as `route` writes it")),
    ("--cover-until", dict(type=float, default=None, metavar="FRACTION",
                           help="with --cover: stop once this fraction, in (0, 1], of the unknown cells that any pose "
                                "can see is covered (default: none, --count and --min-gain end the plan)")),
    ("--tour-from", dict(type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                         help="with --tour: the world point the tour leaves from (default: --start, or the last pose "
                              "of --from-trajectory)")),
    TAUT_FLAG,
    ("--device", dict(default="cuda")),
)
VIEW_SWITCHES: Sequence[Tuple[str, str]] = (
    TAUT_SWITCH,
    ("--cover", "pick the views one after the other, each by the unknown cells the kept ones do not see yet, so that "
                "the plan adds up; a cell may be kept with several headings, and --separation is refused"),
    ("--tour", "also the order to visit the kept views in and the ways between them (tour.json, tour.npz, tour.ply): "
               "the shortest open path from the start, exact up to 12 stops, nearest neighbour and 2-opt above"),
    ("--far", "let --range reach 64 occupancy cells instead of 32: the rays are cast octant by octant around the pose, by "
              "the same rules; twice the range is roughly eight times the rays per pose, so widen --stride with it"),
    ("--portrait", "with --frustum: the camera turned a quarter about its axis, so the two angles change places"),
)


def list_images(root: str) -> List[str]:
    """Folder -> its png, jpg, jpeg, bmp files (each extension group sorted, groups in that order); file -> its
    non-empty lines; anything else is a glob pattern."""
    if os.path.isdir(root):
        return [f for ext in ("png", "jpg", "jpeg", "bmp") for f in sorted(glob.glob(os.path.join(root, "*." + ext)))]
    if os.path.isfile(root):
        return [ln for ln in (raw.strip() for raw in open(root)) if ln]
    return sorted(glob.glob(root))


def build_parser() -> argparse.ArgumentParser:
    top = argparse.ArgumentParser(prog="pi3_slam_amd.cli", description=__doc__.split("\n")[0])
    sub = top.add_subparsers(dest="command", required=True)
    for name, flags, switches in (("create", tuple(CREATE_FLAGS) + tuple(DENSE_CHUNK_FLAGS), CREATE_SWITCHES),
                                  ("reconstruct", tuple(RECON_FLAGS) + tuple(DENSE_MAP_FLAGS) + tuple(LOOP_FLAGS), RECON_SWITCHES),
                                  ("online", tuple(ONLINE_FLAGS) + ONLINE_DENSE_FLAGS + ONLINE_FOLLOW_FLAGS,
                                   ONLINE_SWITCHES),
                                  ("evaluate-map", EVAL_FLAGS, EVAL_SWITCHES), ("route", ROUTE_FLAGS, ROUTE_SWITCHES),
                                  ("frontiers", FRONTIER_FLAGS, (TAUT_SWITCH,)), ("views", VIEW_FLAGS, VIEW_SWITCHES)):
        p = sub.add_parser(name)
        for flag, kw in flags:
            p.add_argument(flag, **kw)
        for flag, text in switches:
            p.add_argument(flag, action="store_true", help=text)
        if name == "create":   # the two tri-state switches of the reference script
            p.add_argument("--metric-depth", dest="metric_depth", action="store_true", default=True)
            p.add_argument("--no-metric-depth", dest="metric_depth", action="store_false")
            p.add_argument("--estimate-intrinsics", action="store_true", default=True)
        if name == "online":   # store_true with default True in the reference: always on there, switchable here
            p.add_argument("--estimate_camera_params", action="store_true", default=True)
            p.add_argument("--do_metric_depth", dest="do_metric_depth", action="store_true", default=True)
            p.add_argument("--no_metric_depth", dest="do_metric_depth", action="store_false")
    return top


def run_create(a: argparse.Namespace) -> None:
    from .chunk_creator import OfflineChunkCreator, OfflineCreatorConfig
    paths = list_images(a.images)
    if not paths:
        raise SystemExit(f"No images found for: {a.images}")
    lo, hi = max(0, a.skip_start), len(paths) - max(0, a.skip_end)
    if lo >= len(paths) or hi <= lo:
        raise SystemExit(f"Invalid frame range after --skip-start {a.skip_start} / --skip-end {a.skip_end}: "
                         f"{len(paths)} images")
    cfg = OfflineCreatorConfig(
        model_path=a.model_path, output_dir=a.output, chunk_length=a.chunk_length, overlap=a.overlap, device=a.device,
        do_metric_depth=a.metric_depth, keypoint_type=a.keypoints, max_num_keypoints=a.max_kp,
        keypoint_detection_threshold=a.kp_threshold, estimate_camera_params=a.estimate_intrinsics,
        num_loader_workers=a.num_workers, cam_dist_path=a.cam_dist_path, moge_model_path=a.moge_model_path,
        keypoint_seed=None if a.keypoint_seed < 0 else a.keypoint_seed, device_resize=a.device_resize,
        hip_graph=a.hip_graph, reuse_overlap_encoder=a.reuse_overlap_encoder,
        **{name: getattr(a, name) for name in option_names(DENSE_CHUNK_FLAGS)})
    OfflineChunkCreator(cfg).process_and_save(paths[lo:hi])


def run_reconstruct(a: argparse.Namespace) -> None:
    from .reconstructor import OfflineReconstructor
    os.makedirs(a.output, exist_ok=True)
    OfflineReconstructor(chunk_dir=a.chunks, output_dir=a.output, chunk_length=a.chunk_length, overlap=a.overlap,
                         max_observations_per_track=a.max_observations_per_track, save_per_chunk=a.save_per_chunk,
                         use_inverse_depth=a.use_inverse_depth, device=a.device,
                         save_observations=a.save_observations, bundle_adjust=not a.no_bundle_adjust,
                         ba_sanity_gate=not a.no_ba_sanity_gate, render_every=a.render_every,
                         render_overview=a.render_overview, render_min_weight=a.render_min_weight,
                         render_splat_scale=a.render_splat_scale, map_follow_poses=a.map_follow_poses,
                         map_follow_tolerance=a.map_follow_tolerance, loop_closure=a.loop_closure,
                         **{name: getattr(a, name) for name in option_names(tuple(DENSE_MAP_FLAGS) + tuple(LOOP_FLAGS))}).run()


def online_image_paths(a: argparse.Namespace) -> List[str]:
    """load_image_paths of the reference's online script (pi3_slam_online_modular.py:66-113) for image directories:
    skip_start / skip_end trim the sorted list; a video needs a decoder this image does not have."""
    if bool(a.image_dir) == bool(a.video_path):
        raise SystemExit("Must specify either --image_dir or --video_path" if not a.image_dir
                         else "Cannot specify both --image_dir and --video_path")
    if a.video_path:
        raise SystemExit("--video_path: no video decoder (torchcodec / cv2) in this build; extract the frames and use --image_dir")
    if a.skip_start < 0 or a.skip_end < 0:
        raise SystemExit("--skip_start / --skip_end must be non-negative")
    paths = list_images(a.image_dir)
    lo, hi = a.skip_start, len(paths) - a.skip_end
    if lo >= hi:
        raise SystemExit(f"No images found after applying frame skipping ({len(paths)} images)")
    return paths[lo:hi]


def run_online(a: argparse.Namespace) -> None:
    """main() of pi3_slam_online_modular.py:186-372 without the viser window: stream the images through Pi3SLAMOnline,
    then trajectory.ply (+ trajectory.tum with --save_tum) under --output_path."""
    from .online import Pi3SLAMOnline
    from .undistortion import create_undistortion_maps
    paths = online_image_paths(a)
    print(f"✅ Total images/frames to process: {len(paths):,}")
    maps = create_undistortion_maps(a.cam_dist_path, device=a.device) if a.cam_dist_path else None
    out_is_dir = os.path.isdir(a.output_path) or a.output_path.endswith("/") or not a.output_path.endswith(".ply")
    out_dir = a.output_path if out_is_dir else os.path.dirname(a.output_path)
    os.makedirs(out_dir or ".", exist_ok=True)
    slam = Pi3SLAMOnline(
        chunk_length=a.chunk_length, overlap=a.overlap, device=a.device, conf_threshold=a.conf_threshold,
        undistortion_maps=maps, cam_scale=a.cam_scale, estimate_camera_params=a.estimate_camera_params,
        keypoint_type=a.keypoint_type, max_num_keypoints=a.max_num_keypoints,
        keypoint_detection_threshold=a.keypoint_detection_threshold,
        save_chunk_reconstructions=a.save_chunk_reconstructions, max_observations_per_track=a.max_observations_per_track,
        do_metric_depth=a.do_metric_depth, model_path=a.model_path,
        use_inverse_depth=a.use_inverse_depth, moge_model_path=a.moge_model_path, hip_graph=not a.no_hip_graph,
        output_dir=out_dir, num_loader_workers=a.num_workers, bundle_adjust=not a.no_bundle_adjust,
        reuse_overlap_encoder=a.reuse_overlap_encoder, dense_voxel_size=a.dense_voxel_size,
        map_follow_poses=a.map_follow_poses, map_follow_tolerance=a.map_follow_tolerance,
        # --dense_mesh is no option of the object: it asks for save_dense_mesh() below
        **{name: getattr(a, name) for name in option_names(ONLINE_DENSE_FLAGS) if name != "dense_mesh"})
    slam.save_transformed_reconstructions = a.save_transformed_reconstructions
    slam.save_debug_reconstructions = a.save_debug_reconstructions
    slam.process_chunks(paths)
    stats = slam.get_statistics()
    print(f"✅ Total chunks processed: {stats['num_chunks']}\n✅ Total frames processed: {stats['num_frames']}")
    if slam.rank != 0:
        return
    ply = os.path.join(out_dir, "trajectory.ply") if out_is_dir else a.output_path
    tum = os.path.join(out_dir, "trajectory.tum") if out_is_dir else a.output_path.replace(".ply", ".tum")
    slam.save_final_result(ply, max_points=a.max_points)
    if a.save_tum:
        slam.save_trajectory_tum(tum, integer_timestamp=a.tum_integer_timestamp)
    print(f"💾 Saved {ply}" + (f" and {tum}" if a.save_tum else ""))
    if a.dense_voxel_size is not None:
        slam.save_dense_map(os.path.join(out_dir or ".", "dense_points.ply"))
    if a.dense_mesh:
        if a.dense_voxel_size is None:
            print("--dense_mesh needs --dense_voxel_size: no dense mesh")
        else:
            slam.save_dense_mesh(os.path.join(out_dir or ".", "dense_mesh.ply"))
    if a.occupancy_cell is not None:
        if a.dense_voxel_size is None:
            print("--occupancy_cell needs --dense_voxel_size: no occupancy grid")
        else:
            slam.save_occupancy(os.path.join(out_dir or ".", "occupancy.npz"))
    if a.render_every is not None:
        if a.dense_voxel_size is None:
            print("--render_every needs --dense_voxel_size: no renders")
        else:
            slam.save_renders(os.path.join(out_dir or ".", "renders"), every=a.render_every, overview=True)


def evaluate_map_transform(a: argparse.Namespace):
    """The similarity evaluate-map applies to the estimate: --transform, or the trajectory pair's alignment, or None."""
    from . import map_eval
    pair = (a.estimate_trajectory, a.reference_trajectory)
    if a.transform and any(pair):
        raise SystemExit("evaluate-map: give --transform or the trajectory pair, not both")
    if any(pair) and not all(pair):
        raise SystemExit("evaluate-map: --estimate-trajectory and --reference-trajectory go together")
    if a.transform:
        return map_eval.read_transform(a.transform)
    if all(pair):
        return map_eval.trajectory_alignment(a.estimate_trajectory, a.reference_trajectory)
    return None


def evaluate_map_icp(a: argparse.Namespace, est: Dict, ref: Dict) -> Optional[Dict]:
    """compare_clouds' icp argument from the --icp flags and the two PLYs' vertices; None without --icp."""
    if a.icp is None:
        if a.icp_scale:
            raise SystemExit("evaluate-map: --icp-scale needs --icp point|plane")
        return None
    if a.icp_iterations < 1:
        raise SystemExit("evaluate-map: --icp-iterations must be at least 1")
    icp = dict(mode=a.icp, with_scale=bool(a.icp_scale), iterations=a.icp_iterations, max_dist=a.icp_max_dist)
    if a.icp == "plane":
        if ref["normals"] is not None:
            icp["ref_normals"] = ref["normals"]
        elif est["normals"] is not None:
            icp["est_normals"] = est["normals"]
        elif a.mesh_surface and (est.get("faces") is not None or ref.get("faces") is not None):
            pass                                   # a mesh side's surface samples carry their face normals
        else:
            raise SystemExit("evaluate-map: --icp plane needs nx ny nz in the reference's or the estimate's PLY")
    return icp


def run_evaluate_map(a: argparse.Namespace) -> None:
    import json

    import numpy as np

    from . import map_eval
    from .export import write_ply
    if a.icp is None and a.icp_scale:              # refused before anything is read
        raise SystemExit("evaluate-map: --icp-scale needs --icp point|plane")
    mesh = {}
    if a.mesh_surface:
        ev, rv = map_eval.read_ply_mesh(a.estimate), map_eval.read_ply_mesh(a.reference)
        if ev["faces"] is None and rv["faces"] is None:
            raise SystemExit("evaluate-map: --mesh-surface needs faces in the estimate's or the reference's PLY")
        mesh = dict(est_faces=ev["faces"], ref_faces=rv["faces"], sample_spacing=a.mesh_sample_spacing,
                    sample_seed=a.mesh_sample_seed)
    else:
        if a.mesh_sample_spacing is not None or a.mesh_sample_seed:
            raise SystemExit("evaluate-map: --mesh-sample-spacing and --mesh-sample-seed need --mesh-surface")
        ev, rv = map_eval.read_ply_vertices(a.estimate), map_eval.read_ply_vertices(a.reference)
    est, ref = ev["points"], rv["points"]
    icp = evaluate_map_icp(a, ev, rv)
    res = map_eval.compare_clouds(est, ref, a.thresholds, max_dist=a.max_dist, transform=evaluate_map_transform(a),
                                  voxel_size=a.voxel_size, device=a.device, **({} if icp is None else {"icp": icp}),
                                  **mesh)
    if a.save_transform:
        applied = res["settings"]["transform"]
        map_eval.write_transform(a.save_transform, np.eye(4) if applied is None else applied)
    if a.error_ply:
        write_ply(res["_points"]["estimate"],
                  map_eval.error_colors(res["_distances"]["estimate"], res["settings"]["max_dist"]), a.error_ply)
    print(json.dumps(map_eval.public(res)) if a.json else map_eval.format_table(res))


def run_route(a: argparse.Namespace) -> None:
    from . import export
    from .grid_route import GridRouter, read_tum_positions
    if (a.start is None) == (a.from_trajectory is None):
        raise SystemExit("route: give --start X Y Z or --from-trajectory TRAJ.tum (one of them)")
    check_taut(a, "route", "--goal X Y Z", a.goal is not None)
    try:
        router = GridRouter(a.radius, a.through_unknown, a.approach_unknown,
                            **({} if a.stand is None else dict(stand=tuple(a.stand), up=a.up)))
        grid = export.read_occupancy(a.occupancy)
        sources = [a.start] if a.start is not None else read_tum_positions(a.from_trajectory)
        field = router.field(grid, sources, a.device)
        route = router.path(field, a.goal) if a.goal is not None else None
        taut = router.taut(field, route, a.taut_span) if a.taut and route is not None else None
    except (ValueError, OSError) as e:
        raise SystemExit(f"route: {e}")
    export.write_route(field, route, a.output, taut)
    c = field.counts
    text = (f"route: {c['traversable']} traversable cells, {c['reachable']} reachable from {c['sources_accepted']} "
            f"sources ({c['sources_blocked']} not traversable, {c['sources_outside']} outside) in {c['sweeps']} sweeps")
    text += stand_text(c, field.settings)
    if a.goal is not None:
        if route is None:
            text += "; the goal cannot be reached"
        else:
            text += f"; {len(route.waypoints)} waypoints, {route.length_m:.3f} m"
            if route.min_clearance_m is not None:
                text += f", clearance >= {route.min_clearance_m:.3f} m"
            if taut is not None:
                text += taut_text(taut)
    print(text)


def run_frontiers(a: argparse.Namespace) -> None:
    from . import export
    from .frontier import FrontierFinder
    from .grid_route import read_tum_positions
    if a.start is not None and a.from_trajectory is not None:
        raise SystemExit("frontiers: give --start X Y Z or --from-trajectory TRAJ.tum, not both")
    if a.route_to is not None and a.start is None and a.from_trajectory is None:
        raise SystemExit("frontiers: --route-to needs a source: --start X Y Z or --from-trajectory TRAJ.tum")
    check_taut(a, "frontiers", "--route-to RANK", a.route_to is not None)
    try:
        finder = FrontierFinder(a.radius, a.min_cells, **({} if a.stand is None else dict(stand=tuple(a.stand), up=a.up)))
        grid = export.read_occupancy(a.occupancy)
        sources = None
        if a.start is not None:
            sources = [a.start]
        elif a.from_trajectory is not None:
            sources = read_tum_positions(a.from_trajectory)
        found = finder.find(grid, sources, a.device)
        route = found.route_to(a.route_to) if a.route_to is not None else None
        taut = found.router.taut(found.field, route, a.taut_span) if a.taut and route is not None else None
    except (ValueError, OSError) as e:
        raise SystemExit(f"frontiers: {e}")
    export.write_frontiers(found, a.output)
    if route is not None:
        export.write_route(found.field, route, a.output, taut)
    c = found.counts
    text = (f"frontiers: {c['frontier_cells']} frontier cells in {c['clusters']} clusters ({c['clusters_dropped']} "
            f"dropped), {c['reachable_clusters']} reachable, {c['sweeps']} sweeps")
    if found.field is not None:
        text += stand_text(found.field.counts, found.field.settings)
    if found.clusters:
        best = found.clusters[0]
        text += f"; the best: {best.cells} cells"
        text += f" at {best.distance_m:.3f} m" if best.reachable else ", not reachable" if sources is not None else ""
    if taut is not None:
        text += f"; the way to cluster {a.route_to}: {route.length_m:.3f} m" + taut_text(taut)
    print(text)


def run_views(a: argparse.Namespace) -> None:
    from . import export
    from .grid_route import read_tum_positions
    from .view_planner import ViewPlanner
    if (a.start is None) == (a.from_trajectory is None):
        raise SystemExit("views: give --start X Y Z or --from-trajectory TRAJ.tum (one of them)")
    if a.cover and a.separation is not None:
        raise SystemExit("views: --separation has no meaning with --cover (a cover keeps views by what they add)")
    if a.cover_until is not None and not a.cover:
        raise SystemExit("views: --cover-until needs --cover")
    if a.tour_from is not None and not a.tour:
        raise SystemExit("views: --tour-from needs --tour")
    check_taut(a, "views", "--route-to RANK or --tour", a.route_to is not None or a.tour)
    try:
        camera = {} if a.frustum is None else dict(frustum=tuple(a.frustum), yaw_steps=a.yaw_steps, pitches_deg=a.pitch,
                                                   up=a.up, portrait=a.portrait, image_width=a.view_image_width)
        fov = a.fov if a.frustum is None or getattr(a, "fov_given", False) else None     # a frustum has its own angles
        if a.stand is not None:
            camera.update(stand=tuple(a.stand), up=a.up)
        planner = ViewPlanner(a.radius, a.range, fov, a.stride, a.count, a.separation, a.max_distance, a.min_gain,
                              a.far, a.unknown_depth, **camera)
        grid = export.read_occupancy(a.occupancy)
        sources = [a.start] if a.start is not None else read_tum_positions(a.from_trajectory)
        if a.cover:
            found = planner.cover(grid, sources, a.device, a.cover_until)
        else:
            found = planner.find(grid, sources, a.device)
        route = found.route_to(a.route_to) if a.route_to is not None else None
        taut = found.router.taut(found.field, route, a.taut_span) if a.taut and route is not None else None
        tour = found.tour(a.tour_from, taut=a.taut, taut_span=a.taut_span) if a.tour else None
    except (ValueError, OSError) as e:
        raise SystemExit(f"views: {e}")
    export.write_views(found, a.output)
    if route is not None:
        export.write_route(found.field, route, a.output, taut)
    if tour is not None:
        export.write_tour(tour, a.output)
    c = found.counts
    text = (f"views: {c['candidates']} candidates, {c['rays']} rays ({c['rays_visible']} visible), {c['views']} views "
            f"kept ({c['low_gain']} candidates below the gain)")
    if a.unknown_depth is not None:
        text += f"; rays end after {a.unknown_depth} unknown cells"
    if a.frustum is not None:
        text += f"; {len(planner.frames)} frusta of {a.frustum[0]:g} x {a.frustum[1]:g} degrees"
    text += stand_text(found.field.counts, found.field.settings)
    if found.views:
        best = found.views[0]
        text += f"; the best: {best.gain} cells at {best.distance_m:.3f} m"
    if found.mode == "cover":
        text += (f"; covered {c['covered']} of {c['seeable']} seeable unknown cells "
                 f"({100.0 * c['covered'] / max(c['seeable'], 1):.1f} %)")
    if taut is not None:
        text += f"; the way to view {a.route_to}: {route.length_m:.3f} m" + taut_text(taut)
    if tour is not None:
        text += (f"; tour: {len(tour.stops)} stops, {tour.distance_m:.2f} m ({tour.rank_order_length_m:.2f} m in rank "
                 f"order), {tour.method}")
        if tour.taut_length_m is not None:
            text += (f", taut {tour.taut_length_m:.2f} m of {tour.length_m:.2f} m over "
                     f"{tour.taut_vertices} vertices")
        if tour.unreachable:
            text += f", {len(tour.unreachable)} stops not reachable from the start"
    print(text)


def main(argv=None) -> None:
    a = build_parser().parse_args(argv)
    {"create": run_create, "reconstruct": run_reconstruct, "online": run_online,
     "evaluate-map": run_evaluate_map, "route": run_route, "frontiers": run_frontiers,
     "views": run_views}[a.command](a)


if __name__ == "__main__":
    main()
