"""Worker of tests/test_dense_map_gpu.py::test_chess_room_end_to_end: stage 2 over a chunk directory whose chunks carry
dense clouds, single process or under torch.distributed.run (PI3_DIST_BACKEND=gloo).  Rank 0 also saves the transform
each collected chunk's cloud was moved by, so the test can fuse the clouds with the oracle."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pi3_slam_amd.dense_map import chunk_transform  # noqa: E402
from pi3_slam_amd.reconstructor import OfflineReconstructor  # noqa: E402


def main():
    chunk_dir, out_dir, ba = sys.argv[1], sys.argv[2], sys.argv[3] == "1"
    rec = OfflineReconstructor(chunk_dir, out_dir, bundle_adjust=ba)
    rec.run()
    if int(os.environ.get("RANK", "0")) == 0:
        torch.save({"transforms": [chunk_transform(d) for d in rec.reconstructions],
                    "rebased": [d.get("_sim3_dense") is not None for d in rec.reconstructions]},
                   os.path.join(out_dir, "dense_transforms.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
