"""Worker of tests/test_render_gpu.py::test_chess_room_end_to_end_renders: stage 2 with renders over a chunk directory
under torch.distributed.run (PI3_DIST_BACKEND=gloo); rank 0 writes the files."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pi3_slam_amd.reconstructor import OfflineReconstructor  # noqa: E402


def main():
    chunk_dir, out_dir = sys.argv[1], sys.argv[2]
    OfflineReconstructor(chunk_dir, out_dir, bundle_adjust=False, render_every=50, render_overview=True).run()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
