"""ops.sweep_until_quiet without a GPU: the loop that GridRouter.relax, FrontierFinder.settle and
MapCleaner.label_components share, driven by a fake launch on a CPU tensor."""
import pytest
import torch

from pi3_slam_amd import ops


def _launcher(first_quiet):
    """A launch whose sweeps 1 .. first_quiet - 1 change something (None: every sweep does) -> (launch, the flags' log)."""
    seen = []

    def launch(flag):
        assert flag.dtype == torch.int32 and flag.shape == (1,) and int(flag) == 0      # zeroed for every launch
        seen.append(flag)
        if first_quiet is None or len(seen) < first_quiet:
            flag.fill_(1)
    return launch, seen


@pytest.mark.parametrize("q", [1, 2, 4, 5, 8, 9])
def test_returns_the_first_quiet_sweep_and_launches_whole_reads(q):
    launch, seen = _launcher(q)
    assert ops.sweep_until_quiet(launch, torch.device("cpu"), 100, "no {sweeps}", 4) == q
    assert len(seen) == 4 * ((q + 3) // 4)


def test_raises_beyond_the_bound():
    launch, seen = _launcher(None)
    with pytest.raises(RuntimeError, match="^the field did not settle in 8 sweeps over 5 cells$"):
        ops.sweep_until_quiet(launch, torch.device("cpu"), 6, "the field did not settle in {sweeps} sweeps over 5 cells", 4)
    assert len(seen) == 8
