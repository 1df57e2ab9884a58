"""The optimizer's lifecycle timelines (tests/_optim_timeline.py) on the device: the cached job table, SGD's first-step flags,
Adam's shared step counters and the crossings between the one-launch path (rk_optim.hip) and the torch-op path, every step
held to the fp64 bounds of tests/_optim_ref.py and to the path its timeline declares.  Every test prints the paths its steps
took and the worst error as a multiple of its bound."""
import pytest
import torch

import _optim_timeline as tl

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("entry", tl.TIMELINES, ids=tl.IDS)
def test_timeline_on_the_device(entry):
    run = tl.run_timeline(entry, DEV)
    assert run.opt.native_steps == run.paths.count("native") and run.opt.torch_steps == run.paths.count("torch")
    assert run.opt.native_steps > 0
