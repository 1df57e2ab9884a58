"""The optimizer's lifecycle timelines (tests/_optim_timeline.py) on CPU tensors.  Every step is the torch-op path's here, so
this run proves the harness, the fp64 reference and the torch twins themselves: each timeline must stay inside the bounds of
tests/_optim_ref.py with nothing native in play.  tests/test_optim_lifecycle_gpu.py runs the same timelines on the device.
Every test prints the paths its steps took and the worst error as a multiple of its bound."""
import math

import numpy as np
import pytest
import torch

import _optim_ref as ref
import _optim_timeline as tl

CPU = torch.device("cpu")


@pytest.mark.parametrize("entry", tl.TIMELINES, ids=tl.IDS)
def test_timeline_on_the_cpu(entry):
    run = tl.run_timeline(entry, CPU)
    assert run.opt.native_steps == 0 and run.opt.torch_steps == len(run.paths) and set(run.paths) == {"torch"}


def test_clip_coef_of_a_nan_norm_is_nan():
    assert math.isnan(ref.clip_coef(math.nan, 1.0)) and ref.clip_coef(math.nan, None) == 1.0
    assert ref.clip_coef(math.inf, 1.0) == 0.0 and ref.clip_coef(0.0, 1.0) == 1.0 and ref.clip_coef(3.0, 1.5) == 1.5 / (3.0 + 1e-6)


def test_ratio_nonfinite_asks_no_less_than_ratio():
    """Finite data: ratio() itself.  A non-finite element must be met by the same one: NaN by NaN, inf by inf of its sign."""
    refv, bound = np.array([1.0, -2.0, 0.0, 4.0]), np.array([0.5, 0.5, 0.0, 0.5])
    out = np.array([1.25, -2.0, 0.0, 3.0])
    assert ref.ratio_nonfinite(out, refv, bound) == ref.ratio(out, refv, bound) == 2.0
    assert ref.ratio_nonfinite(np.array([1.0, -2.0, 1e-30, 4.0]), refv, bound) == math.inf          # bound 0: exact
    nf = np.array([math.nan, -math.inf, 0.0, math.inf])
    assert ref.ratio_nonfinite(nf, nf.copy(), bound) == 0.0
    for i, wrong in ((0, 1.0), (0, math.inf), (1, math.inf), (1, math.nan), (1, -1e38), (3, -math.inf), (2, math.nan)):
        bad = nf.copy()
        bad[i] = wrong
        assert ref.ratio_nonfinite(bad, nf, bound) == math.inf, (i, wrong)
        assert ref.ratio_nonfinite(nf, bad, bound) == math.inf, (i, wrong)
    assert ref.ratio_nonfinite(out, refv, np.array([0.5, math.inf, 0.0, 0.5])) == math.inf          # no bound to hide behind
