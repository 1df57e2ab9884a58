"""Whole-network training steps against an fp64 host reference.

Each case builds one RubiksNet from a seed, deep-copies it three times and runs one `dp.train_step` (SGD, no momentum)
on each copy (tests/_host_reference.py):
    fused   the GPU with the default switches: every fused training path of the product
    stock   the GPU with every fusion switch off: stock PyTorch modules plus the HIP shift operators
    twin    the network on the CPU in float64, its shifts evaluated by the oracles
and compares loss, logits, every parameter gradient (the SET of parameters with a gradient must be the twin's), the
BatchNorm running statistics and counters, and the updated parameters.  The bar calibrates itself per tensor:
err_fused <= 3 err_stock + floor (relative-norm error against the twin; the floor by storage precision and by whether
a ReLU lies between the tensor and the loss, see _host_reference.floor_for), and err_stock itself stays under a fixed
ceiling, so that a fault both GPU paths share is caught as well.

224 x 224 clips of 8 frames, so that the real kernel families run (14 x 14 tiles, 7 x 7 slabs, stride-2 bands).
Measured on the MI355X, worst tensor per case (relative-norm error against fp64, stock / fused), host seconds of the
twin's step:

    case            loss, logits, running stats    gradients          twin s
    tiny            4.2e-7 / 5.1e-7                3.3e-3 / 6.5e-3     4.2
    small-se        2.9e-7 / 4.4e-7                3.8e-3 / 9.7e-3     5.9
    medium          5.8e-7 / 5.0e-7                7.5e-3 / 7.6e-3     6.8
    large           6.5e-7 / 8.4e-7                1.3e-2 / 2.0e-2    10.3
    tiny-aq         3.9e-7 / 5.2e-7                7.1e-3 / 2.1e-2     4.5
    large-aq-bf16   1.3e-2 / 1.1e-2                8.2e-1 / 9.0e-1    11.0

The worst gradients are shift tables and the first layers: fp32 round-off flips the ReLU decision of a few activations
and the backward carries that upstream.  In bf16 the gradients of the 51-block Large-AQ network have all but
decorrelated from fp64, so there the comparison catches a missing, misplaced or garbage gradient, not a subtle one.
"""
import re

import pytest
import torch

import _host_reference as hr

pytestmark = pytest.mark.gpu

SIZE = 224

# name: (tier, variant, clips, bf16)
CASES = {
    "tiny": ("tiny", "rubiks3d", 2, False),
    "small-se": ("small", "rubiks3d", 2, False),
    "medium": ("medium", "rubiks3d", 2, False),
    "large": ("large", "rubiks3d", 2, False),
    "tiny-aq": ("tiny", "rubiks3d-aq", 2, False),
    "large-aq-bf16": ("large", "rubiks3d-aq", 2, True),
}
_DONE = {}


def _case_inputs(name):
    tier, variant, n, _ = CASES[name]
    from rubiksnet_amd import RubiksNet

    torch.manual_seed(11)
    net = RubiksNet(tier, 11, num_frames=8, variant=variant, verbose=False).train()
    clips = torch.randn(n, 8, 3, SIZE, SIZE)
    labels = torch.randint(0, 11, (n,))
    return net, clips, labels


def _run_case(monkeypatch, name):
    if name not in _DONE:
        net, clips, labels = _case_inputs(name)
        _DONE[name] = hr.run_three(monkeypatch, net, clips, labels, bf16=CASES[name][3])
    return _DONE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_train_step_matches_fp64_host_twin(monkeypatch, name):
    res = _run_case(monkeypatch, name)
    dtype = torch.bfloat16 if CASES[name][3] else torch.float32
    rows = hr.check_step(res["fused"], res["stock"], res["twin"], dtype=dtype,
                         label=name)
    print("\n" + hr.summary(rows, name))
    print("%s host twin %.1f s, fused %.2f s, stock %.2f s" % (name, res["twin"]["secs"], res["fused"]["secs"],
                                                             res["stock"]["secs"]))


def test_the_comparator_names_a_perturbed_or_missing_gradient(monkeypatch):
    """A 1e-3 relative error in one gradient of the fused result, or a gradient that never arrived, fails the check
    and is named in its message."""
    import copy

    res = _run_case(monkeypatch, "tiny")
    f32 = torch.float32
    rows = hr.check_step(res["fused"], res["stock"], res["twin"], dtype=f32)
    # a gradient whose bar is well under 1e-3
    key = min((r for r in rows if r[0].startswith("grad:") and not r[0].endswith("shift")), key=lambda r: r[1])[0]
    assert hr.FACTOR * dict((r[0], r[1]) for r in rows)[key] + hr.floor_for(f32, key) < 2.5e-4, key

    bad = copy.deepcopy(res["fused"])
    g = bad["tensors"][key]
    noise = torch.randn(g.shape, dtype=g.dtype, generator=torch.Generator().manual_seed(0))
    bad["tensors"][key] = g + noise * (1e-3 * float(g.norm()) / float(noise.norm()))
    with pytest.raises(AssertionError, match=re.escape("fused %s: err" % key)):
        hr.check_step(bad, res["stock"], res["twin"], dtype=f32)

    dropped = copy.deepcopy(res["fused"])
    name = key[len("grad:"):]
    dropped["grads"].discard(name)
    del dropped["tensors"][key]
    with pytest.raises(AssertionError, match=re.escape("fused: no gradient for %s" % name)):
        hr.check_step(dropped, res["stock"], res["twin"], dtype=f32)
