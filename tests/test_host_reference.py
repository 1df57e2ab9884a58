"""The fp64 host twin of tests/_host_reference.py on its own (no GPU): its 2-D shift and AttentionShift pieces against
the oracles, a whole RubiksNet-Tiny training step on it, and the comparator that judges the GPU steps against it."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import _host_reference as hr
from oracle import attention_oracle
from oracle.torch_shift import OracleShift2D

F64 = torch.float64


@pytest.mark.parametrize("stride,padding", [(1, 0), (2, 0), ((2, 1), (1, 0))])
def test_oracle_shift2d_function_is_the_oracle_and_its_adjoint(oracle, stride, padding):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 6, 9, 8))
    shift = rng.uniform(-1.5, 1.5, (2, 6))
    xt = torch.from_numpy(x).requires_grad_(True)
    st = torch.from_numpy(shift).requires_grad_(True)
    y = OracleShift2D.apply(xt, st, stride, padding, True, False)
    np.testing.assert_array_equal(y.detach().numpy(), oracle.rk2d_forward(x, shift, stride, padding))
    gy = rng.uniform(-1, 1, tuple(y.shape))
    y.backward(torch.from_numpy(gy))
    gx, gs = oracle.rk2d_backward(gy, x, shift, stride, padding, True, True)
    np.testing.assert_array_equal(xt.grad.numpy(), gx)
    np.testing.assert_array_equal(st.grad.numpy(), gs)
    _, raw = oracle.rk2d_backward(gy, x, shift, stride, padding, False, True)
    assert not np.allclose(raw, gs)                  # normalize_grad reached the oracle
    # the shift is linear in x: d(x) is the exact adjoint of the forward
    xs = torch.from_numpy(x).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: OracleShift2D.apply(v, st.detach(), stride, padding, True, False), (xs,))


@pytest.mark.parametrize("golden", ["a", "b", "c", "d"])
def test_twin_attention_shift_matches_the_pinned_oracle(golden_dir, golden):
    """The twin's AttentionShift -- the tap softmax as a torch expression under autograd, then OracleTemporalShift3 --
    against attention_oracle's hand-derived forward / backward (pinned by tests/golden/attention_*.npz)."""
    from rubiksnet_amd.attention_shift import AttentionShift

    data = np.load(os.path.join(golden_dir, "attention_%s.npz" % golden))
    x, weight, gy = (data[k].astype(np.float64) for k in ("x", "weight", "gy"))
    n_segment = int(data["n_segment"])
    layer = AttentionShift(n_segment, num_channels=weight.shape[0]).to(F64)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(weight))
    twin = hr.host_twin(layer)
    xt = torch.from_numpy(x).requires_grad_(True)
    with hr.twin_guard():
        y = twin(xt)
        y.backward(torch.from_numpy(gy))
    np.testing.assert_allclose(y.detach().numpy(), attention_oracle.forward(x, weight, n_segment), rtol=1e-13, atol=1e-13)
    gx, gw = attention_oracle.backward(gy, x, weight, n_segment)
    np.testing.assert_allclose(xt.grad.numpy(), gx, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(twin.weight.grad.numpy(), gw, rtol=1e-8, atol=1e-10)


def _tiny(variant):
    from rubiksnet_amd import RubiksNet

    torch.manual_seed(1)
    net = RubiksNet("tiny", 5, num_frames=8, variant=variant, verbose=False).train()
    return net, torch.randn(1, 8, 3, 32, 32), torch.tensor([3])


@pytest.mark.parametrize("variant", ["rubiks3d", "rubiks3d-aq"])
def test_twin_train_step_on_host(variant):
    """RubiksNet-Tiny at 32 x 32: the twin is fp64 on the CPU, never touches the native library, and a dp.train_step
    gives every trainable parameter a finite gradient and counts one batch in every BatchNorm."""
    net, clips, labels = _tiny(variant)
    twin = hr.host_twin(net)
    assert all(p.dtype == F64 and not p.is_cuda for p in twin.parameters())
    x = clips.to(F64)
    with hr.twin_guard():
        loss, logits = hr.sgd_step(twin, x, labels)
    snap = hr.capture(twin, loss, logits)
    assert snap["grads"] == snap["trainable"] == {n for n, p in net.named_parameters() if p.requires_grad}
    assert all(torch.isfinite(t).all() for t in snap["tensors"].values())
    assert set(snap["counters"].values()) == {1}
    # the step moved every trainable parameter of the twin and none of the model it was copied from
    for name, p in net.named_parameters():
        assert torch.equal(snap["tensors"]["param:" + name], p.detach().double()) != p.requires_grad, name


def test_twin_guard_refuses_the_native_library():
    from rubiksnet_amd import _native

    with hr.twin_guard():
        with pytest.raises(AssertionError, match="native HIP library"):
            _native.lib()


def test_comparator_passes_equal_steps_and_names_a_wrong_or_missing_tensor():
    net, clips, labels = _tiny("rubiks3d")
    twin = hr.host_twin(net)
    with hr.twin_guard():
        loss, logits = hr.sgd_step(twin, clips.to(F64), labels)
    snap = hr.capture(twin, loss, logits)
    rows = hr.check_step(snap, snap, snap, dtype=torch.float32)
    assert all(r[1] == 0.0 and r[2] == 0.0 for r in rows)

    key = "grad:new_fc.weight"
    bad = copy.deepcopy(snap)
    bad["tensors"][key] = bad["tensors"][key] * (1 + 1e-4)
    with pytest.raises(AssertionError, match=re.escape("fused %s: err" % key)):
        hr.check_step(bad, snap, snap, dtype=torch.float32)
    deep = "grad:backbone.layer2.0.conv2.weight"              # behind ReLU kinks: 1e-4 is under the bar there
    bad["tensors"][deep] = bad["tensors"][deep] * (1 + 1e-4)
    with pytest.raises(AssertionError) as err:
        hr.check_step(bad, snap, snap, dtype=torch.float32)
    assert "fused %s" % deep not in str(err.value)
    with pytest.raises(AssertionError, match=re.escape("stock %s: err" % key)):
        hr.check_step(snap, bad, snap, dtype=torch.float32, ceiling=1e-5)

    name = "backbone.layer1.0.as3.rubiks3d.shift"
    dropped = copy.deepcopy(snap)
    dropped["grads"].discard(name)
    del dropped["tensors"]["grad:" + name]
    with pytest.raises(AssertionError, match=re.escape("fused: no gradient for %s" % name)):
        hr.check_step(dropped, snap, snap, dtype=torch.float32)

    counted = copy.deepcopy(snap)
    counted["counters"]["num_batches_tracked:backbone.bn_last"] = 2
    with pytest.raises(AssertionError, match=re.escape("num_batches_tracked:backbone.bn_last = 2")):
        hr.check_step(counted, snap, snap, dtype=torch.float32)

    # a shift-table gradient: its near-zero components are left out, the others are compared
    g = snap["tensors"]["grad:" + name]
    tiny_part = g.abs() < hr.SHIFT_NEAR_ZERO * g.abs().amax(dim=1, keepdim=True)
    flipped = g.clone()
    flipped[tiny_part] *= -1
    assert hr.errors(flipped, g, "grad:" + name)[0] == 0.0
    assert hr.errors(-g, g, "grad:" + name)[0] > 1.0
