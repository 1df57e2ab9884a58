"""Training steps off the beaten path, each against the fp64 host twin (tests/_host_reference.py) with the bars of
tests/test_step_parity_gpu.py: err_fused <= 3 err_stock + floor for every tensor, err_stock under a fixed ceiling,
the set of parameters with a gradient equal to the twin's (and every frozen parameter left with `grad is None`).

    (a) one stage under torch.utils.checkpoint, reentrant and not, around the stage holding the first member of the
        AttentionShift tap group (layer0) and around one that does not (layer1)
    (b) one layer's soft_taps() evaluated under torch.no_grad() inside `presoftened` before the forward
    (c) gradient accumulation: two micro-batches forward + backward, then one step
    (d) frozen parameter subsets (needs_input_grad decides which kernels run)
    (e) model.eval() fine-tuning with frozen statistics and a gradient for the input clips

Two clips of 8 frames at 224 x 224 (two micro-batches of one clip in (c)).
"""
import contextlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint

import _host_reference as hr

pytestmark = pytest.mark.gpu

VARIANTS = {"tiny": "rubiks3d", "tiny-aq": "rubiks3d-aq"}
SIZE = 224


def _inputs(variant, n=2, seed=23):
    from rubiksnet_amd import RubiksNet

    torch.manual_seed(seed)
    net = RubiksNet("tiny", 11, num_frames=8, variant=VARIANTS[variant], verbose=False).train()
    return net, torch.randn(n, 8, 3, SIZE, SIZE), torch.randint(0, 11, (n,))


def _check(res, label, bf16=False):
    dtype = torch.bfloat16 if bf16 else torch.float32
    rows = hr.check_step(res["fused"], res["stock"], res["twin"], dtype=dtype, label=label)
    print("\n" + hr.summary(rows, label) + "\n%s host twin %.1f s" % (label, res["twin"]["secs"]))
    return rows


class _Checkpointed(nn.Module):
    def __init__(self, inner, reentrant):
        super().__init__()
        self.inner = inner
        self.reentrant = reentrant

    def forward(self, x):
        return torch.utils.checkpoint.checkpoint(self.inner, x, use_reentrant=self.reentrant)


# ----------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("reentrant", [True, False], ids=["reentrant", "non_reentrant"])
@pytest.mark.parametrize("stage", ["layer0", "layer1"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_checkpointed_stage(monkeypatch, variant, stage, reentrant):
    """A stage recomputed in the backward: every weight of the model -- the tap weights of the layers batched with
    the checkpointed one included -- gets the twin's gradient; the recompute updates the stage's running statistics a
    second time, as stock PyTorch does.  A reentrant checkpoint hands the stage fresh tensors, so a fused training
    block there runs its own statistics pass (train_block.stats_fallbacks() grows)."""
    net, clips, labels = _inputs(variant)
    backbone = net.backbone
    setattr(backbone, stage, _Checkpointed(getattr(backbone, stage), reentrant))
    res = hr.run_three(monkeypatch, net, clips, labels)
    _check(res, "%s checkpoint(%s, reentrant=%s)" % (variant, stage, reentrant))
    if variant == "tiny" and reentrant:
        assert res["fused"]["fallbacks"] > 0


# ----------------------------------------------------------------------------------------------------------- (b)
def test_soft_taps_read_under_no_grad_inside_presoftened(monkeypatch):
    """Logging the taps of the first layer of a group under no_grad before the step must not cost any layer of that
    group its d(weight)."""
    from rubiksnet_amd import attention_shift

    net, clips, labels = _inputs("tiny-aq")
    first = next(m for m in net.modules() if isinstance(m, attention_shift.AttentionShift))

    def procedure(model, x, y):
        layer = next(m for m in model.modules() if isinstance(m, attention_shift.AttentionShift))
        ctx = attention_shift.presoftened(model) if x.is_cuda else contextlib.nullcontext()
        with ctx:
            with torch.no_grad():
                taps = layer.soft_taps()
            assert not taps.requires_grad
            return hr.sgd_step(model, x, y)

    assert first is net.backbone.layer0[0].conv2[0]
    _check(hr.run_three(monkeypatch, net, clips, labels, procedure), "tiny-aq soft_taps under no_grad")


# ----------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("variant,bf16", [("tiny", False), ("tiny-aq", True)], ids=["tiny-fp32", "tiny-aq-bf16"])
def test_gradient_accumulation(monkeypatch, variant, bf16):
    """Two micro-batches of one clip, each forward + backward as dp.train_step runs them (prepacked weights under bf16,
    presoftened taps), the gradients summed in p.grad, then one SGD step."""
    from rubiksnet_amd import attention_shift, pointwise

    net, clips, labels = _inputs(variant, n=2)

    def procedure(model, x, y):
        opt = torch.optim.SGD(model.parameters(), lr=hr.LR, momentum=0.0)
        opt.zero_grad(set_to_none=True)
        losses, logits = [], []
        for i in range(2):
            gpu = x.is_cuda
            with (pointwise.prepacked(model) if gpu and bf16 else contextlib.nullcontext()):
                with (attention_shift.presoftened(model) if gpu else contextlib.nullcontext()):
                    out = model(x[i:i + 1])
                loss = F.cross_entropy(out, y[i:i + 1]) / 2
                loss.backward()
            losses.append(loss.detach())
            logits.append(out.detach())
        opt.step()
        return sum(losses), torch.cat(logits)

    _check(hr.run_three(monkeypatch, net, clips, labels, procedure, bf16=bf16), "%s accumulate x2" % variant, bf16)


# ----------------------------------------------------------------------------------------------------------- (d)
def _is_bn(net, name):
    module = net.get_submodule(name.rsplit(".", 1)[0])
    return isinstance(module, nn.BatchNorm2d)


FROZEN = {
    "shift_tables": lambda net, name: name.endswith("shift"),
    "bn_affine": lambda net, name: _is_bn(net, name),
    "all_but_new_fc": lambda net, name: not name.startswith("new_fc."),
    # every BN weight and the stem frozen, BN biases trainable
    "bn_weight_and_stem": lambda net, name: (_is_bn(net, name) and name.endswith(".weight")) or name == "backbone.conv1.weight",
}


@pytest.mark.parametrize("subset", list(FROZEN))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_frozen_subset(monkeypatch, variant, subset):
    net, clips, labels = _inputs(variant)
    for name, p in net.named_parameters():
        if FROZEN[subset](net, name):
            p.requires_grad_(False)
    res = hr.run_three(monkeypatch, net, clips, labels)
    _check(res, "%s frozen %s" % (variant, subset))
    for mode in ("fused", "stock", "twin"):
        assert res[mode]["grads"] == res[mode]["trainable"], mode


# ----------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("frozen,input_grad", [("trainable", True), ("all_frozen", True), ("bn_weight_and_stem", True),
                                                ("bn_weight_and_stem", False)])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_eval_mode_fine_tuning(monkeypatch, variant, frozen, input_grad):
    """model.eval() (running statistics frozen, the forward under `prefolded`) with grad mode on: every trainable
    parameter, and the clips when they ask for it, get the twin's gradient.  `all_frozen`: nothing trains, only d(clips)
    is wanted (the backbone's all_frozen walk); `bn_weight_and_stem`: BatchNorms whose weight is frozen and whose bias
    trains, behind a frozen stem -- without an input gradient the first BatchNorm sees an input that needs no gradient
    and a weight that needs none either."""
    net, clips, labels = _inputs(variant, seed=29)
    with torch.no_grad():                      # non-trivial running statistics, as after training
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 2.0)
    net.eval()
    for name, p in net.named_parameters():
        if frozen == "all_frozen" or (frozen == "bn_weight_and_stem" and FROZEN[frozen](net, name)):
            p.requires_grad_(False)
    res = hr.run_three(monkeypatch, net, clips, labels, input_grad=input_grad)
    _check(res, "%s eval %s%s" % (variant, frozen, " + d(clips)" if input_grad else ""))
    for mode in ("fused", "stock"):
        assert (res[mode]["tensors"].get("input_grad") is not None) == input_grad, mode
