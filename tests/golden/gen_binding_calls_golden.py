"""Generates tests/golden/binding_calls.json by IMPORTING the reference's own rubiksnet.shiftlib over a recording
stand-in for its extension module `rubiksnet_cuda`, then driving the reference's layers (forward + backward through
autograd) and primitives (with and without preallocated outputs).  Each call the reference makes into the extension --
function name, positional and keyword arguments, tensors as shape + dtype -- is stored, so that
tests/test_independent_restatement.py can replay exactly those argument lists against rubiksnet_amd.rubiksnet_cuda
without the reference tree.  The reference asserts `x.is_cuda` before it calls the extension; here `is_cuda` reads True
for every tensor of this process, and the recorder returns 0 without computing anything.

    python tests/golden/gen_binding_calls_golden.py <reference checkout>

Run once; commits tests/golden/binding_calls.json.  The reference source never enters the repo."""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("rubiks_shift_3d_forward_float", "rubiks_shift_3d_forward_double", "rubiks_shift_3d_backward_float",
         "rubiks_shift_3d_backward_double", "rubiks2d_forward", "rubiks2d_backward")


def _describe(v):
    if isinstance(v, torch.Tensor):
        return {"tensor": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}
    if isinstance(v, (list, tuple)):
        return [_describe(e) for e in v]
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def main(ref):
    calls = []
    stub = types.ModuleType("rubiksnet_cuda")
    for name in NAMES:
        def rec(*args, _name=name, **kwargs):
            calls.append({"fn": _name, "args": [_describe(a) for a in args],
                          "kwargs": {k: _describe(v) for k, v in sorted(kwargs.items())}})
            return 0
        setattr(stub, name, rec)
    sys.modules["rubiksnet_cuda"] = stub
    torch.Tensor.is_cuda = property(lambda self: True)       # past the reference's device asserts (this process only)
    sys.path.insert(0, ref)
    from rubiksnet.shiftlib import RubiksShift2D, RubiksShift3D
    from rubiksnet.shiftlib.rubiks2d import primitive as p2
    from rubiksnet.shiftlib.rubiks3d import primitive as p3

    torch.manual_seed(0)
    for dtype in (torch.float32, torch.float64):
        for kw in ({}, {"stride": (1, 2, 2), "padding": (0, 1, 1)}, {"quantize": True, "normalize_grad": False},
                   {"normalize_t_factor": 0.5}):
            layer = RubiksShift3D(6, **kw).to(dtype)
            x = torch.rand(2, 4, 6, 8, 8, dtype=dtype, requires_grad=True)
            layer(x).sum().backward()
        x, s = torch.rand(2, 4, 6, 8, 8, dtype=dtype), torch.rand(3, 6, dtype=dtype)
        y = p3.rubiks_shift_3d_forward(x, s, 1, 0, quantize=False, output=torch.empty_like(x))
        p3.rubiks_shift_3d_backward(y, x, s, 1, 0, True, 1.0, False, torch.empty_like(x), torch.empty_like(s))
    for kw in ({}, {"stride": 2, "padding": 1}, {"quantize": True, "normalize_grad": False}):
        layer = RubiksShift2D(6, **kw)
        x = torch.rand(2, 6, 8, 8, requires_grad=True)
        layer(x).sum().backward()
    x, s = torch.rand(2, 6, 8, 8), torch.rand(2, 6)
    y = p2.rubiks2d_forward(x, s, 1, 0, False, torch.empty_like(x))
    p2.rubiks2d_backward(y, x, s, 1, 0, True, True, False, torch.empty_like(x), torch.empty_like(s))

    assert {c["fn"] for c in calls} == set(NAMES), sorted({c["fn"] for c in calls})
    with open(os.path.join(HERE, "binding_calls.json"), "w") as f:
        json.dump(calls, f, indent=1)
        f.write("\n")
    print("%d calls recorded" % len(calls))


if __name__ == "__main__":
    main(sys.argv[1])
