"""The Python bindings ask the same of librubiks_hip, and get the same bits back, as the commit the golden was recorded on.

tests/golden/gen_binding_trace_golden.py holds the scenarios (one per route of `conv1x1`, the stem, `bn_relu*`, the fused
blocks, a RubiksNet-Tiny train step and eval forward) and the recorder; tests/golden/binding_trace_parent.json.gz is its
output.  Each scenario is replayed here under the same recorder: the list of calls into the library -- entry names,
integer and float arguments, which pointers are null, which stream, what the workspace / tile queries returned -- and the
SHA-256 of every output and gradient must be identical (the kernels sum in a fixed order, without atomics)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_binding_trace_golden",
                                               os.path.join(_GOLDEN_DIR, "gen_binding_trace_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return gen.load()


def test_golden_covers_every_scenario(golden):
    assert sorted(golden) == sorted(gen.SCENARIOS)
    for name, rec in golden.items():
        assert (rec["digests"] is None) == (name in gen.TRACE_ONLY), name
        assert bool(rec["calls"]) == (gen.SCENARIOS[name][2] is not None), name


@pytest.mark.parametrize("name", list(gen.SCENARIOS))
def test_same_calls_same_bits(golden, name):
    got, want = gen.run(name), golden[name]
    assert len(got["calls"]) == len(want["calls"]), "%d calls, the golden has %d: %r" % (
        len(got["calls"]), len(want["calls"]), [c[0] for c in got["calls"]])
    for k, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, "call %d differs" % k
    assert got["digests"] == want["digests"]
