"""The give-up record of the in-launch finalizers (include/rubiks_hip.h: rk_fin_status_register; rk_dma.hpp: fin_collect;
rubiksnet_amd/fin_status.py).  A finalizer wave that gives up still writes NaN; with a record it also counts itself and
leaves its launch tag, the Python layer turns that into a RubiksHipError without making the host wait, and a reduction that
is ready touches nothing.  Every deliberate give-up goes through the finalize-only hook (no producer launch is made to
fail), with the poll budget cut to a few thousand polls and restored in `finally`."""
import copy
import threading

import numpy as np
import pytest
import torch

from _util import DEV

pytestmark = pytest.mark.gpu

C_GIVE, P_GIVE = 48, 100          # one finalizer wave per channel (grid = C): 48 give-ups per launch


def _words(rec):
    """the record as unsigned words"""
    return [int(v) & 0xffffffff for v in rec.cpu().tolist()]


def _give_up(record_ptr, dev=DEV, old_hook=False):
    """Only the finalizer waves, over a zero workspace nobody publishes to.  Returns (d(shift), the launch's tag)."""
    from rubiksnet_amd import _native
    L = _native.lib()
    prev = L.rk_debug_set_finalize_spins(4000)
    try:
        with torch.cuda.device(dev):
            ws = torch.zeros(C_GIVE * 3 * P_GIVE * 16, dtype=torch.uint8, device=dev)
            gs = torch.zeros(3, C_GIVE, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            tag = int(L.rk_debug_peek_launch_tag())
            if old_hook:
                rc = L.rk3d_debug_finalize_only_f32(ws.data_ptr(), ws.numel(), C_GIVE, P_GIVE, gs.data_ptr(), 1, 1.0, stream)
            else:
                rc = L.rk3d_debug_finalize_only_status_f32(ws.data_ptr(), ws.numel(), C_GIVE, P_GIVE, gs.data_ptr(), 1, 1.0,
                                                           record_ptr, stream)
            _native.check(rc, "finalize_only")
            torch.cuda.synchronize()
    finally:
        L.rk_debug_set_finalize_spins(prev)
    return gs, tag


def _registered_clean_record(dev=DEV):
    """the device's registered record, which every test here leaves as it found it: zero"""
    from rubiksnet_amd import fin_status
    rec = fin_status.record(dev)
    fin_status.poll(device=dev, sync=True)
    assert _words(rec) == [0, 0, 0, 0]
    return rec


def test_the_record_counts_give_ups_and_keeps_the_first_and_the_last_tag():
    rec = torch.zeros(4, dtype=torch.int32, device=DEV)
    gs, tag = _give_up(rec.data_ptr())
    assert _words(rec) == [C_GIVE, tag, tag, 0]
    assert torch.isnan(gs).all(), "the NaN stays"
    gs, tag2 = _give_up(rec.data_ptr())
    assert tag2 != tag
    assert _words(rec) == [2 * C_GIVE, tag, tag2, 0]
    assert torch.isnan(gs).all()


def test_a_ready_reduction_writes_nothing():
    """The pre-filled workspace of test_finalizer_gpu.py::test_a_finalizer_accepts_exactly_this_launchs_pairs: every pair
    carries this launch's tag, the finalizers sum them -- the record stays zero and d(shift) is what it is without one."""
    from rubiksnet_amd import _native
    L = _native.lib()
    C, P = 5, 70
    vals = np.random.default_rng(0).uniform(-1, 1, (C, 3, P)).astype(np.float32)
    bits = vals.view(np.uint32)

    def run(record_ptr):
        tag = int(L.rk_debug_peek_launch_tag())
        gran = np.empty((C, 3, P, 4), dtype=np.uint32)
        gran[..., 0] = bits
        gran[..., 1] = tag
        gran[..., 2] = ~bits
        gran[..., 3] = (tag * 2654435761 ^ 0x9e3779b9) & 0xffffffff
        ws = torch.from_numpy(gran.reshape(-1).view(np.uint8)).to(DEV)
        gs = torch.zeros(3, C, device=DEV)
        _native.check(L.rk3d_debug_finalize_only_status_f32(ws.data_ptr(), ws.numel(), C, P, gs.data_ptr(), 1, 1.0, record_ptr,
                                                            torch.cuda.current_stream().cuda_stream), "finalize_only")
        torch.cuda.synchronize()
        return gs

    rec = torch.zeros(4, dtype=torch.int32, device=DEV)
    with_record = run(rec.data_ptr())
    without = run(None)
    assert _words(rec) == [0, 0, 0, 0]
    assert torch.isfinite(with_record).all()
    assert torch.equal(with_record, without)


def test_null_is_silent_even_with_a_record_registered():
    rec = _registered_clean_record()
    gs, _ = _give_up(None)
    assert torch.isnan(gs).all()
    assert _words(rec) == [0, 0, 0, 0]
    gs, _ = _give_up(None, old_hook=True)             # rk3d_debug_finalize_only_f32 never reports
    assert torch.isnan(gs).all()
    assert _words(rec) == [0, 0, 0, 0]


def test_poll_raises_once_and_zeroes_the_record():
    from rubiksnet_amd import _native, fin_status
    rec = _registered_clean_record()
    _, tag = _give_up(rec.data_ptr())
    with pytest.raises(_native.RubiksHipError, match=r"cuda:0: %d in-launch" % C_GIVE) as e:
        fin_status.poll(sync=True)
    assert "%#010x" % tag in str(e.value) and "NaN" in str(e.value)
    fin_status.poll(sync=True)
    torch.cuda.synchronize()
    assert _words(rec) == [0, 0, 0, 0]


def _tiny(variant="rubiks3d"):
    from rubiksnet_amd import RubiksNet
    torch.manual_seed(0)
    net = RubiksNet("tiny", num_classes=4, num_frames=8, variant=variant, verbose=False).to(DEV)
    clips = torch.randn(2, 8, 3, 224, 224, device=DEV)
    labels = torch.tensor([1, 3], device=DEV)
    return net, clips, labels


def test_train_step_raises_by_the_end_of_the_next_step_without_a_sync():
    from rubiksnet_amd import _native, dp, fin_status
    rec = _registered_clean_record()
    net, clips, labels = _tiny()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    _give_up(rec.data_ptr())
    with pytest.raises(_native.RubiksHipError, match=r"%d in-launch" % C_GIVE):
        dp.train_step(net, opt, clips, labels)             # queues a snapshot at the latest
        torch.cuda.synchronize()
        dp.train_step(net, opt, clips, labels)             # ... which this one finds completed
    assert torch.isfinite(dp.train_step(net, opt, clips, labels))
    fin_status.poll(sync=True)
    assert _words(rec) == [0, 0, 0, 0]


@pytest.mark.parametrize("variant", ["rubiks3d", "rubiks3d-aq"])
def test_healthy_training_leaves_the_record_clean_and_the_arithmetic_untouched(variant):
    from rubiksnet_amd import _native, dp, fin_status
    L = _native.lib()
    rec = _registered_clean_record()
    net, clips, labels = _tiny(variant)
    twin = copy.deepcopy(net)
    loss = dp.train_step(net, torch.optim.SGD(net.parameters(), lr=0.01), clips, labels)
    fin_status.poll(sync=True)
    assert _words(rec) == [0, 0, 0, 0]
    try:
        with torch.cuda.device(DEV):
            _native.check(L.rk_fin_status_register(None), "unregister")
        loss_plain = dp.train_step(twin, torch.optim.SGD(twin.parameters(), lr=0.01), clips, labels)
        torch.cuda.synchronize()
    finally:
        with torch.cuda.device(DEV):
            _native.check(L.rk_fin_status_register(rec.data_ptr()), "register")
    assert torch.isfinite(loss) and torch.equal(loss, loss_plain)
    for (name, p), q in zip(net.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), name
    fin_status.poll(sync=True)
    assert _words(rec) == [0, 0, 0, 0]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_records_are_per_device():
    from rubiksnet_amd import _native, fin_status
    rec0 = _registered_clean_record("cuda:0")
    rec1 = _registered_clean_record("cuda:1")
    assert rec0.device.index == 0 and rec1.device.index == 1
    _give_up(rec1.data_ptr(), dev="cuda:1")
    fin_status.poll(device=0, sync=True)
    assert _words(rec0) == [0, 0, 0, 0]
    with pytest.raises(_native.RubiksHipError, match=r"cuda:1: %d in-launch" % C_GIVE):
        fin_status.poll(device=1, sync=True)
    fin_status.poll(sync=True)


def test_registration_is_thread_safe():
    from rubiksnet_amd import fin_status
    got = [None] * 8
    start = threading.Barrier(8)

    def work(i):
        start.wait()
        got[i] = fin_status.record(DEV)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(g is got[0] for g in got) and got[0] is fin_status.record(DEV)
    assert got[0].dtype == torch.int32 and got[0].numel() == 4 and got[0].device == torch.device(DEV)
