"""The give-up record of the in-launch finalizers, Python side (include/rubiks_hip.h: rk_fin_status_register).

Every streaming backward finishes its per-channel sums inside the producing launch; a finalizer wave that never sees its
partials gives up after ~2 s and writes NaN into d(shift) / the BatchNorm sums -- long after the entry point returned
RK_OK.  With a record registered for the device, that launch also counts itself in 16 bytes of device memory:
[give-ups, first launch tag, last launch tag, 0].  This module owns one such record per device and looks at it without
ever making the host wait:

    record(device)   allocate + register the device's record (once; kept for the life of the process)
    ensure(device)   the same, as the operators call it in front of a launch
    poll()           raise RubiksHipError when a snapshot of a record shows a give-up; queue the next snapshot

dp.train_step polls after optimizer.step(): a give-up in step k raises at the end of step k + 1 at the latest.
poll(sync=True) waits for a fresh snapshot: the check before a checkpoint is written, or at the end of an epoch.
"""
import threading

import torch

from . import _native

_lock = threading.Lock()
_records = {}          # device index -> _Record


class _Record:
    __slots__ = ("index", "dev", "host", "event", "in_flight")

    def __init__(self, index):
        self.index = index
        self.dev = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", index))
        self.host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.in_flight = False          # a snapshot has been queued and not yet looked at


def _index(device):
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, int):
        return device
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("fin_status: %s is not a GPU" % (device,))
    return torch.cuda.current_device() if device.index is None else device.index


def record(device=None):
    """The device's give-up record, an int32[4] device tensor, allocated zeroed and registered on first use."""
    index = _index(device)
    rec = _records.get(index)
    if rec is None:
        with _lock:
            rec = _records.get(index)
            if rec is None:
                with torch.cuda.device(index):
                    rec = _Record(index)
                    # the zeros must be there before any launch on any stream can report into them (once per device)
                    torch.cuda.current_stream().synchronize()
                    _native.call("rk_fin_status_register", rec.dev.data_ptr())
                _records[index] = rec
    return rec.dev


def ensure(device):
    """Called in front of every launch with in-launch finalizers: the device has its record registered.  A dictionary
    lookup once it has.  (Not from inside a graph capture, which may neither allocate nor synchronise: a launch captured
    before the first eager one carries whatever was registered then.)"""
    index = _index(device)
    if index not in _records and not torch.cuda.is_current_stream_capturing():
        record(index)


def _inspect(rec, errors):
    rec.in_flight = False
    failed, first, last = (int(v) & 0xffffffff for v in rec.host[:3].tolist())
    if failed:
        rec.dev.zero_()              # queued on the current stream: the next snapshot starts from a clean record
        errors.append("cuda:%d: %d in-launch finalizer(s) gave up waiting for their partials (launch tags: first %#010x, "
                      "last %#010x); the d(shift) / BatchNorm sums of those launches are NaN"
                      % (rec.index, failed, first, last))


def poll(device=None, sync=False):
    """Look at the records (of `device`, or of every device that has one) and raise RubiksHipError for a give-up.

    Per device: if the snapshot queued by an earlier poll has completed, read it -- on a give-up queue the zeroing of the
    device record and raise; then queue a new 16-byte snapshot behind the work already on the current stream (at most one
    in flight).  Never waits unless sync=True, which waits for the snapshot just queued and reads that one too.  Does
    nothing for a device without a record (CPU runs) and nothing while the current stream is capturing."""
    if not _records or (device is not None and not isinstance(device, int) and torch.device(device).type != "cuda"):
        return
    errors = []
    with _lock:
        recs = list(_records.values()) if device is None else [r for r in (_records.get(_index(device)),) if r]
        for rec in recs:
            with torch.cuda.device(rec.index):
                if torch.cuda.is_current_stream_capturing():
                    continue
                if rec.in_flight and (sync or rec.event.query()):
                    rec.event.synchronize()
                    _inspect(rec, errors)
                if not rec.in_flight:
                    rec.host.copy_(rec.dev, non_blocking=True)
                    rec.event.record()
                    rec.in_flight = True
                if sync:
                    rec.event.synchronize()
                    _inspect(rec, errors)
    if errors:
        raise _native.RubiksHipError("; ".join(errors))
