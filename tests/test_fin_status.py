"""The give-up record of the in-launch finalizers (include/rubiks_hip.h: rk_fin_status_register), the part that needs no
GPU: the two entry points are exported with the declared signatures, the record is 16 bytes, and a machine without a
device is told so by the library and left alone by the Python layer."""
import ctypes
import os
import re

import torch

from rubiksnet_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rubiks_hip.h")).read()

_CTYPE = {"void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
          "float": ctypes.c_float, "rk_stream_t": ctypes.c_void_p}


def _declared(name):
    """(restype, argtypes) of `name` as include/rubiks_hip.h declares it"""
    m = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % name, HEADER, re.M)
    assert m, "%s is not declared in include/rubiks_hip.h" % name
    args = []
    for a in m.group(2).split(","):
        typ = re.sub(r"\s*\w+$", "", " ".join(a.split())).replace(" *", "*")      # drop the parameter's name
        args.append(_CTYPE[typ])
    return _CTYPE[m.group(1)], args


def test_the_two_entry_points_are_exported_with_the_declared_signatures():
    handle = ctypes.CDLL(_native.LIB_PATH)
    for name in ("rk_fin_status_register", "rk3d_debug_finalize_only_status_f32"):
        assert hasattr(handle, name), "librubiks_hip.so does not export %s" % name
        res, args = _declared(name)
        assert name in _native.SIGNATURES, "%s is missing from _native.SIGNATURES" % name
        assert _native.SIGNATURES[name] == (res, args), name
    assert len(_native.SIGNATURES["rk_fin_status_register"][1]) == 1
    # the finalize-only hook + one pointer (the record) in front of the stream
    old = _native.SIGNATURES["rk3d_debug_finalize_only_f32"][1]
    assert _native.SIGNATURES["rk3d_debug_finalize_only_status_f32"][1] == old[:-1] + [ctypes.c_void_p, old[-1]]


def test_the_record_is_16_bytes():
    m = re.search(r"^#define\s+RK_FIN_STATUS_BYTES\s+(\d+)\s*$", HEADER, re.M)
    assert m and int(m.group(1)) == 16


def test_the_debug_hook_validates_before_it_touches_a_device():
    L = _native.lib()
    one = ctypes.c_void_p(16)
    assert L.rk3d_debug_finalize_only_status_f32(None, 1 << 20, 4, 8, one, 1, 1.0, None, None) == -1
    assert L.rk3d_debug_finalize_only_status_f32(one, 1 << 20, 0, 8, one, 1, 1.0, None, None) == -2
    assert L.rk3d_debug_finalize_only_status_f32(one, 1 << 20, 4, 8, one, 1, 1.0, ctypes.c_void_p(20), None) == -2   # misaligned record
    assert L.rk3d_debug_finalize_only_status_f32(one, 16, 4, 8, one, 1, 1.0, None, None) == -4


def test_without_a_device_registering_says_so_and_poll_is_silent():
    from rubiksnet_amd import fin_status
    import rubiksnet_amd

    assert rubiksnet_amd.fin_status is fin_status and "fin_status" in rubiksnet_amd.__all__
    if torch.cuda.is_available():          # (with a device: tests/test_fin_status_gpu.py; unregistering here would outlive this test)
        return
    assert _native.lib().rk_fin_status_register(None) == -6          # RK_ERR_NO_DEVICE
    assert fin_status.poll() is None
    assert fin_status.poll(sync=True) is None
    assert fin_status.poll(device="cpu") is None
