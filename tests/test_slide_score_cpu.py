"""CPU-only checks of muse_batch_slide_score_windowed / muse_batch_slide_run_windowed (the slide of a resident group and the
windowed pass over the new rows in one kernel): the exports and the plan hook exist on every layer (headers, library, binding), the
kernel's load width follows the rows' alignment and the parity of the shift, and a NULL batch is refused without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _load import ROOT, pkg


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(muse_[a-z0-9_]+)\s*\(", hdr))


def test_exports_declared_exported_and_bound(muse):
    public = ("muse_batch_slide_score_windowed", "muse_batch_slide_run_windowed")
    for name in public:
        assert name in _declared("muse_hip.h")
    assert "muse_test_slide_score_plan" in _declared("muse_hip_test.h")
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for name in public + ("muse_test_slide_score_plan",):
        assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
        assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    assert len(muse.binding.SIGNATURES["muse_batch_slide_score_windowed"][1]) == 5
    assert len(muse.binding.SIGNATURES["muse_batch_slide_run_windowed"][1]) == 16
    # an addition: the ABI version stays
    assert muse.binding.load().muse_abi_version() == 5


def _plan(muse, N, k, wide):
    lb, sb = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = muse.binding.load().muse_test_slide_score_plan(N, k, 1 if wide else 0, ctypes.byref(lb), ctypes.byref(sb))
    return rc, int(lb.value), int(sb.value)


@pytest.mark.parametrize("N,k,wide,want", [
    (4096, 16, True, (16, 16)), (4096, 1, True, (8, 16)), (4096, 4096, True, (16, 16)), (4096, 4095, True, (8, 16)),
    (4096, 16, False, (8, 8)), (4095, 16, False, (8, 8)), (4095, 1, False, (8, 8)), (2, 0, True, (16, 16)),
])
def test_slide_score_plan_widths(muse, N, k, wide, want):
    assert _plan(muse, N, k, wide) == (0,) + want


def test_slide_score_plan_rule_over_a_sweep(muse):
    """16-byte loads iff the rows are wide and k is even; 16-byte stores iff the rows are wide; rows of an odd length are never wide"""
    for N in (2, 3, 63, 64, 65, 480, 1023, 1024, 1025, 1433, 4096, 5000, 40000, 65536):
        for k in sorted({0, 1, 2, 3, 7, 16, 63, 64, 65, 255, 256, 257, N // 2, N - 1, N}):
            if k > N:
                continue
            for wide in ((False, True) if N % 2 == 0 else (False,)):
                rc, lb, sb = _plan(muse, N, k, wide)
                assert rc == 0, (N, k, wide)
                assert lb == (16 if wide and k % 2 == 0 else 8), (N, k, wide, lb)
                assert sb == (16 if wide else 8), (N, k, wide, sb)


def test_slide_score_plan_refuses_bad_arguments(muse):
    E = muse.binding.MUSE_ERR_INVALID
    L = muse.binding.load()
    assert _plan(muse, 1, 0, False)[0] == E        # N < 2: no series the window pass takes
    assert _plan(muse, 8, -1, False)[0] == E
    assert _plan(muse, 8, 9, False)[0] == E
    assert _plan(muse, 9, 2, True)[0] == E         # rows of an odd length cannot all be 16-byte aligned
    out = ctypes.c_int32(0)
    assert L.muse_test_slide_score_plan(8, 2, 1, None, ctypes.byref(out)) == E
    assert L.muse_test_slide_score_plan(8, 2, 1, ctypes.byref(out), None) == E


def test_null_batch_is_refused_without_a_device(muse):
    B = muse.binding
    t = np.zeros(4)
    assert B.load().muse_batch_slide_score_windowed(None, B.dptr(t), 4, 4, 7) == B.MUSE_ERR_INVALID
    o_s, o_l, o_v = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1)
    cnt, mean = ctypes.c_int32(0), ctypes.c_double(0)
    rc = B.load().muse_batch_slide_run_windowed(None, B.dptr(t), 4, 4, None, 0, 7, 1, 0.0, 0, 1, B.i64ptr(o_s), B.i32ptr(o_l),
                                                B.dptr(o_v), ctypes.byref(cnt), ctypes.byref(mean))
    assert rc == B.MUSE_ERR_INVALID


def test_device_batch_has_both_methods():
    m = pkg().muse
    assert hasattr(m.DeviceBatch, "slide_score_windowed") and hasattr(m.DeviceBatch, "slide_run_windowed")
