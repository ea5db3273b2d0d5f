"""CPU-only checks of the lag profiles (muse_batch_lag_profile / _lag_profile_device): the exports and their mirrors exist on every
layer, the planner (muse_test_lag_profile_plan) against a restatement over a grid, the lag checks, and the refusals the Python mirror
makes without reaching the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _load import ROOT, pkg

EXPORTS = (("muse_batch_lag_profile", 7), ("muse_batch_lag_profile_device", 7))
HOOKS = (("muse_test_lag_profile_plan", 7),)
ROWS = 127                                       # 2 MUSE_LAG_WINDOW_MAX + 1: the table rows of one launch


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def fft_len(N):
    n = 1
    while n < N:
        n *= 2
    return n


# ------------------------------------------------------------------ 1. every layer
def test_exports_declared_exported_and_bound(muse):
    hdrs = {}
    for h in ("muse_hip.h", "muse_hip_test.h"):
        hdrs[h] = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for names, h in ((EXPORTS, "muse_hip.h"), (HOOKS, "muse_hip_test.h")):
        for name, nargs in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdrs[h]).group(1)
            assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_the_profile_forms(muse):
    import importlib
    mod = importlib.import_module(muse.__name__ + ".lag_profile")
    for name in ("lag_profile", "lag_profile_into", "lag_profile_plan", "LagProfiles"):
        assert callable(getattr(muse, name, None)), name
        assert getattr(muse, name) is getattr(mod, name)
    # no public callable joins muse.py or its classes: the recorded mirror stays as it is
    for holder in (muse.muse, muse.DeviceBatch, muse.Batch, muse.Muse):
        assert not [a for a in dir(holder) if "profile" in a.lower()], holder
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert "muse_batch_lag_profile(" in hpp
    assert re.search(r"\bLagProfile\s*\(", hpp) and re.search(r"\bLagProfiles\s*\(", hpp)
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert "C.muse_batch_lag_profile(" in go and re.search(r"func \(b \*Batch\) LagProfile\(", go)


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    lib = B.load()
    out = (ctypes.c_double * 4)()
    assert lib.muse_batch_lag_profile(None, None, 0, 0, 3, out, 4) == B.MUSE_ERR_INVALID
    assert lib.muse_last_error()
    assert lib.muse_batch_lag_profile_device(None, None, 0, 0, 3, None, 4) == B.MUSE_ERR_INVALID
    n = ctypes.c_int32(-5)
    one = (ctypes.c_int32 * 1)()
    assert lib.muse_test_lag_profile_plan(480, 0, 3, None, one, one, 1) == B.MUSE_ERR_INVALID
    assert lib.muse_test_lag_profile_plan(480, 0, 3, ctypes.byref(n), None, None, 1) == B.MUSE_ERR_INVALID
    assert lib.muse_test_lag_profile_plan(480, 0, 3, ctypes.byref(n), one, one, -1) == B.MUSE_ERR_INVALID
    assert lib.muse_test_lag_profile_plan(1, 0, 0, ctypes.byref(n), one, one, 1) == B.MUSE_ERR_INVALID
    assert n.value == -5
    assert lib.muse_test_lag_profile_plan(70000, -7, 7, ctypes.byref(n), one, one, 1) == B.MUSE_ERR_UNSUPPORTED
    # cap smaller than the plan: the count is whole, the arrays hold the first cap launches
    two = (ctypes.c_int32 * 2)(-9, -9)
    rows = (ctypes.c_int32 * 2)(-9, -9)
    assert lib.muse_test_lag_profile_plan(4096, -200, 200, ctypes.byref(n), two, rows, 1) == B.MUSE_OK
    assert n.value == 4 and list(two) == [-200, -9] and list(rows) == [ROWS, -9]


# ------------------------------------------------------------------ 2. the planner against its restatement
def restated(lo, hi):
    """consecutive launches of up to 127 lags from lo on, the last one taking what is left"""
    out = []
    while lo <= hi:
        w = min(ROWS, hi - lo + 1)
        out.append((lo, w))
        lo += w
    return out


WIDTHS = (1, 2, 15, 16, 17, 32, 48, 126, 127, 128, 143, 144, 253, 254, 255, 256, 381, 400, 508, 509)


@pytest.mark.parametrize("N", (64, 100, 480, 1433, 4096, 40000, 65536))
def test_plan_matches_the_restatement(muse, N):
    n = fft_len(N)
    lo_min, hi_max = -(n // 2 - 1), n // 2
    assert 127 in WIDTHS and 254 in WIDTHS and 381 in WIDTHS and 16 in WIDTHS and 32 in WIDTHS and 144 in WIDTHS
    seen = 0
    widths = set(WIDTHS) | {n}                                       # every lag of the length too
    for W in sorted(widths):
        if W > n:
            continue
        starts = {lo_min, hi_max - W + 1, -(W // 2), 0, 1, -W, -W + 1, 5}
        for lo in sorted(starts):
            hi = lo + W - 1
            if lo < lo_min or hi > hi_max:
                continue
            plan = muse.lag_profile_plan(N, lo, hi)
            assert plan == restated(lo, hi), (N, lo, hi)
            assert all(1 <= w <= ROWS for _, w in plan)
            assert plan[0][0] == lo and plan[-1][0] + plan[-1][1] - 1 == hi
            assert all(a[0] + a[1] == b[0] for a, b in zip(plan, plan[1:]))          # consecutive: no gap, no overlap
            assert sum(w for _, w in plan) == W
            assert (len(plan) == 1) == (W <= ROWS)
            seen += 1
    assert seen >= 20


@pytest.mark.parametrize("N", (64, 480, 1433, 4096))
def test_plan_refuses_lags_outside_the_length(muse, N):
    B = muse.binding
    n = fft_len(N)
    for lo, hi in ((0, n // 2 + 1), (-(n // 2), 0), (-(n // 2), n // 2), (n // 2 + 1, n // 2 + 1), (-n, -n), (3, 2), (0, -1),
                   (2 ** 31 - 1, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)):
        with pytest.raises(muse.MuseError) as e:
            muse.lag_profile_plan(N, lo, hi)
        assert e.value.status == B.MUSE_ERR_INVALID and e.value.message, (N, lo, hi)
    assert muse.lag_profile_plan(N, -(n // 2 - 1), n // 2) == restated(-(n // 2 - 1), n // 2)   # the widest: every lag


# ------------------------------------------------------------------ 3. the Python mirror's own refusals
class _Never:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


class _FakeBatch:
    """what lag_profile_into reads of a DeviceBatch before it calls C"""

    class dgroup:
        M = 5

    class engine:
        device = 0

    _h = None


def test_lag_profile_into_refuses_before_any_c_call(muse, monkeypatch):
    import importlib
    import torch
    B = muse.binding
    mod = importlib.import_module(muse.__name__ + ".lag_profile")
    monkeypatch.setattr(mod.B, "load", lambda: _Never())
    K, lo, hi = 5, -3, 4
    W = hi - lo + 1
    for tensor, word in ((torch.zeros((K, W), dtype=torch.float32), "float64"),
                         (torch.zeros((K, W), dtype=torch.float64), "device"),
                         (torch.zeros((K, W - 1), dtype=torch.float64), "shape"),
                         (torch.zeros((K * W,), dtype=torch.float64), "shape"),
                         (torch.zeros((K, 2 * W), dtype=torch.float64)[:, ::2], "contiguous"),
                         (np.zeros((K, W)), "torch")):
        with pytest.raises(muse.MuseError) as e:
            muse.lag_profile_into(_FakeBatch, lo, hi, tensor)
        assert e.value.status == B.MUSE_ERR_INVALID and word in e.value.message, (word, e.value.message)
    # a list sets the rows: [3, W] for three entries, the group's five are wrong then
    with pytest.raises(muse.MuseError) as e:
        muse.lag_profile_into(_FakeBatch, lo, hi, torch.zeros((K, W), dtype=torch.float64), series=[0, 1, 1])
    assert e.value.status == B.MUSE_ERR_INVALID and "[3, %d]" % W in e.value.message


def test_lag_profiles_refuses_a_sharded_batch(muse):
    class Sharded:
        _engines = [object(), object()]

    with pytest.raises(muse.MuseError) as e:
        muse.LagProfiles(Sharded(), 1, 15, scores=[])
    assert e.value.status == muse.binding.MUSE_ERR_UNSUPPORTED and "one device" in e.value.message and "2 engines" in e.value.message
