"""CPU-only checks of muse_batch_slide_score_in_window / _slide_run_in_window / _slide_run (a resident group slid and scored inside a
window of any width, or unwindowed, in one call): the exports and the hooks exist on every layer with the declared argument counts,
the dispatch (muse_test_slide_in_window_plan) is the table include/muse_hip_test.h gives, restated here, and NULL handles are refused
without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _slidein as SI
from _load import ROOT, pkg

EXPORTS = {"muse_batch_slide_score_in_window": 5, "muse_batch_slide_run_in_window": 16, "muse_batch_slide_run": 16}
HOOKS = {"muse_test_slide_in_window_plan": 5, "muse_test_slide_in_window_force": 2, "muse_test_last_slide_path": 2}


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


# ------------------------------------------------------------------ 1. every layer
def test_exports_declared_exported_and_bound(muse):
    hdrs = {}
    for h in ("muse_hip.h", "muse_hip_test.h"):
        hdrs[h] = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for names, h in ((EXPORTS, "muse_hip.h"), (HOOKS, "muse_hip_test.h")):
        for name, nargs in names.items():
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdrs[h]).group(1)
            assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    for k, v in (("UNSUPPORTED", 0), ("MFMA", 1), ("FUSED", 2), ("TWO_STEP", 3)):
        m = re.search(r"#define\s+MUSE_SLIDE_IN_WINDOW_%s\s+(\d+)" % k, hdrs["muse_hip_test.h"])
        assert m and int(m.group(1)) == v == getattr(muse.binding, "MUSE_SLIDE_IN_WINDOW_" + k)
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_and_documents_carry_the_calls(muse):
    for name in ("slide_score_in_window", "slide_run_in_window", "slide_run", "last_slide_path"):
        assert callable(getattr(muse.DeviceBatch, name, None)), name
    assert callable(getattr(muse.Engine, "slide_in_window_force", None))
    assert callable(getattr(muse, "slide_in_window_plan", None))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name


def test_null_handles_are_refused_without_a_device(muse):
    B = muse.binding
    L = B.load()
    t = np.zeros(4)
    w = ctypes.c_int32(5)
    assert L.muse_batch_slide_score_in_window(None, B.dptr(t), 4, 4, 100) == B.MUSE_ERR_INVALID
    o_s, o_l, o_v = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1)
    cnt, mean = ctypes.c_int32(0), ctypes.c_double(0)
    for fn in (L.muse_batch_slide_run_in_window, L.muse_batch_slide_run):
        rc = fn(None, B.dptr(t), 4, 4, None, 0, 100, 1, 0.0, 0, 1, B.i64ptr(o_s), B.i32ptr(o_l), B.dptr(o_v), ctypes.byref(cnt),
                ctypes.byref(mean))
        assert rc == B.MUSE_ERR_INVALID
    assert L.muse_test_last_slide_path(None, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_slide_in_window_force(None, 1) == B.MUSE_ERR_INVALID


# ------------------------------------------------------------------ 2. the dispatch
NS = (2, 100, 256, 257, 480, 2048, 2049, 3000, 4096, 5000, 65536, 70000)


def _pass_table(muse, N, f32, max_lag):
    """muse_batch_score_in_window's table (include/muse_hip.h), restated: 'plain', 'mfma', 'masked' or None"""
    n = muse.next_pow2(float(N))
    L = min(max_lag, n // 2)
    if L == n // 2:
        return "plain"
    if not f32 and L <= 63 and n <= 65536:
        return "mfma"
    if n in (512, 1024, 2048, 4096):
        return "masked"
    return None


def _table(muse, N, f32, max_lag, k):
    """the rules of muse_test_slide_in_window_plan, restated: the pass's table decides UNSUPPORTED and MFMA; a plain or masked pass is
    FUSED at FFT length 4096 and TWO_STEP at every other length; k takes no part"""
    B = muse.binding
    how = _pass_table(muse, N, f32, max_lag)
    if how is None:
        return B.MUSE_SLIDE_IN_WINDOW_UNSUPPORTED
    if how == "mfma":
        return B.MUSE_SLIDE_IN_WINDOW_MFMA
    return B.MUSE_SLIDE_IN_WINDOW_FUSED if muse.next_pow2(float(N)) == 4096 else B.MUSE_SLIDE_IN_WINDOW_TWO_STEP


def _lags(muse, N):
    n = muse.next_pow2(float(N))
    return (0, 7, 63, 64, 2047, n // 2, 10 * n)


def test_planner_is_the_table(muse):
    B = muse.binding
    seen = set()
    for N in NS:
        for f32 in (False, True):
            for max_lag in _lags(muse, N):
                for k in (0, 1, 16, N):
                    if k > N:       # (N = 2: no series slides by more than its length -- refused, as the call refuses it)
                        w = ctypes.c_int32(-1)
                        assert B.load().muse_test_slide_in_window_plan(N, int(f32), max_lag, k, ctypes.byref(w)) == B.MUSE_ERR_INVALID
                        continue
                    got = muse.slide_in_window_plan(N, f32, max_lag, k)
                    assert got == _table(muse, N, f32, max_lag, k), (N, f32, max_lag, k, got)
                    seen.add(got)
    assert seen == {B.MUSE_SLIDE_IN_WINDOW_UNSUPPORTED, B.MUSE_SLIDE_IN_WINDOW_MFMA, B.MUSE_SLIDE_IN_WINDOW_FUSED,
                    B.MUSE_SLIDE_IN_WINDOW_TWO_STEP}
    # the rows the issue names: the fused kernel serves every window and both storages at FFT length 4096 but the direct product's
    assert muse.slide_in_window_plan(4096, False, 2048, 16) == B.MUSE_SLIDE_IN_WINDOW_FUSED
    assert muse.slide_in_window_plan(3000, False, 256, 1) == B.MUSE_SLIDE_IN_WINDOW_FUSED
    assert muse.slide_in_window_plan(2049, True, 0, 16) == B.MUSE_SLIDE_IN_WINDOW_FUSED
    assert muse.slide_in_window_plan(4096, False, 63, 16) == B.MUSE_SLIDE_IN_WINDOW_MFMA
    assert muse.slide_in_window_plan(480, False, 100, 16) == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
    assert muse.slide_in_window_plan(5000, True, 8192, 16) == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
    assert muse.slide_in_window_plan(5000, False, 100, 16) == B.MUSE_SLIDE_IN_WINDOW_UNSUPPORTED


def test_unsupported_and_mfma_exactly_where_the_pass_is(muse):
    B = muse.binding
    for N in NS:
        for f32 in (False, True):
            for max_lag in _lags(muse, N):
                own = muse.in_window_plan(N, f32, max_lag)
                got = muse.slide_in_window_plan(N, f32, max_lag, 1)
                assert (got == B.MUSE_SLIDE_IN_WINDOW_UNSUPPORTED) == (own == B.MUSE_IN_WINDOW_UNSUPPORTED), (N, f32, max_lag)
                assert (got == B.MUSE_SLIDE_IN_WINDOW_MFMA) == (own == B.MUSE_IN_WINDOW_MFMA), (N, f32, max_lag)


def test_planner_refuses_bad_arguments(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    E = B.MUSE_ERR_INVALID
    assert L.muse_test_slide_in_window_plan(1, 0, 5, 0, ctypes.byref(w)) == E
    assert L.muse_test_slide_in_window_plan(512, 0, -1, 1, ctypes.byref(w)) == E
    assert L.muse_test_slide_in_window_plan(512, 0, 5, -1, ctypes.byref(w)) == E
    assert L.muse_test_slide_in_window_plan(512, 0, 5, 513, ctypes.byref(w)) == E
    assert L.muse_test_slide_in_window_plan(512, 0, 5, 1, None) == E
    assert L.muse_test_slide_in_window_plan(512, 0, 5, 512, ctypes.byref(w)) == 0


# ------------------------------------------------------------------ 3. the oracle case of the GPU suite
def test_oracle_flags_no_tie_on_the_gpu_suites_inputs(oracle):
    """tests/test_gpu_slide_in_window.py excuses no row of its oracle comparison: on its inputs (the slid rows) the oracle has a score
    for every row and no rounding-decided argmax"""
    ref, rows, tails, slid = SI.oracle_case()
    assert slid.shape == (SI.ORACLE_M, SI.ORACLE_N) and np.array_equal(slid[:, -SI.ORACLE_K:], tails)
    olag, omv, gap = oracle.batch_scores(ref, slid, nthreads=4)
    assert not np.isnan(omv).any() and (omv != 0).all()
    assert not (gap < 1e-12).any()
