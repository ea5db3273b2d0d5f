"""CPU-only checks of the window as an argument (muse_batch_score_in_window / _run_in_window): the exports and their mirrors exist on
every layer, the dispatch (muse_test_in_window_plan) is the table include/muse_hip.h gives, the masking rule of the WIN kernels --
out-of-window entries replaced by +0.0, then the unrestricted maxAbsIndex -- equals the lag-window definition (tests/_window.py) on
the oracle's correlations, and the oracle by itself flags no tie on the inputs tests/test_gpu_in_window.py uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _inwindow as IW
import _window as W
from _load import ROOT, pkg

EXPORTS = ("muse_batch_score_in_window", "muse_batch_run_in_window")
HOOKS = ("muse_test_in_window_plan", "muse_test_in_window_force_transform", "muse_test_last_in_window_path")


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _same(a, b):
    return a[0] == b[0] and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1])))


# ------------------------------------------------------------------ 1. every layer
def test_exports_declared_exported_and_bound(muse):
    hdrs = {}
    for h in ("muse_hip.h", "muse_hip_test.h"):
        hdrs[h] = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for names, h in ((EXPORTS, "muse_hip.h"), (HOOKS, "muse_hip_test.h")):
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    # the prototypes: argument counts of the header and of the binding agree
    for name, nargs in (("muse_batch_score_in_window", 2), ("muse_batch_run_in_window", 13), ("muse_test_in_window_plan", 4),
                        ("muse_test_in_window_force_transform", 2), ("muse_test_last_in_window_path", 2)):
        h = hdrs["muse_hip.h"] if name in EXPORTS else hdrs["muse_hip_test.h"]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, h).group(1)
        assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    # MUSE_LAG_WINDOW_MAX keeps its value and its meaning: the widest window of the direct product
    m = re.search(r"#define\s+MUSE_LAG_WINDOW_MAX\s+(\d+)", hdrs["muse_hip.h"])
    assert m and int(m.group(1)) == muse.binding.MUSE_LAG_WINDOW_MAX == 63
    for k, v in (("UNSUPPORTED", 0), ("PLAIN", 1), ("MFMA", 2), ("MASKED", 3)):
        m = re.search(r"#define\s+MUSE_IN_WINDOW_%s\s+(\d+)" % k, hdrs["muse_hip_test.h"])
        assert m and int(m.group(1)) == v == getattr(muse.binding, "MUSE_IN_WINDOW_" + k)
    assert muse.binding.load().muse_abi_version() == 5               # backward compatible additions: the ABI version stays


def test_mirrors_carry_run_in_window(muse):
    assert callable(getattr(muse.Batch, "RunInWindow", None))
    for name in ("score_in_window", "run_in_window", "last_in_window_path"):
        assert callable(getattr(muse.DeviceBatch, name, None)), name
    assert callable(getattr(muse.Engine, "in_window_force_transform", None))
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bvoid\s+RunInWindow\s*\(", hpp) and "muse_batch_run_in_window(" in hpp
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func \(b \*Batch\) RunInWindow\(groupByLabels \[\]string\) error", go) and "C.muse_batch_run_in_window(" in go
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    # the C++ program the GPU suite runs is built with the rest
    assert os.path.exists(muse.build.build_in_window_test())


def test_no_gpu_fails_loudly_not_with_a_crash(muse):
    import torch
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    assert L.muse_batch_score_in_window(None, 100) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_in_window(None, None, 0, 100, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert L.muse_test_last_in_window_path(None, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_in_window_force_transform(None, 1) == B.MUSE_ERR_INVALID
    assert L.muse_test_in_window_plan(1, 0, 5, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_in_window_plan(512, 0, -1, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_in_window_plan(512, 0, 5, None) == B.MUSE_ERR_INVALID
    if torch.cuda.is_available():
        return
    with pytest.raises(muse.MuseError) as e:
        eng = muse.Engine(0)
        dg = muse.DeviceGroup.from_rows(eng, np.zeros((2, 512)))
        muse.DeviceBatch(eng, dg, np.arange(512.0)).score_in_window(100)
    assert e.value.status == B.MUSE_ERR_NO_DEVICE


# ------------------------------------------------------------------ 2. the dispatch
def _table(muse, N, f32, max_lag):
    """the table of include/muse_hip.h (muse_batch_score_in_window), restated"""
    B = muse.binding
    n = muse.next_pow2(float(N))
    L = min(max_lag, n // 2)
    if L == n // 2:
        return B.MUSE_IN_WINDOW_PLAIN
    if not f32 and L <= 63 and n <= 65536:
        return B.MUSE_IN_WINDOW_MFMA
    if n in (512, 1024, 2048, 4096):
        return B.MUSE_IN_WINDOW_MASKED
    return B.MUSE_IN_WINDOW_UNSUPPORTED


@pytest.mark.parametrize("N", [2, 64, 255, 480, 512, 1433, 3000, 4096, 5000, 70000])
def test_plan_is_the_table(muse, N):
    B = muse.binding
    n = muse.next_pow2(float(N))
    for f32 in (False, True):
        for max_lag in (0, 63, 64, n // 2 - 1, n // 2, n // 2 + 5):
            assert muse.in_window_plan(N, f32, max_lag) == _table(muse, N, f32, max_lag), (N, f32, max_lag)
    # the cells the issue spells out
    if N in (480, 512, 1433, 3000, 4096):
        assert muse.in_window_plan(N, False, 64) == B.MUSE_IN_WINDOW_MASKED
        assert muse.in_window_plan(N, True, 0) == B.MUSE_IN_WINDOW_MASKED
        assert muse.in_window_plan(N, False, 63) == B.MUSE_IN_WINDOW_MFMA
    if N in (64, 255, 5000, 70000):
        assert muse.in_window_plan(N, True, 0) == B.MUSE_IN_WINDOW_UNSUPPORTED
        assert muse.in_window_plan(N, False, 0) == (B.MUSE_IN_WINDOW_MFMA if N <= 65536 else B.MUSE_IN_WINDOW_UNSUPPORTED)
    if N in (5000, 70000):
        assert muse.in_window_plan(N, False, 64) == B.MUSE_IN_WINDOW_UNSUPPORTED
    if N == 70000:
        assert muse.in_window_plan(N, False, 65536) == muse.in_window_plan(N, True, 70000) == B.MUSE_IN_WINDOW_PLAIN
    assert muse.in_window_plan(N, False, n // 2) == muse.in_window_plan(N, True, 10 * n) == B.MUSE_IN_WINDOW_PLAIN


# ------------------------------------------------------------------ 3. the masking rule is the definition
def _ccs(oracle, N, M, seed):
    ref, rows = W.make_case(N, M, seed=seed)
    X, n = oracle.ref_spectrum(ref)
    return [oracle.xcorr_with_x(X, y, n)[0] for y in rows], n


def _with_edge_rows(ccs, n, L, rng):
    """the make_case correlations plus: a NaN planted outside the window, an all-zero window around a far winner, and a window of
    zeros with NaN outside"""
    out = list(ccs)
    base = next(c for c in ccs if c is not None and not np.isnan(c).any())
    outside = np.arange(min(L, n // 2) + 1, n - min(L, n // 2))
    if len(outside):
        a = base.copy()
        a[rng.choice(outside)] = np.nan
        out.append(a)
        b = np.zeros(n)
        b[rng.choice(outside)] = 0.75
        out.append(b)
        c = np.zeros(n)
        c[outside] = np.nan
        out.append(c)
    return out


def test_masking_rule_equals_the_definition_every_window_at_512(oracle):
    ccs, n = _ccs(oracle, 512, 12, seed=5)
    assert n == 512 and any(c is None for c in ccs)                   # (the constant row: sigma == 0)
    rng = np.random.default_rng(1)
    for L in range(0, n // 2 + 1):
        for cc in _with_edge_rows(ccs, n, L, rng):
            want = W.windowed(cc, n, L)[:2]
            assert _same(IW.masked_argmax(cc, n, L), want), L
            assert _same(IW.masked_argmax_fast(cc, n, L), want), L


@pytest.mark.parametrize("N", [4096, 3000])
def test_masking_rule_equals_the_definition_at_4096(oracle, N):
    ccs, n = _ccs(oracle, N, 12, seed=6)
    assert n == 4096
    rng = np.random.default_rng(2)
    for L in (0, 1, 63, 64, 65, 100, 255, 256, 257, 511, 512, 1000, 1024, 2047, 2048, 5000):
        for cc in _with_edge_rows(ccs, n, L, rng):
            want = W.windowed(cc, n, L)[:2]
            assert _same(IW.masked_argmax_fast(cc, n, L), want), L
        assert _same(IW.masked_argmax(ccs[0], n, L), W.windowed(ccs[0], n, L)[:2])


def test_masking_rule_edge_cases():
    n = 16
    cc = np.zeros(n)
    assert IW.masked_argmax(cc, n, 3) == (0, 0.0)
    cc[9] = np.nan                                                   # a NaN outside +-3 does not survive; inside +-7 it is skipped
    cc[2] = -0.5
    assert IW.masked_argmax(cc, n, 3) == (2, -0.5) == W.windowed(cc, n, 3)[:2]
    assert IW.masked_argmax(cc, n, 7) == (2, -0.5) == W.windowed(cc, n, 7)[:2]
    cc[:] = np.nan
    l, v = IW.masked_argmax(cc, n, 3)
    assert l == 0 and np.isnan(v)                                    # cc[0] is always inside
    cc = np.zeros(n)
    cc[8] = 1.0                                                      # index n / 2 is lag +n/2: inside only at L = n / 2
    assert IW.masked_argmax(cc, n, 7) == (0, 0.0) and IW.masked_argmax(cc, n, 8) == (8, 1.0)
    assert IW.masked_argmax(None, n, 3) == (0, 0.0)


# ------------------------------------------------------------------ 4. the oracle flags no tie the GPU tests could hide behind
def _noise_ties_within_cap(tie, keep):
    return int((tie & keep).sum()) * 1000 <= len(tie)               # tests/test_gpu_lag_window.py: at most 1 in 1000 noise rows


@pytest.mark.parametrize("N", IW.PARITY_NS)
def test_oracle_flags_no_tie_parity_inputs(oracle, N):
    ref, rows = IW.parity_case(N)
    n = muse_n = 1 << (N - 1).bit_length()
    exp, _, _, n2 = W.expect(oracle, ref, rows, IW.parity_Ls(n))
    assert n2 == muse_n
    keep = W.plain_rows(IW.PARITY_M)
    for L in IW.parity_Ls(n):
        assert _noise_ties_within_cap(exp[L][2], keep), (N, L)


@pytest.mark.parametrize("N", IW.EDGE_NS)
def test_oracle_flags_no_tie_planted_inputs(oracle, N):
    ref, rows, n, where = IW.edge_case(N)
    exp, _, _, _ = W.expect(oracle, ref, rows, IW.edge_Ls(n))
    for L in IW.edge_Ls(n):
        assert not exp[L][2].any(), (N, L)                           # planted rows: zero ties
        r, lags = where[L]
        inside = np.abs(lags) <= L
        assert np.array_equal(exp[L][0][r][inside], lags[inside])    # the definition finds the planted lag where it is inside
        assert np.all(np.abs(exp[L][0][r]) <= L)


def test_oracle_flags_no_tie_other_inputs(oracle):
    ref, rows = IW.redo_case()
    exp, _, _, _ = W.expect(oracle, ref, rows, (IW.REDO_L,))
    assert _noise_ties_within_cap(exp[IW.REDO_L][2], W.plain_rows(IW.REDO_M))
    for N in IW.F32_NS:
        ref, rows = IW.f32_case(N)
        exp, _, _, _ = W.expect(oracle, ref, rows, IW.F32_LS)
        for L in IW.F32_LS:
            assert _noise_ties_within_cap(exp[L][2], W.plain_rows(IW.F32_M)), (N, L)
    ref, rows = IW.run_case()
    exp, _, _, _ = W.expect(oracle, ref, rows, (IW.RUN_L,))
    assert _noise_ties_within_cap(exp[IW.RUN_L][2], W.plain_rows(IW.RUN_M))
