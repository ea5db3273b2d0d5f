"""CPU-only checks of the one-sided / asymmetric lag window (muse_batch_score_in_lag_range / _run_in_lag_range): the exports and
their mirrors exist on every layer, the dispatch (muse_test_lag_range_plan) is the table include/muse_hip.h gives and agrees with
muse_test_in_window_plan on symmetric ranges, the numpy helper (tests/_lagrange.py) is the definition, the two kernels' rules --
the product table's position-to-lag mapping with an origin, the two-bound mask -- restated in numpy equal it, and the oracle by
itself flags no tie on the inputs tests/test_gpu_lag_range.py uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagrange as LR
import _window as W
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_in_lag_range", 3), ("muse_batch_run_in_lag_range", 14))
HOOKS = (("muse_test_lag_range_plan", 5), ("muse_test_last_in_window_path", 2))


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
        for name, nargs in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdrs[h]).group(1)
            assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    at = go.index("C.muse_batch_run_in_lag_range(") + len("C.muse_batch_run_in_lag_range(")
    depth, commas = 1, 0
    while depth:                                                     # the call's arguments: commas outside nested parentheses
        c = go[at]
        depth += (c == "(") - (c == ")")
        commas += c == "," and depth == 1
        at += 1
    assert commas + 1 == 14
    assert re.search(r"func \(b \*Batch\) RunInLagRange\(groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_run_in_lag_range(muse):
    assert callable(getattr(muse.Batch, "RunInLagRange", None))
    for name in ("score_in_lag_range", "scores_in_lag_range", "run_in_lag_range"):
        assert callable(getattr(muse.DeviceBatch, name, None)), name
    assert callable(getattr(muse, "lag_range_plan", None))
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bvoid\s+RunInLagRange\s*\(", hpp) and "muse_batch_run_in_lag_range(" in hpp
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    assert os.path.exists(muse.build.build_lag_range_test())          # the C++ program the GPU suite runs is built with the rest


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    assert L.muse_batch_score_in_lag_range(None, -7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_in_lag_range(None, None, 0, -7, 0, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert L.muse_test_lag_range_plan(1, 0, -5, 5, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_lag_range_plan(512, 0, 1, 5, ctypes.byref(w)) == B.MUSE_ERR_INVALID     # excludes lag 0
    assert L.muse_test_lag_range_plan(512, 0, -5, -1, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert L.muse_test_lag_range_plan(512, 0, -5, 5, None) == B.MUSE_ERR_INVALID


# ------------------------------------------------------------------ 2. the dispatch
def _table(muse, N, f32, lo, hi):
    """the table of include/muse_hip.h (muse_batch_score_in_lag_range), restated"""
    B = muse.binding
    n = muse.next_pow2(float(N))
    hi = min(hi, n // 2)
    lo = max(lo, -(n // 2 - 1))
    if hi == n // 2 and lo == -(n // 2 - 1):
        return B.MUSE_IN_WINDOW_PLAIN
    if not f32 and n <= 65536 and hi - lo + 1 <= 127:
        return B.MUSE_IN_WINDOW_MFMA
    if n in (512, 1024, 2048, 4096):
        return B.MUSE_IN_WINDOW_MASKED
    return B.MUSE_IN_WINDOW_UNSUPPORTED


PLAN_NS = [2, 64, 255, 480, 512, 1433, 3000, 4096, 5000, 40000, 70000]


@pytest.mark.parametrize("N", PLAN_NS)
def test_plan_is_the_table(muse, N):
    n = muse.next_pow2(float(N))
    ends = sorted(e for e in {0, 1, 7, 15, 16, 26, 40, 60, 63, 64, 100, 126, 127, 200, 300, n // 2 - 2, n // 2 - 1, n // 2,
                              n // 2 + 1, 10 * n} if e >= 0)
    for f32 in (False, True):
        for a in ends:
            for b in ends:
                assert muse.lag_range_plan(N, f32, -a, b) == _table(muse, N, f32, -a, b), (N, f32, -a, b)
        for L in ends:                                               # symmetric: muse_batch_score_in_window's table, row for row
            assert muse.lag_range_plan(N, f32, -L, L) == muse.in_window_plan(N, f32, L), (N, f32, L)


def test_plan_pinned_rows(muse):
    B = muse.binding
    P = muse.lag_range_plan
    assert P(4096, False, -126, 0) == B.MUSE_IN_WINDOW_MFMA
    assert P(4096, False, -127, 0) == B.MUSE_IN_WINDOW_MASKED
    assert P(4096, True, -7, 0) == B.MUSE_IN_WINDOW_MASKED
    assert P(5000, False, -126, 0) == B.MUSE_IN_WINDOW_MFMA
    assert P(5000, False, -127, 0) == B.MUSE_IN_WINDOW_UNSUPPORTED
    assert P(70000, False, 0, 7) == B.MUSE_IN_WINDOW_UNSUPPORTED
    assert P(200, False, -100, 60) == B.MUSE_IN_WINDOW_UNSUPPORTED
    for f32 in (False, True):
        assert P(4096, f32, -2047, 2048) == P(4096, f32, -5000, 5000) == P(4096, f32, -2047, 1 << 30) == B.MUSE_IN_WINDOW_PLAIN
        assert P(4096, f32, -2046, 2048) == P(4096, f32, -2047, 2047) == B.MUSE_IN_WINDOW_MASKED


def test_five_plan_hooks_are_one_planner(muse):
    """the identities the five plan hooks share now that each is a call of one function: range(-L, L) is window(L); many(R) is
    the single plan with MASKED read as MASKED_EACH at R = 1 and as MASKED at R >= 2 unless float32 at n <= 2048; the slide plan is
    UNSUPPORTED / MFMA exactly where the window plan is"""
    B = muse.binding
    for N in (2, 63, 64, 65, 480, 512, 1000, 2048, 3000, 4096, 5000, 8192, 65536, 70000):
        n = muse.next_pow2(float(N))
        h = n // 2
        ends = sorted(e for e in {0, 1, 7, 62, 63, 64, 126, 127, 128, h - 1, h, h + 1} if e >= 0)
        for f32 in (False, True):
            def many_of(single, R):
                if single != B.MUSE_IN_WINDOW_MASKED:
                    return single
                return B.MUSE_IN_WINDOW_MASKED if R >= 2 and not (f32 and n <= 2048) else B.MUSE_IN_WINDOW_MASKED_EACH
            for L in ends:
                win = muse.in_window_plan(N, f32, L)
                assert muse.lag_range_plan(N, f32, -L, L) == win, (N, f32, L)
                for R in (1, 2, 8):
                    assert muse.many_in_window_plan(N, f32, L, R) == muse.many_lag_range_plan(N, f32, -L, L, R) == many_of(win, R), (N, f32, L, R)
                for k in (0, 1, N):
                    slide = muse.slide_in_window_plan(N, f32, L, k)
                    assert (slide == B.MUSE_SLIDE_IN_WINDOW_UNSUPPORTED) == (win == B.MUSE_IN_WINDOW_UNSUPPORTED), (N, f32, L, k)
                    assert (slide == B.MUSE_SLIDE_IN_WINDOW_MFMA) == (win == B.MUSE_IN_WINDOW_MFMA), (N, f32, L, k)
            for a in ends:
                for b in ends:
                    single = muse.lag_range_plan(N, f32, -a, b)
                    for R in (1, 2, 8):
                        assert muse.many_lag_range_plan(N, f32, -a, b, R) == many_of(single, R), (N, f32, -a, b, R)


# ------------------------------------------------------------------ 3. the helper is the definition
def _brute(cc, n, lo, hi):
    """the definition, spelled out index by index"""
    hi = min(hi, n // 2)
    lo = max(lo, -(n // 2 - 1))
    mi, mval = 0, 0.0
    for i in list(range(0, hi + 1)) + list(range(n + lo, n)):
        if abs(cc[i]) > abs(mval):
            mval, mi = cc[i], i
    return (mi if mi <= n // 2 else mi - n), float(cc[mi])


def test_helper_is_the_brute_force_definition():
    rng = np.random.default_rng(11)
    for n in (16, 64, 256):
        for trial in range(40):
            cc = rng.standard_normal(n)
            if trial % 4 == 1:
                cc[rng.integers(0, n, n // 4)] = np.nan
            if trial % 4 == 2:
                cc[rng.integers(0, n, n // 2)] = 0.0
            if trial % 8 == 3:
                cc[:] = 0.0
                cc[rng.integers(0, n)] = 0.5
            if trial % 8 == 7:
                cc[:] = np.nan
            for _ in range(12):
                lo, hi = -int(rng.integers(0, n)), int(rng.integers(0, n))
                want = _brute(cc, n, lo, hi)
                assert _same(LR.ranged(cc, n, lo, hi)[:2], want), (n, lo, hi)
                assert _same(LR.ranged_fast(cc, n, lo, hi)[:2], want), (n, lo, hi)
                assert LR.ranged(cc, n, lo, hi)[2] == LR.ranged_fast(cc, n, lo, hi)[2]
            for L in (0, 1, 5, n // 2 - 1):                          # symmetric below n / 2: tests/_window.py's window
                assert _same(LR.ranged(cc, n, -L, L)[:2], W.windowed(cc, n, L)[:2]), (n, L)
                assert LR.ranged(cc, n, -L, L)[2] == W.windowed(cc, n, L)[2]
            for L in (n // 2, 3 * n):                                # every lag (index n / 2 is lag +n/2 only)
                assert _same(LR.ranged(cc, n, -L, L)[:2], W.windowed(cc, n, L)[:2]), (n, L)
    assert LR.ranged(None, 16, -3, 0) == (0, 0.0, False)


# ------------------------------------------------------------------ 4. / 5. the kernels' rules are the definition
def _ccs(oracle, N, M, seed):
    ref, rows = W.make_case(N, M, seed=seed)
    X, n = oracle.ref_spectrum(ref)
    ccs = [oracle.xcorr_with_x(X, y, n)[0] for y in rows]
    ccs = [c for c in ccs if c is not None]
    z = np.zeros(n)
    z[n // 2 + 3] = 0.75                                             # a window of zeros around a far winner
    nn = np.full(n, np.nan)
    nn[0] = 0.25
    return ccs + [z, nn, np.zeros(n)], n


def test_table_mapping_with_an_origin_equals_the_definition_at_256(oracle):
    ccs, n = _ccs(oracle, 256, 12, seed=5)
    assert n == 256
    for lo in range(0, -127, -1):
        for hi in range(0, 127 + lo):                                # W = hi - lo + 1 <= 127
            for cc in (ccs[0], ccs[-3], ccs[-2]):                    # (ranged_fast: checked against the loop in test 3)
                assert _same(LR.table_argmax(cc, n, lo, hi), LR.ranged_fast(cc, n, lo, hi)[:2]), (lo, hi)
    for lo, hi in ((0, 0), (-126, 0), (0, 126), (-100, 26), (-3, 40), (-15, 0), (-16, 0)):
        for cc in ccs:
            assert _same(LR.table_argmax(cc, n, lo, hi), LR.ranged(cc, n, lo, hi)[:2]), (lo, hi)


def test_two_bound_mask_equals_the_definition_at_512(oracle):
    ccs, n = _ccs(oracle, 512, 12, seed=6)
    assert n == 512
    for lo in (0, -1, -255, -256, -257):
        for hi in range(0, n // 2 + 2):
            for cc in (ccs[0], ccs[4], ccs[-3], ccs[-2], ccs[-1]):
                assert _same(LR.masked_argmax(cc, n, lo, hi), LR.ranged(cc, n, lo, hi)[:2]), (lo, hi)


@pytest.mark.parametrize("N", [4096, 3000])
def test_two_bound_mask_equals_the_definition_at_4096_block_boundaries(oracle, N):
    ccs, n = _ccs(oracle, N, 12, seed=7)
    assert n == 4096
    ends = sorted({0, 1, 2047, 2048, 5000} | {256 * k + d for k in range(1, 8) for d in (-1, 0, 1)})
    for a in ends:
        for b in ends:
            for cc in (ccs[0], ccs[-3], ccs[-2]):
                assert _same(LR.masked_argmax(cc, n, -a, b), LR.ranged_fast(cc, n, -a, b)[:2]), (-a, b)


# ------------------------------------------------------------------ 6. the oracle flags no tie the GPU tests could hide behind
def _within_cap(ties, rows):
    return ties * 1000 <= rows                                       # at most 1 in 1000 noise rows


def test_oracle_ties_direct_product_inputs(oracle):
    ties = total = 0
    for N in LR.MFMA_NS:
        ref, rows = LR.mfma_case(N)
        exp, _, _, _ = LR.expect(oracle, ref, rows, LR.MFMA_RANGES)
        keep = W.plain_rows(LR.PARITY_M)
        for k in LR.MFMA_RANGES:
            ties += int((exp[k][2] & keep).sum())
            total += int(keep.sum())
    print("direct-product inputs: %d ties of %d" % (ties, total))
    assert _within_cap(ties, total)


def test_oracle_ties_masked_inputs(oracle):
    ties = total = 0
    for N in LR.MASKED_NS:
        for f32 in (False, True):
            ref, rows = LR.masked_case(N, f32)
            n = 1 << (N - 1).bit_length()
            rs = LR.masked_ranges(n, f32)
            exp, _, _, _ = LR.expect(oracle, ref, rows, rs)
            keep = W.plain_rows(LR.PARITY_M)
            for k in rs:
                ties += int((exp[k][2] & keep).sum())
                total += int(keep.sum())
    print("masked inputs: %d ties of %d" % (ties, total))
    assert _within_cap(ties, total)


def test_oracle_flags_no_tie_planted_inputs(oracle):
    for N, (lo, hi) in LR.EDGE_CASES:
        ref, rows, n, planted = LR.edge_case(N, lo, hi)
        exp, _, _, _ = LR.expect(oracle, ref, rows, ((lo, hi),))
        lag, _, tie = exp[(lo, hi)]
        assert not tie.any(), (N, lo, hi)                            # planted rows: zero ties
        inside = (planted >= lo) & (planted <= hi)
        assert inside.sum() >= 7 and (~inside).sum() == 2
        assert np.array_equal(lag[inside], planted[inside])          # the definition finds the planted lag where it is inside
        assert np.all((lag >= lo) & (lag <= hi))


def test_oracle_ties_run_inputs(oracle):
    for N in LR.RUN_NS:
        ref, rows = LR.run_case(N)
        exp, _, _, _ = LR.expect(oracle, ref, rows, LR.RUN_RANGES)
        for k in LR.RUN_RANGES:
            assert not (exp[k][2] & W.plain_rows(LR.RUN_M)).any(), (N, k)
    ref, rows = LR.cpp_case()
    exp, _, _, _ = LR.expect(oracle, ref, rows, LR.CPP_RANGES)
    for k in LR.CPP_RANGES:
        assert not exp[k][2].any(), k
