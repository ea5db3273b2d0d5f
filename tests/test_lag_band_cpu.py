"""CPU-only checks of the lag bands (muse_batch_score_in_lag_band / _run_in_lag_band): the exports and their mirrors exist on every
layer, the dispatch (muse_test_lag_band_plan) is the table include/muse_hip.h gives and is muse_test_signed_lag_range_plan for a band
that holds lag 0, the numpy helper (tests/_lagband.py) is the definition in two forms, the two kernels' rules -- the band scan of the
product table with its (0, +0.0) outcome, the interval mask in front of the unchanged maxAbsIndex -- restated in numpy equal it, and
the oracle by itself flags, on the inputs tests/test_gpu_lag_band.py uses, NO tie: the GPU tests demand exact lags on every row."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LS
import _signed as SG
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_in_lag_band", 4), ("muse_batch_run_in_lag_band", 14))
HOOKS = (("muse_test_lag_band_plan", 6),)


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _same(a, b):
    return a[0] == b[0] and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1])))


def _call_args(text, call):
    """the number of arguments of the first `call(` in text: commas outside nested parentheses"""
    at = text.index(call) + len(call)
    depth, commas = 1, 0
    while depth:
        c = text[at]
        depth += (c == "(") - (c == ")")
        commas += c == "," and depth == 1
        at += 1
    return commas + 1


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
    assert _call_args(go, "C.muse_batch_run_in_lag_band(") == 14
    assert re.search(r"func \(b \*Batch\) RunInLagBand\(groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert re.search(r"func \(b \*Batch\) RunSignedInLagBand\(groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_the_band_calls(muse):
    for name in ("RunInLagBand", "RunSignedInLagBand"):
        assert callable(getattr(muse.Batch, name, None)), name
    for name in ("score_in_lag_band", "scores_in_lag_band", "run_in_lag_band"):
        assert callable(getattr(muse.DeviceBatch, name, None)), name
    assert callable(getattr(muse, "lag_band_plan", None))
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bvoid\s+RunInLagBand\s*\(", hpp) and re.search(r"\bvoid\s+RunSignedInLagBand\s*\(", hpp)
    assert _call_args(hpp, "muse_batch_run_in_lag_band(") == 14
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    assert os.path.exists(muse.build.build_lag_band_test())          # the C++ program the GPU suite runs is built with the rest


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    for sign in (0, 1, -1, 2, -2):
        assert L.muse_batch_score_in_lag_band(None, 1, 7, sign) == B.MUSE_ERR_INVALID
        assert L.muse_batch_run_in_lag_band(None, None, 0, 1, 7, 5, 0.0, sign, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    P = L.muse_test_lag_band_plan
    assert P(1, 0, 1, 5, 1, ctypes.byref(w)) == B.MUSE_ERR_INVALID          # N < 2
    assert P(512, 0, 5, 1, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID        # lag_lo > lag_hi
    assert P(512, 0, 0, -1, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(64, 0, 100, 226, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID     # empty after clipping (n = 64: lags -31 .. 32)
    assert P(64, 0, -226, -100, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(64, 0, 33, 33, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(64, 0, -32, -32, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, 1, 5, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID        # sign 2
    assert P(512, 0, 1, 5, -2, ctypes.byref(w)) == B.MUSE_ERR_INVALID       # sign -2
    assert P(512, 0, 1, 5, 1, None) == B.MUSE_ERR_INVALID                   # NULL path
    assert w.value == 5                                                     # nothing written by a refusal
    assert P(512, 0, 1, 5, 1, ctypes.byref(w)) == 0 and w.value == B.MUSE_IN_WINDOW_MFMA
    assert P(64, 0, 32, 33, 0, ctypes.byref(w)) == 0 and w.value == B.MUSE_IN_WINDOW_MFMA     # clipped to (32, 32)
    assert P(64, 0, -40, -31, 0, ctypes.byref(w)) == 0 and w.value == B.MUSE_IN_WINDOW_MFMA   # clipped to (-31, -31)


# ------------------------------------------------------------------ 2. the dispatch
def _table(muse, N, f32, lo, hi):
    """the table of include/muse_hip.h (muse_batch_score_in_lag_band) for a band without lag 0, restated; None: empty"""
    B = muse.binding
    n = muse.next_pow2(float(N))
    c = LB.clip(n, lo, hi)
    if c is None:
        return None
    lo, hi = c
    if not f32 and n <= 65536 and hi - lo + 1 <= 127:
        return B.MUSE_IN_WINDOW_MFMA
    return B.MUSE_IN_WINDOW_MASKED if n in (512, 1024, 2048, 4096) else B.MUSE_IN_WINDOW_UNSUPPORTED


PLAN_NS = [64, 100, 257, 480, 512, 1000, 3000, 4096, 5000, 40000, 65536, 65537, 70000]


@pytest.mark.parametrize("N", PLAN_NS)
def test_plan_is_the_table(muse, N):
    n = muse.next_pow2(float(N))
    ends = sorted({1, 2, 7, 16, 17, 40, 100, 126, 127, 128, 129, 200, 226, 230, 300, n // 2 - 1, n // 2, n // 2 + 1, 10 * n})
    seen = set()
    for f32 in (False, True):
        for a in ends:
            for b in ends:
                if a > b:
                    continue
                for lo, hi in ((a, b), (-b, -a)):
                    want = _table(muse, N, f32, lo, hi)
                    for sign in LB.SIGNS:
                        if want is None:
                            with pytest.raises(muse.MuseError) as e:
                                muse.lag_band_plan(N, f32, lo, hi, sign)
                            assert e.value.status == muse.binding.MUSE_ERR_INVALID, (N, f32, lo, hi, sign)
                        else:
                            assert muse.lag_band_plan(N, f32, lo, hi, sign) == want, (N, f32, lo, hi, sign)
                    seen.add(want)
    assert muse.binding.MUSE_IN_WINDOW_PLAIN not in seen             # a band without lag 0 is never every lag


def test_plan_pinned_rows(muse):
    B = muse.binding
    P = muse.lag_band_plan
    for s in LB.SIGNS:
        assert P(4096, False, 1, 127, s) == B.MUSE_IN_WINDOW_MFMA            # W = 127
        assert P(4096, False, 1, 128, s) == B.MUSE_IN_WINDOW_MASKED          # W = 128
        assert P(4096, False, -127, -1, s) == B.MUSE_IN_WINDOW_MFMA
        assert P(4096, False, -128, -1, s) == B.MUSE_IN_WINDOW_MASKED
        assert P(4096, False, 200, 230, s) == B.MUSE_IN_WINDOW_MFMA          # far from zero: the rows of the band alone count
        assert P(4096, True, 1, 7, s) == B.MUSE_IN_WINDOW_MASKED             # float32 storage
        assert P(480, True, 200, 230, s) == B.MUSE_IN_WINDOW_MASKED
        assert P(5000, False, 1, 200, s) == B.MUSE_IN_WINDOW_UNSUPPORTED     # n = 8192, wide
        assert P(5000, True, 1, 7, s) == B.MUSE_IN_WINDOW_UNSUPPORTED
        assert P(5000, False, 1, 127, s) == B.MUSE_IN_WINDOW_MFMA
        assert P(65536, False, 20000, 20126, s) == B.MUSE_IN_WINDOW_MFMA     # N = 65536, narrow
        assert P(65536, False, 1, 128, s) == B.MUSE_IN_WINDOW_UNSUPPORTED
        assert P(65537, False, 1, 7, s) == B.MUSE_IN_WINDOW_UNSUPPORTED      # n = 131072


@pytest.mark.parametrize("N", (100, 480, 3000, 5000))
def test_a_band_holding_zero_is_the_signed_range_plan(muse, N):
    n = muse.next_pow2(float(N))
    for f32 in (False, True):
        for lo in (0, -1, -7, -126, -200, -(n // 2 - 1), -10 * n):
            for hi in (0, 1, 7, 126, 300, n // 2, 10 * n):
                for s in LB.SIGNS:
                    assert muse.lag_band_plan(N, f32, lo, hi, s) == muse.signed_lag_range_plan(N, f32, lo, hi, s), (N, f32, lo, hi, s)


# ------------------------------------------------------------------ 3. the definition, twice, and the kernels' rules
def _bands_at(n, bands):
    return [b for b in bands if LB.clip(n, *b)]


def _agree(cc, n, lo, hi, s, tag):
    a = LB.banded(cc, n, lo, hi, s)
    b = LB.banded_fast(cc, n, lo, hi, s)
    assert _same(a, b) and a[2] == b[2], (tag, a, b)
    if cc is not None:
        t = LB.table_scan(cc, n, lo, hi, s)
        m = LB.interval_mask_argmax(cc, n, lo, hi, s)
        assert _same(a, t) and _same(a, m), (tag, a, t, m)
        assert not (a[1] == 0.0 and np.signbit(a[1]))
    clo, chi = LB.clip(n, lo, hi)
    assert a[0] == 0 or clo <= a[0] <= chi, (tag, a)
    return a


def _parity_inputs():
    for N in LB.MFMA_NS:
        yield "mfma", N, False, LB.mfma_case(N), LB.MFMA_BANDS
    for M in LB.SMALL_MS:
        yield "mfma M=%d" % M, LB.SMALL_M_N, False, LB.mfma_case(LB.SMALL_M_N, M), LB.MFMA_BANDS
    for N in LB.MASKED_NS:
        for f32 in (False, True):
            n = LS.fft_len(N)
            yield "masked", N, f32, LB.masked_case(N, f32), LB.masked_bands(n) + list(LB.MASKED_FORCED)


def test_forms_agree_and_the_oracle_flags_no_tie(oracle):
    """the loop, the vectorised form and both kernel rules agree on every parity input, band and sign; the oracle flags no tie on
    any row; both signed outcomes occur (a row with a value of the sign, a row with none)"""
    ties, won, none = 0, {1: 0, -1: 0}, {1: 0, -1: 0}
    for kind, N, f32, (ref, rows), bands in _parity_inputs():
        ccs, n = LB.slices(oracle, ref, rows)
        for lo, hi in _bands_at(n, bands):
            for s in LB.SIGNS:
                for r, cc in enumerate(ccs):
                    a = _agree(cc, n, lo, hi, s, (kind, N, f32, lo, hi, s, r))
                    ties += a[2]
                    if s and cc is not None and not np.isnan(a[1]):
                        if a[1] != 0.0:
                            assert s * a[1] > 0
                            won[s] += 1
                        else:
                            none[s] += 1
    assert ties == 0
    assert min(won.values()) > 0 and min(none.values()) > 0, (won, none)


def test_far_bands_are_empty_at_short_lengths():
    for n in (64, 128):
        for b in LB.FAR_BANDS:
            assert LB.clip(n, *b) is None
        assert len(_bands_at(n, LB.MFMA_BANDS)) == len(LB.MFMA_BANDS) - len(LB.FAR_BANDS)
    assert LB.clip(512, 257, 510) is None and LB.clip(512, -512, -257) is None
    assert LB.clip(512, 256, 511) == (256, 256) and LB.clip(64, 5, 131) == (5, 32)


def test_a_band_holding_zero_is_the_signed_range(oracle):
    ref, rows = LB.mfma_case(480)
    ccs, n = LB.slices(oracle, ref, rows)
    for lo, hi in ((0, 7), (-7, 0), (-40, 3), (0, 0), (-300, 20), (-10 * n, 10 * n)):
        for s in LB.SIGNS:
            for cc in ccs:
                assert LB.banded(cc, n, lo, hi, s) == SG.signed_ranged(cc, n, lo, hi, s) or (cc is not None and np.isnan(cc).all())
                assert _same(LB.banded_fast(cc, n, lo, hi, s), SG.signed_ranged_fast(cc, n, lo, hi, s))


@pytest.mark.parametrize("N,band", LB.EDGE_CASES)
def test_edges_every_winner_planted_inside_the_band_is_found(oracle, N, band):
    lo, hi = band
    ref, rows, n, planted = LB.edge_case(N, lo, hi)
    assert sorted(planted.tolist()) == sorted({lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, -1, 0, 1})
    ccs, n2 = LB.slices(oracle, ref, rows)
    assert n2 == n == N
    inside = found = 0
    for r, cc in enumerate(ccs):
        for s in LB.SIGNS:
            a = _agree(cc, n, lo, hi, s, (N, band, s, r))
            assert not a[2]
            assert a[0] == 0 or lo <= a[0] <= hi
        a = LB.banded(cc, n, lo, hi, 0)
        if lo <= planted[r] <= hi:
            inside += 1
            found += a[0] == planted[r]
        else:
            assert a[0] != planted[r] or planted[r] == 0           # (lag 0 is the "none" answer too; its value is then +0.0)
            if planted[r] == 0:
                assert lo <= a[0] <= hi                              # the noise inside the band wins, never cc[0]
    assert inside == found == 4


def test_zeros_band_gives_lag_zero_plus_zero(oracle):
    ref, rows, zr = LB.zeros_case()
    ccs, n = LB.slices(oracle, ref, rows)
    for lo, hi in LB.ZEROS_BANDS:
        idx = LB.band_indices(n, lo, hi)
        assert np.all(np.abs(ccs[zr][idx]) < 1e-15)                  # the oracle's slice is zero to rounding there ...
    exact = np.zeros(n)                                              # ... and the definition on exact zeros is (0, +0.0)
    exact[0] = 0.7
    for lo, hi in LB.ZEROS_BANDS:
        for s in LB.SIGNS:
            for f in (LB.banded, LB.banded_fast):
                lag, mv, tie = f(exact, n, lo, hi, s)
                assert lag == 0 and mv == 0.0 and not np.signbit(mv) and not tie
            assert LB.table_scan(exact, n, lo, hi, s) == (0, 0.0) and LB.interval_mask_argmax(exact, n, lo, hi, s) == (0, 0.0)
