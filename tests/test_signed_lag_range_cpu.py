"""CPU-only checks of the signed best match (muse_batch_score_signed_in_lag_range / _run_signed_in_lag_range): the exports and
their mirrors exist on every layer, the dispatch (muse_test_signed_lag_range_plan) is the table include/muse_hip.h gives and is
muse_test_lag_range_plan for sign 0, the numpy helper (tests/_signed.py) is the definition, the two kernels' rules -- the scan key
of the product table, the sign in the mask -- restated in numpy equal it, and the oracle by itself shows, on the inputs
tests/test_gpu_signed_lag_range.py uses, no tie those tests could hide behind and the rows that filtering could not have produced."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagrange as LR
import _signed as SG
import _window as W
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_signed_in_lag_range", 4), ("muse_batch_run_signed_in_lag_range", 14))
HOOKS = (("muse_test_signed_lag_range_plan", 6), ("muse_test_last_in_window_path", 2))


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
    assert _call_args(go, "C.muse_batch_run_signed_in_lag_range(") == 14
    assert re.search(r"func \(b \*Batch\) RunSignedInLagRange\(groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert re.search(r"func \(b \*Batch\) RunSigned\(groupByLabels \[\]string\) error", go)
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_the_signed_calls(muse):
    for name in ("RunSignedInLagRange", "RunSigned"):
        assert callable(getattr(muse.Batch, name, None)), name
    for name in ("score_signed_in_lag_range", "scores_signed_in_lag_range", "run_signed_in_lag_range"):
        assert callable(getattr(muse.DeviceBatch, name, None)), name
    assert callable(getattr(muse, "signed_lag_range_plan", None))
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bvoid\s+RunSignedInLagRange\s*\(", hpp) and re.search(r"\bvoid\s+RunSigned\s*\(", hpp)
    assert _call_args(hpp, "muse_batch_run_signed_in_lag_range(") == 14
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    assert os.path.exists(muse.build.build_signed_lag_range_test())   # the C++ program the GPU suite runs is built with the rest


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    for sign in (0, 1, -1, 2, -2):
        assert L.muse_batch_score_signed_in_lag_range(None, -7, 0, sign) == B.MUSE_ERR_INVALID
        assert L.muse_batch_run_signed_in_lag_range(None, None, 0, -7, 0, 5, 0.0, sign, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    P = L.muse_test_signed_lag_range_plan
    assert P(1, 0, -5, 5, 1, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, 1, 5, 1, ctypes.byref(w)) == B.MUSE_ERR_INVALID       # lag_lo > 0
    assert P(512, 0, -5, -1, -1, ctypes.byref(w)) == B.MUSE_ERR_INVALID    # lag_hi < 0
    assert P(512, 0, -5, 5, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID      # sign 2
    assert P(512, 0, -5, 5, -2, ctypes.byref(w)) == B.MUSE_ERR_INVALID     # sign -2
    assert P(512, 0, -5, 5, 1, None) == B.MUSE_ERR_INVALID                 # NULL path
    assert w.value == 5                                                    # nothing written by a refusal
    assert P(512, 0, -5, 5, 1, ctypes.byref(w)) == 0 and w.value == B.MUSE_IN_WINDOW_MFMA


# ------------------------------------------------------------------ 2. the dispatch
def _table(muse, N, f32, lo, hi, sign):
    """the table of include/muse_hip.h (muse_batch_score_signed_in_lag_range), restated"""
    B = muse.binding
    n = muse.next_pow2(float(N))
    hi = min(hi, n // 2)
    lo = max(lo, -(n // 2 - 1))
    masked_len = n in (512, 1024, 2048, 4096)
    if hi == n // 2 and lo == -(n // 2 - 1):
        if sign == 0:
            return B.MUSE_IN_WINDOW_PLAIN
        return B.MUSE_IN_WINDOW_MASKED if masked_len else B.MUSE_IN_WINDOW_UNSUPPORTED
    if not f32 and n <= 65536 and hi - lo + 1 <= 127:
        return B.MUSE_IN_WINDOW_MFMA
    return B.MUSE_IN_WINDOW_MASKED if masked_len else B.MUSE_IN_WINDOW_UNSUPPORTED


PLAN_NS = [64, 100, 257, 480, 512, 1000, 3000, 4096, 5000, 40000, 70000]


@pytest.mark.parametrize("N", PLAN_NS)
def test_plan_is_the_table(muse, N):
    n = muse.next_pow2(float(N))
    ends = sorted(e for e in {0, 1, 7, 15, 16, 26, 40, 60, 63, 64, 100, 126, 127, 200, 300, n // 2 - 2, n // 2 - 1, n // 2,
                              n // 2 + 1, 10 * n} if e >= 0)
    for f32 in (False, True):
        for a in ends:
            for b in ends:
                for sign in (0, 1, -1):
                    assert muse.signed_lag_range_plan(N, f32, -a, b, sign) == _table(muse, N, f32, -a, b, sign), (N, f32, -a, b, sign)
                assert muse.signed_lag_range_plan(N, f32, -a, b, 0) == muse.lag_range_plan(N, f32, -a, b), (N, f32, -a, b)


def test_plan_pinned_rows(muse):
    B = muse.binding
    P = muse.signed_lag_range_plan
    for s in (1, -1):
        assert P(4096, False, -126, 0, s) == B.MUSE_IN_WINDOW_MFMA
        assert P(4096, False, -127, 0, s) == B.MUSE_IN_WINDOW_MASKED
        assert P(4096, True, -7, 0, s) == B.MUSE_IN_WINDOW_MASKED
        assert P(40000, False, -63, 63, s) == B.MUSE_IN_WINDOW_MFMA
        assert P(5000, False, -200, 0, s) == P(5000, True, -7, 0, s) == B.MUSE_IN_WINDOW_UNSUPPORTED
        for f32 in (False, True):
            for N in (480, 1000, 1433, 3000, 4096):                  # every lag: the masked kernels, bounds at their widest
                assert P(N, f32, -(1 << 30), 1 << 30, s) == B.MUSE_IN_WINDOW_MASKED
                assert P(N, f32, -(1 << 30), 1 << 30, 0) == B.MUSE_IN_WINDOW_PLAIN
            for N in (64, 100, 256, 5000, 40000, 70000):
                assert P(N, f32, -(1 << 30), 1 << 30, s) == B.MUSE_IN_WINDOW_UNSUPPORTED
                assert P(N, f32, -(1 << 30), 1 << 30, 0) == B.MUSE_IN_WINDOW_PLAIN


# ------------------------------------------------------------------ 3. the helper is the definition
def _brute(cc, n, lo, hi, sign):
    """the definition, spelled out index by index (a slice of nothing but NaN is a NaN / Inf series: (0, NaN))"""
    hi = min(hi, n // 2)
    lo = max(lo, -(n // 2 - 1))
    if all(np.isnan(v) for v in cc):
        return 0, float("nan")
    mi, best = 0, 0.0
    for i in list(range(0, hi + 1)) + list(range(n + lo, n)):
        if (sign > 0 and cc[i] > best) or (sign < 0 and -cc[i] > -best):
            best, mi = cc[i], i
    return (mi if mi <= n // 2 else mi - n), float(best)


def _random_ccs(rng, n, trials):
    for trial in range(trials):
        cc = rng.standard_normal(n)
        if trial % 4 == 1:
            cc[rng.integers(0, n, n // 4)] = np.nan
        if trial % 4 == 2:
            cc[rng.integers(0, n, n // 2)] = 0.0
        if trial % 8 == 3:
            cc[:] = 0.0
            cc[rng.integers(0, n)] = 0.5
        if trial % 8 == 5:
            cc = -np.abs(cc)                                         # nothing positive anywhere
        if trial % 8 == 7:
            cc[:] = np.nan
        if trial % 8 == 6:
            cc[rng.integers(0, n, n // 2)] = -0.0
        yield cc


def test_helper_is_the_brute_force_definition():
    rng = np.random.default_rng(12)
    for n in (16, 64, 256):
        for cc in _random_ccs(rng, n, 40):
            for _ in range(12):
                lo, hi = -int(rng.integers(0, n)), int(rng.integers(0, n))
                for sign in SG.SIGNS:
                    want = _brute(cc, n, lo, hi, sign)
                    got, fast = SG.signed_ranged(cc, n, lo, hi, sign), SG.signed_ranged_fast(cc, n, lo, hi, sign)
                    assert _same(got[:2], want) and _same(fast[:2], want), (n, lo, hi, sign)
                    assert got[2] == fast[2]
                    if np.isnan(got[1]):
                        assert got[0] == 0 and np.isnan(cc).all()
                    elif got[1] == 0.0:                              # no value of the sign: (0, +0.0), sign bit clear
                        assert got[0] == 0 and not np.signbit(got[1]) and not np.signbit(fast[1])
                    else:
                        assert np.sign(got[1]) == sign
                assert SG.signed_ranged(cc, n, lo, hi, 0) == LR.ranged(cc, n, lo, hi) or np.isnan(LR.ranged(cc, n, lo, hi)[1])
                assert SG.signed_ranged_fast(cc, n, lo, hi, 0) == LR.ranged_fast(cc, n, lo, hi) or np.isnan(LR.ranged_fast(cc, n, lo, hi)[1])
    for sign in (0, 1, -1):
        assert SG.signed_ranged(None, 16, -3, 0, sign) == SG.signed_ranged_fast(None, 16, -3, 0, sign) == (0, 0.0, False)


def test_invariant_unsigned_winner_of_the_sign_is_the_signed_result():
    rng = np.random.default_rng(13)
    seen = 0
    for n in (16, 64, 256):
        for cc in _random_ccs(rng, n, 40):
            for _ in range(12):
                lo, hi = -int(rng.integers(0, n)), int(rng.integers(0, n))
                ul, uv, _ = LR.ranged(cc, n, lo, hi)
                for sign in SG.SIGNS:
                    if sign * uv > 0:
                        assert SG.signed_ranged(cc, n, lo, hi, sign)[:2] == (ul, uv), (n, lo, hi, sign)
                        seen += 1
    assert seen > 500


# ------------------------------------------------------------------ 4. / 5. the kernels' rules are the definition
def _ccs(oracle, N, M, seed):
    ref, rows = SG.make_case(N, M, seed=seed)
    X, n = oracle.ref_spectrum(ref)
    ccs = [oracle.xcorr_with_x(X, y, n)[0] for y in rows]
    ccs = [c for c in ccs if c is not None]
    z = np.zeros(n)
    z[n // 2 + 3] = 0.75                                             # a window of zeros around a far winner
    nn = np.full(n, np.nan)
    nn[0] = 0.25
    return ccs + [z, -z, nn, -nn, np.zeros(n)], n


def test_signed_table_scan_equals_the_definition_at_256(oracle):
    ccs, n = _ccs(oracle, 256, 16, seed=5)
    assert n == 256
    for sign in (0, 1, -1):
        for lo in range(0, -127, -3):
            for hi in range(0, 127 + lo, 2):                         # W = hi - lo + 1 <= 127
                for cc in (ccs[0], ccs[2], ccs[-5], ccs[-3]):
                    assert _same(SG.table_argmax(cc, n, lo, hi, sign), SG.signed_ranged_fast(cc, n, lo, hi, sign)[:2]), (lo, hi, sign)
        for lo, hi in ((0, 0), (-126, 0), (0, 126), (-100, 26), (-3, 40), (-15, 0), (-16, 0)):
            for cc in ccs:
                assert _same(SG.table_argmax(cc, n, lo, hi, sign), SG.signed_ranged(cc, n, lo, hi, sign)[:2]), (lo, hi, sign)
    for lo, hi in ((0, 0), (-100, 26)):                              # sign 0: tests/_lagrange.py's restatement
        for cc in ccs:
            assert _same(SG.table_argmax(cc, n, lo, hi, 0), LR.table_argmax(cc, n, lo, hi))


def test_signed_mask_equals_the_definition_at_512(oracle):
    ccs, n = _ccs(oracle, 512, 16, seed=6)
    assert n == 512
    for sign in (0, 1, -1):
        for lo in (0, -1, -255, -256, -257):
            for hi in range(0, n // 2 + 2, 3):
                for cc in (ccs[0], ccs[2], ccs[4], ccs[-5], ccs[-4], ccs[-3], ccs[-2], ccs[-1]):
                    assert _same(SG.masked_argmax(cc, n, lo, hi, sign), SG.signed_ranged(cc, n, lo, hi, sign)[:2]), (lo, hi, sign)
    for cc in ccs:
        assert _same(SG.masked_argmax(cc, n, -64, 300, 0), LR.masked_argmax(cc, n, -64, 300))


@pytest.mark.parametrize("N", [4096, 3000])
def test_signed_mask_equals_the_definition_at_4096_block_boundaries(oracle, N):
    ccs, n = _ccs(oracle, N, 16, seed=7)
    assert n == 4096
    ends = sorted({0, 1, 2047, 2048, 5000} | {256 * k + d for k in range(1, 8, 2) for d in (-1, 0, 1)})
    for sign in SG.SIGNS:
        for a in ends:
            for b in ends:
                for cc in (ccs[0], ccs[2], ccs[-5]):
                    assert _same(SG.masked_argmax(cc, n, -a, b, sign), SG.signed_ranged_fast(cc, n, -a, b, sign)[:2]), (-a, b, sign)


# ------------------------------------------------------------------ 6. conditions on the shared GPU inputs, on the oracle alone
def _conditions(exp, ranges, M, tag):
    """no tie on the plain rows, the planted ones among them (M = 35: 1 in 1000 is none), and per sign what filtering could not produce: rows whose unsigned in-range
    winner has the OTHER sign while the signed value is nonzero (>= 4 plain rows in some range), and rows with no value of the sign
    in some range (>= 2), the (0, +0.0) outcome"""
    plain = SG.plain_rows(M)
    for s in SG.SIGNS:
        recovered = empty = 0
        for lo, hi in ranges:
            lag, mv, tie = exp[(lo, hi, s)]
            assert not (tie & plain).any(), (tag, lo, hi, s, np.nonzero(tie & plain)[0])
            ulag, umv, utie = exp[(lo, hi, 0)]
            other = plain & (s * umv < 0) & (mv != 0.0)
            recovered = max(recovered, int(other.sum()))
            none = plain & ~np.isnan(mv) & (mv == 0.0) & (umv != 0.0)
            assert np.all(lag[none] == 0) and not np.signbit(mv[none]).any()
            empty = max(empty, int(none.sum()))
            inv = ~utie & (s * umv > 0)                              # the invariant on the shared inputs
            assert np.array_equal(lag[inv], ulag[inv]) and np.array_equal(mv[inv], umv[inv]), (tag, lo, hi, s)
        assert recovered >= 4, (tag, s, recovered)
        assert empty >= 2, (tag, s, empty)


def test_oracle_conditions_direct_product_inputs(oracle):
    for N in LR.MFMA_NS:
        ref, rows = SG.mfma_case(N)
        exp, _ = SG.expect(oracle, ref, rows, LR.MFMA_RANGES)
        for lo, hi in LR.MFMA_RANGES:
            assert not (exp[(lo, hi, 0)][2] & SG.plain_rows(SG.PARITY_M)).any(), (N, lo, hi)
        _conditions(exp, LR.MFMA_RANGES, SG.PARITY_M, "direct N=%d" % N)


def test_oracle_conditions_masked_inputs(oracle):
    for N in LR.MASKED_NS:
        for f32 in (False, True):
            ref, rows = SG.masked_case(N, f32)
            n = 1 << (N - 1).bit_length()
            rs = LR.masked_ranges(n, f32) + [(-(n // 2 - 1), n // 2)] + ([(0, 0)] if not f32 else [])
            exp, _ = SG.expect(oracle, ref, rows, rs)
            _conditions(exp, rs, SG.PARITY_M, "masked N=%d f32=%d" % (N, f32))


def test_oracle_flags_no_tie_planted_inputs(oracle):
    for N, (lo, hi) in LR.EDGE_CASES:
        ref, rows, n, planted, sgn = SG.edge_case(N, lo, hi)
        exp, _ = SG.expect(oracle, ref, rows, ((lo, hi),), signs=SG.SIGNS)
        inside = (planted >= lo) & (planted <= hi)
        assert inside.sum() >= 7 and (~inside).sum() == 2
        for s in SG.SIGNS:
            lag, mv, tie = exp[(lo, hi, s)]
            assert not tie.any(), (N, lo, hi, s)
            own = sgn == s
            assert own.sum() >= 4
            assert np.array_equal(lag[inside & own], planted[inside & own])   # found with the right sign where it is inside
            assert np.all(s * mv[inside & own] > 0)
            assert np.all((lag >= lo) & (lag <= hi))


def test_oracle_conditions_run_inputs(oracle):
    """no ties; and for each sign at least one label group that the signed Run selects and run_in_lag_range with the same
    sign_filter drops: its first-by-magnitude member has the other sign, a member's best value of the sign passes.  With signed group
    scores (abs_scores 0, Muse.Run's clamp): under Batch.Run's magnitudes (abs_scores 1, muse_batch.go:74) every score is >= 0 and the
    reference's own filter passes every group for SignFilter_POS and none for SignFilter_NEG, whatever the argmax."""
    gid, G = SG.run_groups()
    for N in SG.RUN_NS:
        ref, rows = SG.run_case(N)
        exp, _ = SG.expect(oracle, ref, rows, SG.RUN_RANGES + ((-20, 20),))
        for k in exp:                                                # the Run tests compare ORDER and lags: no tie on any row
            assert not exp[k][2].any() or k[2] == 0, (N, k)
            assert not (exp[k][2] & SG.plain_rows(SG.RUN_M)).any(), (N, k)
        for lo, hi in SG.RUN_RANGES:
            L = max(-lo, hi)
            for s in SG.SIGNS:
                signed = oracle.results(exp[(lo, hi, s)][0], exp[(lo, hi, s)][1], gid, G, False, L, G, 0.0, s)
                plain = oracle.results(exp[(lo, hi, 0)][0], exp[(lo, hi, 0)][1], gid, G, False, L, G, 0.0, s)
                gained = set(gid[signed[0]].tolist()) - set(gid[plain[0]].tolist())
                assert len(gained) >= 1, (N, lo, hi, s)
    ref, rows = SG.cpp_case()
    exp, _ = SG.expect(oracle, ref, rows, SG.CPP_RANGES + ((-SG.CPP_SIGNED_MAXLAG, SG.CPP_SIGNED_MAXLAG),), signs=SG.SIGNS)
    for k in exp:
        assert not exp[k][2].any(), k
