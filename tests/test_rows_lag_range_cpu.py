"""CPU-only checks of Muse.Run inside a lag range (muse_batch_run_rows_in_lag_range / _run_row_ptrs_in_lag_range /
_run_group_rows_in_lag_range): the exports and hooks exist on every layer, the dispatch (muse_test_rows_lag_range_plan, a pure host
function) equals the table of include/muse_hip.h restated in Python, the panel kernels' merge rule restated in numpy equals the
definition -- with exact ties planted across two panels and across the lag-0 boundary -- and, on exactly the inputs the GPU tests
use, the oracle by itself flags no tie inside any tested range: the GPU tests compare the lag of every row."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagrange as LR
import _rowslagrange as RL
from _load import ROOT, pkg

EXPORTS = {"muse_batch_run_rows_in_lag_range": 9, "muse_batch_run_row_ptrs_in_lag_range": 8, "muse_batch_run_group_rows_in_lag_range": 9}
HOOKS = {"muse_test_rows_lag_range_plan": 8, "muse_test_run_rows_in_lag_range_scores": 8}


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(muse_[a-z0-9_]+)\s*\(([^)]*)\)", hdr):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


# ------------------------------------------------------------------ 1. exports
def test_exports_declared_exported_and_bound(muse):
    lib = ctypes.CDLL(muse.build.LIB)
    out = subprocess.check_output(["nm", "-D", "--defined-only", muse.build.LIB], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T muse_" in l}
    for header, names in (("muse_hip.h", EXPORTS), ("muse_hip_test.h", HOOKS)):
        declared = _declared(header)
        for name, nargs in names.items():
            assert declared.get(name) == nargs, "%s: %s declared with %s arguments" % (header, name, declared.get(name))
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert len(muse.binding.SIGNATURES[name][1]) == nargs, "binding.SIGNATURES: %s" % name
    assert {n for n in exported if re.search(r"_(rows|row_ptrs)_in_lag_range$", n)} == set(EXPORTS)
    assert not any(h in _declared("muse_hip.h") for h in HOOKS)
    hdr = open(os.path.join(ROOT, "include", "muse_hip.h")).read()
    assert re.search(r"#define MUSE_HIP_ABI_VERSION 5\b", hdr)                      # additions only
    assert re.search(r"#define MUSE_RUN_ROWS_LAG_RANGE_MAX 2048\b", hdr) and muse.binding.MUSE_RUN_ROWS_LAG_RANGE_MAX == 2048
    B = muse.binding
    assert (B.MUSE_ROWS_LAG_RANGE_UNSUPPORTED, B.MUSE_ROWS_LAG_RANGE_PLAIN, B.MUSE_ROWS_LAG_RANGE_WINDOW, B.MUSE_ROWS_LAG_RANGE_SPLIT,
            B.MUSE_ROWS_LAG_RANGE_PANELS) == (RL.UNSUPPORTED, RL.PLAIN, RL.WINDOW, RL.SPLIT, RL.PANELS)
    test_hdr = open(os.path.join(ROOT, "include", "muse_hip_test.h")).read()
    for name, v in (("UNSUPPORTED", 0), ("PLAIN", 1), ("WINDOW", 2), ("SPLIT", 3), ("PANELS", 4)):
        assert re.search(r"#define MUSE_ROWS_LAG_RANGE_%s %d\b" % (name, v), test_hdr)


def test_mirrors_name_the_exports_and_run_in_lag_range(muse):
    src = lambda *p: open(os.path.join(ROOT, "go-muse_amd", *p)).read()
    py, hpp, go = src("muse.py"), src("host", "muse.hpp"), src("go", "muse_hip.go")
    for name in EXPORTS:
        assert name in py, name
    for meth in ("run_rows_in_lag_range", "run_row_ptrs_in_lag_range", "run_group_rows_in_lag_range", "run_rows_in_lag_range_scores"):
        assert callable(getattr(muse.DeviceBatch, meth))
    assert callable(muse.Muse.RunInLagRange) and callable(muse.rows_lag_range_plan)
    assert "muse_batch_run_row_ptrs_in_lag_range(" in hpp and "muse_batch_run_group_rows_in_lag_range(" in hpp
    muse_cls = hpp[hpp.index("class Muse {"):]
    assert re.search(r"void RunInLagRange\(const std::vector<SeriesPtr> &compGraphs, int lagLo, int lagHi\)", muse_cls)
    assert "C.muse_batch_run_rows_in_lag_range(" in go
    assert re.search(r"func \(m \*Muse\) RunInLagRange\(compGraphs \[\]\*Series, lagLo, lagHi int\) error", go)
    prog = src("host", "muse_rows_lag_range_test.cpp")
    assert "RunInLagRange" in prog and os.path.exists(muse.build.build_rows_lag_range_test())


def test_python_run_in_lag_range_checks_its_arguments_first(muse):
    """Muse.RunInLagRange checks the range and the lengths before anything touches a device -- a Muse needs a device to exist, so
    the checks are exercised on an object built without its constructor"""
    m = object.__new__(muse.Muse)
    m.refN = 8
    m.Results = muse.NewResults(5, 5, 0.0, muse.SignFilter_ANY)
    for lo, hi in ((1, 7), (-7, -1)):
        with pytest.raises(muse.MuseError) as e:
            m.RunInLagRange([muse.NewSeries(np.arange(8.0), None)], lo, hi)
        assert e.value.status == muse.binding.MUSE_ERR_INVALID
    with pytest.raises(muse.MuseError) as e:
        m.RunInLagRange([muse.NewSeries(np.arange(7.0), None)], -3, 0)
    assert e.value.status == muse.binding.MUSE_ERR_LENGTH
    assert m.RunInLagRange([], -3, 0) is None        # muse.go:47-50: nothing to compare


def test_null_handles_and_bad_plan_arguments_are_argument_errors(muse):
    B = muse.binding
    L = B.load()
    INV = B.MUSE_ERR_INVALID
    rec = np.zeros(1, dtype=B.RECORD_DTYPE)
    st = ctypes.c_uint8(7)
    x = np.zeros((2, 16))
    assert L.muse_batch_run_rows_in_lag_range(None, B.dptr(x), 2, 16, -7, 0, 0, B.recptr(rec), ctypes.byref(st)) == INV
    assert L.muse_batch_run_row_ptrs_in_lag_range(None, None, 2, -7, 0, 0, B.recptr(rec), ctypes.byref(st)) == INV
    assert L.muse_batch_run_group_rows_in_lag_range(None, None, None, 2, -7, 0, 0, B.recptr(rec), ctypes.byref(st)) == INV
    lag, mv = np.zeros(2, dtype=np.int32), np.zeros(2)
    assert L.muse_test_run_rows_in_lag_range_scores(None, B.dptr(x), 2, 16, -7, 0, B.i32ptr(lag), B.dptr(mv)) == INV
    p = ctypes.c_int32(0)
    for args in ((0, 4096, 256, -7, 0), (5, 1, 256, -7, 0), (5, 4096, 0, -7, 0), (5, 4096, 256, 1, 7), (5, 4096, 256, -7, -1)):
        assert L.muse_test_rows_lag_range_plan(*args, ctypes.byref(p), None, None) == INV
    assert L.muse_test_rows_lag_range_plan(5, 4096, 256, -7, 0, None, None, None) == INV
    assert L.muse_test_rows_lag_range_plan(5, 4096, 256, -7, 0, ctypes.byref(p), None, None) == 0 and p.value == RL.SPLIT


# ------------------------------------------------------------------ 2. the plan
@pytest.mark.parametrize("num_cus", [1, 64, 256])
def test_plan_is_the_table(muse, num_cus):
    seen = set()
    for N in RL.PLAN_NS:
        n = RL.fft_len(N)
        every = [(-(n // 2 - 1), n // 2), (-(n // 2), n // 2), (-(n // 2 - 1) - 5, n // 2 + 9)]   # clip to every lag
        for M in RL.PLAN_MS:
            for lo, hi in RL.PLAN_RANGES + tuple(every):
                got = muse.rows_lag_range_plan(M, N, num_cus, lo, hi)
                want = RL.plan(M, N, num_cus, lo, hi)
                assert got == want, (M, N, num_cus, lo, hi, got, want)
                seen.add(got[0])
                path, panels, S = got
                clo, chi = LR.clip(n, lo, hi)
                Wd = chi - clo + 1
                if (lo, hi) in every:
                    assert path == RL.PLAIN
                if path == RL.PANELS:
                    assert 128 <= Wd <= 2048 and panels == -(-Wd // 128) and 1 <= S <= (N + 1023) // 1024
                    assert S == 1 or (M + 15) // 16 * panels * S <= num_cus        # never more workgroups than CUs
                if path in (RL.WINDOW, RL.SPLIT):
                    # the windowed call's own planner: a symmetric range's (path, S) is what window_rows_plan gives
                    S0, _ = muse.window_rows_plan(M, N, num_cus)
                    assert Wd <= 127 and panels == 1 and S == S0 and (path == RL.SPLIT) == (S0 > 1)
                if path == RL.UNSUPPORTED:
                    assert N > 65536 or Wd > 2048
    assert seen == {RL.UNSUPPORTED, RL.PLAIN, RL.WINDOW, RL.PANELS} | ({RL.SPLIT} if num_cus > 1 else set())
    # the rows of the issue's table, by name
    assert muse.rows_lag_range_plan(17, 2500, 256, -127, 0)[0] == RL.PANELS          # 128 lags
    assert muse.rows_lag_range_plan(17, 2500, 256, -126, 0)[0] in (RL.WINDOW, RL.SPLIT)
    assert muse.rows_lag_range_plan(17, 5000, 256, 0, 2047)[:2] == (RL.PANELS, 16)
    assert muse.rows_lag_range_plan(17, 5000, 256, 0, 2048)[0] == RL.UNSUPPORTED      # 2049 lags
    assert muse.rows_lag_range_plan(17, 70000, 256, -7, 0)[0] == RL.UNSUPPORTED
    assert muse.rows_lag_range_plan(17, 70000, 256, -(1 << 30), 1 << 30)[0] == RL.PLAIN
    assert muse.rows_lag_range_plan(17, 300, 256, -5000, 5000)[0] == RL.PLAIN


# ------------------------------------------------------------------ 3. the merge rule
def test_panel_merge_is_the_definition_on_random_cc():
    rng = np.random.default_rng(11)
    for n in (256, 512, 4096):
        for lo, hi in ((-128, 0), (-127, 100), (-100, 155), (-300, 20), (0, 2047), (-1000, 1047), (-200, 50)):
            for _ in range(6):
                cc = rng.standard_normal(n)
                cc[rng.integers(0, n, 5)] = np.nan
                want = LR.ranged(cc, n, lo, hi)
                assert RL.panel_merge(cc, n, lo, hi) == want[:2], (n, lo, hi)
                assert LR.table_argmax(cc, n, lo, hi) == want[:2]
            # nothing above zero, and NaN only: index 0 stands
            z = np.zeros(n)
            assert RL.panel_merge(z, n, lo, hi) == LR.ranged(z, n, lo, hi)[:2] == (0, 0.0)
            z[3 % n] = np.nan
            assert RL.panel_merge(z, n, lo, hi) == (0, 0.0)


def test_panel_merge_with_exact_ties():
    n, lo, hi = 4096, -300, 200            # table rows 0 .. 500: panels 0 .. 3, lag 0 is row 300 (panel 2)
    base = 0.25 * np.random.default_rng(12).random(n)

    def both(cc):
        want = LR.ranged(cc, n, lo, hi)[:2]
        assert RL.panel_merge(cc, n, lo, hi) == want
        return want
    # two equal maxima in two different panels, both negative lags: the earlier scan position (the lower lag) wins
    cc = base.copy()
    cc[(-290) % n] = cc[(-20) % n] = 0.9
    assert both(cc) == (-290, 0.9)
    # opposite signs, equal magnitude, two panels, both positive: the smaller lag wins
    cc = base.copy()
    cc[10], cc[150] = -0.9, 0.9
    assert both(cc) == (10, -0.9)
    # across the lag-0 boundary: a positive lag beats an equal negative one -- though its row comes later in the table
    cc = base.copy()
    cc[(-250) % n] = cc[120] = 0.9
    assert both(cc) == (120, 0.9)
    cc = base.copy()
    cc[(-1) % n] = cc[0] = 0.9
    assert both(cc) == (0, 0.9)
    cc = base.copy()
    cc[(-1) % n] = cc[200] = -0.9           # the last scanned positive lag against the first negative one below zero
    assert both(cc) == (200, -0.9)
    # three panels tie: the definition's first index
    cc = base.copy()
    cc[(-300) % n] = cc[(-100) % n] = cc[199] = 0.9
    assert both(cc) == (199, 0.9)
    # a tie outside the range does not count
    cc = base.copy()
    cc[201] = cc[(-301) % n] = 5.0
    cc[(-5) % n] = 0.9
    assert both(cc) == (-5, 0.9)


# ------------------------------------------------------------------ 4. the GPU tests' inputs hold no tie
def _no_tie(exp, keys, rows=None):
    for k in keys:
        tie = exp[k][2] if rows is None else exp[k][2][rows]
        assert not tie.any(), (k, np.nonzero(tie)[0])


@pytest.mark.parametrize("N", [c[0] for c in RL.PARITY])
def test_no_ties_in_the_parity_inputs(oracle, N):
    ranges = [c[2] for c in RL.PARITY if c[0] == N][0]
    ref, rows, exp, n = RL.parity_case(oracle, N)
    _no_tie(exp, ranges)
    M = rows.shape[0] - RL.SPECIALS
    for k in ranges:                                   # the special rows are what they are said to be
        lag, mv, _ = exp[k]
        assert np.isnan(mv[M]) and lag[M] == 0 and (lag[M + 1], mv[M + 1]) == (0, 0.0)
        assert np.isfinite(mv[M + 2]) and np.isfinite(mv[M + 3]) and mv[M + 3] != 0.0
        lo, hi = LR.clip(n, *k)
        assert np.all((lag >= lo) & (lag <= hi))


def test_no_ties_in_the_other_inputs(oracle):
    for N in RL.NARROW_NS:
        _, _, exp, _ = RL.narrow_case(oracle, N)
        _no_tie(exp, RL.NARROW_RANGES + (RL.NARROW_L,))
    _, _, exp, _ = RL.across_case(oracle)
    wide, narrow = RL.ACROSS[2:]
    _no_tie(exp, (wide, narrow))
    inside = (exp[wide][0] >= narrow[0]) & (exp[wide][0] <= narrow[1]) & np.isfinite(exp[wide][1]) & (exp[wide][1] != 0)
    assert inside.sum() >= 1 and (~inside).sum() >= 1   # rows whose wide winner lies inside the narrow range exist, and others
    _, _, exp, _ = RL.winner_case(oracle)
    _no_tie(exp, RL.WINNER[2])
    for which in (0, 1):
        _, _, exp, _ = RL.cache_case(oracle, which)
        _no_tie(exp, RL.CACHE[2])
    _, _, exp, _ = RL.callers_case(oracle)
    _no_tie(exp, RL.CALLERS[2])


def test_no_ties_in_the_general_path_and_mirror_inputs(oracle):
    ref, rows, pick = RL.general_case()
    N, M, rng_, K = RL.GENERAL
    assert rows.shape == (M, N) and M * N > 1 << 24 and (M - 1) * N <= 1 << 24 and len(pick) == K
    exp, _, _, _ = LR.expect(oracle, ref, rows[pick], (rng_,))
    _no_tie(exp, (rng_,))
    ref, rows = RL.mirror_series()
    exp, glag, _, _ = LR.expect(oracle, ref, rows, RL.MIRROR[3])
    _no_tie(exp, RL.MIRROR[3])
    for k in RL.MIRROR[3]:
        assert (exp[k][0] != glag).sum() * 4 >= len(glag)          # a filter of the unwindowed result cannot pass


def test_the_exact_zero_row_is_rounding_noise_in_the_oracle(oracle):
    """the row of the exact-zero case: the oracle's transform leaves rounding noise inside the range (below the absolute score
    tolerance of 1e-12) where the direct product sums exact zeros -- the GPU test expects the definition's (0, cc[0]) = (0, 0.0)
    for that row and the oracle's answer for the others"""
    ref, rows, zr = RL.zeros_case()
    N, (lo, hi) = RL.ZEROS
    assert ref.sum() == 0.0 and rows[zr].sum() == 0.0 and rows[zr, 0] == 0.0
    at = np.nonzero(rows[zr])[0]
    for t in at:
        idx = t + np.arange(lo, hi + 1)
        assert np.all(ref[idx[(idx >= 0) & (idx < N)]] == 0.0)
    X, n = oracle.ref_spectrum(ref)
    cc, _, _, _ = oracle.xcorr_with_x(X, rows[zr], n)
    assert np.abs(cc[LR.range_indices(n, lo, hi)]).max() < 1e-12
    exp, _, _, _ = LR.expect(oracle, ref, rows[:zr], ((lo, hi),))
    _no_tie(exp, ((lo, hi),))
