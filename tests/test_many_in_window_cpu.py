"""CPU-only checks of many references inside a lag window of any width (muse_batch_score_many_in_window / _run_many_in_window): the
exports and their mirrors exist on every layer, the dispatch (muse_test_many_in_window_plan) is the table include/muse_hip.h gives,
the quotient form of the mask the many-references n = 4096 kernel uses keeps exactly the window's indices, bad lists and a missing
device are answered with a status, and the oracle by itself flags no tie on the inputs tests/test_gpu_many_in_window.py uses
(tests/_manyinwindow.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _inwindow as IW
import _lagsweep as LS
import _manyinwindow as MW
import _window as W
from _load import ROOT, pkg

EXPORTS = ("muse_batch_score_many_in_window", "muse_batch_run_many_in_window")
HOOKS = ("muse_test_many_in_window_plan",)


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
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
    for name in HOOKS:                                               # the hooks are in the test header only
        assert not re.search(r"\b%s\b" % name, hdrs["muse_hip.h"]), name
    for name, nargs in (("muse_batch_score_many_in_window", 3), ("muse_batch_run_many_in_window", 14),
                        ("muse_test_many_in_window_plan", 5)):
        h = hdrs["muse_hip.h"] if name in EXPORTS else hdrs["muse_hip_test.h"]
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, h).group(1)
        assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    # the prototypes are those of the windowed many-references forms, argument for argument
    assert muse.binding.SIGNATURES["muse_batch_score_many_in_window"] == muse.binding.SIGNATURES["muse_batch_score_many_windowed"]
    assert muse.binding.SIGNATURES["muse_batch_run_many_in_window"] == muse.binding.SIGNATURES["muse_batch_run_many_windowed"]
    m = re.search(r"#define\s+MUSE_IN_WINDOW_MASKED_EACH\s+(\d+)", hdrs["muse_hip_test.h"])
    assert m and int(m.group(1)) == 4 == muse.binding.MUSE_IN_WINDOW_MASKED_EACH == MW.MASKED_EACH
    for k, v in (("UNSUPPORTED", MW.UNSUPPORTED), ("PLAIN", MW.PLAIN), ("MFMA", MW.MFMA), ("MASKED", MW.MASKED)):
        assert getattr(muse.binding, "MUSE_IN_WINDOW_" + k) == v
    assert muse.binding.load().muse_abi_version() == 5               # backward compatible additions: the ABI version stays


def test_mirrors_carry_run_many_in_window(muse):
    for name in ("RunManyInWindow", "run_many_in_window", "score_many_in_window", "scores_many_in_window", "many_in_window_plan"):
        assert callable(getattr(muse, name, None)), name
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bstatic\s+void\s+RunManyInWindow\s*\(", hpp) and "muse_batch_run_many_in_window(" in hpp
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func RunManyInWindow\(batches \[\]\*Batch, groupByLabels \[\]string\) error", go)
    assert "C.muse_batch_run_many_in_window(" in go
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    # the C++ program the GPU suite runs is built with the rest and stays out of the history
    exe = muse.build.build_many_in_window_test()
    assert os.path.exists(exe) and exe == muse.build.MANY_IN_WINDOW_TEST
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert os.path.relpath(exe, ROOT) in ignored


def test_bad_lists_and_no_gpu_are_a_status_not_a_crash(muse):
    import torch
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    run_tail = (None, 0, 100, 5, 0.0, 0, 1, None, None, None, None, None)
    assert L.muse_batch_score_many_in_window(None, 2, 100) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_window(None, 2, *run_tail) == B.MUSE_ERR_INVALID
    two = (ctypes.c_void_p * 2)(None, None)
    assert L.muse_batch_score_many_in_window(two, 0, 100) == B.MUSE_ERR_INVALID          # R < 1
    assert L.muse_batch_score_many_in_window(two, 2, 100) == B.MUSE_ERR_INVALID          # a NULL batch in the list
    assert L.muse_batch_run_many_in_window(two, 2, *run_tail) == B.MUSE_ERR_INVALID
    assert B.load().muse_last_error()
    for args in ((1, 0, 5, 2, ctypes.byref(w)), (512, 0, -1, 2, ctypes.byref(w)), (512, 0, 5, 0, ctypes.byref(w)), (512, 0, 5, 2, None)):
        assert L.muse_test_many_in_window_plan(*args) == B.MUSE_ERR_INVALID, args[:4]
    if torch.cuda.is_available():
        return
    with pytest.raises(muse.MuseError) as e:
        eng = muse.Engine(0)
        dg = muse.DeviceGroup.from_rows(eng, np.zeros((2, 512)))
        muse.score_many_in_window([muse.DeviceBatch(eng, dg, np.arange(512.0)), muse.DeviceBatch(eng, dg, np.arange(512.0)[::-1])], 100)
    assert e.value.status == B.MUSE_ERR_NO_DEVICE


# ------------------------------------------------------------------ 2. the dispatch
@pytest.mark.parametrize("N", [256, 257, 480, 512, 1000, 2048, 3000, 4096, 4097, 16384, 65536, 65537])
def test_plan_is_the_table(muse, N):
    n = LS.fft_len(N)
    for f32 in (False, True):
        for max_lag in (0, 63, 64, n // 2 - 1, n // 2, 10 * n):
            for R in (1, 2, 8):
                assert muse.many_in_window_plan(N, f32, max_lag, R) == MW.plan_table(N, f32, max_lag, R), (N, f32, max_lag, R)
    # the cells the header spells out
    assert muse.many_in_window_plan(N, False, n // 2, 8) == muse.many_in_window_plan(N, True, 10 * n, 1) == MW.PLAIN
    if N <= 65536:
        assert muse.many_in_window_plan(N, False, 63, 8) == MW.MFMA
    if N in (4096, 3000):
        assert muse.many_in_window_plan(N, False, 64, 2) == muse.many_in_window_plan(N, True, 7, 8) == MW.MASKED
        assert muse.many_in_window_plan(N, False, 64, 1) == muse.many_in_window_plan(N, True, 7, 1) == MW.MASKED_EACH
    if N in (257, 480, 512, 1000, 2048):
        assert muse.many_in_window_plan(N, False, 64, 2) == MW.MASKED
        assert muse.many_in_window_plan(N, False, 64, 1) == muse.many_in_window_plan(N, True, 64, 8) == MW.MASKED_EACH
    if N in (256, 4097, 16384, 65536, 65537):
        assert muse.many_in_window_plan(N, False, 64, 8) == muse.many_in_window_plan(N, True, 7, 8) == MW.UNSUPPORTED
    # R == 1 on the masked lengths is the single-batch dispatch's masked pass
    for f32 in (False, True):
        for max_lag in (0, 64, n // 2 - 1):
            single = muse.in_window_plan(N, f32, max_lag)
            many = muse.many_in_window_plan(N, f32, max_lag, 1)
            assert (many == MW.MASKED_EACH) == (single == MW.MASKED) and (many == single or single == MW.MASKED)


# ------------------------------------------------------------------ 3. the quotient form of the mask keeps the window
@pytest.mark.parametrize("n,step", [(4096, 256), (512, 32)])
def test_quotient_rule_keeps_exactly_the_window(n, step):
    Ls = range(0, n // 2 + 2) if n == 512 else (0, 1, 63, 64, 100, 255, 256, 257, 511, 512, 513, 1000, 2047, 2048, 2049, 5000)
    for L in Ls:
        want = np.zeros(n, dtype=bool)
        want[W.window_indices(n, L)] = True
        assert np.array_equal(MW.quotient_rule(n, step, L), want), L


# ------------------------------------------------------------------ 4. the oracle flags no tie the GPU tests could hide behind
def _noise_ties_within_cap(tie, keep):
    return int((tie & keep).sum()) * 1000 <= len(tie)               # tests/test_in_window_cpu.py: at most 1 in 1000 noise rows


def _ties(oracle, refs, rows, Ls, keep):
    for r, ref in enumerate(refs):
        exp, _, _, _ = W.expect(oracle, ref, rows, Ls)
        for L in Ls:
            assert _noise_ties_within_cap(exp[L][2], keep), (r, L, np.nonzero(exp[L][2] & keep)[0][:8])


@pytest.mark.parametrize("N", IW.PARITY_NS)
def test_oracle_flags_no_tie_parity_inputs(oracle, N):
    ref, rows = IW.parity_case(N)
    _ties(oracle, MW.refs_of(ref, MW.PARITY_ROLLS), rows, MW.parity_Ls(LS.fft_len(N)), W.plain_rows(IW.PARITY_M))


@pytest.mark.parametrize("N", IW.EDGE_NS)
def test_oracle_flags_no_tie_planted_inputs(oracle, N):
    ref, rows, n, where = IW.edge_case(N)
    for ref_r in MW.refs_of(ref, MW.EDGE_ROLLS):
        exp, _, _, _ = W.expect(oracle, ref_r, rows, IW.edge_Ls(n))
        for L in IW.edge_Ls(n):
            assert not exp[L][2].any(), (N, L)                       # planted rows: zero ties
            assert np.all(np.abs(exp[L][0]) <= L)
    exp, _, _, _ = W.expect(oracle, ref, rows, IW.edge_Ls(n))
    for L in IW.edge_Ls(n):                                          # the unrolled reference finds the planted lag where it is inside
        r, lags = where[L]
        inside = np.abs(lags) <= L
        assert np.array_equal(exp[L][0][r][inside], lags[inside])


@pytest.mark.parametrize("N,M", MW.LOOP_CASES)
def test_oracle_flags_no_tie_loop_inputs(oracle, N, M):
    ref, rows = MW.loop_case(N, M)
    _ties(oracle, MW.refs_of(ref, MW.ROLLS3), rows, (MW.LOOP_L,), W.plain_rows(M))


def test_oracle_flags_no_tie_other_inputs(oracle):
    ref, rows = IW.redo_case()
    _ties(oracle, MW.refs_of(ref, MW.ROLLS3), rows, (IW.REDO_L,), W.plain_rows(IW.REDO_M))
    for N in MW.F32_ONE_PASS_NS + (MW.F32_EACH_N,):
        ref, rows = IW.f32_case(N)
        _ties(oracle, MW.refs_of(ref, MW.ROLLS3), rows, IW.F32_LS, W.plain_rows(IW.F32_M))
    for N in MW.IDENT_NS:
        ref, rows = MW.ident_case(N)
        _ties(oracle, MW.refs_of(ref, MW.ROLLS3), rows, (100,), W.plain_rows(MW.IDENT_M))
    ref, rows = IW.run_case()
    _ties(oracle, MW.refs_of(ref, MW.ROLLS3), rows, (IW.RUN_L,), W.plain_rows(IW.RUN_M))
    refs, rows = MW.cpp_case()
    for ref in refs:
        exp, _, _, _ = W.expect(oracle, ref, rows, (MW.CPP_L,))
        assert not exp[MW.CPP_L][2].any()
