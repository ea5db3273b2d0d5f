"""CPU-only checks of the many-references lag range (muse_batch_score_many_in_lag_range / _run_many_in_lag_range): the exports and
their mirrors exist on every layer, the dispatch (muse_test_many_lag_range_plan) is the table include/muse_hip.h gives and agrees
with muse_test_many_in_window_plan on symmetric ranges and with muse_test_lag_range_plan for one reference, the packed kernel's
planner in table rows W (muse_test_window_many_plan_rows) equals the planner in L on odd W and keeps its tile, launch and LDS
invariants on every W, and the oracle by itself flags no tie on a continuous-noise row of the inputs
tests/test_gpu_many_lag_range.py uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagrange as LR
import _manylagrange as MLR
import _window as W
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_many_in_lag_range", 4), ("muse_batch_run_many_in_lag_range", 15))
HOOKS = (("muse_test_many_lag_range_plan", 6), ("muse_test_window_many_plan_rows", 8))


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    return m


def _call_args(text, call):
    """the number of arguments of the first call of `call` in text: commas outside nested parentheses"""
    at = text.index(call + "(") + len(call) + 1
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
    assert _call_args(go, "C.muse_batch_run_many_in_lag_range") == 15
    assert _call_args(go, "C.muse_batch_run_many_in_window") == 14
    assert re.search(r"func RunManyInLagRange\(batches \[\]\*Batch, groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_run_many_in_lag_range(muse):
    for name in ("RunManyInLagRange", "score_many_in_lag_range", "scores_many_in_lag_range", "run_many_in_lag_range",
                 "many_lag_range_plan", "window_many_plan_rows"):
        assert callable(getattr(muse, name, None)), name
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bstatic\s+void\s+RunManyInLagRange\s*\(", hpp) and "muse_batch_run_many_in_lag_range(" in hpp
    assert _call_args(hpp, "muse_batch_run_many_in_lag_range") == 15
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, _ in EXPORTS:
        assert name in integ, "INTEGRATION.md does not list %s" % name
    assert os.path.exists(muse.build.build_many_lag_range_test())     # the C++ program the GPU suite runs is built with the rest


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    assert L.muse_batch_score_many_in_lag_range(None, 2, -7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_lag_range(None, 2, None, 0, -7, 0, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    P = L.muse_test_many_lag_range_plan
    assert P(1, 0, -5, 5, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, 1, 5, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID     # excludes lag 0
    assert P(512, 0, -5, -1, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, -5, 5, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, -5, 5, 2, None) == B.MUSE_ERR_INVALID
    n = ctypes.c_int32(0)
    Q = L.muse_test_window_many_plan_rows
    for R, Wd in ((0, 8), (2, 0), (2, 128)):
        assert Q(R, Wd, ctypes.byref(n), None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert Q(2, 8, None, None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert Q(2, 127, ctypes.byref(n), None, None, None, None, None) == B.MUSE_OK and n.value == 2


# ------------------------------------------------------------------ 2. the dispatch
PLAN_NS = [2, 64, 255, 480, 512, 1433, 3000, 4096, 5000, 40000, 70000]


@pytest.mark.parametrize("N", PLAN_NS)
def test_plan_is_the_table(muse, N):
    B = muse.binding
    n = muse.next_pow2(float(N))
    ends = sorted(e for e in {0, 1, 62, 63, 64, 125, 126, 127, 128, n // 2 - 2, n // 2 - 1, n // 2, n // 2 + 1, 10 * n} if e >= 0)
    for f32 in (False, True):
        for R in (1, 2, 8):
            for a in ends:
                for b in ends:
                    got = muse.many_lag_range_plan(N, f32, -a, b, R)
                    assert got == MLR.plan_table(N, f32, -a, b, R), (N, f32, -a, b, R)
                    if R == 1:                                       # one reference: the single form's table, its MASKED taken each
                        one = muse.lag_range_plan(N, f32, -a, b)
                        assert got == (B.MUSE_IN_WINDOW_MASKED_EACH if one == B.MUSE_IN_WINDOW_MASKED else one), (N, f32, -a, b)
            for L in ends:                                           # symmetric: muse_batch_score_many_in_window's table, row for row
                assert muse.many_lag_range_plan(N, f32, -L, L, R) == muse.many_in_window_plan(N, f32, L, R), (N, f32, L, R)


def test_plan_pinned_rows(muse):
    P = muse.many_lag_range_plan
    assert P(4096, False, -126, 0, 8) == MLR.MFMA and P(4096, False, -127, 0, 8) == MLR.MASKED
    assert P(4096, False, -127, 0, 1) == MLR.MASKED_EACH
    assert P(4096, True, -7, 0, 4) == MLR.MASKED and P(480, True, -7, 0, 4) == MLR.MASKED_EACH
    assert P(1000, False, -300, 20, 3) == MLR.MASKED
    assert P(5000, False, -126, 0, 4) == MLR.MFMA and P(5000, False, -200, 0, 4) == MLR.UNSUPPORTED
    assert P(5000, True, -7, 0, 4) == MLR.UNSUPPORTED and P(70000, False, 0, 7, 4) == MLR.UNSUPPORTED
    assert P(100, False, -1000, 63, 4) == MLR.MFMA                   # FFT length 128: -63 .. 63 is 127 lags, -63 .. 64 is every lag
    assert P(100, False, -1000, 70, 4) == P(100, False, -64, 300, 4) == MLR.PLAIN
    for f32 in (False, True):
        assert P(4096, f32, -2047, 2048, 3) == P(4096, f32, -5000, 1 << 30, 3) == MLR.PLAIN


# ------------------------------------------------------------------ 3. the planner in table rows
def _same_plan(a, b):
    return a["launches"] == b["launches"] and a["max_refs"] == b["max_refs"] and \
        all(np.array_equal(a[k], b[k]) for k in ("launch_of", "tiles_of", "img_of", "kc_of"))


def test_planner_in_rows_is_the_planner_in_L_on_odd_rows(muse):
    for L in range(0, 64):
        for R in range(1, 18):
            assert _same_plan(muse.window_many_plan_rows(R, 2 * L + 1), muse.window_many_plan(R, L)), (L, R)


def test_planner_invariants_on_every_row_count(muse):
    for Wd in range(1, 128):
        for R in range(1, 25):
            p = muse.window_many_plan_rows(R, Wd)
            want = MLR.plan_rows(R, Wd)
            refs = np.bincount(p["launch_of"], minlength=p["launches"])
            assert p["launches"] == len(want) and p["max_refs"] == MLR.plan_max_refs(Wd), (Wd, R)
            assert np.all(np.diff(p["launch_of"]) >= 0)                # consecutive launches
            for l in range(p["launches"]):
                k, tiles = int(refs[l]), int(p["tiles_of"][l])
                assert (k, tiles) == want[l] and tiles == (k * Wd + 15) // 16 and 1 <= tiles <= 8, (Wd, R, l)
                if Wd > 48:
                    assert k == 1, (Wd, R)
                if k > 1:                                              # a packed launch: the images' budget and the launch's LDS
                    img, kc = int(p["img_of"][l]), int(p["kc_of"][l])
                    assert img == MLR.plan_img(Wd, kc) and kc == MLR.plan_kc(Wd, k)
                    assert img % 32 == (Wd + 2) % 32 and img >= kc + Wd - 1 and kc in (256, 512, 1024)
                    assert k * img <= 4608 and MLR.launch_lds_bytes(k, Wd) <= 64 * 1024, (Wd, R, l)
                    # the bank argument (xcorr_window_many.hip): a tile's rows of m references span 16 + 2 m doubles modulo 32
                    for t in range(tiles):
                        rows = range(16 * t, min(16 * t + 16, k * Wd))
                        m = len({rr // Wd for rr in rows})
                        assert m <= 8 or Wd == 1, (Wd, R, l, t, m)


def test_planner_pinned_table(muse):
    for (Wd, R), want in MLR.PLAN_TABLE.items():
        p = muse.window_many_plan_rows(R, Wd)
        refs = np.bincount(p["launch_of"], minlength=p["launches"])
        assert [(int(refs[l]), int(p["tiles_of"][l])) for l in range(p["launches"])] == want, (Wd, R)
    # [-31, 0] packs four references where +-31 packed none
    assert muse.window_many_plan_rows(4, 32)["launches"] == 1 and muse.window_many_plan(4, 31)["launches"] == 4


# ------------------------------------------------------------------ 4. the oracle flags no tie the GPU tests could hide behind
@pytest.mark.parametrize("N", MLR.PARITY_NS)
def test_oracle_flags_no_tie_on_noise_rows(oracle, N):
    ref, rows, refs = MLR.case(N)
    M = rows.shape[0]
    keep = W.plain_rows(M)
    exps, n = MLR.expectations(oracle, refs, rows, MLR.ranges_of(N), Ls=MLR.CPU_RANGES_SYM)
    for r, (exp, glag, gmv) in enumerate(exps):
        for k in MLR.ranges_of(N):
            assert not (exp[k][2] & keep).any(), (N, r, k, np.nonzero(exp[k][2] & keep)[0][:5])
            lo, hi = LR.clip(n, *k)
            assert np.all((exp[k][0] >= lo) & (exp[k][0] <= hi))
    if True:   # filtering the symmetric window's answer cannot pass: winners inside +-63 on the other side of both halves
        for exp, _, _ in exps[:4]:
            sym = exp[63][0]
            for lo, hi in ((-63, 0), (0, 63)):
                assert int((keep & ((sym < lo) | (sym > hi))).sum()) >= 59, (N, lo, hi)


@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", LR.MASKED_NS)
def test_oracle_flags_no_tie_on_masked_inputs(oracle, N, f32):
    ref, rows, refs = MLR.masked_case(N, f32)
    keep = W.plain_rows(rows.shape[0])
    n = muse_n = 1 << (N - 1).bit_length()
    exps, n2 = MLR.expectations(oracle, refs[:MLR.MASKED_R], rows, LR.masked_ranges(n, f32))
    assert n2 == muse_n
    for r, (exp, _, _) in enumerate(exps):
        for k, (lag, mv, tie) in exp.items():
            assert not (tie & keep).any(), (N, f32, r, k)
