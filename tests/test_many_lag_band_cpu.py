"""CPU-only checks of the many-references lag band (muse_batch_score_many_in_lag_band / _run_many_in_lag_band): the exports and their
mirrors exist on every layer, the dispatch (muse_test_many_lag_band_plan) is the table include/muse_hip.h gives, equals
muse_test_many_lag_range_plan where the call delegates and muse_test_lag_band_plan for one reference, the packed kernel's planner
keeps its tile, image and LDS invariants on every W of the bands, the Python mirror refuses what it must without a device, and the
oracle by itself flags no tie on the inputs tests/test_gpu_many_lag_band.py uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LSW
import _manylagband as MLB
import _manylagrange as MLR
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_many_in_lag_band", 5), ("muse_batch_run_many_in_lag_band", 15))
HOOKS = (("muse_test_many_lag_band_plan", 7),)


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
        for name, nargs in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, hdrs[h]), "%s does not declare %s" % (h, name)
            assert hasattr(lib, name) and name in exported, "libmuse_hip.so does not export %s" % name
            assert name in muse.binding.SIGNATURES, "binding.SIGNATURES lacks %s" % name
            args = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdrs[h]).group(1)
            assert len(args.split(",")) == nargs == len(muse.binding.SIGNATURES[name][1]), name
    assert muse.binding.load().muse_abi_version() == 5               # additions only: the ABI version stays


def test_mirrors_carry_the_many_band_forms(muse):
    for name in ("RunManyInLagBand", "RunManySignedInLagBand", "score_many_in_lag_band", "scores_many_in_lag_band",
                 "run_many_in_lag_band", "many_lag_band_plan"):
        assert callable(getattr(muse, name, None)), name
        assert getattr(muse, name) is getattr(muse.many_band, name)
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    assert re.search(r"\bstatic\s+void\s+RunManyInLagBand\s*\(", hpp) and re.search(r"\bstatic\s+void\s+RunManySignedInLagBand\s*\(", hpp)
    assert hpp.count("muse_batch_run_many_in_lag_band(") == 2
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func RunManyInLagBand\(batches \[\]\*Batch, groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert re.search(r"func RunManySignedInLagBand\(batches \[\]\*Batch, groupByLabels \[\]string, lagLo, lagHi int\) error", go)
    assert "C.muse_batch_run_many_in_lag_band(" in go
    assert os.path.exists(muse.build.build_many_lag_band_test())      # the C++ program the GPU suite runs is built with the rest


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    w = ctypes.c_int32(5)
    assert L.muse_batch_score_many_in_lag_band(None, 2, 1, 7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_lag_band(None, 2, None, 0, 1, 7, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    P = L.muse_test_many_lag_band_plan
    assert P(1, 0, 1, 5, 0, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID
    assert P(512, 0, 5, 1, 0, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID       # lag_lo > lag_hi
    assert P(512, 0, 1, 5, 2, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID       # sign 2
    assert P(512, 0, 1, 5, 0, 0, ctypes.byref(w)) == B.MUSE_ERR_INVALID       # R 0
    assert P(64, 0, 100, 226, 0, 2, ctypes.byref(w)) == B.MUSE_ERR_INVALID    # empty after clipping
    assert P(512, 0, 1, 5, 0, 2, None) == B.MUSE_ERR_INVALID
    assert w.value == 5
    assert P(512, 0, 1, 5, 1, 2, ctypes.byref(w)) == B.MUSE_OK and w.value == MLB.MFMA


def test_python_refusals_need_no_device(muse):
    B = muse.binding
    for fn in (lambda: muse.score_many_in_lag_band([], 7, 1), lambda: muse.scores_many_in_lag_band([], 7, 1, 1),
               lambda: muse.run_many_in_lag_band([], 7, 1), lambda: muse.score_many_in_lag_band([], 1, 7, 2),
               lambda: muse.scores_many_in_lag_band([], 1, 7, -2), lambda: muse.run_many_in_lag_band([], 1, 7, sign_filter=3),
               lambda: muse.RunManyInLagBand([], None, 7, 1), lambda: muse.RunManySignedInLagBand([], None, 7, 1)):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == B.MUSE_ERR_INVALID and e.value.message

    class Sharded:                                                   # (what the feed looks at before it touches a device)
        _engines = [object(), object()]

        class Results:
            SignFilter = 7
    for fn in (muse.RunManyInLagBand, muse.RunManySignedInLagBand):
        with pytest.raises(muse.MuseError) as e:
            fn([Sharded()], None, 1, 7)
        assert e.value.status == B.MUSE_ERR_UNSUPPORTED and "one device" in e.value.message
    Sharded._engines = None
    with pytest.raises(muse.MuseError) as e:                         # the shared SignFilter is the argmax's sign: -1 .. 1
        muse.RunManySignedInLagBand([Sharded()], None, 1, 7)
    assert e.value.status == B.MUSE_ERR_INVALID
    assert muse.RunManyInLagBand([], None, 1, 7) is None


# ------------------------------------------------------------------ 2. the dispatch
PLAN_NS = [64, 100, 255, 480, 512, 1025, 1433, 3000, 4096, 5000, 40000, 70000]


@pytest.mark.parametrize("N", PLAN_NS)
def test_plan_is_the_table(muse, N):
    B = muse.binding
    n = muse.next_pow2(float(N))
    ends = sorted({-10 * n, -(n // 2), -(n // 2 - 1), -256, -200, -128, -127, -126, -20, -7, -1, 0, 1, 2, 7, 8, 48, 49, 100, 126, 127, 128,
                   230, n // 2 - 1, n // 2, n // 2 + 1, 10 * n})
    seen = set()
    for f32 in (False, True):
        for R in (1, 2, 8, 17):
            for lo in ends:
                for hi in ends:
                    if lo > hi or LB.clip(n, lo, hi) is None:
                        continue
                    for s in MLB.SIGNS:
                        got = muse.many_lag_band_plan(N, f32, lo, hi, s, R)
                        assert got == MLB.plan_table(N, f32, lo, hi, s, R), (N, f32, lo, hi, s, R, got)
                        seen.add(got)
                        if s == 0 and lo <= 0 <= hi:                 # the call delegates: the range hook, row for row
                            assert got == muse.many_lag_range_plan(N, f32, lo, hi, R)
                        if R == 1:                                   # one reference: the single form's table, its MASKED taken each
                            one = muse.lag_band_plan(N, f32, lo, hi, s)
                            assert got == (B.MUSE_IN_WINDOW_MASKED_EACH if one == B.MUSE_IN_WINDOW_MASKED else one), (N, f32, lo, hi, s)
                        if not (s == 0 and lo <= 0 <= hi):
                            assert got != MLB.PLAIN
    assert MLB.MFMA in seen or N > 65536


def test_plan_pinned_rows(muse):
    P = muse.many_lag_band_plan
    assert P(4096, False, 1, 7, 0, 8) == P(4096, False, 200, 230, -1, 8) == P(4096, False, -7, 0, 1, 8) == MLB.MFMA
    assert P(1000, False, -300, -20, 0, 3) == P(1000, False, 1, 128, 1, 2) == MLB.MASKED
    assert P(1000, False, -300, -20, 0, 1) == P(1000, True, 1, 7, 0, 4) == MLB.MASKED_EACH
    for s in MLB.SIGNS:                                              # n = 4096: one pass on either storage
        assert P(4096, False, 1, 200, s, 4) == P(3000, True, 1, 7, s, 4) == MLB.MASKED
        assert P(4096, False, 1, 200, s, 1) == P(480, True, 1, 200, s, 4) == MLB.MASKED_EACH
    assert P(4096, False, -200, 0, 0, 4) == P(4096, False, -200, 0, 1, 4) == MLB.MASKED
    assert P(1000, False, -5000, 5000, 1, 4) == MLB.MASKED and P(1000, False, -5000, 5000, 0, 4) == MLB.PLAIN   # every lag under a sign
    assert P(5000, False, -5000, 5000, 1, 4) == P(5000, False, 1, 200, 0, 4) == P(70000, False, 1, 7, 0, 4) == MLB.UNSUPPORTED
    assert P(5000, False, 100, 226, 0, 4) == MLB.MFMA


# ------------------------------------------------------------------ 3. the planner on the bands' W
def test_planner_invariants_on_the_bands(muse):
    for lo, hi in MLB.BANDS:
        Wd = hi - lo + 1
        for R in range(1, 18):
            p = muse.window_many_plan_rows(R, Wd)
            refs = np.bincount(p["launch_of"], minlength=p["launches"])
            assert [(int(refs[l]), int(p["tiles_of"][l])) for l in range(p["launches"])] == MLR.plan_rows(R, Wd), (Wd, R)
            for l in range(p["launches"]):
                k, tiles = int(refs[l]), int(p["tiles_of"][l])
                assert 1 <= tiles <= 8 and tiles == (k * Wd + 15) // 16, (Wd, R, l)
                if Wd > 48:
                    assert k == 1, (Wd, R)
                if k > 1:
                    assert k * int(p["img_of"][l]) <= 4608 and MLR.launch_lds_bytes(k, Wd) <= 64 * 1024, (Wd, R, l)
    assert sorted({hi - lo + 1 for lo, hi in MLB.BANDS} & {1, 2, 7, 8, 16, 17, 32, 48, 49, 127}) == [1, 2, 7, 8, 16, 17, 32, 48, 49, 127]


# ------------------------------------------------------------------ 4. the oracle flags no tie the GPU tests could hide behind
def test_oracle_flags_no_tie_on_the_direct_inputs(oracle):
    entries = 0
    for N in MLB.DIRECT_NS:
        ref, rows, refs = MLB.case(N)
        exps, n = MLB.expectations(oracle, refs[:MLB.TIE_RS], rows, MLB.BANDS)
        for r, exp in enumerate(exps):
            for k, (lag, mv, tie) in exp.items():
                assert not tie.any(), (N, r, k, np.nonzero(tie)[0][:5])
                entries += len(tie)
    assert entries == 56070


@pytest.mark.parametrize("N", MLB.MASKED_NS)
def test_oracle_flags_no_tie_on_the_masked_inputs(oracle, N):
    n = LSW.fft_len(N)
    for f32 in (False, True):
        ref, rows, refs = MLB.masked_case(N, f32)
        exps, n2 = MLB.expectations(oracle, refs[:4], rows, LB.masked_bands(n))
        assert n2 == n
        for r, exp in enumerate(exps):
            for k, (lag, mv, tie) in exp.items():
                assert not tie.any(), (N, f32, r, k)
