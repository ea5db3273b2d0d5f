"""CPU-only checks of the many-references lag bands (muse_batch_score_many_in_lag_bands / _run_many_in_lag_bands): the exports and
their mirrors exist on every layer, NULL and bad arguments fail loudly, the Python mirror refuses what it must without a device,
the planner (muse_test_many_lag_bands_plan) keeps its tile, row, image and LDS invariants on random lists and gives the launches
tests/_manylagbands.py writes down for the named assignments, and the oracle by itself flags no tie on the tuples
tests/test_gpu_many_lag_bands.py uses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LSW
import _manylagbands as MB
import _manylagrange as MLR
from _load import ROOT, pkg

EXPORTS = (("muse_batch_score_many_in_lag_bands", 5), ("muse_batch_run_many_in_lag_bands", 16))
HOOKS = (("muse_test_many_lag_bands_plan", 12),)
MFMA = 2


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


def test_mirrors_carry_the_many_bands_forms(muse):
    for name in ("RunManyInLagBands", "RunManySignedInLagBands", "RunManySigned", "score_many_in_lag_bands", "scores_many_in_lag_bands",
                 "run_many_in_lag_bands", "many_lag_bands_plan"):
        assert callable(getattr(muse, name, None)), name
        assert getattr(muse, name) is getattr(muse.many_bands, name)
    hpp = open(os.path.join(ROOT, "go-muse_amd", "host", "muse.hpp")).read()
    for name in ("RunManyInLagBands", "RunManySignedInLagBands", "RunManySigned"):
        assert re.search(r"\bstatic\s+void\s+%s\s*\(" % name, hpp), name
    assert "muse_batch_run_many_in_lag_bands(" in hpp
    go = open(os.path.join(ROOT, "go-muse_amd", "go", "muse_hip.go")).read()
    assert re.search(r"func RunManyInLagBands\(batches \[\]\*Batch, groupByLabels \[\]string, bands \[\]\[2\]int\) error", go)
    assert re.search(r"func RunManySignedInLagBands\(batches \[\]\*Batch, groupByLabels \[\]string, bands \[\]\[2\]int\) error", go)
    assert re.search(r"func RunManySigned\(batches \[\]\*Batch, groupByLabels \[\]string\) error", go)
    assert "C.muse_batch_run_many_in_lag_bands(" in go


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_null_and_bad_arguments_fail_loudly(muse):
    B = muse.binding
    L = B.load()
    lo, hi, sg = _i32(1, -7), _i32(7, -1), _i32(0, 1)
    assert L.muse_batch_score_many_in_lag_bands(None, 2, lo, hi, sg) == B.MUSE_ERR_INVALID
    tn, thr = _i32(5, 5), (ctypes.c_double * 2)(0.0, 0.0)
    assert L.muse_batch_run_many_in_lag_bands(None, 2, None, 0, lo, hi, tn, thr, sg, 1, 5, None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_lag_bands(None, 2, None, 0, lo, hi, None, thr, sg, 1, 5, None, None, None, None, None) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_many_in_lag_bands(None, 2, None, 0, lo, hi, tn, thr, sg, 1, 4, None, None, None, None, None) == B.MUSE_ERR_INVALID
    P = L.muse_test_many_lag_bands_plan
    out = [_i32(5, 5) for _ in range(5)]
    n = ctypes.c_int32(5)

    def plan(N, R, lo, hi, sg, path=out[0], of=out[1], launches=ctypes.byref(n), tiles=out[2], kc=out[3], img0=out[4]):
        return P(N, 0, R, lo, hi, sg, path, of, launches, tiles, kc, img0)
    assert plan(1, 2, lo, hi, sg) == B.MUSE_ERR_INVALID                       # N < 2
    assert plan(512, 0, lo, hi, sg) == B.MUSE_ERR_INVALID                     # R 0
    assert plan(512, 2, None, hi, sg) == B.MUSE_ERR_INVALID and plan(512, 2, lo, None, sg) == B.MUSE_ERR_INVALID
    assert plan(512, 2, _i32(1, 7), _i32(7, 1), sg) == B.MUSE_ERR_INVALID     # lag_lo > lag_hi at index 1
    assert plan(512, 2, lo, hi, _i32(0, 2)) == B.MUSE_ERR_INVALID             # sign 2 at index 1
    assert plan(100, 2, _i32(1, 100), _i32(7, 226), sg) == B.MUSE_ERR_INVALID # empty after clipping at n = 128, index 1
    for k in ("path", "of", "launches", "tiles", "kc", "img0"):
        assert plan(512, 2, lo, hi, sg, **{k: None}) == B.MUSE_ERR_INVALID
    assert n.value == 5 and all(list(a) == [5, 5] for a in out)               # the outputs are as they were
    assert plan(512, 2, lo, hi, None) == B.MUSE_OK and n.value == 1           # sign NULL: by magnitude
    assert list(out[0]) == [MFMA, MFMA] and list(out[1]) == [0, 0] and out[2][0] == 1 and out[3][0] == 1024


def test_python_refusals_need_no_device(muse):
    B = muse.binding
    for fn in (lambda: muse.score_many_in_lag_bands([None], [(7, 1)]), lambda: muse.scores_many_in_lag_bands([None, None], [(1, 7), (7, 1)]),
               lambda: muse.run_many_in_lag_bands([None], [(7, 1)]), lambda: muse.score_many_in_lag_bands([None], [(1, 7)], 2),
               lambda: muse.scores_many_in_lag_bands([None, None], [(1, 7), (1, 7)], [0, -2]),
               lambda: muse.run_many_in_lag_bands([None], [(1, 7)], sign_filter=3),
               lambda: muse.score_many_in_lag_bands([None, None], [(1, 7)]),                    # one band for two batches
               lambda: muse.run_many_in_lag_bands([None, None], [(1, 7), (1, 7)], top_n=[5]),  # one top_n for two batches
               lambda: muse.many_lag_bands_plan(480, False, [(1, 7), (9, 8)])):
        with pytest.raises(muse.MuseError) as e:                     # (the checks come before the handles are touched)
            fn()
        assert e.value.status == B.MUSE_ERR_INVALID and e.value.message

    class Res:
        def __init__(self, max_lag, sign):
            self.MaxLag, self.SignFilter = max_lag, sign

    class Fake:                                                       # (what the feed looks at before it touches a device)
        def __init__(self, engines, max_lag=5, sign=0):
            self._engines, self.Results = engines, Res(max_lag, sign)
    for fn in (lambda b: muse.RunManyInLagBands(b, None, [(1, 7)]), lambda b: muse.RunManySignedInLagBands(b, None, [(1, 7)]),
               lambda b: muse.RunManySigned(b, None)):
        with pytest.raises(muse.MuseError) as e:
            fn([Fake([object(), object()])])
        assert e.value.status == B.MUSE_ERR_UNSUPPORTED and "one device" in e.value.message
    with pytest.raises(muse.MuseError) as e:                         # each batch's own SignFilter is its argmax's sign: -1 .. 1
        muse.RunManySignedInLagBands([Fake(None, sign=7)], None, [(1, 7)])
    assert e.value.status == B.MUSE_ERR_INVALID
    with pytest.raises(muse.MuseError) as e:
        muse.RunManySigned([Fake(None, max_lag=-1)], None)
    assert e.value.status == B.MUSE_ERR_INVALID
    with pytest.raises(muse.MuseError) as e:
        muse.RunManyInLagBands([Fake(None), Fake(None)], None, [(1, 7)])
    assert e.value.status == B.MUSE_ERR_INVALID
    assert muse.RunManyInLagBands([], None, []) is None and muse.RunManySigned([], None) is None


# ------------------------------------------------------------------ 2. the planner
def place(Ws, kc):
    """tests' own statement of the image placement: img0[0] = 0, img0[j + 1] the smallest offset >= img0[j] + kc + W_j - 1 with
    img0[j + 1] - img0[j] = W_j + 2 (mod 32); returns (img0, the offset behind the last image)"""
    at, out = 0, []
    for Wd in Ws:
        out.append(at)
        step = kc + Wd - 1
        while step % 32 != (Wd + 2) % 32:
            step += 1
        at += step
    return out, at


def check_plan(p, Ws, tag):
    """the invariants of a plan for references of Ws[r] table rows on the direct product (0: not on it)"""
    R = len(Ws)
    assert len(p["launch_of"]) == R and len(p["tiles_of"]) == len(p["kc_of"]) == p["launches"], tag
    first_seen = []
    for r in range(R):
        l = int(p["launch_of"][r])
        assert (l == -1) == (Ws[r] == 0), (tag, r)
        if l >= 0 and l not in first_seen:
            first_seen.append(l)
    assert first_seen == list(range(p["launches"])), (tag, "launches are numbered by their first member")
    for l in range(p["launches"]):
        mem = [r for r in range(R) if p["launch_of"][r] == l]
        rows, tiles, kc = sum(Ws[r] for r in mem), int(p["tiles_of"][l]), int(p["kc_of"][l])
        assert 1 <= tiles <= 8 and tiles == (rows + 15) // 16 and rows <= 128, (tag, l)
        if len(mem) == 1:
            assert kc == 1024 and p["img0"][mem[0]] == 0, (tag, l)
            continue
        assert all(Ws[r] <= 48 for r in mem), (tag, l, "W > 48 is always alone")
        assert kc in (256, 512, 1024), (tag, l)
        img0, end = place([Ws[r] for r in mem], kc)
        assert [int(p["img0"][r]) for r in mem] == img0, (tag, l)
        assert end <= 4608 and place([Ws[r] for r in mem], 256)[1] <= 4608, (tag, l)
        assert kc == 1024 or place([Ws[r] for r in mem], 2 * kc)[1] > 4608, (tag, l, "the largest chunk that fits")
        for a, b in zip(mem, mem[1:]):
            d = int(p["img0"][b]) - int(p["img0"][a])
            assert d % 32 == (Ws[a] + 2) % 32 and d >= kc + Ws[a] - 1, (tag, l, "congruent, no overlap")
        parts = max(1, 16 // len(mem))
        assert 8 * (max(end, tiles * 256) + 128 + len(mem) * parts * 48) <= 64 * 1024, (tag, l)
    # the greedy cut: a packable reference opens a launch only when it does not fit the open one
    open_mem = None
    for r in range(R):
        if Ws[r] == 0 or Ws[r] > 48:
            continue
        l = int(p["launch_of"][r])
        if open_mem is not None and l != open_mem[0]:
            w = [Ws[q] for q in open_mem[1]] + [Ws[r]]
            assert sum(w) > 128 or place(w, 256)[1] > 4608, (tag, r, "closed a launch that had room")
            open_mem = None
        if open_mem is None:
            open_mem = (l, [])
        open_mem[1].append(r)


def band_of_rows(rng, Wd):
    """a band or range of Wd lags inside +-200"""
    lo = int(rng.integers(-200, 201 - Wd))
    return lo, lo + Wd - 1


def test_planner_invariants_on_random_lists(muse):
    rng = np.random.default_rng(20)
    mixed = 0
    for R in range(1, 18):
        for trial in range(40):
            kind = trial % 4
            top = (3, 17, 48, 127)[kind]
            Ws = [int(rng.integers(1, top + 1)) for _ in range(R)]
            bands = [band_of_rows(rng, Wd) for Wd in Ws]
            signs = [int(rng.integers(-1, 2)) for _ in range(R)]
            p = muse.many_lag_bands_plan(1000, False, bands, signs)
            assert list(p["path"]) == [MFMA] * R
            check_plan(p, Ws, (R, trial, Ws))
            mixed += p["launches"] < R
    assert mixed > 300
    # references off the direct product take no launch: more than 127 lags, float32 storage
    p = muse.many_lag_bands_plan(1000, False, [(1, 7), (1, 200), (-7, -1)], [0, 1, -1])
    assert list(p["path"]) == [MFMA, 3, MFMA] and list(p["launch_of"]) == [0, -1, 0] and p["launches"] == 1
    check_plan(p, [7, 0, 7], "one masked")
    p = muse.many_lag_bands_plan(1000, True, [(1, 7), (-7, -1)], None)
    assert list(p["path"]) == [3, 3] and list(p["launch_of"]) == [-1, -1] and p["launches"] == 0


@pytest.mark.parametrize("N", MB.DIRECT_NS)
def test_named_assignments_plan_as_written(muse, N):
    n = LSW.fft_len(N)
    for name, assign in MB.ASSIGNMENTS:
        bands, signs = MB.bands_of(assign), MB.signs_of(assign)
        clipped = [LB.clip(n, lo, hi) for lo, hi in bands]
        if any(c is None for c in clipped):
            assert name == "FAR" and N == 100
            with pytest.raises(muse.MuseError) as e:
                muse.many_lag_bands_plan(N, False, bands, signs)
            assert e.value.status == muse.binding.MUSE_ERR_INVALID
            continue
        p = muse.many_lag_bands_plan(N, False, bands, signs)
        Ws = [hi - lo + 1 for lo, hi in clipped]
        check_plan(p, Ws, (name, N))
        if name == "UNIFORM":                                        # a uniform list gives the launches of window_many_plan_rows
            q = muse.window_many_plan_rows(len(assign), Ws[0])
            assert p["launches"] == q["launches"] and list(p["launch_of"]) == list(q["launch_of"])
            assert list(p["tiles_of"]) == list(q["tiles_of"]) and list(p["kc_of"]) == list(q["kc_of"])
            assert [int(p["img0"][r]) for r in range(len(assign))] == [r * int(q["img_of"][0]) for r in range(len(assign))]
            continue
        if Ws != [hi - lo + 1 for lo, hi in bands]:                  # (n = 128 clips CUT and ALONE: the invariants above hold)
            assert N == 100
            continue
        got = [(tuple(r for r in range(len(assign)) if p["launch_of"][r] == l), int(p["tiles_of"][l]), int(p["kc_of"][l]))
               for l in range(p["launches"])]
        assert got == MB.LAUNCHES[name], (name, N, got)


@pytest.mark.parametrize("Wd", (1, 2, 3, 7, 8, 16, 17, 32, 48, 49, 127))
def test_uniform_lists_plan_as_the_uniform_planner(muse, Wd):
    for R in range(1, 18):
        p = muse.many_lag_bands_plan(1000, False, [(1, Wd)] * R, 1)
        q = muse.window_many_plan_rows(R, Wd)
        assert p["launches"] == q["launches"] and list(p["launch_of"]) == list(q["launch_of"]), (Wd, R)
        assert list(p["tiles_of"]) == list(q["tiles_of"]), (Wd, R)
        assert [(int(c), int(t)) for c, t in zip(np.bincount(p["launch_of"]), p["tiles_of"])] == MLR.plan_rows(R, Wd)
        for l in range(p["launches"]):
            mem = [r for r in range(R) if p["launch_of"][r] == l]
            if len(mem) > 1:
                assert int(p["kc_of"][l]) == int(q["kc_of"][l]) == MLR.plan_kc(Wd, len(mem))
                assert [int(p["img0"][r]) for r in mem] == [k * MLR.plan_img(Wd, int(p["kc_of"][l])) for k in range(len(mem))]


# ------------------------------------------------------------------ 3. the oracle flags no tie the GPU tests could hide behind
def test_oracle_flags_no_tie_on_the_gpu_tests_tuples(oracle):
    tuples = MB.tuples()
    assert len(tuples) == TUPLES
    entries = 0
    for N in MB.DIRECT_NS:
        exp, n = MB.expectations(oracle, N)
        for (r, lo, hi, s) in tuples:
            if LB.clip(n, lo, hi) is None:
                assert N == 100 and (lo, hi) in MB.bands_of(MB.FAR)
                continue
            lag, mv, tie = exp[(r, lo, hi, s)]
            assert not tie.any(), (N, r, lo, hi, s, np.nonzero(tie)[0][:5])
            entries += len(tie)
    assert entries == (4 * TUPLES - FAR_TUPLES) * MB.M


def test_oracle_flags_no_tie_on_the_other_gpu_inputs(oracle):
    """the 200-lag reference of the GPU test's list that leaves the direct product, and the Run form's references"""
    ref, rows, refs = MB.case(MB.WIDE_N)
    (lo, hi), s = MB.WIDE
    exp, n = LB.expect(oracle, refs[MB.WIDE_REF], rows, ((lo, hi),), (s,))
    assert n == 512 and not exp[(lo, hi, s)][2].any()
    for N in MB.RUN_NS:
        ref, rows = LB.run_case(N)
        refs = MLR.make_refs(ref, N, 1000 + N)
        for r, ((lo, hi), s) in enumerate(MB.RUN_ASSIGN):
            exp, n = LB.expect(oracle, refs[r], rows, ((lo, hi),), (s,))
            assert not exp[(lo, hi, s)][2].any(), (N, r)


TUPLES = 43      # (reference, lo, hi, sign) tuples of tests/_manylagbands.py's lists
FAR_TUPLES = 6  # of them inside FAR's bands: empty at N = 100
