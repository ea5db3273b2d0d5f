"""GPU tests of the window as an argument (muse_batch_score_in_window / _run_in_window, run with -m gpu on an MI355X): lag windows
wider than MUSE_LAG_WINDOW_MAX, and windows over float32-storage groups, from the transform kernels with a masked argmax (the WIN
builds of xcorr_r16_fold.hip, xcorr_r16_occ4.hip and xcorr_small.hip), through the C ABI.

Expected values never come from the code under test: per series, the definition in include/muse_hip.h applied in numpy
(tests/_window.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those windowed
(lag, mv).  Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact except rows the
ORACLE flags as ties (two top |cc| inside the window within 1e-12 relative); tests/test_in_window_cpu.py checks on the same inputs
(tests/_inwindow.py) that the oracle flags none on planted rows and no more than 1 in 1000 noise rows.  Planted winners are held to
tests/_lagsweep.py's bound against the long-double score at the planted index."""
import subprocess

import numpy as np
import pytest

import _inwindow as IW
import _lagsweep as LSW
import _window as W
from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
SCORE_ATOL = 1e-12


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return m


@pytest.fixture(scope="module")
def eng(muse):
    return muse.get_engine(0)


def check(lag, mv, elag, emv, tie, tag=""):
    """scores to tolerance, NaN pattern equal, lags exact off the oracle's ties; returns the worst relative score error"""
    lag, mv, elag, emv, tie = map(np.asarray, (lag, mv, elag, emv, tie))
    nan_e = np.isnan(emv)
    assert np.array_equal(np.isnan(mv), nan_e), "%s NaN pattern: %s vs %s" % (tag, np.nonzero(np.isnan(mv))[0][:8], np.nonzero(nan_e)[0][:8])
    ok = ~nan_e
    err = np.abs(mv[ok] - emv[ok])
    rel = err / np.maximum(np.abs(emv[ok]), 1e-300)
    worst = float(rel[np.abs(emv[ok]) > 0].max()) if (np.abs(emv[ok]) > 0).any() else 0.0
    print("%s: worst score rel err %.3e, ties %d of %d" % (tag, worst, int(tie.sum()), len(tie)))
    err = np.where(tie[ok], np.abs(np.abs(mv[ok]) - np.abs(emv[ok])), err)
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "%s score mismatch: worst rel %.3e" % (tag, worst)
    bad = (lag != elag) & ~tie
    assert not bad.any(), "%s lag mismatches at rows %s: %s vs %s" % (tag, np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    return worst


def _masked(muse, db):
    return db.last_in_window_path() == muse.binding.MUSE_IN_WINDOW_MASKED


# ------------------------------------------------------------------ 1. parity against the definition
@pytest.mark.parametrize("N", IW.PARITY_NS)
def test_parity_wide_windows(muse, eng, oracle, N):
    """make_case rows with the eight specials (NaN, Inf, 1e+-100 and mean 1e6 go through the redo kernel at n = 4096), an odd row
    count, windows whose edge lies inside a lane range, on a 256-index register block and on a wave boundary"""
    ref, rows = IW.parity_case(N)
    n = LSW.fft_len(N)
    Ls = IW.parity_Ls(n)
    exp, glag, gmv, n2 = W.expect(oracle, ref, rows, Ls)
    assert n2 == n
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == n
    for L in Ls:
        lag, mv = db.scores_in_window(L)
        assert _masked(muse, db), (N, L, db.last_in_window_path())
        assert db.lag_window() == -1 and db.last_run_path() == 0
        check(lag, mv, *exp[L], tag="parity N=%d L=%d" % (N, L))
        assert np.all(np.abs(lag) <= L)
        name = eng.kernel_name(db)
        assert name.endswith(", true>") and name.startswith("xcorr_fused_n4096_fold<" if n == 4096 else "xcorr_fused_small<"), name
    # some rows have their global winner outside a window of 64 and some inside: the mask is not vacuous
    keep = W.plain_rows(IW.PARITY_M)
    inside = np.abs(glag) <= Ls[0]
    assert (inside & keep).sum() >= 4 and (~inside & keep).sum() >= 4
    db.scores()
    assert db.last_in_window_path() == 0 and not eng.kernel_name(db).endswith(", true>")
    db.close()
    dg.close()


# ------------------------------------------------------------------ 2. window edges from planted winners
@pytest.mark.parametrize("N", IW.EDGE_NS)
def test_edges_from_planted_winners(muse, eng, oracle, N):
    """a code planted at the lags +-(L - 1), +-L comes back there, with the long-double score at that index; planted at +-(L + 1) it is
    outside: the result lies inside the window and is the definition's on the oracle's cc -- an off-by-one on either side, on the
    positive or the wrapped half, shows"""
    ref, rows, n, where = IW.edge_case(N)
    exp, _, _, _ = W.expect(oracle, ref, rows, IW.edge_Ls(n))
    bounds, _ = LSW.row_bounds(n, rows)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    xs_pad = LSW.ld_ref(ref, n)
    for L in IW.edge_Ls(n):
        lag, mv = db.scores_in_window(L)
        assert _masked(muse, db)
        r, planted = where[L]
        for row, pl in zip(r, planted):
            if abs(int(pl)) <= L:
                assert lag[row] == pl, (N, L, row, lag[row], pl)
                want = LSW.ld_score_at(ref, rows[row], n, int(pl) % n, xs_pad)
                assert abs(np.longdouble(mv[row]) - want) <= bounds[row], (N, L, row, mv[row], float(want), bounds[row])
            else:
                assert abs(int(lag[row])) <= L, (N, L, row, lag[row], pl)
        check(lag, mv, *exp[L], tag="edges N=%d L=%d" % (N, L))
        assert not exp[L][2].any()
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. identities
def test_identities(muse, eng, oracle):
    N = 1024
    ref, rows = W.make_case(N, 101, seed=9)
    n = LSW.fft_len(N)
    for f32 in (False, True):
        dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
        plain = muse.DeviceBatch(eng, dg, ref)
        plag, pmv = plain.scores()
        db = muse.DeviceBatch(eng, dg, ref)
        for L in (n // 2, n // 2 + 1, 10 * n):                      # the window is every lag: the plain pass, bit for bit
            lag, mv = db.scores_in_window(L)
            assert db.last_in_window_path() == muse.binding.MUSE_IN_WINDOW_PLAIN
            assert lag.tobytes() == plag.tobytes() and mv.tobytes() == pmv.tobytes(), (f32, L)
        db.close()
        plain.close()
        dg.close()
    for N in (1024, 4096):
        ref, rows = W.make_case(N, 101, seed=9 + N)
        dg = muse.DeviceGroup.from_rows(eng, rows)
        own = muse.DeviceBatch(eng, dg, ref)
        db = muse.DeviceBatch(eng, dg, ref)
        for L in (0, 7, 63):
            own.set_lag_window(L)
            wlag, wmv = own.scores()
            lag, mv = db.scores_in_window(L)                         # up to the cap on float64 rows: the direct product, bit for bit
            assert db.last_in_window_path() == muse.binding.MUSE_IN_WINDOW_MFMA and db.lag_window() == -1
            assert lag.tobytes() == wlag.tobytes() and mv.tobytes() == wmv.tobytes(), (N, L)
            own_in = own.scores_in_window(L)                         # a batch whose own window equals the call's is accepted
            assert own_in[0].tobytes() == wlag.tobytes() and own.lag_window() == L
            eng.in_window_force_transform(True)                      # the same window through the masked transform kernels
            try:
                flag, fmv = db.scores_in_window(L)
                assert _masked(muse, db)
            finally:
                eng.in_window_force_transform(False)
            assert np.array_equal(flag, wlag), (N, L, np.nonzero(flag != wlag)[0][:8])
            ok = ~np.isnan(wmv)
            assert np.array_equal(np.isnan(fmv), ~ok)
            assert np.all(np.abs(fmv[ok] - wmv[ok]) <= SCORE_RTOL * np.abs(wmv[ok]) + SCORE_ATOL), (N, L)
        a = db.scores_in_window(100)
        b = db.scores_in_window(100)                                 # two masked passes in a row: bit-identical
        assert _masked(muse, db) and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        for h in (own, db, dg):
            h.close()


# ------------------------------------------------------------------ 4. the redo paths at n = 4096
def test_redo_paths_keep_the_window(muse, eng, oracle):
    """every second row scaled by 1e30: every pair's sigmas are too far apart for one shared transform, the default kernel lists
    them all (a dense list: the rescaling kernel redoes every pair), and the second pass goes to the rescaling kernel directly"""
    ref, rows = IW.redo_case()
    L = IW.REDO_L
    exp, glag, _, _ = W.expect(oracle, ref, rows, (L,))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores_in_window(L)
    assert _masked(muse, db)
    assert len(db.redo_pairs()) > 0
    check(lag, mv, *exp[L], tag="redo pass 1")
    assert np.all(np.abs(lag) <= L) and (np.abs(glag) > L).sum() > IW.REDO_M // 8
    lag2, mv2 = db.scores_in_window(L)
    assert _masked(muse, db)
    assert eng.kernel_name(db).startswith("xcorr_fused_n4096_occ4"), eng.kernel_name(db)
    check(lag2, mv2, *exp[L], tag="redo pass 2")
    assert lag2.tobytes() == lag.tobytes() and mv2.tobytes() == mv.tobytes()
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. float32 storage
@pytest.mark.parametrize("N", IW.F32_NS)
def test_float32_groups_get_a_window(muse, eng, oracle, N):
    ref, stored = IW.f32_case(N)
    n = LSW.fft_len(N)
    dg = muse.DeviceGroup.from_rows(eng, stored, f32=True)
    rows = dg.read(0, IW.F32_M)
    assert np.array_equal(rows, stored, equal_nan=True)                        # (the rounded rows the CPU test checked for ties)
    exp, _, _, _ = W.expect(oracle, ref, rows, IW.F32_LS)
    db = muse.DeviceBatch(eng, dg, ref)
    for L in IW.F32_LS:
        lag, mv = db.scores_in_window(L)
        want = muse.binding.MUSE_IN_WINDOW_PLAIN if L >= n // 2 else muse.binding.MUSE_IN_WINDOW_MASKED
        assert db.last_in_window_path() == want, (N, L)
        check(lag, mv, *exp[L], tag="f32 N=%d L=%d" % (N, L))
        assert np.all(np.abs(lag) <= L)
    # the old entry points still refuse the group
    for fn in (lambda: db.set_lag_window(7), lambda: db.slide_score_windowed(np.zeros((IW.F32_M, 1)), 7)):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == muse.binding.MUSE_ERR_UNSUPPORTED
    db.close()
    dg.close()


# ------------------------------------------------------------------ 6. the spectrum cache is not touched
def test_spectrum_cache_untouched(muse, eng, oracle):
    N, M, L = 4096, 64, 100
    ref, rows = W.make_case(N, M, seed=41)
    eng.spectrum_cache_limits(min_rows=16)
    try:
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        db.scores()
        before = db.scores()                                         # the second pass builds the cache
        cached = dg.spectrum_cache()
        assert cached[0] == M and cached[1] > 0
        assert eng.kernel_name(db).startswith("xcorr_cached_n4096")
        lag, mv = db.scores_in_window(L)
        assert _masked(muse, db)
        exp, _, _, _ = W.expect(oracle, ref, rows, (L,))
        check(lag, mv, *exp[L], tag="beside the cache")
        assert dg.spectrum_cache() == cached
        after = db.scores()
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        assert dg.spectrum_cache() == cached
        # a group scored in a window only never starts a cache: the masked pass does not count as a pass over the rows
        dg2 = muse.DeviceGroup.from_rows(eng, rows)
        db2 = muse.DeviceBatch(eng, dg2, ref)
        for _ in range(3):
            db2.scores_in_window(L)
        assert dg2.spectrum_cache() == (0, 0)
        db2.scores()
        assert dg2.spectrum_cache() == (0, 0)                        # (the first unwindowed pass: a group scored once pays nothing)
        for h in (db, db2, dg, dg2):
            h.close()
    finally:
        eng.spectrum_cache_limits()


# ------------------------------------------------------------------ 7. the Run form
def _assert_run(got, want):
    idx, lag, score = got[0], got[1], got[2]
    oi, ol, osc = want[0], want[1], want[2]
    assert lag.tolist() == ol.tolist()
    assert np.allclose(score, osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert idx.tolist() == oi.tolist()


def test_run_in_window_matches_the_selection_on_the_definition(muse, eng, oracle):
    """run_in_window ungrouped and grouped (G = 7) equals the oracle's Results.Update / Fetch (oracle.results: the selection every Run
    test of this suite is held to) fed with the definition's per-row pairs; Batch.RunInWindow of the Python mirror agrees"""
    N, M, G, L = IW.RUN_N, IW.RUN_M, IW.RUN_G, IW.RUN_L
    ref, rows = IW.run_case()
    exp, glag, gmv, n = W.expect(oracle, ref, rows, (L,))
    wlag, wmv, tie = exp[L]
    assert not (tie & W.plain_rows(M)).any()
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    gid = (np.arange(M) * 5 % G).astype(np.int32)
    for sign, thr in ((0, 0.0), (1, 0.0), (-1, 0.0), (0, 0.35)):
        got = db.run_in_window(L, None, 0, 20, thr, sign, True)
        assert _masked(muse, db) and db.last_run_path() == 0 and db.lag_window() == -1
        _assert_run(got, oracle.results(wlag, wmv, None, 0, True, L, 20, thr, sign))
        got = db.run_in_window(L, gid, G, 20, thr, sign, True)
        _assert_run(got, oracle.results(wlag, wmv, gid, G, True, L, 20, thr, sign))
        got = db.run_in_window(L, gid, G, 20, thr, sign, False)
        _assert_run(got, oracle.results(wlag, wmv, gid, G, False, L, 20, thr, sign))
    # the windowed Run keeps series today's Run drops
    today = oracle.results(glag, gmv, None, 0, True, L, M, 0.0, 0)
    now = oracle.results(wlag, wmv, None, 0, True, L, M, 0.0, 0)
    got = db.run_in_window(L, None, 0, M, 0.0, 0, True)
    assert len(got[0]) == len(now[0]) >= len(today[0]) and got[1].tolist() == now[1].tolist()
    with pytest.raises(muse.MuseError) as e:
        db.run_in_window(L, None, 0, 20, 0.0, 2, True)
    assert e.value.status == muse.binding.MUSE_ERR_INVALID
    db.close()
    dg.close()
    # the label-level mirror
    hosts = 6
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
    b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"graph": "ref"})), comp, res, 8, engine=eng)
    with pytest.raises(muse.MuseError) as e:                          # RunWindowed keeps its cap
        b.RunWindowed(None)
    assert e.value.status == muse.binding.MUSE_ERR_UNSUPPORTED
    for by, g, Gn in ((None, None, 0), (["graph"], (np.arange(M) // hosts).astype(np.int32), M // hosts)):
        b.RunInWindow(by)
        got, mean = res.Fetch()
        oi, ol, osc, omean = oracle.results(wlag, wmv, g, Gn, True, L, 12, 0.0, 0)
        assert len(got) == len(oi) > 0
        assert [s.Lag for s in got] == ol.tolist()
        assert np.allclose([s.PercentScore for s in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
        assert [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
        assert abs(mean - omean) < 1e-9
    b.Run(None)                                                       # Run is the Run it was
    got, _ = res.Fetch()
    oi, ol, osc, _ = oracle.results(glag, gmv, None, 0, True, L, 12, 0.0, 0)
    assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()


def _lcg_series(N, i):
    """host/muse_in_window_test.cpp's series() (host/muse_window_test.cpp's), bit for bit (32-bit LCG, exact arithmetic)"""
    s = (12345 + 977 * i) & 0xFFFFFFFF

    def lcg():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        return s
    shift = 0 if i < 0 else (0 if i % 3 == 0 else int(lcg() % 241) - 120)
    amp = 1.0 + 2.0 * (((lcg() >> 8) / 16777216.0 - 0.5) + 0.5)
    y = np.zeros(N)
    for t in range(N):
        u = t - shift
        y[t] = (amp if N // 2 - 12 <= u < N // 2 + 12 else 0.0) + 0.5 * ((lcg() >> 8) / 16777216.0 - 0.5)
    return y


def test_cpp_batch_run_in_window(muse, oracle):
    """Batch::RunInWindow of the C++ host mirror (host/muse_in_window_test.cpp) Fetches what the oracle gives"""
    exe = muse.build.build_in_window_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "in-window ok" in r.stdout, r.stdout + r.stderr
    N, M, L = 1000, 240, 100
    ref = _lcg_series(N, -1)
    rows = np.stack([_lcg_series(N, i) for i in range(M)])
    exp, glag, gmv, n = W.expect(oracle, ref, rows, (L,))
    wlag, wmv, tie = exp[L]
    assert not tie.any()
    for case, gid, G in (("nil", None, 0), ("graph", (np.arange(M) // 6).astype(np.int32), M // 6)):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(case + " ")]
        oi, ol, osc, _ = oracle.results(wlag, wmv, gid, G, True, L, 12, 0.0, 0)
        assert len(lines) == len(oi) == 12
        assert [int(l[1]) for l in lines] == oi.tolist()
        assert [int(l[2]) for l in lines] == ol.tolist()
        assert np.allclose([float(l[3]) for l in lines], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_everything_as_it_was(muse, eng):
    B = muse.binding
    rng = np.random.default_rng(8)

    def setup(N, M=6, f32=False):
        ref = rng.standard_normal(N)
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        db = muse.DeviceBatch(eng, dg, ref)
        return dg, db, db.scores()

    def refused(db, base, fn, status, window=-1):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message, e.value
        now = db.read_scores()
        assert now[0].tobytes() == base[0].tobytes() and now[1].tobytes() == base[1].tobytes()
        assert db.lag_window() == window

    dg, db, base = setup(1024)
    refused(db, base, lambda: db.score_in_window(-1), B.MUSE_ERR_INVALID)
    refused(db, base, lambda: db.run_in_window(-1), B.MUSE_ERR_INVALID)
    db.set_lag_window(7)
    base7 = db.scores()
    refused(db, base7, lambda: db.score_in_window(100), B.MUSE_ERR_INVALID, window=7)
    refused(db, base7, lambda: db.run_in_window(100), B.MUSE_ERR_INVALID, window=7)
    for N in (5000, 70000, 200):
        dg, db, base = setup(N, M=3)
        refused(db, base, lambda: db.score_in_window(100), B.MUSE_ERR_UNSUPPORTED)
        refused(db, base, lambda: db.run_in_window(100), B.MUSE_ERR_UNSUPPORTED)
        assert db.last_in_window_path() == 0
    dg, db, base = setup(5000, f32=True)
    refused(db, base, lambda: db.score_in_window(7), B.MUSE_ERR_UNSUPPORTED)
    # a kernel forced by a test hook that has no masked build: refused, not run unmasked
    dg, db, base = setup(1024)
    eng.set_kernel(11)
    try:
        with pytest.raises(muse.MuseError) as e:
            db.score_in_window(100)
        assert e.value.status == B.MUSE_ERR_UNSUPPORTED
    finally:
        eng.set_kernel(0)
    lag, mv = db.scores_in_window(100)
    assert _masked(muse, db) and np.all(np.abs(lag) <= 100)


# ------------------------------------------------------------------ 9. scale
def test_full_size_1m_x_4096_window_200(muse, eng, oracle):
    """1 M x 4096 with L = 200: sampled rows against the oracle, as the full-size test of the direct product samples them"""
    M, N, L = 1_000_000, 4096, 200
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores_in_window(L)
    assert _masked(muse, db)
    assert np.all(np.abs(lag) <= L) and np.all(np.abs(mv[~np.isnan(mv)]) <= 1.0 + 1e-9)
    rng = np.random.default_rng(1)
    starts = np.sort(rng.choice(M // 256, 16, replace=False)) * 256
    for s0 in starts:                                       # 16 x 256 = 4096 sampled rows
        rows = dg.read(int(s0), 256)
        exp, _, _, _ = W.expect(oracle, ref, rows, (L,))
        check(lag[s0:s0 + 256], mv[s0:s0 + 256], *exp[L], tag="scale rows %d.." % s0)
        assert int(exp[L][2].sum()) <= 1
    zero = mv == 0
    assert 500 < zero.sum() < 1500 and np.all(lag[zero] == 0)            # ~1/1024 constant rows
    ones = np.abs(mv - 1.0) < 1e-12
    assert 500 < ones.sum() < 1500 and np.all(lag[ones] == 0)            # ~1/1024 copies of ref
    db.close()
    dg.close()
