"""GPU tests of the one-sided / asymmetric lag window (muse_batch_score_in_lag_range / _run_in_lag_range, run with -m gpu on an
MI355X): the direct product over a table with an explicit origin (xcorr_window.hip, window_device.h) and the transform kernels'
masked argmax with two independent bounds, through the C ABI and its mirrors.

Expected values never come from the code under test: per series, the definition in include/muse_hip.h applied in numpy
(tests/_lagrange.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact except rows the ORACLE flags as
ties (two top |cc| inside the range within 1e-12 relative); tests/test_lag_range_cpu.py checks on the same inputs that the oracle
flags none on planted rows and no more than 1 in 1000 noise rows.  Planted winners are held to tests/_lagsweep.py's bound against
the long-double score at the planted index."""
import subprocess

import numpy as np
import pytest

import _lagrange as LR
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


def _inside(lag, n, lo, hi):
    lo, hi = LR.clip(n, lo, hi)
    return np.all((lag >= lo) & (lag <= hi))


# ------------------------------------------------------------------ 1. the direct product
@pytest.mark.parametrize("N", LR.MFMA_NS)
def test_direct_product_parity(muse, eng, oracle, N):
    """make_case rows with the eight specials; N = n (the range clipped at n / 2), an odd stride (narrow loads), two chunks with a
    short last one; ranges of 1 .. 127 rows: one row, one full tile, one row more than a tile, both sides, both asymmetric ways"""
    B = muse.binding
    ref, rows = LR.mfma_case(N)
    exp, glag, gmv, n = LR.expect(oracle, ref, rows, LR.MFMA_RANGES, Ls=(63,))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == n
    for lo, hi in LR.MFMA_RANGES:
        lag, mv = db.scores_in_lag_range(lo, hi)
        assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA, (N, lo, hi, db.last_in_window_path())
        assert db.lag_window() == -1 and db.last_run_path() == 0
        check(lag, mv, *exp[(lo, hi)], tag="direct N=%d [%d, %d]" % (N, lo, hi))
        assert _inside(lag, n, lo, hi), (N, lo, hi)
        clo, chi = LR.clip(n, lo, hi)
        assert eng.kernel_name(db).startswith("xcorr_window_mfma<%d, " % ((chi - clo + 1 + 15) // 16)), eng.kernel_name(db)
    # filtering the symmetric window's answer could not have produced these: some rows' winner inside +-63 lies on the other side
    keep = W.plain_rows(LR.PARITY_M)
    sym = exp[63][0]
    for lo, hi in ((-63, 0), (0, 63)):
        lost = keep & ((sym < lo) | (sym > hi))
        assert lost.sum() >= 2, (N, lo, hi, int(lost.sum()))
        assert np.any(exp[(lo, hi)][1][lost] != 0.0)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 2. the masked transform pass
@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", LR.MASKED_NS)
def test_masked_parity(muse, eng, oracle, N, f32):
    """ranges wider than 127 lags (float32 storage: narrow ones too) with their two bounds apart: inside a lane range, on a 256-index
    register block, one side empty, one side whole.  Float32 groups are checked against the rows as stored."""
    B = muse.binding
    ref, rows = LR.masked_case(N, f32)
    n = LSW.fft_len(N)
    ranges = LR.masked_ranges(n, f32)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    if f32:
        assert np.array_equal(dg.read(0, LR.PARITY_M), rows, equal_nan=True)
    exp, _, _, n2 = LR.expect(oracle, ref, rows, ranges)
    assert n2 == n
    db = muse.DeviceBatch(eng, dg, ref)
    masked = 0
    for lo, hi in ranges:
        lag, mv = db.scores_in_lag_range(lo, hi)
        assert db.lag_window() == -1 and db.last_run_path() == 0
        check(lag, mv, *exp[(lo, hi)], tag="masked N=%d f32=%d [%d, %d]" % (N, f32, lo, hi))
        assert _inside(lag, n, lo, hi), (N, lo, hi)
        if LR.clip(n, lo, hi) == (-(n // 2 - 1), n // 2):            # (n = 512: -255 .. 256 is every lag -- the plain pass)
            assert n == 512 and db.last_in_window_path() == B.MUSE_IN_WINDOW_PLAIN
            continue
        masked += 1
        assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, (N, f32, lo, hi, db.last_in_window_path())
        name = eng.kernel_name(db)
        assert name.endswith(", true>") and name.startswith("xcorr_fused_n4096_fold<" if n == 4096 else "xcorr_fused_small<"), name
        if n == 4096:
            assert len(db.redo_pairs()) > 0                          # the specials went through the rescaling kernel, window kept
    assert masked >= len(ranges) - 1
    db.scores()
    assert db.last_in_window_path() == 0 and eng.kernel_name(db) != name   # (the build without the mask again)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. edges from planted winners
@pytest.mark.parametrize("N,rng", LR.EDGE_CASES)
def test_edges_from_planted_winners(muse, eng, oracle, N, rng):
    """a code planted at the lags lo-1, lo, lo+1, -1, 0, 1, hi-1, hi, hi+1: inside the range it comes back there with the long-double
    score at that index; outside, the result lies inside the range and is the definition's on the oracle's cc"""
    B = muse.binding
    lo, hi = rng
    ref, rows, n, planted = LR.edge_case(N, lo, hi)
    exp, _, _, _ = LR.expect(oracle, ref, rows, (rng,))
    bounds, _ = LSW.row_bounds(n, rows)
    xs_pad = LSW.ld_ref(ref, n)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores_in_lag_range(lo, hi)
    assert db.last_in_window_path() == (B.MUSE_IN_WINDOW_MFMA if hi - lo + 1 <= 127 else B.MUSE_IN_WINDOW_MASKED)
    for row, pl in enumerate(planted):
        if lo <= int(pl) <= hi:
            assert lag[row] == pl, (N, rng, row, lag[row], pl)
            want = LSW.ld_score_at(ref, rows[row], n, int(pl) % n, xs_pad)
            assert abs(np.longdouble(mv[row]) - want) <= bounds[row], (N, rng, row, mv[row], float(want), bounds[row])
        else:
            assert lo <= int(lag[row]) <= hi, (N, rng, row, lag[row], pl)
    check(lag, mv, *exp[rng], tag="edges N=%d [%d, %d]" % (N, lo, hi))
    assert not exp[rng][2].any()
    db.close()
    dg.close()


# ------------------------------------------------------------------ 4. identities
@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", (1024, 3000))
def test_symmetric_range_is_the_window_bit_for_bit(muse, eng, N, f32):
    ref, rows = W.make_case(N, 35, seed=70 + N)
    n = LSW.fft_len(N)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    a, b = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dg, ref)
    for L in (0, 7, 63, 64, 200, n // 2 - 1, n // 2, 10 * n):
        wl, wm = a.scores_in_window(L)
        rl, rm = b.scores_in_lag_range(-L, L)
        assert a.last_in_window_path() == b.last_in_window_path() == muse.in_window_plan(N, f32, L)
        assert rl.tobytes() == wl.tobytes() and rm.tobytes() == wm.tobytes(), (N, f32, L)
    for h in (a, b, dg):
        h.close()


def test_rows_won_inside_the_range_keep_their_bits(muse, eng):
    """a row whose best match inside +-max(-lo, hi) lies inside lo .. hi has that match in the range too: the same lag and -- each lag
    row of the product being its own dot product in the same order, the mask a select -- the same bits, MFMA against MFMA and
    MASKED against MASKED.  Two calls give the same bytes; afterwards the batch is the batch it was."""
    B = muse.binding
    N = 1024
    ref, rows = W.make_case(N, 101, seed=9)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db, sym = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dg, ref)
    plain = sym.scores()
    for lo, hi in ((-7, 0), (0, 7), (-63, 0), (0, 63), (-40, 3), (-3, 40), (-200, 0), (0, 200), (-64, 300), (-300, 64)):
        L = max(-lo, hi)
        wl, wm = sym.scores_in_window(L)
        rl, rm = db.scores_in_lag_range(lo, hi)
        assert db.last_in_window_path() == sym.last_in_window_path() == (B.MUSE_IN_WINDOW_MFMA if L <= 63 else B.MUSE_IN_WINDOW_MASKED)
        same = (wl >= lo) & (wl <= hi)
        assert same.sum() >= 30 and (~same).sum() >= 5, (lo, hi, int(same.sum()))
        assert np.array_equal(rl[same], wl[same]) and rm[same].tobytes() == wm[same].tobytes(), (lo, hi)
        again = db.scores_in_lag_range(lo, hi)
        assert again[0].tobytes() == rl.tobytes() and again[1].tobytes() == rm.tobytes()
    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
    now = db.scores()
    assert now[0].tobytes() == plain[0].tobytes() and now[1].tobytes() == plain[1].tobytes()
    assert db.last_in_window_path() == 0 and db.lag_window() == -1
    # the cached tables are keyed: a symmetric window behind a range, and the other way round, on ONE batch
    a = db.scores_in_window(7)
    r = db.scores_in_lag_range(-7, 0)
    b = db.scores_in_window(7)
    r2 = db.scores_in_lag_range(-7, 0)
    s = sym.scores_in_window(7)
    assert a[1].tobytes() == b[1].tobytes() == s[1].tobytes() and a[0].tobytes() == b[0].tobytes() == s[0].tobytes()
    assert r[1].tobytes() == r2[1].tobytes() and r[0].tobytes() == r2[0].tobytes()
    db.set_lag_window(7)                                             # an own window equal to a symmetric range is accepted, and kept
    own = db.scores_in_lag_range(-7, 7)
    assert own[1].tobytes() == a[1].tobytes() and db.lag_window() == 7
    for h in (db, sym, dg):
        h.close()


def test_one_window_type_own_window_at_half_the_length_and_every_table_shape(muse, eng, oracle):
    """the window +-L and the lag range are one description (origin, rows) of a table, cached under one key.
    (a) a batch's own window at L = n / 2 keeps the symmetric form's table: origin 32, 31 lags below zero, 65 rows in five tiles
    (N = n = 64, M = 33: two full 16-row tiles and one row; seed chosen on the CPU: the oracle flags no tie, row 32 wins at lag +32 and
    row 11 at lag -31, the two ends of the scan).
    (b) one batch walks every table shape in turn; after every step its bytes are a fresh batch's for the same call."""
    B = muse.binding
    # (a)
    ref, rows = W.make_case(64, 33, seed=6478)
    exp, _, _, n = LR.expect(oracle, ref, rows, (), Ls=(32,))
    assert n == 64 and not exp[32][2].any() and exp[32][0][32] == 32 and exp[32][0][11] == -31
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    db.set_lag_window(63)
    lag, mv = db.scores()
    check(lag, mv, *exp[32], tag="own window 63 at n = 64")
    assert db.lag_window() == 63 and db.last_in_window_path() == 0
    assert eng.kernel_name(db).startswith("xcorr_window_mfma<5, "), eng.kernel_name(db)
    db.close()
    dg.close()
    # (b)
    ref, rows = W.make_case(1024, 33, seed=6478)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    win = lambda L: (lambda b: b.scores_in_window(L))
    rng = lambda lo, hi: (lambda b: b.scores_in_lag_range(lo, hi))
    own7 = lambda b: (b.set_lag_window(7), b.scores())[1]
    off = lambda b: (b.set_lag_window(-1), b.scores_in_lag_range(-3, 40))[1]
    steps = (("window 7", win(7), -1, B.MUSE_IN_WINDOW_MFMA), ("range -7 .. 0", rng(-7, 0), -1, B.MUSE_IN_WINDOW_MFMA),
             ("range 0 .. 7", rng(0, 7), -1, B.MUSE_IN_WINDOW_MFMA), ("range -7 .. 7", rng(-7, 7), -1, B.MUSE_IN_WINDOW_MFMA),
             ("window 7 again", win(7), -1, B.MUSE_IN_WINDOW_MFMA), ("own window 7", own7, 7, 0),
             ("range -7 .. 7 under the own window", rng(-7, 7), 7, B.MUSE_IN_WINDOW_MFMA),
             ("window off, range -3 .. 40", off, -1, B.MUSE_IN_WINDOW_MFMA), ("window 40", win(40), -1, B.MUSE_IN_WINDOW_MFMA))
    for tag, call, own, path in steps:
        got = call(db)
        fresh = muse.DeviceBatch(eng, dg, ref)
        want = call(fresh)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), tag
        assert db.lag_window() == own, (tag, db.lag_window())                # (what was last set: no call touches it)
        assert db.last_in_window_path() == fresh.last_in_window_path() == path, (tag, db.last_in_window_path())
        assert eng.kernel_name(db) == eng.kernel_name(fresh), tag
        fresh.close()
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_everything_as_it_was(muse, eng):
    B = muse.binding
    rng = np.random.default_rng(8)

    def setup(N, M=6, f32=False):
        ref = rng.standard_normal(N)
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        db = muse.DeviceBatch(eng, dg, ref)
        return dg, db, db.scores()

    def refused(db, base, fn, status, window=-1, path=0):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message, e.value
        now = db.read_scores()
        assert now[0].tobytes() == base[0].tobytes() and now[1].tobytes() == base[1].tobytes()
        assert db.lag_window() == window and db.last_in_window_path() == path

    L = B.load()
    assert L.muse_batch_score_in_lag_range(None, -7, 0) == B.MUSE_ERR_INVALID
    assert L.muse_batch_run_in_lag_range(None, None, 0, -7, 0, 5, 0.0, 0, 1, None, None, None, None, None) == B.MUSE_ERR_INVALID
    dg, db, base = setup(1024)
    base = db.scores_in_lag_range(-300, 20)                          # (an origin other than the default to leave alone)
    P = B.MUSE_IN_WINDOW_MASKED
    for lo, hi in ((1, 7), (-7, -1), (1, 0), (0, -1)):
        refused(db, base, lambda: db.score_in_lag_range(lo, hi), B.MUSE_ERR_INVALID, path=P)
        refused(db, base, lambda: db.run_in_lag_range(lo, hi), B.MUSE_ERR_INVALID, path=P)
    refused(db, base, lambda: db.run_in_lag_range(-7, 0, sign_filter=2), B.MUSE_ERR_INVALID, path=P)
    refused(db, base, lambda: db.run_in_lag_range(-7, 0, group_id=np.zeros(6, dtype=np.int32), G=-1), B.MUSE_ERR_INVALID, path=P)
    db.set_lag_window(7)
    base7 = db.scores()
    for lo, hi in ((-7, 0), (0, 7), (-5, 5), (-200, 7)):
        refused(db, base7, lambda: db.score_in_lag_range(lo, hi), B.MUSE_ERR_INVALID, window=7)
        refused(db, base7, lambda: db.run_in_lag_range(lo, hi), B.MUSE_ERR_INVALID, window=7)
    for N, f32, (lo, hi) in ((5000, False, (-200, 0)), (5000, True, (-7, 0)), (200, False, (-100, 60)), (70000, False, (0, 7))):
        dg, db, base = setup(N, M=3, f32=f32)
        refused(db, base, lambda: db.score_in_lag_range(lo, hi), B.MUSE_ERR_UNSUPPORTED)
        refused(db, base, lambda: db.run_in_lag_range(lo, hi), B.MUSE_ERR_UNSUPPORTED)
    # a kernel forced by a test hook that has no masked build: refused, not run unmasked
    dg, db, base = setup(1024)
    eng.set_kernel(11)
    try:
        refused(db, base, lambda: db.score_in_lag_range(-200, 0), B.MUSE_ERR_UNSUPPORTED)
    finally:
        eng.set_kernel(0)
    lag, mv = db.scores_in_lag_range(-200, 0)
    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED and np.all((lag >= -200) & (lag <= 0))


# ------------------------------------------------------------------ 6. the Run forms
def _assert_run(got, want):
    idx, lag, score = got[0], got[1], got[2]
    oi, ol, osc = want[0], want[1], want[2]
    assert lag.tolist() == ol.tolist()
    assert np.allclose(score, osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert idx.tolist() == oi.tolist()
    assert abs(got[3] - want[3]) < 1e-9 or (np.isnan(got[3]) and np.isnan(want[3]))    # (an empty selection has no mean)


@pytest.mark.parametrize("N", LR.RUN_NS)
def test_run_in_lag_range_matches_the_selection_on_the_definition(muse, eng, oracle, N):
    """run_in_lag_range ungrouped and grouped by host equals the oracle's Results.Update / Fetch fed with the definition's per-row
    pairs (order, lags, scores, mean); Batch.RunInLagRange of the Python mirror agrees"""
    M, hosts = LR.RUN_M, 6
    ref, rows = LR.run_case(N)
    exp, glag, gmv, n = LR.expect(oracle, ref, rows, LR.RUN_RANGES)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    gid = (np.arange(M) % hosts).astype(np.int32)
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    for lo, hi in LR.RUN_RANGES:
        wlag, wmv, tie = exp[(lo, hi)]
        assert not (tie & W.plain_rows(M)).any()
        L = max(-lo, hi)
        for sign, thr in ((0, 0.0), (1, 0.0), (-1, 0.0), (0, 0.35)):
            got = db.run_in_lag_range(lo, hi, None, 0, 20, thr, sign, True)
            assert db.last_in_window_path() in (2, 3) and db.last_run_path() == 0 and db.lag_window() == -1
            _assert_run(got, oracle.results(wlag, wmv, None, 0, True, L, 20, thr, sign))
            got = db.run_in_lag_range(lo, hi, gid, hosts, 20, thr, sign, True)
            _assert_run(got, oracle.results(wlag, wmv, gid, hosts, True, L, 20, thr, sign))
            got = db.run_in_lag_range(lo, hi, gid, hosts, 20, thr, sign, False)
            _assert_run(got, oracle.results(wlag, wmv, gid, hosts, False, L, 20, thr, sign))
        res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
        b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"graph": "ref"})), comp, res, 8, engine=eng)
        for by, g, Gn in ((None, None, 0), (["host"], gid, hosts)):
            b.RunInLagRange(by, lo, hi)
            got, mean = res.Fetch()
            oi, ol, osc, omean = oracle.results(wlag, wmv, g, Gn, True, L, 12, 0.0, 0)
            assert len(got) == len(oi) > 0
            assert [s.Lag for s in got] == ol.tolist()
            assert np.allclose([s.PercentScore for s in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
            assert [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
            assert abs(mean - omean) < 1e-9
        b.Run(None)                                                   # Run is the Run it was
        got, _ = res.Fetch()
        oi, ol, osc, _ = oracle.results(glag, gmv, None, 0, True, L, 12, 0.0, 0)
        assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
    db.close()
    dg.close()


def test_cpp_batch_run_in_lag_range(muse, oracle):
    """Batch::RunInLagRange of the C++ host mirror (host/muse_lag_range_test.cpp), in a fresh process, Fetches what the oracle gives"""
    exe = muse.build.build_lag_range_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lag-range ok" in r.stdout, r.stdout + r.stderr
    ref, rows = LR.cpp_case()
    M = LR.CPP_M
    exp, _, _, _ = LR.expect(oracle, ref, rows, LR.CPP_RANGES)
    for lo, hi in LR.CPP_RANGES:
        wlag, wmv, tie = exp[(lo, hi)]
        assert not tie.any()
        for case, gid, G in (("nil", None, 0), ("graph", (np.arange(M) // 6).astype(np.int32), M // 6)):
            key = "%s[%d,%d] " % (case, lo, hi)
            lines = [l.split() for l in r.stdout.splitlines() if l.startswith(key)]
            oi, ol, osc, _ = oracle.results(wlag, wmv, gid, G, True, 300, 12, 0.0, 0)
            assert len(lines) == len(oi) == 12
            assert [int(l[1]) for l in lines] == oi.tolist()
            assert [int(l[2]) for l in lines] == ol.tolist()
            assert np.allclose([float(l[3]) for l in lines], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)


# ------------------------------------------------------------------ 7. many workgroups
def test_many_workgroups(muse, eng, oracle):
    """20 000 x 480 synthetic rows (1250 workgroups of the direct product): 64 sampled rows against the oracle on both paths"""
    B = muse.binding
    M, N = 20000, 480
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    ranges = ((-31, 0), (0, 200))
    got = {}
    for (lo, hi), path in zip(ranges, (B.MUSE_IN_WINDOW_MFMA, B.MUSE_IN_WINDOW_MASKED)):
        got[(lo, hi)] = db.scores_in_lag_range(lo, hi)
        assert db.last_in_window_path() == path
        lag, mv = got[(lo, hi)]
        assert np.all((lag >= lo) & (lag <= hi)) and np.all(np.abs(mv[~np.isnan(mv)]) <= 1.0 + 1e-9)
    starts = np.sort(np.random.default_rng(1).choice(M // 16, 4, replace=False)) * 16
    starts[-1] = M - 16                                              # (the last workgroup)
    for s0 in starts:                                                # 4 x 16 = 64 sampled rows
        rows = dg.read(int(s0), 16)
        exp, _, _, _ = LR.expect(oracle, ref, rows, ranges)
        for k in ranges:
            check(got[k][0][s0:s0 + 16], got[k][1][s0:s0 + 16], *exp[k], tag="rows %d.. [%d, %d]" % (s0, k[0], k[1]))
            assert int(exp[k][2].sum()) == 0
    db.close()
    dg.close()
