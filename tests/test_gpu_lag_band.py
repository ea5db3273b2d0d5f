"""GPU tests of the lag bands (muse_batch_score_in_lag_band / _run_in_lag_band, run with -m gpu on an MI355X): the direct product
over a table of the band's own rows (xcorr_window_band_mfma, window_device.h) and the transform kernels with the argmax masked to the
one index interval (the _band kernels of xcorr_r16_fold.hip, xcorr_r16_occ4.hip, xcorr_small.hip), through the C ABI and its mirrors.

Expected values never come from the code under test: per series, the definition in include/muse_hip.h applied in numpy
(tests/_lagband.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact on EVERY row:
tests/test_lag_band_cpu.py checks on the same inputs that the oracle flags no tie.

One exception, stated where it is made (test_outcomes_zero_band...): a band of exact zeros comes out as exactly (0, +0.0) from the
direct product, whose sums over zeros are zeros; a transform returns rounding noise of the order 1e-17 there, so on the masked path
the row is held to the score tolerance against the definition's +0.0 and its lag to the band, and the exact "nothing wins" outcome
of that path is shown by the signed passes over a band that holds no value of the sign."""
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _lagsweep as LSW
import _signed as SG
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


def check(lag, mv, exp, n, band, sign, tag):
    """scores to tolerance, NaN pattern equal, lags exact on every row (the oracle flags no tie); every lag inside the clipped band or
    0, every value of the sign, and where the definition finds nothing exactly (lag 0, +0.0).  Returns the rows with nothing."""
    elag, emv, tie = exp
    assert not tie.any(), tag
    lag, mv = np.asarray(lag), np.asarray(mv)
    nan_e = np.isnan(emv)
    assert np.array_equal(np.isnan(mv), nan_e), "%s NaN pattern: %s vs %s" % (tag, np.nonzero(np.isnan(mv))[0][:8], np.nonzero(nan_e)[0][:8])
    ok = ~nan_e
    err = np.abs(mv[ok] - emv[ok])
    nz = np.abs(emv[ok]) > 0
    worst = float((err[nz] / np.abs(emv[ok][nz])).max()) if nz.any() else 0.0
    print("%s: worst score rel err %.3e" % (tag, worst))
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "%s score mismatch: worst rel %.3e" % (tag, worst)
    bad = lag != elag
    assert not bad.any(), "%s lag mismatches at rows %s: %s vs %s" % (tag, np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    clo, chi = LB.clip(n, *band)
    assert np.all(((lag >= clo) & (lag <= chi)) | (lag == 0)), tag
    if sign:
        assert np.all(sign * mv[ok] >= 0), (tag, mv[ok][sign * mv[ok] < 0][:5])
    none = ok & (emv == 0.0)
    assert np.all(lag[none] == 0) and np.all(mv[none] == 0.0) and not np.signbit(mv[none]).any(), tag
    return int(none.sum())


def snapshot(eng, db):
    lag, mv = db.read_scores()
    return lag.tobytes(), mv.tobytes(), db.last_run_path(), db.last_in_window_path(), eng.kernel_name(db), db.lag_window()


def refused(muse, eng, db, fn, status):
    before = snapshot(eng, db)
    with pytest.raises(muse.MuseError) as e:
        fn()
    assert e.value.status == status and e.value.message, e.value
    assert snapshot(eng, db) == before


# ------------------------------------------------------------------ 1. the direct product
def _direct(muse, eng, oracle, N, M):
    B = muse.binding
    ref, rows = LB.mfma_case(N, M)
    exp, n = LB.expect(oracle, ref, rows, LB.MFMA_BANDS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == n
    db.scores()
    none = 0
    for lo, hi in LB.MFMA_BANDS:
        c = LB.clip(n, lo, hi)
        for s in LB.SIGNS:
            if c is None:                                            # (the far bands at n = 64 and 128)
                refused(muse, eng, db, lambda: db.score_in_lag_band(lo, hi, s), B.MUSE_ERR_INVALID)
                continue
            lag, mv = db.scores_in_lag_band(lo, hi, s)
            assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA == muse.lag_band_plan(N, False, lo, hi, s), (N, lo, hi, s)
            assert db.lag_window() == -1 and db.last_run_path() == 0
            none += check(lag, mv, exp[(lo, hi, s)], n, (lo, hi), s, "direct N=%d M=%d [%d, %d] sign %+d" % (N, M, lo, hi, s))
            name = eng.kernel_name(db)
            assert name.startswith("xcorr_window_band_mfma<%d, " % ((c[1] - c[0] + 1 + 15) // 16)) and name.endswith(", %d>" % s), name
    db.close()
    dg.close()
    return none, n


@pytest.mark.parametrize("N", LB.MFMA_NS)
def test_direct_product_band_scan(muse, eng, oracle, N):
    none, n = _direct(muse, eng, oracle, N, LB.PARITY_M)
    assert none >= 4                                                 # (the constant row, and rows with no value of the sign)
    if n <= 128:
        assert all(LB.clip(n, *b) is None for b in LB.FAR_BANDS)


@pytest.mark.parametrize("M", LB.SMALL_MS)
def test_direct_product_row_counts(muse, eng, oracle, M):
    _direct(muse, eng, oracle, LB.SMALL_M_N, M)


# ------------------------------------------------------------------ 2. the masked transform pass
def _masked_name(n, s):
    return ("xcorr_fused_n4096_fold_band<" if n == 4096 else "xcorr_fused_small_band<%d, " % (n.bit_length() - 1)), ", %d>" % s


@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", LB.MASKED_NS)
def test_masked_pass_interval_mask(muse, eng, oracle, N, f32):
    """bands that straddle the per-register index step (256 at n = 4096, n / 16 below), the whole positive and the whole negative
    side, single indices; float32 groups are checked against the rows as stored.  Narrow float64 bands take the direct product (the
    plan decides; checked against it) and run again on the masked pass under muse_test_in_window_force_transform."""
    B = muse.binding
    ref, rows = LB.masked_case(N, f32)
    n = LSW.fft_len(N)
    bands = LB.masked_bands(n) + list(LB.MASKED_FORCED)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    if f32:
        assert np.array_equal(dg.read(0, LB.PARITY_M), rows, equal_nan=True)
    exp, n2 = LB.expect(oracle, ref, rows, bands)
    assert n2 == n
    db = muse.DeviceBatch(eng, dg, ref)
    db.scores()
    masked = 0
    for force in (False, True):
        eng.in_window_force_transform(force)
        try:
            for lo, hi in bands:
                c = LB.clip(n, lo, hi)
                for s in LB.SIGNS:
                    if c is None:                                    # ((257, 510) and (-512, -257) at n = 512)
                        refused(muse, eng, db, lambda: db.score_in_lag_band(lo, hi, s), B.MUSE_ERR_INVALID)
                        continue
                    plan = muse.lag_band_plan(N, f32, lo, hi, s)
                    if force and plan != B.MUSE_IN_WINDOW_MFMA:
                        continue                                     # (ran on the masked pass in the first round)
                    lag, mv = db.scores_in_lag_band(lo, hi, s)
                    path = db.last_in_window_path()
                    assert path == (B.MUSE_IN_WINDOW_MASKED if force else plan), (N, f32, lo, hi, s, path)
                    assert db.lag_window() == -1 and db.last_run_path() == 0
                    check(lag, mv, exp[(lo, hi, s)], n, (lo, hi), s, "masked N=%d f32=%d force=%d [%d, %d] sign %+d" % (N, f32, force, lo, hi, s))
                    if path == B.MUSE_IN_WINDOW_MASKED:
                        masked += 1
                        name = eng.kernel_name(db)
                        head, tail = _masked_name(n, s)
                        assert name.startswith(head) and name.endswith(tail), name
                        if n == 4096:
                            assert len(db.redo_pairs()) > 0          # the specials went through the rescaling kernel, band and sign kept
        finally:
            eng.in_window_force_transform(False)
    assert masked >= 3 * 8
    db.scores()
    assert db.last_in_window_path() == 0 and "band" not in eng.kernel_name(db)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. handed-over pairs and forced kernels at n = 4096
def test_masked_pass_handed_over_pairs_keep_the_band(muse, eng, oracle):
    """mixed units (sigmas far apart in most pairs): the default n = 4096 kernel lists those pairs and the rescaling kernel behind it
    redoes them -- a dense list: every pair -- in its band build, band and sign kept; both variants forced by the test hook run their
    band builds; a forced variant without one is refused, not run unmasked"""
    B = muse.binding
    N, M = 4096, 63
    ref, rows = SG.make_case(N, M, seed=15000)
    rows[9::2] *= 1e9                                                # every second plain row in other units
    bands = ((100, 300), (-300, -100))
    exp, n = LB.expect(oracle, ref, rows, bands)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for lo, hi in bands:
        for s in LB.SIGNS:
            for k in range(2):
                lag, mv = db.scores_in_lag_band(lo, hi, s)
                assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
                check(lag, mv, exp[(lo, hi, s)], n, (lo, hi), s, "hand-off pass %d [%d, %d] sign %+d" % (k, lo, hi, s))
                assert len(db.redo_pairs()) > 0
    for variant, kname in ((10, "xcorr_fused_n4096_fold_band<"), (7, "xcorr_fused_n4096_occ4_band<")):
        eng.set_kernel(variant)
        try:
            for lo, hi in bands:
                for s in LB.SIGNS:
                    lag, mv = db.scores_in_lag_band(lo, hi, s)
                    assert eng.kernel_name(db).startswith(kname) and eng.kernel_name(db).endswith(", %d>" % s), eng.kernel_name(db)
                    check(lag, mv, exp[(lo, hi, s)], n, (lo, hi), s, "forced %d [%d, %d] sign %+d" % (variant, lo, hi, s))
        finally:
            eng.set_kernel(0)
    db.scores()
    for variant in (1, 11):                                          # the generic and the Stockham kernels have no band build
        eng.set_kernel(variant)
        try:
            refused(muse, eng, db, lambda: db.score_in_lag_band(100, 300, 1), B.MUSE_ERR_UNSUPPORTED)
        finally:
            eng.set_kernel(0)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 4. edges from planted winners
# every case on the path the plan gives; the narrow bands (the direct product) on the masked path as well
EDGE_PARAMS = [(N, band, False) for N, band in LB.EDGE_CASES] + [(N, band, True) for N, band in LB.EDGE_CASES if band[1] - band[0] + 1 <= 127]


@pytest.mark.parametrize("N,band,force", EDGE_PARAMS)
def test_edges_from_planted_winners(muse, eng, oracle, N, band, force):
    """a code planted at the lags lo-1, lo, lo+1, hi-1, hi, hi+1, -1, 0, 1: planted inside the band it comes back at sign 0 with the
    long-double score at that index; planted at lag 0, lo-1 or hi+1 the row reports the definition's in-band answer, never the
    planted lag.  On the path the plan gives and, for the narrow bands, on the masked path as well."""
    B = muse.binding
    lo, hi = band
    plan = muse.lag_band_plan(N, False, lo, hi, 0)
    assert plan == (B.MUSE_IN_WINDOW_MFMA if hi - lo + 1 <= 127 else B.MUSE_IN_WINDOW_MASKED)
    ref, rows, n, planted = LB.edge_case(N, lo, hi)
    exp, _ = LB.expect(oracle, ref, rows, (band,))
    bounds, _ = LSW.row_bounds(n, rows)
    xs_pad = LSW.ld_ref(ref, n)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    eng.in_window_force_transform(force)
    try:
        for s in LB.SIGNS:
            lag, mv = db.scores_in_lag_band(lo, hi, s)
            assert db.last_in_window_path() == (B.MUSE_IN_WINDOW_MASKED if force else plan)
            check(lag, mv, exp[(lo, hi, s)], n, band, s, "edges N=%d [%d, %d] force=%d sign %+d" % (N, lo, hi, force, s))
            found = 0
            for row, pl in enumerate(planted):
                if lo <= int(pl) <= hi and s == 0:
                    assert lag[row] == pl, (N, band, row, lag[row], pl, mv[row])
                    want = LSW.ld_score_at(ref, rows[row], n, int(pl) % n, xs_pad)
                    assert abs(np.longdouble(mv[row]) - want) <= bounds[row], (N, band, row, mv[row], float(want), bounds[row])
                    found += 1
                elif not lo <= int(pl) <= hi:
                    assert lag[row] == 0 or lo <= int(lag[row]) <= hi, (N, band, s, row, lag[row], pl)
                    assert lag[row] != pl or (pl == 0 and mv[row] == 0.0), (N, band, s, row, lag[row], pl, mv[row])
            assert s != 0 or found == 4
    finally:
        eng.in_window_force_transform(False)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. bit identities
def _bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", (1024, 3000))
def test_bit_identities(muse, eng, oracle, N, f32):
    """a band that holds lag 0 IS scores_signed_in_lag_range, in both call orders on one batch and with band calls in between (the
    tables of the two forms do not leak into each other); on the direct product a row whose [0, hi] / [lo, 0] winner lies inside
    the band carries that call's mv bits and lag; two band calls give the same bytes; a band pass leaves nothing behind"""
    B = muse.binding
    ref, rows = LB.masked_case(N, f32)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    db, un = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dg, ref)
    plain = un.scores()
    for lo, hi in ((0, 7), (-7, 0), (-40, 3), (-200, 0), (-64, 300), (-7, 7)):
        for s in LB.SIGNS:
            want = un.scores_signed_in_lag_range(lo, hi, s)
            db.scores_in_lag_band(1, 8 - lo, s)                      # (a band table of the same row count in front)
            a = db.scores_in_lag_band(lo, hi, s)
            assert _bits(a, want) and db.last_in_window_path() == un.last_in_window_path() and eng.kernel_name(db) == eng.kernel_name(un), (N, f32, lo, hi, s)
            b = db.scores_signed_in_lag_range(lo, hi, s)
            assert _bits(b, want)
            db.scores_in_lag_band(lo - 9, -1, s)
            assert _bits(db.scores_signed_in_lag_range(lo, hi, s), want) and _bits(db.scores_in_lag_band(lo, hi, s), want), (N, f32, lo, hi, s)
    kept = 0
    for (lo, hi), (rlo, rhi) in (((1, 63), (0, 63)), ((3, 40), (0, 40)), ((-63, -1), (-63, 0)), ((-40, -20), (-40, 0)), ((100, 126), (0, 126))):
        rng = un.scores_in_lag_range(rlo, rhi)
        direct = un.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA
        band = db.scores_in_lag_band(lo, hi, 0)
        again = db.scores_in_lag_band(lo, hi, 0)
        assert _bits(band, again), (N, f32, lo, hi)
        if direct and db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA:
            inside = (rng[0] >= lo) & (rng[0] <= hi) & ~np.isnan(rng[1]) & (rng[1] != 0.0)
            assert np.array_equal(band[0][inside], rng[0][inside]) and band[1][inside].tobytes() == rng[1][inside].tobytes(), (N, f32, lo, hi)
            kept += int(inside.sum())
        for s in (1, -1):
            assert _bits(db.scores_in_lag_band(lo, hi, s), db.scores_in_lag_band(lo, hi, s))
    assert f32 or kept >= 10
    assert _bits(db.scores(), plain) and db.last_in_window_path() == 0 and db.lag_window() == -1
    for h in (db, un, dg):
        h.close()


# ------------------------------------------------------------------ 6. outcomes
@pytest.mark.parametrize("force", (False, True))
def test_outcomes_zero_band_constant_nan_inf(muse, eng, oracle, force):
    """a band of exact zeros (tests/_rowslagrange.py's construction: the reference is zero wherever the row's two spikes reach) is
    (0, +0.0) for every sign on the direct product.  On the masked path the transform leaves rounding noise where the definition
    has zeros (this module's docstring): the row is held to the score tolerance against +0.0 and to a lag of the band or 0."""
    B = muse.binding
    ref, rows, zr = LB.zeros_case()
    exp, n = LB.expect(oracle, ref, rows, LB.ZEROS_BANDS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    eng.in_window_force_transform(force)
    try:
        for lo, hi in LB.ZEROS_BANDS:
            for s in LB.SIGNS:
                lag, mv = db.scores_in_lag_band(lo, hi, s)
                assert db.last_in_window_path() == (B.MUSE_IN_WINDOW_MASKED if force else B.MUSE_IN_WINDOW_MFMA)
                print("zeros force=%d [%d, %d] sign %+d: row %d -> (%d, %.3e)" % (force, lo, hi, s, zr, lag[zr], mv[zr]))
                if not force:
                    assert lag[zr] == 0 and mv[zr] == 0.0 and not np.signbit(mv[zr]), (lo, hi, s, lag[zr], mv[zr])
                else:
                    assert abs(mv[zr]) <= SCORE_ATOL and (lag[zr] == 0 or lo <= lag[zr] <= hi), (lo, hi, s, lag[zr], mv[zr])
                    assert s * mv[zr] >= 0
                others = np.arange(len(rows)) != zr
                e = exp[(lo, hi, s)]
                check(lag[others], mv[others], (e[0][others], e[1][others], e[2][others]), n, (lo, hi), s,
                      "zeros case force=%d [%d, %d] sign %+d" % (force, lo, hi, s))
    finally:
        eng.in_window_force_transform(False)
    db.close()
    dg.close()


@pytest.mark.parametrize("N", (1000, 4096))
def test_outcomes_specials_and_negation(muse, eng, oracle, N):
    """the constant row is (0, 0.0), the NaN and the Inf rows (0, NaN), on both paths and every sign; sign -1 on rows y against sign
    +1 on rows -y: the same lags, values equal and opposite; a band with no value of the sign is exactly (0, +0.0) on both paths"""
    ref, rows = LB.masked_case(N, False)
    n = LSW.fft_len(N)
    bands = ((3, 40), (-40, -3), (100, 300), (-300, -100))
    exp, _ = LB.expect(oracle, ref, rows, bands)
    dg, dn = muse.DeviceGroup.from_rows(eng, rows), muse.DeviceGroup.from_rows(eng, -rows)
    db, bn = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dn, ref)
    none = {2: 0, 3: 0}
    for lo, hi in bands:
        for s in LB.SIGNS:
            lag, mv = db.scores_in_lag_band(lo, hi, s)
            path = db.last_in_window_path()
            assert (lag[3], mv[3]) == (0, 0.0) and not np.signbit(mv[3])
            assert lag[4] == 0 and np.isnan(mv[4]) and lag[5] == 0 and np.isnan(mv[5])
            k = check(lag, mv, exp[(lo, hi, s)], n, (lo, hi), s, "specials N=%d [%d, %d] sign %+d" % (N, lo, hi, s))
            if s:
                none[path] += k - 1                                  # (beyond the constant row)
                b = bn.scores_in_lag_band(lo, hi, -s)
                assert bn.last_in_window_path() == path
                ok = ~np.isnan(mv)
                assert np.array_equal(lag, b[0]), (N, lo, hi, s)
                assert np.allclose(-b[1][ok], mv[ok], rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert none[2] > 0 and none[3] > 0, none
    for h in (db, bn, dg, dn):
        h.close()


# ------------------------------------------------------------------ 7. the Run form
def _same_selection(idx, lag, score, oi, ol, osc):
    """the selection in the oracle's order: the sort key |score| to tolerance position by position, every series with the oracle's
    lag and signed score, and a series at another position than the oracle's only among keys that agree within the tolerance.  (tests/_window.py's make_case holds
    the reference and its negated copy, rows 1 and 2: off lag 0 their magnitudes are equal and unclamped, so their order under
    abs_scores is decided by the last bit.)"""
    idx, lag, score, oi, ol, osc = (np.asarray(a) for a in (idx, lag, score, oi, ol, osc))
    assert len(idx) == len(oi)
    assert np.allclose(np.abs(score), np.abs(osc), rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert sorted(zip(idx.tolist(), lag.tolist())) == sorted(zip(oi.tolist(), ol.tolist()))
    where = {int(s): k for k, s in enumerate(oi.tolist())}
    for k, s in enumerate(idx.tolist()):
        j = where[int(s)]
        assert abs(score[k] - osc[j]) <= SCORE_RTOL * abs(osc[j]) + SCORE_ATOL, (k, j, s, score[k], osc[j])
        assert j == k or abs(abs(osc[j]) - abs(osc[k])) <= SCORE_RTOL * abs(osc[k]) + SCORE_ATOL, (k, j, s, osc[j], osc[k])


def _assert_run(got, want):
    _same_selection(got[0], got[1], got[2], want[0], want[1], want[2])
    assert abs(got[3] - want[3]) < 1e-9 or (np.isnan(got[3]) and np.isnan(want[3]))    # (an empty selection has no mean)


@pytest.mark.parametrize("N", LB.RUN_NS)
def test_run_in_lag_band_matches_the_selection_on_the_definition(muse, eng, oracle, N):
    """run_in_lag_band ungrouped and in label groups of 3 equals the oracle's group maximum, passed() and Fetch fed with the
    definition's per-series (lag, mv), MaxLag = max(|lo|, |hi|); Run(); Run() gives identical results; Batch.RunInLagBand and
    RunSignedInLagBand of the Python mirror agree"""
    M = LB.RUN_M
    ref, rows = LB.run_case(N)
    exp, n = LB.expect(oracle, ref, rows, LB.RUN_BANDS)
    gid, G = LB.run_groups()
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    labels = [{"trio": "t%02d" % (i // LB.RUN_GROUP), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    selected = 0
    for lo, hi in LB.RUN_BANDS:
        L = max(abs(lo), abs(hi))
        for s in LB.SIGNS:
            wlag, wmv, tie = exp[(lo, hi, s)]
            assert not tie.any()
            for ab in (True, False):
                for thr in (0.0, 0.35):
                    got = db.run_in_lag_band(lo, hi, None, 0, 20, thr, s, ab)
                    assert db.last_in_window_path() in (2, 3) and db.last_run_path() == 0 and db.lag_window() == -1
                    _assert_run(got, oracle.results(wlag, wmv, None, 0, ab, L, 20, thr, s))
                    again = db.run_in_lag_band(lo, hi, None, 0, 20, thr, s, ab)
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], again[:3]))
                    selected += len(got[0])
                    got = db.run_in_lag_band(lo, hi, gid, G, 20, thr, s, ab)
                    _assert_run(got, oracle.results(wlag, wmv, gid, G, ab, L, 20, thr, s))
        for signed, s, filt in ((False, 0, muse.SignFilter_ANY), (True, 0, muse.SignFilter_ANY), (True, 1, muse.SignFilter_POS),
                                (True, -1, muse.SignFilter_NEG)):
            res = muse.NewResults(L, 12, 0.0, filt)
            b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"trio": "ref"})), comp, res, 8, engine=eng)
            for by, g, Gn in ((None, None, 0), (["trio"], gid, G)):
                (b.RunSignedInLagBand if signed else b.RunInLagBand)(by, lo, hi)
                got, mean = res.Fetch()
                oi, ol, osc, omean = oracle.results(exp[(lo, hi, s)][0], exp[(lo, hi, s)][1], g, Gn, s == 0, L, 12, 0.0, s)
                _same_selection([int(sc.Labels.labels["i"]) for sc in got], [sc.Lag for sc in got], [sc.PercentScore for sc in got], oi, ol, osc)
                assert len(oi) == 0 or abs(mean - omean) < 1e-9
                selected += len(got)
    assert selected > 100
    db.close()
    dg.close()


def test_cpp_batch_run_in_lag_band(muse, oracle):
    """Batch::RunInLagBand and RunSignedInLagBand of the C++ host mirror (host/muse_lag_band_test.cpp), in a fresh process, Fetch
    what the oracle gives"""
    exe = muse.build.build_lag_band_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lag-band ok" in r.stdout, r.stdout + r.stderr
    ref, rows = LB.cpp_case()
    M = rows.shape[0]
    exp, _ = LB.expect(oracle, ref, rows, LB.CPP_BANDS)
    graphs = (np.arange(M) // 6).astype(np.int32)

    def compare(key, want):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(key + " ")]
        oi, ol, osc, _ = want
        assert len(lines) == len(oi) and len(oi) > 0, (key, len(lines), len(oi))
        _same_selection([int(l[1]) for l in lines], [int(l[2]) for l in lines], [float(l[3]) for l in lines], oi, ol, osc)

    for s, ch in ((0, "0"), (1, "+"), (-1, "-")):
        for lo, hi in LB.CPP_BANDS:
            wlag, wmv, tie = exp[(lo, hi, s)]
            assert not tie.any()
            compare("nil%s[%d,%d]" % (ch, lo, hi), oracle.results(wlag, wmv, None, 0, s == 0, 300, 12, 0.0, s))
            compare("graph%s[%d,%d]" % (ch, lo, hi), oracle.results(wlag, wmv, graphs, M // 6, s == 0, 300, 12, 0.0, s))


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_everything_as_it_was(muse, eng):
    """after each refusal the scores, muse_batch_last_run_path, muse_test_last_in_window_path, the kernel name and the batch's own
    window are what a snapshot in front of it recorded"""
    B = muse.binding
    rng = np.random.default_rng(8)

    def setup(N, M=6, f32=False):
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        db = muse.DeviceBatch(eng, dg, rng.standard_normal(N))
        db.scores()
        return dg, db

    dg, db = setup(1024)
    db.scores_in_lag_band(20, 300, 1)                                # (a band pass's scores to leave alone)
    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
    for s in LB.SIGNS:
        for lo, hi in ((7, 1), (0, -1), (-1, -7), (513, 600), (-900, -512), (600, 10 ** 6)):
            refused(muse, eng, db, lambda: db.score_in_lag_band(lo, hi, s), B.MUSE_ERR_INVALID)
            refused(muse, eng, db, lambda: db.run_in_lag_band(lo, hi, sign_filter=s), B.MUSE_ERR_INVALID)
    for s in (2, -2, 7):
        refused(muse, eng, db, lambda: db.score_in_lag_band(1, 7, s), B.MUSE_ERR_INVALID)
        refused(muse, eng, db, lambda: db.run_in_lag_band(1, 7, sign_filter=s), B.MUSE_ERR_INVALID)
    refused(muse, eng, db, lambda: db.run_in_lag_band(1, 7, group_id=np.zeros(6, dtype=np.int32), G=-1, sign_filter=1), B.MUSE_ERR_INVALID)
    db.set_lag_window(7)
    db.scores()
    for lo, hi in ((1, 7), (-7, -1), (0, 7), (3, 5)):
        refused(muse, eng, db, lambda: db.score_in_lag_band(lo, hi, 0), B.MUSE_ERR_INVALID)
    own = db.scores_in_lag_band(-7, 7, -1)                           # the batch's own window equal to the symmetric band: accepted, and kept
    assert db.lag_window() == 7 and np.all(own[1][~np.isnan(own[1])] <= 0)
    # not built: wide bands and float32 storage outside FFT lengths 512 ... 4096
    for N, f32, (lo, hi) in ((5000, False, (1, 200)), (5000, True, (1, 7)), (40000, False, (1, 128)), (9000, True, (-100, -1)), (70000, False, (3, 5))):
        dg, db = setup(N, M=3, f32=f32)
        for s in LB.SIGNS:
            refused(muse, eng, db, lambda: db.score_in_lag_band(lo, hi, s), B.MUSE_ERR_UNSUPPORTED)
            refused(muse, eng, db, lambda: db.run_in_lag_band(lo, hi, sign_filter=s), B.MUSE_ERR_UNSUPPORTED)
    # a kernel forced by a test hook that has no band build: refused, not run unmasked
    dg, db = setup(1024)
    eng.set_kernel(11)
    try:
        refused(muse, eng, db, lambda: db.score_in_lag_band(1, 200, 1), B.MUSE_ERR_UNSUPPORTED)
    finally:
        eng.set_kernel(0)
    lag, mv = db.scores_in_lag_band(1, 200, 1)
    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED and np.all((lag >= 0) & (lag <= 200)) and np.all(mv >= 0)
