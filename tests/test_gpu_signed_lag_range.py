"""GPU tests of the signed best match (muse_batch_score_signed_in_lag_range / _run_signed_in_lag_range, run with -m gpu on an
MI355X): the direct product with the signed scan (xcorr_window_signed_mfma, window_device.h) and the transform kernels' masked
argmax with the sign in the mask (the _signed kernels of xcorr_r16_fold.hip, xcorr_r16_occ4.hip, xcorr_small.hip), through the C ABI
and its mirrors.

Expected values never come from the code under test: per series, the definition in include/muse_hip.h applied in numpy
(tests/_signed.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those (lag, mv).
Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact except rows the ORACLE flags as
ties (the two largest values of the sign inside the range within 1e-12 relative); tests/test_signed_lag_range_cpu.py checks on the
same inputs that the oracle flags none on the plain rows, and that the rows show what filtering could not have produced."""
import subprocess

import numpy as np
import pytest

import _lagrange as LR
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
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "%s score mismatch: worst rel %.3e" % (tag, worst)
    bad = (lag != elag) & ~tie
    assert not bad.any(), "%s lag mismatches at rows %s: %s vs %s" % (tag, np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    return worst


def check_signed(lag, mv, exp, n, lo, hi, sign, tag):
    """check(), and what the sign adds: every lag inside the range, every nonzero value of the sign, and where the definition finds
    no value of the sign exactly (lag 0, +0.0) -- the sign bit clear"""
    elag, emv, tie = exp
    check(lag, mv, elag, emv, tie, tag)
    clo, chi = LR.clip(n, lo, hi)
    assert np.all((lag >= clo) & (lag <= chi)), tag
    num = ~np.isnan(mv)
    assert np.all(sign * mv[num] >= 0), (tag, mv[num][sign * mv[num] < 0][:5])
    none = ~np.isnan(emv) & (emv == 0.0)
    assert np.all(lag[none] == 0) and np.all(mv[none] == 0.0) and not np.signbit(mv[none]).any(), tag
    return int(none.sum())


# ------------------------------------------------------------------ 1. the direct product
@pytest.mark.parametrize("N", LR.MFMA_NS)
def test_direct_product_signed_scan(muse, eng, oracle, N):
    B = muse.binding
    ref, rows = SG.mfma_case(N)
    exp, n = SG.expect(oracle, ref, rows, LR.MFMA_RANGES, signs=SG.SIGNS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.n == n
    none = 0
    for lo, hi in LR.MFMA_RANGES:
        clo, chi = LR.clip(n, lo, hi)
        for s in SG.SIGNS:
            lag, mv = db.scores_signed_in_lag_range(lo, hi, s)
            assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA, (N, lo, hi, s, db.last_in_window_path())
            assert db.lag_window() == -1 and db.last_run_path() == 0
            none += check_signed(lag, mv, exp[(lo, hi, s)], n, lo, hi, s, "direct N=%d [%d, %d] sign %+d" % (N, lo, hi, s))
            name = eng.kernel_name(db)
            assert name.startswith("xcorr_window_signed_mfma<%d, " % ((chi - clo + 1 + 15) // 16)) and name.endswith(", %d>" % s), name
    assert none >= 4                                                 # (beyond the constant row: rows with no value of the sign)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 2. the masked transform pass
@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", LR.MASKED_NS)
def test_masked_pass_signed_mask(muse, eng, oracle, N, f32):
    """tests/_lagrange.py's masked ranges and the whole range (with a sign the masked kernels too, both bounds at their widest);
    float32 groups are checked against the rows as stored"""
    B = muse.binding
    ref, rows = SG.masked_case(N, f32)
    n = LSW.fft_len(N)
    ranges = LR.masked_ranges(n, f32) + [(-(n // 2 - 1), n // 2), (-10 * n, 10 * n)]
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    if f32:
        assert np.array_equal(dg.read(0, SG.PARITY_M), rows, equal_nan=True)
    exp, n2 = SG.expect(oracle, ref, rows, ranges, signs=SG.SIGNS)
    assert n2 == n
    db = muse.DeviceBatch(eng, dg, ref)
    for lo, hi in ranges:
        for s in SG.SIGNS:
            lag, mv = db.scores_signed_in_lag_range(lo, hi, s)
            assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED, (N, f32, lo, hi, s, db.last_in_window_path())
            assert db.lag_window() == -1 and db.last_run_path() == 0
            check_signed(lag, mv, exp[(lo, hi, s)], n, lo, hi, s, "masked N=%d f32=%d [%d, %d] sign %+d" % (N, f32, lo, hi, s))
            name = eng.kernel_name(db)
            assert name.startswith("xcorr_fused_n4096_fold_signed<" if n == 4096 else "xcorr_fused_small_signed<%d, " % (n.bit_length() - 1)), name
            assert name.endswith(", %s>" % ("true" if s < 0 else "false")), name
            if n == 4096:
                assert len(db.redo_pairs()) > 0                      # the specials went through the rescaling kernel, window and sign kept
    db.scores()
    assert db.last_in_window_path() == 0 and "signed" not in eng.kernel_name(db)
    db.close()
    dg.close()


def test_masked_pass_handed_over_pairs_keep_the_sign(muse, eng, oracle):
    """mixed units (sigmas far apart in most pairs): the default n = 4096 kernel lists those pairs and the rescaling kernel behind
    it redoes them -- a dense list: every pair -- in its signed build, window and sign kept"""
    B = muse.binding
    N, M = 4096, 64
    ref, rows = SG.make_case(N, M, seed=15000)
    rows[9::2] *= 1e9                                                # every second plain row in other units
    lo, hi = -300, 100
    exp, n = SG.expect(oracle, ref, rows, ((lo, hi),), signs=SG.SIGNS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for s in SG.SIGNS:
        for k in range(2):
            lag, mv = db.scores_signed_in_lag_range(lo, hi, s)
            assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED
            check_signed(lag, mv, exp[(lo, hi, s)], n, lo, hi, s, "hand-off pass %d sign %+d" % (k, s))
            assert len(db.redo_pairs()) > 0
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. bitwise ties to the existing passes
def _bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("N", (1024, 3000))
def test_sign_zero_and_the_invariant_bit_for_bit(muse, eng, oracle, N, f32):
    """sign 0 is scores_in_lag_range on the direct product, the masked pass and the plain one; a row whose unsigned in-range winner
    has the sign (and is no tie for the oracle) has the unsigned pass's bits in the signed one, both on the same path; a signed pass
    leaves nothing behind: the unsigned pass after it gives its bits again.
    The symmetric score_in_window, score_many_windowed and slide_score_windowed passes take none of the new arguments; their kernels'
    resource lines are the parent's (profiles/signed_lag_range_resources.txt) and the existing tests hold them to their oracle paths
    as before.  Values recorded from the parent commit are not kept in the tree: here the window is tied to sign 0 instead."""
    B = muse.binding
    ref, rows = SG.masked_case(N, f32)
    n = LSW.fft_len(N)
    ranges = ((-7, 0), (0, 63), (-40, 3), (-200, 0), (-64, 300), (-(n // 2 - 1), n // 2))
    exp, _ = SG.expect(oracle, ref, rows, ranges)
    dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    db, un = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dg, ref)
    kept = 0
    for lo, hi in ranges:
        u = un.scores_in_lag_range(lo, hi)
        upath = un.last_in_window_path()
        assert upath == muse.lag_range_plan(N, f32, lo, hi)
        z = db.scores_signed_in_lag_range(lo, hi, 0)
        assert _bits(z, u) and db.last_in_window_path() == upath and eng.kernel_name(db) == eng.kernel_name(un), (N, f32, lo, hi)
        ulag, umv, utie = exp[(lo, hi, 0)]
        for s in SG.SIGNS:
            g = db.scores_signed_in_lag_range(lo, hi, s)
            if db.last_in_window_path() == upath:                    # (every lag: PLAIN against MASKED, values equal to rounding only)
                same = ~utie & (s * umv > 0)
                assert same.sum() >= 3, (N, f32, lo, hi, s)
                assert np.array_equal(g[0][same], u[0][same]) and g[1][same].tobytes() == u[1][same].tobytes(), (N, f32, lo, hi, s)
                kept += int(same.sum())
            again = db.scores_in_lag_range(lo, hi)
            assert _bits(again, u) and db.last_in_window_path() == upath, (N, f32, lo, hi, s)
    assert kept >= 60
    for L in (7, 63, 200):
        w = un.scores_in_window(L)
        assert _bits(db.scores_signed_in_lag_range(-L, L, 0), w)
        db.scores_signed_in_lag_range(-L, L, 1)
        assert _bits(un.scores_in_window(L), w) and _bits(db.scores_in_window(L), w)
    plain = un.scores()
    db.scores_signed_in_lag_range(-7, 0, -1)
    assert _bits(db.scores(), plain) and db.last_in_window_path() == 0 and db.lag_window() == -1
    for h in (db, un, dg):
        h.close()


# ------------------------------------------------------------------ 4. negation
@pytest.mark.parametrize("N", (1000, 4096))
def test_negated_rows_swap_the_signs(muse, eng, oracle, N):
    """signed(-1) on rows y against signed(+1) on rows -y: the same lags off ties, values equal and opposite"""
    ref, rows = SG.masked_case(N, False)
    n = LSW.fft_len(N)
    ranges = ((-40, 3), (-300, 100), (-(n // 2 - 1), n // 2))
    exp, _ = SG.expect(oracle, ref, rows, ranges, signs=(-1,))
    dg, dn = muse.DeviceGroup.from_rows(eng, rows), muse.DeviceGroup.from_rows(eng, -rows)
    db, bn = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, dn, ref)
    for lo, hi in ranges:
        a = db.scores_signed_in_lag_range(lo, hi, -1)
        b = bn.scores_signed_in_lag_range(lo, hi, 1)
        assert db.last_in_window_path() == bn.last_in_window_path()
        tie = exp[(lo, hi, -1)][2]
        check(b[0], -b[1], a[0], a[1], tie, tag="negation N=%d [%d, %d]" % (N, lo, hi))
        ok = ~np.isnan(a[1])
        exact = np.array_equal(-b[1][ok], a[1][ok]) and np.array_equal(a[0], b[0])       # (numerically: -(+0.0) counts as +0.0)
        print("negation N=%d [%d, %d] path %d: bitwise opposite %s" % (N, lo, hi, db.last_in_window_path(), exact))
    for h in (db, bn, dg, dn):
        h.close()


# ------------------------------------------------------------------ 5. edges from planted winners
@pytest.mark.parametrize("N,rng", LR.EDGE_CASES)
def test_edges_from_planted_winners(muse, eng, oracle, N, rng):
    """a code planted at the lags lo-1, lo, lo+1, -1, 0, 1, hi-1, hi, hi+1, positive on the even rows and negative on the odd ones:
    under its own sign a row's planted lag comes back just inside each bound, with the long-double score at that index; a lag
    planted just outside is never reported"""
    B = muse.binding
    lo, hi = rng
    ref, rows, n, planted, sgn = SG.edge_case(N, lo, hi)
    exp, _ = SG.expect(oracle, ref, rows, (rng,), signs=SG.SIGNS)
    bounds, _ = LSW.row_bounds(n, rows)
    xs_pad = LSW.ld_ref(ref, n)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for s in SG.SIGNS:
        lag, mv = db.scores_signed_in_lag_range(lo, hi, s)
        assert db.last_in_window_path() == (B.MUSE_IN_WINDOW_MFMA if hi - lo + 1 <= 127 else B.MUSE_IN_WINDOW_MASKED)
        for row, pl in enumerate(planted):
            if lo <= int(pl) <= hi and sgn[row] == s:
                assert lag[row] == pl and s * mv[row] > 0, (N, rng, s, row, lag[row], pl, mv[row])
                want = LSW.ld_score_at(ref, rows[row], n, int(pl) % n, xs_pad)
                assert abs(np.longdouble(mv[row]) - want) <= bounds[row], (N, rng, s, row, mv[row], float(want), bounds[row])
            else:
                assert lo <= int(lag[row]) <= hi, (N, rng, s, row, lag[row], pl)
                if not lo <= int(pl) <= hi:
                    assert lag[row] != pl
        check_signed(lag, mv, exp[(lo, hi, s)], n, lo, hi, s, "edges N=%d [%d, %d] sign %+d" % (N, lo, hi, s))
        assert not exp[(lo, hi, s)][2].any()
    db.close()
    dg.close()


# ------------------------------------------------------------------ 6. the Run form
def _assert_run(got, want):
    idx, lag, score = got[0], got[1], got[2]
    oi, ol, osc = want[0], want[1], want[2]
    assert lag.tolist() == ol.tolist()
    assert np.allclose(score, osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert idx.tolist() == oi.tolist()
    assert abs(got[3] - want[3]) < 1e-9 or (np.isnan(got[3]) and np.isnan(want[3]))    # (an empty selection has no mean)


@pytest.mark.parametrize("N", SG.RUN_NS)
def test_run_signed_in_lag_range_matches_the_selection_on_the_definition(muse, eng, oracle, N):
    """run_signed_in_lag_range ungrouped and in label groups of 3 equals the oracle's group maximum, passed() and Fetch fed with the
    definition's per-series (lag, mv) of the sign; with signed group scores it selects groups that run_in_lag_range with the same
    sign_filter drops; sign_filter 0 is run_in_lag_range.  Batch.RunSignedInLagRange and RunSigned of the Python mirror agree."""
    M = SG.RUN_M
    ref, rows = SG.run_case(N)
    exp, n = SG.expect(oracle, ref, rows, SG.RUN_RANGES + ((-20, 20),))
    gid, G = SG.run_groups()
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    labels = [{"trio": "t%02d" % (i // SG.RUN_GROUP), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    for lo, hi in SG.RUN_RANGES:
        L = max(-lo, hi)
        for s in SG.SIGNS:
            wlag, wmv, tie = exp[(lo, hi, s)]
            for ab in (True, False):
                for thr in (0.0, 0.35):
                    got = db.run_signed_in_lag_range(lo, hi, None, 0, 20, thr, s, ab)
                    assert db.last_in_window_path() in (2, 3) and db.last_run_path() == 0 and db.lag_window() == -1
                    _assert_run(got, oracle.results(wlag, wmv, None, 0, ab, L, 20, thr, s))
                    got = db.run_signed_in_lag_range(lo, hi, gid, G, 20, thr, s, ab)
                    _assert_run(got, oracle.results(wlag, wmv, gid, G, ab, L, 20, thr, s))
            signed = db.run_signed_in_lag_range(lo, hi, gid, G, G, 0.0, s, False)
            plain = db.run_in_lag_range(lo, hi, gid, G, G, 0.0, s, False)
            gained = set(gid[signed[0]].tolist()) - set(gid[plain[0]].tolist())
            assert len(gained) >= 1 and not set(gid[plain[0]].tolist()) - set(gid[signed[0]].tolist()), (N, lo, hi, s)
        for ab in (True, False):
            a = db.run_signed_in_lag_range(lo, hi, gid, G, 20, 0.0, 0, ab)
            b = db.run_in_lag_range(lo, hi, gid, G, 20, 0.0, 0, ab)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
        # the Python mirror: Scores carry the signed value under a sign (abs_scores False)
        for s, filt in ((1, muse.SignFilter_POS), (-1, muse.SignFilter_NEG)):
            res = muse.NewResults(L, 12, 0.0, filt)
            b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"trio": "ref"})), comp, res, 8, engine=eng)
            for by, g, Gn in ((None, None, 0), (["trio"], gid, G)):
                b.RunSignedInLagRange(by, lo, hi)
                got, mean = res.Fetch()
                oi, ol, osc, omean = oracle.results(exp[(lo, hi, s)][0], exp[(lo, hi, s)][1], g, Gn, False, L, 12, 0.0, s)
                assert len(got) == len(oi) > 0
                assert [sc.Lag for sc in got] == ol.tolist()
                assert np.allclose([sc.PercentScore for sc in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
                assert [int(sc.Labels.labels["i"]) for sc in got] == oi.tolist()
                assert abs(mean - omean) < 1e-9
    for s, filt in ((1, muse.SignFilter_POS), (-1, muse.SignFilter_NEG)):       # RunSigned: the range -MaxLag .. MaxLag
        res = muse.NewResults(20, 12, 0.0, filt)
        b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"trio": "ref"})), comp, res, 8, engine=eng)
        b.RunSigned(["trio"])
        got, _ = res.Fetch()
        oi, ol, osc, _ = oracle.results(exp[(-20, 20, s)][0], exp[(-20, 20, s)][1], gid, G, False, 20, 12, 0.0, s)
        assert len(got) == len(oi) > 0 and [sc.Lag for sc in got] == ol.tolist()
        assert np.allclose([sc.PercentScore for sc in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
        assert [int(sc.Labels.labels["i"]) for sc in got] == oi.tolist()
    res = muse.NewResults(20, 12, 0.0, muse.SignFilter_ANY)                      # SignFilter_ANY: RunInLagRange
    b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"trio": "ref"})), comp, res, 8, engine=eng)
    b.RunSigned(["trio"])
    got, _ = res.Fetch()
    b.RunInLagRange(["trio"], -20, 20)
    want, _ = res.Fetch()
    assert [(sc.Lag, sc.PercentScore) for sc in got] == [(sc.Lag, sc.PercentScore) for sc in want] and len(got) > 0
    db.close()
    dg.close()


# ------------------------------------------------------------------ 7. the C++ mirror
def test_cpp_batch_run_signed_in_lag_range(muse, oracle):
    """Batch::RunSignedInLagRange and RunSigned of the C++ host mirror (host/muse_signed_lag_range_test.cpp), in a fresh process,
    Fetch what the oracle gives"""
    exe = muse.build.build_signed_lag_range_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "signed lag-range ok" in r.stdout, r.stdout + r.stderr
    ref, rows = SG.cpp_case()
    M = LR.CPP_M
    Ls = SG.CPP_SIGNED_MAXLAG
    exp, _ = SG.expect(oracle, ref, rows, SG.CPP_RANGES + ((-Ls, Ls),), signs=SG.SIGNS)
    graphs = (np.arange(M) // 6).astype(np.int32)

    def compare(key, want):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(key + " ")]
        oi, ol, osc, _ = want
        assert len(lines) == len(oi) == 12, (key, len(lines), len(oi))
        assert [int(l[1]) for l in lines] == oi.tolist(), key
        assert [int(l[2]) for l in lines] == ol.tolist(), key
        assert np.allclose([float(l[3]) for l in lines], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL), key

    for s, ch in ((1, "+"), (-1, "-")):
        for lo, hi in SG.CPP_RANGES:
            wlag, wmv, tie = exp[(lo, hi, s)]
            assert not tie.any()
            compare("nil%s[%d,%d]" % (ch, lo, hi), oracle.results(wlag, wmv, None, 0, False, 300, 12, 0.0, s))
            compare("graph%s[%d,%d]" % (ch, lo, hi), oracle.results(wlag, wmv, graphs, M // 6, False, 300, 12, 0.0, s))
        wlag, wmv, _ = exp[(-Ls, Ls, s)]
        compare("signed%s[%d,%d]" % (ch, -Ls, Ls), oracle.results(wlag, wmv, None, 0, False, Ls, 12, 0.0, s))


# ------------------------------------------------------------------ 8. refusals
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

    dg, db, base = setup(1024)
    base = db.scores_signed_in_lag_range(-300, 20, 1)                # (a signed pass's scores to leave alone)
    P = B.MUSE_IN_WINDOW_MASKED
    for s in (1, -1):
        for lo, hi in ((1, 7), (-7, -1), (1, 0), (0, -1)):
            refused(db, base, lambda: db.score_signed_in_lag_range(lo, hi, s), B.MUSE_ERR_INVALID, path=P)
            refused(db, base, lambda: db.run_signed_in_lag_range(lo, hi, sign_filter=s), B.MUSE_ERR_INVALID, path=P)
    for s in (2, -2, 7):
        refused(db, base, lambda: db.score_signed_in_lag_range(-7, 0, s), B.MUSE_ERR_INVALID, path=P)
        refused(db, base, lambda: db.run_signed_in_lag_range(-7, 0, sign_filter=s), B.MUSE_ERR_INVALID, path=P)
    refused(db, base, lambda: db.run_signed_in_lag_range(-7, 0, group_id=np.zeros(6, dtype=np.int32), G=-1, sign_filter=1), B.MUSE_ERR_INVALID, path=P)
    db.set_lag_window(7)
    base7 = db.scores()
    for lo, hi in ((-7, 0), (0, 7), (-200, 7)):
        refused(db, base7, lambda: db.score_signed_in_lag_range(lo, hi, 1), B.MUSE_ERR_INVALID, window=7)
    own = db.scores_signed_in_lag_range(-7, 7, -1)                   # the batch's own window equal to the range: accepted, and kept
    assert db.lag_window() == 7 and np.all(own[1][~np.isnan(own[1])] <= 0)
    # not built: 200 lags, every lag and float32 storage outside FFT lengths 512 ... 4096
    for N, f32, (lo, hi) in ((5000, False, (-200, 0)), (5000, False, (-(1 << 20), 1 << 20)), (5000, True, (-7, 0)), (200, False, (-100, 60)),
                             (200, False, (-(1 << 20), 1 << 20))):
        dg, db, base = setup(N, M=3, f32=f32)
        for s in (1, -1):
            refused(db, base, lambda: db.score_signed_in_lag_range(lo, hi, s), B.MUSE_ERR_UNSUPPORTED)
            refused(db, base, lambda: db.run_signed_in_lag_range(lo, hi, sign_filter=s), B.MUSE_ERR_UNSUPPORTED)
    dg, db, base = setup(5000, M=3)                                  # sign 0 at every lag is the plain pass, whatever the length
    z = db.scores_signed_in_lag_range(-(1 << 20), 1 << 20, 0)
    assert z[0].tobytes() == base[0].tobytes() and z[1].tobytes() == base[1].tobytes() and db.last_in_window_path() == B.MUSE_IN_WINDOW_PLAIN
    # a kernel forced by a test hook that has no masked build: refused, not run unmasked
    dg, db, base = setup(1024)
    eng.set_kernel(11)
    try:
        refused(db, base, lambda: db.score_signed_in_lag_range(-200, 0, 1), B.MUSE_ERR_UNSUPPORTED)
    finally:
        eng.set_kernel(0)
    lag, mv = db.scores_signed_in_lag_range(-200, 0, 1)
    assert db.last_in_window_path() == B.MUSE_IN_WINDOW_MASKED and np.all((lag >= -200) & (lag <= 0)) and np.all(mv >= 0)
