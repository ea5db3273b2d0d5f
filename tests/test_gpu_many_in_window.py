"""GPU tests of many references inside a lag window of any width (muse_batch_score_many_in_window / _run_many_in_window, run with
-m gpu on an MI355X): ONE masked pass of the many-references transform kernels (the WIN builds of xcorr_fused_n4096_fold_multi and
of the MULTI xcorr_fused_small), the redo of listed pairs with the window, and the dispatch around it, through the C ABI.

Expected values never come from the code under test: per series and reference, the definition in include/muse_hip.h applied in
numpy (tests/_window.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those windowed
(lag, mv).  Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal, lags exact except rows the
ORACLE flags as ties; tests/test_many_in_window_cpu.py checks on the same inputs (tests/_manyinwindow.py) that the oracle flags
none.  References are np.roll(ref0, s): a roll by s moves every global lag by +s, so every reference sees other rows inside and
outside the window."""
import subprocess

import numpy as np
import pytest

import _inwindow as IW
import _lagsweep as LSW
import _manyinwindow as MW
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


def _one_pass_name(n):
    return "xcorr_fused_n4096_fold_multi<" if n == 4096 else "xcorr_fused_small<%d, " % (n.bit_length() - 1)


def _assert_one_masked_pass(muse, eng, dbs, n):
    """every batch's scores came by the masked path, from the WIN instantiation of the many-references kernel"""
    for db in dbs:
        assert db.last_in_window_path() == muse.binding.MUSE_IN_WINDOW_MASKED, db.last_in_window_path()
        assert db.lag_window() == -1 and db.last_run_path() == 0
        name = eng.kernel_name(db)
        assert name.startswith(_one_pass_name(n)) and name.endswith(", true>"), name
        if n != 4096:
            assert ", true, false, true>" in name, name          # MULTI, float64 rows, WIN


def _batches(muse, eng, dg, refs):
    return [muse.DeviceBatch(eng, dg, r) for r in refs]


def _close(*hs):
    for h in hs:
        h.close()


# ------------------------------------------------------------------ 1. parity against the definition
@pytest.mark.parametrize("N", IW.PARITY_NS)
def test_parity_four_references(muse, eng, oracle, N):
    """make_case rows with the eight specials (NaN, Inf, 1e+-100 and mean 1e6 go through the redo kernel at n = 4096), an odd row
    count, four rolled references, windows whose edge lies inside a lane range, on a 256-index register block and at n/2 - 1"""
    ref0, rows = IW.parity_case(N)
    n = LSW.fft_len(N)
    Ls = MW.parity_Ls(n)
    refs = MW.refs_of(ref0, MW.PARITY_ROLLS)
    assert muse.many_in_window_plan(N, False, Ls[0], len(refs)) == MW.MASKED
    exps = [W.expect(oracle, r, rows, Ls) for r in refs]
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    assert all(db.n == n for db in dbs)
    for L in Ls:
        got = muse.scores_many_in_window(dbs, L)
        _assert_one_masked_pass(muse, eng, dbs, n)
        for r, (lag, mv) in enumerate(got):
            check(lag, mv, *exps[r][0][L], tag="parity N=%d L=%d ref %d" % (N, L, r))
            assert np.all(np.abs(lag) <= L)
    # for some reference at least four noise rows have their global winner inside the narrowest window and four outside
    keep = W.plain_rows(IW.PARITY_M)
    assert any(((np.abs(e[1]) <= Ls[0]) & keep).sum() >= 4 and ((np.abs(e[1]) > Ls[0]) & keep).sum() >= 4 for e in exps)
    # ... and the references do not see the same rows inside
    assert len({tuple(np.abs(e[1]) <= Ls[0]) for e in exps}) > 1
    _close(*dbs, dg)


# ------------------------------------------------------------------ 2. window edges from planted winners
@pytest.mark.parametrize("N", IW.EDGE_NS)
def test_edges_from_planted_winners(muse, eng, oracle, N):
    """for the unrolled reference a code planted at +-(L - 1), +-L comes back there with the long-double score at that index, at
    +-(L + 1) the result lies inside the window; the references rolled by +-1 see every planted lag moved by one: all three are the
    definition's on the oracle's cc"""
    ref0, rows, n, where = IW.edge_case(N)
    Ls = IW.edge_Ls(n)
    refs = MW.refs_of(ref0, MW.EDGE_ROLLS)
    exps = [W.expect(oracle, r, rows, Ls)[0] for r in refs]
    bounds, _ = LSW.row_bounds(n, rows)
    xs_pad = LSW.ld_ref(ref0, n)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    for L in Ls:
        got = muse.scores_many_in_window(dbs, L)
        _assert_one_masked_pass(muse, eng, dbs, n)
        lag, mv = got[0]
        r, planted = where[L]
        for row, pl in zip(r, planted):
            if abs(int(pl)) <= L:
                assert lag[row] == pl, (N, L, row, lag[row], pl)
                want = LSW.ld_score_at(ref0, rows[row], n, int(pl) % n, xs_pad)
                assert abs(np.longdouble(mv[row]) - want) <= bounds[row], (N, L, row, mv[row], float(want), bounds[row])
            else:
                assert abs(int(lag[row])) <= L, (N, L, row, lag[row], pl)
        for k, (lag, mv) in enumerate(got):
            check(lag, mv, *exps[k][L], tag="edges N=%d L=%d ref %d" % (N, L, k))
            assert not exps[k][L][2].any() and np.all(np.abs(lag) <= L)
    _close(*dbs, dg)


# ------------------------------------------------------------------ 3. workgroups that loop, one case per kernel family
@pytest.mark.parametrize("N,M", MW.LOOP_CASES)
def test_workgroups_that_loop(muse, eng, oracle, N, M):
    """at least three iterations per resident workgroup on 256 CUs, an odd row count"""
    ref0, rows = MW.loop_case(N, M)
    n = LSW.fft_len(N)
    L = MW.LOOP_L
    refs = MW.refs_of(ref0, MW.ROLLS3)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    got = muse.scores_many_in_window(dbs, L)
    _assert_one_masked_pass(muse, eng, dbs, n)
    for r, (lag, mv) in enumerate(got):
        exp, _, _, _ = W.expect(oracle, refs[r], rows, (L,))
        check(lag, mv, *exp[L], tag="loop N=%d M=%d ref %d" % (N, M, r))
        assert np.all(np.abs(lag) <= L)
    _close(*dbs, dg)


# ------------------------------------------------------------------ 4. the redo at n = 4096 keeps the window, per reference
def test_redo_keeps_the_window(muse, eng, oracle):
    """every second row scaled by 1e30: every pair's sigmas are too far apart for one shared transform, reference 0 lists them all
    and every reference's redo launch follows that list with the window"""
    ref0, rows = IW.redo_case()
    L = IW.REDO_L
    refs = MW.refs_of(ref0, MW.ROLLS3)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    first = muse.scores_many_in_window(dbs, L)
    _assert_one_masked_pass(muse, eng, dbs, 4096)
    assert len(dbs[0].redo_pairs()) > 0
    for r, (lag, mv) in enumerate(first):
        exp, glag, _, _ = W.expect(oracle, refs[r], rows, (L,))
        check(lag, mv, *exp[L], tag="redo ref %d" % r)
        assert np.all(np.abs(lag) <= L) and (np.abs(glag) > L).sum() > IW.REDO_M // 8
    second = muse.scores_many_in_window(dbs, L)
    for a, b in zip(first, second):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _close(*dbs, dg)


# ------------------------------------------------------------------ 5. float32 storage
@pytest.mark.parametrize("N", MW.F32_ONE_PASS_NS + (MW.F32_EACH_N,))
def test_float32_groups(muse, eng, oracle, N):
    """FFT length 4096: one masked pass, also at windows the float64 groups hand to the direct product; N = 480: the MULTI builds of
    the short lengths read float64 rows only -- single masked passes, batch after batch"""
    ref0, stored = IW.f32_case(N)
    n = LSW.fft_len(N)
    refs = MW.refs_of(ref0, MW.ROLLS3)
    dg = muse.DeviceGroup.from_rows(eng, stored, f32=True)
    rows = dg.read(0, IW.F32_M)
    assert np.array_equal(rows, stored, equal_nan=True)              # (the rounded rows the CPU test checked for ties)
    dbs = _batches(muse, eng, dg, refs)
    one_pass = N in MW.F32_ONE_PASS_NS
    for L in IW.F32_LS:
        want = MW.PLAIN if L >= n // 2 else (MW.MASKED if one_pass else MW.MASKED_EACH)
        assert muse.many_in_window_plan(N, True, L, len(refs)) == want, (N, L)
        got = muse.scores_many_in_window(dbs, L)
        if want == MW.MASKED:
            _assert_one_masked_pass(muse, eng, dbs, n)
        elif want == MW.MASKED_EACH:
            for db in dbs:
                assert db.last_in_window_path() == MW.MASKED
                assert eng.kernel_name(db) == "xcorr_fused_small<%d, %s, false, true, true>" % (n.bit_length() - 1, "true" if N < n else "false")
        for r, (lag, mv) in enumerate(got):
            exp, _, _, _ = W.expect(oracle, refs[r], rows, (L,))
            check(lag, mv, *exp[L], tag="f32 N=%d L=%d ref %d" % (N, L, r))
            assert np.all(np.abs(lag) <= L)
    _close(*dbs, dg)


# ------------------------------------------------------------------ 6. identities
@pytest.mark.parametrize("N", MW.IDENT_NS)
def test_identities(muse, eng, N):
    ref0, rows = MW.ident_case(N)
    n = LSW.fft_len(N)
    refs = MW.refs_of(ref0, MW.ROLLS3)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    own = _batches(muse, eng, dg, refs)

    def same(a, b):
        return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(a, b))

    before = [db.scores() for db in dbs]                             # (each batch's own plain pass)
    plain = muse.scores_many(own)
    for L in (n // 2, n // 2 + 1, 10 * n):                          # the window is every lag: scores_many, bytes equal
        assert same(muse.scores_many_in_window(dbs, L), plain), (N, L)
        assert all(db.last_in_window_path() == 0 for db in dbs)
    for L in (0, 7, 63):                                             # up to the cap on float64 rows: scores_many_windowed, bytes equal
        want = muse.scores_many_windowed(own, L)
        assert same(muse.scores_many_in_window(dbs, L), want), (N, L)
        assert all(db.lag_window() == -1 for db in dbs)
    L = 100
    a = muse.scores_many_in_window(dbs, L)
    _assert_one_masked_pass(muse, eng, dbs, n)
    b = muse.scores_many_in_window(dbs, L)                           # two masked passes in a row: bit-identical
    assert same(a, b)
    for r, db in enumerate(own):                                     # each batch's own masked pass: the same lags, scores to rounding
        lag, mv = db.scores_in_window(L)
        assert np.array_equal(a[r][0], lag), (N, r, np.nonzero(a[r][0] != lag)[0][:8])
        ok = ~np.isnan(mv)
        assert np.array_equal(np.isnan(a[r][1]), ~ok)
        assert np.all(np.abs(a[r][1][ok] - mv[ok]) <= SCORE_RTOL * np.abs(mv[ok]) + SCORE_ATOL), (N, r)
    one = muse.scores_many_in_window(dbs[:1], L)                     # R == 1: the single masked pass
    assert muse.many_in_window_plan(N, False, L, 1) == MW.MASKED_EACH
    assert same(one, [own[0].read_scores()]) and dbs[0].last_in_window_path() == MW.MASKED
    assert eng.kernel_name(dbs[0]) == eng.kernel_name(own[0])
    assert eng.kernel_name(dbs[0]).startswith("xcorr_fused_n4096_fold<" if n == 4096 else "xcorr_fused_small<%d, false, false, " % (n.bit_length() - 1))
    muse.scores_many_in_window(dbs, L)
    for r, db in enumerate(dbs):                                     # afterwards scores() is the plain pass again
        lag, mv = db.scores()
        assert db.last_in_window_path() == 0 and db.lag_window() == -1
        assert not eng.kernel_name(db).endswith(", true>")
        assert lag.tobytes() == before[r][0].tobytes() and mv.tobytes() == before[r][1].tobytes()
    _close(*dbs, *own, dg)


# ------------------------------------------------------------------ 7. refusals leave everything as it was
def test_refusals_leave_everything_as_it_was(muse, eng):
    B = muse.binding
    rng = np.random.default_rng(8)

    def setup(N, M=6, R=2, f32=False):
        dg = muse.DeviceGroup.from_rows(eng, rng.standard_normal((M, N)), f32=f32)
        dbs = [muse.DeviceBatch(eng, dg, rng.standard_normal(N)) for _ in range(R)]
        return dg, dbs, [db.scores() for db in dbs]

    def state(db):
        return db.read_scores(), db.lag_window(), db.last_in_window_path(), eng.kernel_name(db)

    def refused(dbs, fn, status):
        before = [state(db) for db in dbs]
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message, e.value
        for db, was in zip(dbs, before):
            now = state(db)
            assert now[0][0].tobytes() == was[0][0].tobytes() and now[0][1].tobytes() == was[0][1].tobytes()
            assert now[1:] == was[1:], (now[1:], was[1:])

    for N in (1024, 4096):
        dg, dbs, _ = setup(N)
        refused(dbs, lambda: muse.score_many_in_window(dbs, -1), B.MUSE_ERR_INVALID)
        refused(dbs, lambda: muse.run_many_in_window(dbs, None, 0, -1), B.MUSE_ERR_INVALID)
        refused(dbs, lambda: muse.run_many_in_window(dbs, None, 0, 100, 5, 0.0, 2), B.MUSE_ERR_INVALID)   # (sign_filter)
        refused(dbs, lambda: muse.score_many_in_window([dbs[0], dbs[1], dbs[0]], 100), B.MUSE_ERR_INVALID)   # a duplicate
        dg2, dbs2, _ = setup(N)
        both = dbs + dbs2
        refused(both, lambda: muse.score_many_in_window([dbs[0], dbs2[0]], 100), B.MUSE_ERR_INVALID)         # mixed groups
        dbs[1].set_lag_window(7)                                                                             # a window of its own that differs
        dbs[1].scores()
        refused(dbs, lambda: muse.score_many_in_window(dbs, 100), B.MUSE_ERR_INVALID)
        refused(dbs, lambda: muse.run_many_in_window(dbs, None, 0, 100), B.MUSE_ERR_INVALID)
        got = muse.scores_many_in_window(dbs, 7)                     # ... and one that equals the call's is accepted and kept
        assert dbs[1].lag_window() == 7 and np.all(np.abs(got[1][0]) <= 7)
        dbs[1].set_lag_window(-1)
        # a kernel forced by a test hook that has no masked build: refused, never run unmasked
        for db in dbs:
            db.scores()
        eng.set_kernel(11)
        try:
            refused(dbs, lambda: muse.score_many_in_window(dbs, 100), B.MUSE_ERR_UNSUPPORTED)
        finally:
            eng.set_kernel(0)
        got = muse.scores_many_in_window(dbs, 100)
        _assert_one_masked_pass(muse, eng, dbs, N)
        assert all(np.all(np.abs(g[0]) <= 100) for g in got)
        _close(*dbs, *dbs2, dg, dg2)
    dg, dbs, _ = setup(5000, M=3)                                    # no masked build at this length
    refused(dbs, lambda: muse.score_many_in_window(dbs, 100), B.MUSE_ERR_UNSUPPORTED)
    refused(dbs, lambda: muse.run_many_in_window(dbs, None, 0, 100), B.MUSE_ERR_UNSUPPORTED)
    _close(*dbs, dg)
    dg, dbs, _ = setup(5000, M=3, f32=True)
    refused(dbs, lambda: muse.score_many_in_window(dbs, 7), B.MUSE_ERR_UNSUPPORTED)
    _close(*dbs, dg)
    # the old entry points go on refusing what they refused
    dg, dbs, _ = setup(1024)
    with pytest.raises(muse.MuseError) as e:
        muse.score_many_windowed(dbs, 100)
    assert e.value.status == B.MUSE_ERR_UNSUPPORTED
    _close(*dbs, dg)


# ------------------------------------------------------------------ 8. the Run form
def _assert_run(idx, lag, score, want, wmv):
    """the selection is the oracle's, position by position.  Where the oracle's own |score| of two series agree to TIE_GAP (rows 1 and
    2 of make_case: the reference and its negative), their order -- and which of them wins a label group -- is decided by the last
    bit, and the many-references kernels round a series by its place in the pair: there either series is accepted, with its own lag
    and score (the single-reference tests see both rounded alike and never meet this)"""
    oi, ol, osc = (np.asarray(v) for v in want[:3])
    idx, lag, score = np.asarray(idx), np.asarray(lag), np.asarray(score, dtype=np.float64)
    assert len(idx) == len(oi)
    assert np.allclose(np.abs(score), np.abs(osc), rtol=SCORE_RTOL, atol=SCORE_ATOL)
    for k in range(len(oi)):
        if idx[k] != oi[k]:
            a, b = abs(wmv[idx[k]]), abs(wmv[oi[k]])
            assert abs(a - b) <= W.TIE_GAP * max(a, b), (k, idx[k], oi[k], a, b)
            others = np.concatenate([idx[:k], idx[k + 1:]])
            assert idx[k] not in others
        else:
            assert lag[k] == ol[k] and abs(score[k] - osc[k]) <= SCORE_RTOL * abs(osc[k]) + SCORE_ATOL, (k, idx[k])


def test_run_many_in_window_matches_the_selection_on_the_definition(muse, eng, oracle):
    """run_many_in_window ungrouped and grouped (G = 7) equals the oracle's Results.Update / Fetch fed with the definition's per-row
    pairs of every reference; RunManyInWindow of the Python mirror Fetches what each batch's own RunInWindow Fetches"""
    N, M, G, L = IW.RUN_N, IW.RUN_M, IW.RUN_G, IW.RUN_L
    ref0, rows = IW.run_case()
    n = LSW.fft_len(N)
    refs = MW.refs_of(ref0, MW.ROLLS3)
    exps = [W.expect(oracle, r, rows, (L,))[0][L] for r in refs]
    for wlag, wmv, tie in exps:
        assert not (tie & W.plain_rows(M)).any()
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = _batches(muse, eng, dg, refs)
    gid = (np.arange(M) * 5 % G).astype(np.int32)
    for sign, thr in ((0, 0.0), (1, 0.0), (-1, 0.0), (0, 0.35)):
        for g, Gn, ab in ((None, 0, True), (gid, G, True), (gid, G, False)):
            got = muse.run_many_in_window(dbs, g, Gn, L, 20, thr, sign, ab)
            _assert_one_masked_pass(muse, eng, dbs, n)
            for r in range(len(refs)):
                _assert_run(*got[r][:3], oracle.results(exps[r][0], exps[r][1], g, Gn, ab, L, 20, thr, sign), exps[r][1])
    _close(*dbs, dg)
    # the label-level mirror
    hosts = 6
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])

    def batches():
        rs = [muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY) for _ in refs]
        return rs, [muse.NewBatch(muse.NewSeries(r, muse.NewLabels({"graph": "ref%d" % k})), comp, rs[k], 8, engine=eng)
                    for k, r in enumerate(refs)]

    for by, g, Gn in ((None, None, 0), (["graph"], (np.arange(M) // hosts).astype(np.int32), M // hosts)):
        rs, bs = batches()
        muse.RunManyInWindow(bs, by)
        rs1, bs1 = batches()
        for k in range(len(refs)):
            got, mean = rs[k].Fetch()
            oi, ol, osc, omean = oracle.results(exps[k][0], exps[k][1], g, Gn, True, L, 12, 0.0, 0)
            assert len(got) == len(oi) > 0
            mine = ([int(s.Labels.labels["i"]) for s in got], [s.Lag for s in got], [s.PercentScore for s in got])
            _assert_run(*mine, (oi, ol, osc), exps[k][1])
            assert abs(mean - omean) < 1e-9
            bs1[k].RunInWindow(by)                                   # what the batch's own RunInWindow Fetches
            one, _ = rs1[k].Fetch()
            _assert_run(*mine, ([int(s.Labels.labels["i"]) for s in one], [s.Lag for s in one], [s.PercentScore for s in one]), exps[k][1])
    # Results settings that differ: one RunInWindow per batch
    rs, bs = batches()
    rs[1].MaxLag = L + 1
    muse.RunManyInWindow(bs, None)
    got, _ = rs[0].Fetch()
    oi, ol, _, _ = oracle.results(exps[0][0], exps[0][1], None, 0, True, L, 12, 0.0, 0)
    assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
    got, _ = rs[1].Fetch()
    assert len(got) == 12 and all(abs(s.Lag) <= L + 1 for s in got)


def test_cpp_batch_run_many_in_window(muse, oracle):
    """Batch::RunManyInWindow of the C++ host mirror (host/muse_many_in_window_test.cpp) Fetches what the oracle gives, and what each
    batch's own RunInWindow Fetches (checked by the program)"""
    exe = muse.build.build_many_in_window_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "many in-window ok" in r.stdout, r.stdout + r.stderr
    refs, rows = MW.cpp_case()
    M, L = MW.CPP_M, MW.CPP_L
    for k, ref in enumerate(refs):
        exp, _, _, _ = W.expect(oracle, ref, rows, (L,))
        wlag, wmv, tie = exp[L]
        assert not tie.any()
        for case, gid, G in (("nil", None, 0), ("graph", (np.arange(M) // 6).astype(np.int32), M // 6)):
            lines = [l.split() for l in r.stdout.splitlines() if l.startswith("%s%d " % (case, k))]
            oi, ol, osc, _ = oracle.results(wlag, wmv, gid, G, True, L, 12, 0.0, 0)
            assert len(lines) == len(oi) == 12
            assert [int(l[1]) for l in lines] == oi.tolist()
            assert [int(l[2]) for l in lines] == ol.tolist()
            assert np.allclose([float(l[3]) for l in lines], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
