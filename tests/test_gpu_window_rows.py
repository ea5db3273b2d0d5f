"""GPU tests of the windowed Muse.Run (muse_batch_run_rows_windowed / _run_row_ptrs_windowed / _run_group_rows_windowed and the
split-K kernels of xcorr_window_split.hip; run with -m gpu on an MI355X).

Expected values never come from the code under test: per series, the lag-window definition in include/muse_hip.h applied in numpy
(tests/_window.py) to the correlation slice `oracle.xcorr_with_x` returns; the group's winner, the rule of muse_batch_run_rows
(include/muse_hip.h) applied in numpy to those per-series pairs.  Tolerances are the project's: scores 1e-6 relative + 1e-12
absolute, NaN pattern equal, lags exact off rows the ORACLE flags as ties (two largest |cc| inside the window within 1e-12
relative); for the seeds used here the oracle flags no continuous-noise row at any window, which the tests assert of the oracle
alone.  MUSE_TEST_WORST=<file> appends the worst relative score error of every case (profiles/window_rows_parity.txt).

Figures of the test's own inputs, computed on the CPU from the oracle alone: in every M >= 15 case of test 1 between 5 of 17 and
30 of 50 rows have their global best lag outside L = 7 (asserted: at least a quarter -- a build that filters the unwindowed result
fails on each of them); over the continuous-noise rows
of every case of test 4 the two largest |clamped scores| differ by at least 9.4e-6 relative (asserted > 1e-7 before comparing)."""
import os
import subprocess
import threading

import numpy as np
import pytest

import _window as W
from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
SCORE_ATOL = 1e-12
WIN_KC = 1024
LENGTHS = [1025, 2048, 2049, 3000, 4096, 5000]    # odd stride + one-sample last chunk; whole chunks; padded lengths, partial pieces
MS = (1, 15, 16, 17, 50)                           # a lone row, a partial block, a block boundary, more than one block
LS = (0, 1, 7, 8, 15, 31, 63)


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


_CASES = {}


def case(oracle, N, M):
    """(ref, rows, exp[L] = (lag, mv, tie), glag, n) of make_case(N, M, seed=1000+N+M, scaled=False): computed once, never changed"""
    if (N, M) not in _CASES:
        ref, rows = W.make_case(N, M, seed=1000 + N + M, scaled=False)
        exp, glag, gmv, n = W.expect(oracle, ref, rows, LS)
        for a in (ref, rows, glag):
            a.setflags(write=False)
        _CASES[(N, M)] = (ref, rows, exp, glag, n)
    return _CASES[(N, M)]


def _record(tag, worst):
    path = os.environ.get("MUSE_TEST_WORST")
    if path:
        with open(path, "a") as f:
            f.write("%s %.3e\n" % (tag, worst))


def check(lag, mv, elag, emv, tie, tag=None):
    """scores to tolerance, NaN pattern equal, lags exact off the oracle's ties; returns the worst relative score error"""
    lag, mv, elag, emv, tie = map(np.asarray, (lag, mv, elag, emv, tie))
    nan_e = np.isnan(emv)
    assert np.array_equal(np.isnan(mv), nan_e), "NaN pattern: %s vs %s" % (np.nonzero(np.isnan(mv))[0][:8], np.nonzero(nan_e)[0][:8])
    ok = ~nan_e
    err = np.abs(mv[ok] - emv[ok])
    nz = np.abs(emv[ok]) > 0
    worst = float((err[nz] / np.abs(emv[ok][nz])).max()) if nz.any() else 0.0
    if tag:
        print("%s: worst score rel err %.3e, ties %d of %d" % (tag, worst, int(tie.sum()), len(tie)))
        _record(tag, worst)
    err = np.where(tie[ok], np.abs(np.abs(mv[ok]) - np.abs(emv[ok])), err)
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "score mismatch: worst rel %.3e" % worst
    bad = (lag != elag) & ~tie
    assert not bad.any(), "lag mismatches at rows %s: %s vs %s" % (np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    return worst


def winner(lag, mv, abs_scores):
    """muse_batch_run_rows's rule for one label group applied to per-row (lag, mv): (series, lag, score, state, gap) -- the member
    with the largest |clamped score| among the members whose score is a number, the first one on ties; state 2 when the first
    member scores NaN, 0 for no member; gap = relative distance between the two largest |clamped scores|"""
    if len(mv) == 0:
        return -1, 0, 0.0, 0, np.inf
    v = np.clip(mv, -1.0, 1.0)
    if abs_scores:
        v = np.abs(v)
    a = np.where(np.isnan(v), -1.0, np.abs(v))
    k = int(np.argmax(a))
    top = np.sort(a)[::-1]
    gap = (top[0] - top[1]) / top[0] if len(top) > 1 and top[0] > 0 else np.inf
    state = 2 if np.isnan(v[0]) else 1
    if a[k] < 0:
        return -1, 0, 0.0, state, gap
    return k, int(lag[k]), float(v[k]), state, gap


def assert_winner(got, want):
    rec, state = got
    k, lag, score, estate, gap = want
    assert state == estate
    if estate == 1:
        assert gap > 1e-7
        assert int(rec["series"]) == k and int(rec["lag"]) == lag
        assert abs(float(rec["score"]) - score) <= SCORE_RTOL * abs(score) + SCORE_ATOL


class forced:
    """the windowed Muse.Run of `eng` in S slices for the length of a with-block (0 = the planner)"""

    def __init__(self, eng, S, always_copy=False):
        self.eng, self.S, self.copy = eng, S, always_copy

    def __enter__(self):
        self.eng.window_rows_slices(self.S)
        self.eng.rows_always_copy(self.copy)

    def __exit__(self, *a):
        self.eng.window_rows_slices(0)
        self.eng.rows_always_copy(False)


def template(muse, eng, ref):
    probe = muse.DeviceGroup(eng, len(ref), 0)
    return muse.DeviceBatch(eng, probe, ref), probe


# ------------------------------------------------------------------ 1. per-row parity of the split kernels
@pytest.mark.parametrize("N", LENGTHS)
def test_split_parity(muse, eng, oracle, N):
    chunks = (N + WIN_KC - 1) // WIN_KC
    for M in MS:
        ref, rows, exp, glag, n = case(oracle, N, M)
        keep = W.plain_rows(M)
        if M >= 15:
            assert (np.abs(glag) > 7).sum() * 4 >= M           # a filter of the unwindowed result cannot pass
        tmpl, probe = template(muse, eng, ref)
        for L in LS:
            elag, emv, tie = exp[L]
            assert not tie[keep].any()                          # the oracle by itself yields no tie on continuous noise
            for S in sorted({2, min(3, chunks), chunks}):
                with forced(eng, S):
                    lag, mv = tmpl.run_rows_windowed_scores(rows, L)
                check(lag, mv, elag, emv, tie, tag="split N=%d M=%d L=%d S=%d" % (N, M, L, S) if M == MS[-1] else None)
                assert np.all(np.abs(lag) <= L)
        assert tmpl.lag_window() == -1
        tmpl.close()
        probe.close()


# ------------------------------------------------------------------ 2. one slice is today's kernel, bit for bit
@pytest.mark.parametrize("N", [2, 8, 100, 480, 1024, 4096])
def test_one_slice_is_the_batch_kernel(muse, eng, N):
    M = 40
    ref, rows = W.make_case(N, M, seed=2000 + N, scaled=False)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    tmpl, probe = template(muse, eng, ref)
    for L in (0, 7, 63):
        db.set_lag_window(L)
        blag, bmv = db.scores()
        for always_copy in (True, False):                       # the copied rows, and the zero-copy path (rows read from pinned memory)
            with forced(eng, 1, always_copy):
                lag, mv = tmpl.run_rows_windowed_scores(rows, L)
            assert lag.tobytes() == blag.tobytes() and mv.tobytes() == bmv.tobytes(), (N, L, always_copy)
        if N <= 1024:                                           # one chunk: the planner has nothing to split -- the same bits
            lag, mv = tmpl.run_rows_windowed_scores(rows, L)
            assert lag.tobytes() == blag.tobytes() and mv.tobytes() == bmv.tobytes()


# ------------------------------------------------------------------ 3. run to run
def test_split_is_deterministic(muse, eng, oracle):
    ref, rows, exp, _, _ = case(oracle, 5000, 50)
    tmpl, probe = template(muse, eng, ref)
    with forced(eng, 3):
        a = tmpl.run_rows_windowed_scores(rows, 15)
        b = tmpl.run_rows_windowed_scores(rows, 15)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    check(*a, *exp[15])


# ------------------------------------------------------------------ 4. winner and state
@pytest.mark.parametrize("N", LENGTHS)
def test_winner_and_state(muse, eng, oracle, N):
    M = 50
    ref, rows, exp, _, n = case(oracle, N, M)
    keep = W.plain_rows(M)
    plain = np.ascontiguousarray(rows[keep])
    K = len(plain)
    tmpl, probe = template(muse, eng, ref)
    src = muse.DeviceGroup.from_rows(eng, rows)                 # resident: the whole case; the lists name its plain rows
    at = np.nonzero(keep)[0].astype(np.int64)
    src32 = muse.DeviceGroup.from_rows(eng, plain, f32=True)
    exp32, _, _, _ = W.expect(oracle, ref, src32.read(0, K), (7, 31))
    rng = np.random.default_rng(N)
    perm = rng.integers(0, K, 60)                               # a permuted list with duplicates
    perm[1] = perm[0]
    for L in (7, 31):
        elag, emv, _ = exp[L]
        for S in (0, 2):
            for ab in (False, True):
                with forced(eng, S):
                    want = winner(elag[keep], emv[keep], ab)
                    assert_winner(tmpl.run_rows_windowed(plain, L, abs_scores=ab), want)
                    assert_winner(tmpl.run_row_ptrs_windowed([r.copy() for r in plain], L, abs_scores=ab), want)
                    # resident rows: an ascending contiguous run (scored where it lies), a permuted list, float32 storage
                    lo = int(at[5])
                    run = np.arange(lo, lo + 30, dtype=np.int64)
                    assert keep[run].all()
                    assert_winner(tmpl.run_group_rows_windowed(src, run, L, abs_scores=ab), winner(elag[run], emv[run], ab))
                    assert_winner(tmpl.run_group_rows_windowed(src, at[perm], L, abs_scores=ab),
                                  _with_duplicates(elag, emv, at[perm], ab))
                    e32 = exp32[L]
                    assert_winner(tmpl.run_group_rows_windowed(src32, np.arange(K), L, abs_scores=ab), winner(e32[0], e32[1], ab))
        # a group whose first member is the NaN row: state 2; no member: state 0
        with_nan = np.concatenate([rows[4:5], plain])
        assert np.isnan(with_nan[0]).any()
        for S in (0, 2):
            with forced(eng, S):
                rec, state = tmpl.run_rows_windowed(with_nan, L)
                assert state == 2
                rec, state = tmpl.run_rows_windowed(np.zeros((0, N)), L)
                assert state == 0 and int(rec["series"]) == -1
                rec, state = tmpl.run_group_rows_windowed(src, np.zeros(0, dtype=np.int64), L)
                assert state == 0
    assert tmpl.lag_window() == -1


def _with_duplicates(elag, emv, idx, ab):
    """a list with duplicates may name the winning row more than once: the first position attaining the maximum wins (np.argmax:
    the first maximum); the gap that has to be open is the one between DIFFERENT rows"""
    k, lag, score, state, _ = winner(elag[idx], emv[idx], ab)
    u = np.unique(idx)
    return k, lag, score, state, winner(elag[u], emv[u], ab)[4]


# ------------------------------------------------------------------ 5. many callers on one template
@pytest.mark.parametrize("M,N,S", [(50, 480, 0), (20, 5000, 0), (20, 5000, 3)])
def test_many_callers(muse, eng, oracle, M, N, S):
    ref, rows = W.make_case(N, M + 5, seed=3000 + N, scaled=False)
    rows = np.ascontiguousarray(rows[W.plain_rows(M + 5)])
    tmpl, probe = template(muse, eng, ref)
    with forced(eng, S):
        single = {L: tmpl.run_rows_windowed(rows, L) for L in (7, 15)}
        exp, _, _, _ = W.expect(oracle, ref, rows, (7, 15))
        for L in (7, 15):
            assert_winner(single[L], winner(exp[L][0], exp[L][1], False))
        bad = []

        def work(k):
            try:
                for i in range(20):
                    L = (7, 15)[(i + k) % 2]                      # windows alternate: the slot's table key changes
                    rec, state = tmpl.run_rows_windowed(rows, L)
                    if state != single[L][1] or rec.tobytes() != single[L][0].tobytes():
                        bad.append((k, i, L))
            except Exception as e:   # reported by the calling thread
                bad.append((k, repr(e)))
        threads = [threading.Thread(target=work, args=(k,)) for k in range(16)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not bad, bad[:5]


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handles_as_they_were(muse, eng, oracle):
    B = muse.binding
    N, M = 480, 20
    ref, rows = W.make_case(N, M + 5, seed=77, scaled=False)
    rows = np.ascontiguousarray(rows[W.plain_rows(M + 5)])
    tmpl, probe = template(muse, eng, ref)
    src = muse.DeviceGroup.from_rows(eng, rows)
    base = tmpl.run_rows(rows)

    def refused(status, fn, window=-1):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message
        assert tmpl.lag_window() == window
        if window < 0:
            again = tmpl.run_rows(rows)
            assert again[1] == base[1] and again[0].tobytes() == base[0].tobytes()

    forms = (lambda L: tmpl.run_rows_windowed(rows, L), lambda L: tmpl.run_row_ptrs_windowed(list(rows), L),
             lambda L: tmpl.run_group_rows_windowed(src, np.arange(M), L))
    for f in forms:
        refused(B.MUSE_ERR_INVALID, lambda: f(-1))
        refused(B.MUSE_ERR_UNSUPPORTED, lambda: f(B.MUSE_LAG_WINDOW_MAX + 1))
    refused(B.MUSE_ERR_LENGTH, lambda: tmpl.run_rows_windowed(rows[:, :N - 1].copy(), 7))
    short = muse.DeviceGroup.from_rows(eng, rows[:, :N - 1].copy())
    refused(B.MUSE_ERR_LENGTH, lambda: tmpl.run_group_rows_windowed(short, np.arange(3), 7))
    refused(B.MUSE_ERR_INVALID, lambda: tmpl.run_group_rows_windowed(src, np.array([0, M]), 7))
    # the template's own window: on and different is refused, on and equal is accepted; the unwindowed forms go on refusing it
    want = tmpl.run_rows_windowed(rows, 7)
    tmpl.set_lag_window(15)
    for f in forms:
        refused(B.MUSE_ERR_INVALID, lambda: f(7), window=15)
    refused(B.MUSE_ERR_UNSUPPORTED, lambda: tmpl.run_rows(rows), window=15)
    tmpl.set_lag_window(7)
    for f in forms:
        got = f(7)
        assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()
    assert tmpl.lag_window() == 7
    tmpl.set_lag_window(-1)
    again = tmpl.run_rows(rows)
    assert again[1] == base[1] and again[0].tobytes() == base[0].tobytes()
    exp, _, _, _ = W.expect(oracle, ref, rows, (7,))
    assert_winner(want, winner(exp[7][0], exp[7][1], False))
    # series longer than 65536 samples
    Nh = 70000
    rng = np.random.default_rng(4)
    refh, rowsh = rng.standard_normal(Nh), rng.standard_normal((3, Nh))
    th, ph = template(muse, eng, refh)
    baseh = th.run_rows(rowsh)
    with pytest.raises(muse.MuseError) as e:
        th.run_rows_windowed(rowsh, 7)
    assert e.value.status == B.MUSE_ERR_UNSUPPORTED
    againh = th.run_rows(rowsh)
    assert th.lag_window() == -1 and againh[1] == baseh[1] and againh[0].tobytes() == baseh[0].tobytes()


# ------------------------------------------------------------------ 7. mirrors
def _lcg_series(N, i):
    """host/muse_rows_window_test.cpp's series(), bit for bit (32-bit LCG, exact arithmetic)"""
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


@pytest.fixture(scope="module")
def mirror_case(muse, oracle):
    """three label groups of 6 x 480 and what a Results fed from the oracle Fetches: windowed (L = 15) and today's"""
    N, G, K, L = 480, 3, 6, 15
    ref = _lcg_series(N, -1)
    rows = np.stack([_lcg_series(N, i) for i in range(G * K)])
    exp, glag, gmv, n = W.expect(oracle, ref, rows, (L,))
    assert not exp[L][2].any()
    assert (np.abs(glag) > L).sum() * 4 >= G * K

    def fetch(lag, mv):
        res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
        for g in range(G):
            k, wl, ws, state, gap = winner(lag[g * K:(g + 1) * K], mv[g * K:(g + 1) * K], False)
            assert state == 1 and gap > 1e-7
            res.Update(muse.Score(muse.NewLabels({"id": str(g * K + k)}), wl, ws))
        return [(s.Labels.labels["id"], s.Lag, s.PercentScore) for s in res.Fetch()[0]]
    want_win, want_run = fetch(exp[L][0], exp[L][1]), fetch(glag, gmv)
    assert len(want_win) >= 1 and want_win != want_run
    return N, G, K, L, ref, rows, want_win, want_run


def _assert_fetch(got, want):
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
    assert np.allclose([g[2] for g in got], [w[2] for w in want], rtol=SCORE_RTOL, atol=SCORE_ATOL)


def test_python_muse_run_windowed(muse, eng, mirror_case):
    N, G, K, L, ref, rows, want_win, want_run = mirror_case
    series = [muse.NewSeries(rows[i], muse.NewLabels({"id": str(i), "graph": "g%d" % (i // K)})) for i in range(G * K)]
    refs = muse.NewSeries(ref, muse.NewLabels({"id": "ref"}))

    def fetched(res):
        return [(s.Labels.labels["id"], s.Lag, s.PercentScore) for s in res.Fetch()[0]]
    res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
    m = muse.New(refs, res, engine=eng)
    for g in range(G):
        m.RunWindowed(series[g * K:(g + 1) * K])
    _assert_fetch(fetched(res), want_win)
    for g in range(G):                                          # Run on the same object afterwards is today's
        m.Run(series[g * K:(g + 1) * K])
    today = fetched(res)
    _assert_fetch(today, want_run)
    fresh_res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
    fresh = muse.New(refs, fresh_res, engine=eng)
    for g in range(G):
        fresh.Run(series[g * K:(g + 1) * K])
    assert fetched(fresh_res) == today
    # the same with the series resident in one group on the engine (scored where they lie), reuse on and off
    comp = muse.NewGroup("all")
    comp.Add(*series)
    muse.NewBatch(refs, comp, muse.NewResults(L, 5, 0.0, muse.SignFilter_ANY), 4, engine=eng).Run(None)
    assert m._resident(series[:K]) is not None
    for on in (True, False):
        eng.reuse_resident_rows(on)
        try:
            for g in range(G):
                m.RunWindowed(series[g * K:(g + 1) * K])
            _assert_fetch(fetched(res), want_win)
        finally:
            eng.reuse_resident_rows(True)
    # a window outside the cap
    wide = muse.New(refs, muse.NewResults(muse.binding.MUSE_LAG_WINDOW_MAX + 1, 12, 0.0, muse.SignFilter_ANY), engine=eng)
    with pytest.raises(muse.MuseError) as e:
        wide.RunWindowed(series[:K])
    assert e.value.status == muse.binding.MUSE_ERR_UNSUPPORTED


def test_cpp_muse_run_windowed(muse, mirror_case):
    N, G, K, L, ref, rows, want_win, want_run = mirror_case
    exe = muse.build.build_rows_window_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rows window ok" in r.stdout, r.stdout + r.stderr
    for tag, want in (("win", want_win), ("run", want_run)):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(tag + " ")]
        _assert_fetch([(l[1], int(l[2]), float(l[3])) for l in lines], want)


# ------------------------------------------------------------------ 8. groups too large for a slot
def test_general_path_just_above_the_slot_limit(muse, eng, oracle):
    N, M = 4096, 4100                                           # 4100 x 4096 > 2^24 elements (ROWS_SLOT_MAX_ELEMS)
    L = 15
    ref, rows = W.make_case(N, M + 5, seed=8, scaled=False)
    rows = np.ascontiguousarray(rows[W.plain_rows(M + 5)])
    assert rows.shape[0] == M and M * N > 1 << 24
    tmpl, probe = template(muse, eng, ref)
    lag, mv = tmpl.run_rows_windowed_scores(rows, L)
    rec, state = tmpl.run_rows_windowed(rows, L)
    assert tmpl.lag_window() == -1
    pick = np.sort(np.random.default_rng(9).choice(M, 64, replace=False))
    exp, _, _, _ = W.expect(oracle, ref, rows[pick], (L,))
    check(lag[pick], mv[pick], *exp[L], tag="general 4100x4096 L=15")
    # the winner: the record is the group rule applied to the call's own per-row pairs, and its row checks out against the oracle
    k, wl, ws, estate, gap = winner(lag, mv, False)
    assert state == estate == 1 and int(rec["series"]) == k and int(rec["lag"]) == wl and float(rec["score"]) == ws
    ew, _, _, _ = W.expect(oracle, ref, rows[k:k + 1], (L,))
    check(lag[k:k + 1], mv[k:k + 1], *ew[L])
    src = muse.DeviceGroup.from_rows(eng, rows)
    rec2, state2 = tmpl.run_group_rows_windowed(src, np.arange(M)[::-1].copy(), L)
    assert state2 == 1 and int(rec2["lag"]) == wl and abs(float(rec2["score"]) - ws) <= SCORE_RTOL * abs(ws) + SCORE_ATOL
