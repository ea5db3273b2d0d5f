"""GPU tests of Muse.Run inside a lag range (muse_batch_run_rows_in_lag_range / _run_row_ptrs_in_lag_range /
_run_group_rows_in_lag_range and the panel kernels of xcorr_window_panels.hip; run with -m gpu on an MI355X).

Expected values never come from the code under test: per series, the lag-range definition in include/muse_hip.h applied in numpy
(tests/_lagrange.py) to the correlation slice `oracle.xcorr_with_x` returns; the group's winner, the rule of muse_batch_run_rows
applied in numpy to those per-series pairs.  Tolerances are the project's: scores 1e-6 relative + 1e-12 absolute, NaN pattern equal,
lags exact on EVERY row: tests/test_rows_lag_range_cpu.py asserts, on exactly these inputs (tests/_rowslagrange.py), that the oracle
flags no tie inside any tested range.  Every case carries a NaN row, a constant row, a quiet row of two opposite impulses and a row
that starts 50 sigma off; a row whose range holds exact zeros only needs a reference that is exactly zero off its pulses and has a
case of its own (test_a_range_of_exact_zeros): the transform oracle leaves rounding noise where the direct product sums zeros."""
import subprocess
import threading

import numpy as np
import pytest

import _lagrange as LR
import _rowslagrange as RL
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


def check(lag, mv, elag, emv, tie, tag=None):
    """scores to tolerance, NaN pattern equal, lags exact on every row (the oracle flags no tie: asserted here too)"""
    lag, mv, elag, emv, tie = map(np.asarray, (lag, mv, elag, emv, tie))
    assert not tie.any()
    nan_e = np.isnan(emv)
    assert np.array_equal(np.isnan(mv), nan_e), "NaN pattern: %s vs %s" % (np.nonzero(np.isnan(mv))[0][:8], np.nonzero(nan_e)[0][:8])
    ok = ~nan_e
    err = np.abs(mv[ok] - emv[ok])
    nz = np.abs(emv[ok]) > 0
    worst = float((err[nz] / np.abs(emv[ok][nz])).max()) if nz.any() else 0.0
    if tag:
        print("%s: worst score rel err %.3e" % (tag, worst))
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "%s score mismatch: worst rel %.3e" % (tag, worst)
    bad = lag != elag
    assert not bad.any(), "%s lag mismatches at rows %s: %s vs %s" % (tag, np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    return worst


def winner(lag, mv, abs_scores):
    """muse_batch_run_rows's rule for one label group applied to per-row (lag, mv): (series, lag, score, state, gap)"""
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
    """the slice count of the windowed Muse.Run of `eng` for the length of a with-block (0 = the planner)"""

    def __init__(self, eng, S):
        self.eng, self.S = eng, S

    def __enter__(self):
        self.eng.window_rows_slices(self.S)

    def __exit__(self, *a):
        self.eng.window_rows_slices(0)


def template(muse, eng, ref):
    probe = muse.DeviceGroup(eng, len(ref), 0)
    return muse.DeviceBatch(eng, probe, ref), probe


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------ 1. parity through the scores hook
@pytest.mark.parametrize("N", [c[0] for c in RL.PARITY])
def test_parity(muse, eng, oracle, N):
    _, M, ranges, slices = [c for c in RL.PARITY if c[0] == N][0]
    ref, rows, exp, n = RL.parity_case(oracle, N)
    tmpl, probe = template(muse, eng, ref)
    for lo, hi in ranges:
        path, panels, S0 = muse.rows_lag_range_plan(rows.shape[0], N, eng.device_info()[1], lo, hi)
        assert path == RL.PANELS and panels == -(-(hi - lo + 1) // 128)
        for S in slices:
            with forced(eng, S):
                lag, mv = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
            check(lag, mv, *exp[(lo, hi)], tag="panels N=%d M=%d [%d, %d] S=%d (planner %d)" % (N, rows.shape[0], lo, hi, S, S0))
            assert np.all((lag >= lo) & (lag <= hi))
    assert tmpl.lag_window() == -1
    tmpl.close()
    probe.close()


def test_a_range_of_exact_zeros(muse, eng, oracle):
    ref, rows, zr = RL.zeros_case()
    lo, hi = RL.ZEROS[1]
    exp, _, _, _ = LR.expect(oracle, ref, rows[:zr], ((lo, hi),))
    tmpl, probe = template(muse, eng, ref)
    for S in (1, 3):
        with forced(eng, S):
            lag, mv = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
        check(lag[:zr], mv[:zr], *exp[(lo, hi)], tag="zeros S=%d" % S)
        assert lag[zr] == 0 and mv[zr] == 0.0          # only zeros in the range: index 0 stands, (0, cc[0])


# ------------------------------------------------------------------ 2. narrow ranges: the existing kernels, from any origin
@pytest.mark.parametrize("N", RL.NARROW_NS)
def test_narrow_ranges(muse, eng, oracle, N):
    ref, rows, exp, n = RL.narrow_case(oracle, N)
    chunks = (N + RL.WIN_KC - 1) // RL.WIN_KC
    tmpl, probe = template(muse, eng, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for lo, hi in RL.NARROW_RANGES:
        assert muse.rows_lag_range_plan(rows.shape[0], N, eng.device_info()[1], lo, hi)[0] in (RL.WINDOW, RL.SPLIT)
        blag, bmv = db.scores_in_lag_range(lo, hi)
        check(blag, bmv, *exp[(lo, hi)])
        for S in sorted({0, 1, 2, min(3, chunks)}):
            with forced(eng, S):
                got = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
            check(*got, *exp[(lo, hi)], tag="narrow N=%d [%d, %d] S=%d" % (N, lo, hi, S))
            if S == 1:                                # one slice: the batch's direct product, bit for bit
                assert same_bytes(got, (blag, bmv)), (N, lo, hi)
    # a symmetric range IS the windowed call, at every S
    L = RL.NARROW_L
    for S in sorted({0, 1, 2, min(3, chunks)}):
        with forced(eng, S):
            a = tmpl.run_rows_in_lag_range_scores(rows, -L, L)
            b = tmpl.run_rows_windowed_scores(rows, L)
        assert same_bytes(a, b), (N, S)
        check(*a, *exp[L])
    assert tmpl.lag_window() == -1


# ------------------------------------------------------------------ 3. the same bits whichever panel holds the lag
def test_same_bits_across_panels(muse, eng, oracle):
    N, M, wide, narrow = RL.ACROSS
    assert N % 2 == 0
    ref, rows, exp, n = RL.across_case(oracle)
    tmpl, probe = template(muse, eng, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    nlag, nmv = db.scores_in_lag_range(*narrow)
    with forced(eng, 1):
        lag, mv = tmpl.run_rows_in_lag_range_scores(rows, *wide)
    check(lag, mv, *exp[wide])
    inside = (lag >= narrow[0]) & (lag <= narrow[1]) & np.isfinite(mv) & (mv != 0)
    assert inside.sum() >= 1
    assert np.array_equal(lag[inside], nlag[inside]) and mv[inside].tobytes() == nmv[inside].tobytes()


# ------------------------------------------------------------------ 4. run to run
def test_panels_are_deterministic(muse, eng, oracle):
    ref, rows, exp, n = RL.parity_case(oracle, 5000)
    lo, hi = RL.PARITY[4][2][0]
    tmpl, probe = template(muse, eng, ref)
    with forced(eng, 3):
        a = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
        b = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
    assert same_bytes(a, b)
    check(*a, *exp[(lo, hi)])


# ------------------------------------------------------------------ 5. winner and state
def test_winner_and_state(muse, eng, oracle):
    N, M, ranges = RL.WINNER
    ref, rows, exp, n = RL.winner_case(oracle)
    keep = RL.plain_rows(M)
    plain = np.ascontiguousarray(rows[keep])
    K = len(plain)
    tmpl, probe = template(muse, eng, ref)
    src = muse.DeviceGroup.from_rows(eng, rows)
    at = np.nonzero(keep)[0].astype(np.int64)
    src32 = muse.DeviceGroup.from_rows(eng, plain, f32=True)
    exp32, _, _, _ = LR.expect(oracle, ref, src32.read(0, K), ranges)
    strided = np.zeros((K, N + 6))
    strided[:, :N] = plain
    perm = np.random.default_rng(N).permutation(K)[:20]
    for k in ranges:
        lo, hi = k
        elag, emv, _ = exp[k]
        assert not exp32[k][2].any()
        for S in (0, 2):
            for ab in (False, True):
                with forced(eng, S):
                    want = winner(elag[keep], emv[keep], ab)
                    assert_winner(tmpl.run_rows_in_lag_range(plain, lo, hi, abs_scores=ab), want)
                    assert_winner(tmpl.run_rows_in_lag_range(strided[:, :N], lo, hi, abs_scores=ab), want)      # a row stride
                    assert_winner(tmpl.run_row_ptrs_in_lag_range([r.copy() for r in plain], lo, hi, abs_scores=ab), want)
                    # resident rows: an ascending contiguous run (scored where it lies), a permuted list, float32 storage
                    run = np.arange(2, 22, dtype=np.int64)
                    assert keep[run].all()
                    assert_winner(tmpl.run_group_rows_in_lag_range(src, run, lo, hi, abs_scores=ab), winner(elag[run], emv[run], ab))
                    assert_winner(tmpl.run_group_rows_in_lag_range(src, at[perm], lo, hi, abs_scores=ab),
                                  winner(elag[at[perm]], emv[at[perm]], ab))
                    e32 = exp32[k]
                    assert_winner(tmpl.run_group_rows_in_lag_range(src32, np.arange(K), lo, hi, abs_scores=ab), winner(e32[0], e32[1], ab))
        # a group whose first member is the NaN row: state 2; no member: state 0
        with_nan = np.concatenate([rows[M:M + 1], plain])
        assert np.isnan(with_nan[0]).any()
        rec, state = tmpl.run_rows_in_lag_range(with_nan, lo, hi)
        assert state == 2
        rec, state = tmpl.run_rows_in_lag_range(np.zeros((0, N)), lo, hi)
        assert state == 0 and int(rec["series"]) == -1
        rec, state = tmpl.run_group_rows_in_lag_range(src, np.zeros(0, dtype=np.int64), lo, hi)
        assert state == 0
    assert tmpl.lag_window() == -1


# ------------------------------------------------------------------ 6. the slot's table cache
def test_table_cache(muse, eng, oracle):
    N, M, ranges = RL.CACHE
    ref, rows, exp, n = RL.cache_case(oracle, 0)
    ref2, rows2, exp2, _ = RL.cache_case(oracle, 1)
    tmpl, probe = template(muse, eng, ref)
    tmpl2, probe2 = template(muse, eng, ref2)
    order = [ranges[0], ranges[1], ranges[2], ranges[1], ranges[0], ranges[0], ranges[2], ranges[1]]
    for k in order:                                     # the same W at another origin, a narrow table in between
        check(*tmpl.run_rows_in_lag_range_scores(rows, *k), *exp[k], tag="cache [%d, %d]" % k)
    for k in order[:4]:                                 # another reference: the same keys must not serve it
        check(*tmpl2.run_rows_in_lag_range_scores(rows2, *k), *exp2[k], tag="cache, second reference [%d, %d]" % k)
        check(*tmpl.run_rows_in_lag_range_scores(rows, *k), *exp[k])


# ------------------------------------------------------------------ 7. many callers on one template
def test_many_callers(muse, eng, oracle):
    N, M, ranges = RL.CALLERS
    ref, rows, exp, n = RL.callers_case(oracle)
    tmpl, probe = template(muse, eng, ref)
    single = {}
    for k in ranges:
        single[k] = tmpl.run_rows_in_lag_range_scores(rows, *k)
        check(*single[k], *exp[k])
    bad = []

    def work(t):
        try:
            for i in range(12):
                k = ranges[(i + t) % len(ranges)]       # ranges alternate: the slot's table key changes
                got = tmpl.run_rows_in_lag_range_scores(rows, *k)
                if not same_bytes(got, single[k]):
                    bad.append((t, i, k))
        except Exception as e:   # reported by the calling thread
            bad.append((t, repr(e)))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad[:5]


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handles_as_they_were(muse, eng, oracle):
    B = muse.binding
    ref, rows, exp, n = RL.parity_case(oracle, 5000)
    N = 5000
    good = RL.PARITY[4][2][0]
    tmpl, probe = template(muse, eng, ref)
    src = muse.DeviceGroup.from_rows(eng, rows)
    idx = np.arange(rows.shape[0])

    def refused(status, fn, window=-1, t=tmpl):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status and e.value.message
        assert t.lag_window() == window

    forms = (lambda lo, hi: tmpl.run_rows_in_lag_range(rows, lo, hi), lambda lo, hi: tmpl.run_row_ptrs_in_lag_range(list(rows), lo, hi),
             lambda lo, hi: tmpl.run_group_rows_in_lag_range(src, idx, lo, hi),
             lambda lo, hi: tmpl.run_rows_in_lag_range_scores(rows, lo, hi))
    for f in forms:
        refused(B.MUSE_ERR_INVALID, lambda: f(1, 7))
        refused(B.MUSE_ERR_INVALID, lambda: f(-7, -1))
        refused(B.MUSE_ERR_UNSUPPORTED, lambda: f(0, 2048))                 # 2049 lags
        refused(B.MUSE_ERR_UNSUPPORTED, lambda: f(-1024, 1024))
        check(*tmpl.run_rows_in_lag_range_scores(rows, *good), *exp[good])  # a good call behind every refusal
    refused(B.MUSE_ERR_LENGTH, lambda: tmpl.run_rows_in_lag_range(rows[:, :N - 1].copy(), -200, 50))
    refused(B.MUSE_ERR_INVALID, lambda: tmpl.run_group_rows_in_lag_range(src, np.array([0, rows.shape[0]]), -200, 50))
    # the template's own window: on and not this range is refused, on and equal to a symmetric range is accepted
    want = tmpl.run_rows_in_lag_range_scores(rows, -7, 7)
    tmpl.set_lag_window(7)
    for f in forms:
        refused(B.MUSE_ERR_INVALID, lambda: f(-7, 8), window=7)
        refused(B.MUSE_ERR_INVALID, lambda: f(-200, 50), window=7)
    assert same_bytes(tmpl.run_rows_in_lag_range_scores(rows, -7, 7), want) and tmpl.lag_window() == 7
    tmpl.set_lag_window(-1)
    check(*tmpl.run_rows_in_lag_range_scores(rows, *good), *exp[good])
    # series longer than 65536 samples: every lag is the unwindowed call, anything else is not built
    Nh = 70000
    rng = np.random.default_rng(4)
    refh, rowsh = rng.standard_normal(Nh), rng.standard_normal((3, Nh))
    th, ph = template(muse, eng, refh)
    baseh = th.run_rows(rowsh)
    refused(B.MUSE_ERR_UNSUPPORTED, lambda: th.run_rows_in_lag_range(rowsh, -200, 50), t=th)
    refused(B.MUSE_ERR_UNSUPPORTED, lambda: th.run_rows_in_lag_range(rowsh, -7, 0), t=th)
    againh = th.run_rows_in_lag_range(rowsh, -(1 << 30), 1 << 30)
    assert againh[1] == baseh[1] and againh[0].tobytes() == baseh[0].tobytes()
    againh = th.run_rows(rowsh)
    assert th.lag_window() == -1 and againh[1] == baseh[1] and againh[0].tobytes() == baseh[0].tobytes()


def test_every_lag_is_the_unwindowed_call(muse, eng, oracle):
    ref, rows, exp, n = RL.parity_case(oracle, 300)
    keep = RL.plain_rows(rows.shape[0] - RL.SPECIALS)
    plain = np.ascontiguousarray(rows[keep])
    tmpl, probe = template(muse, eng, ref)
    base = tmpl.run_rows(plain)
    for lo, hi in ((-255, 256), (-5000, 5000)):
        got = tmpl.run_rows_in_lag_range(plain, lo, hi)
        assert got[1] == base[1] and got[0].tobytes() == base[0].tobytes()


# ------------------------------------------------------------------ 9. groups too large for a slot
def test_general_path_just_above_the_slot_limit(muse, eng, oracle):
    N, M, (lo, hi), K = RL.GENERAL
    ref, rows, pick = RL.general_case()
    assert rows.shape == (M, N) and M * N > 1 << 24
    tmpl, probe = template(muse, eng, ref)
    lag, mv = tmpl.run_rows_in_lag_range_scores(rows, lo, hi)
    rec, state = tmpl.run_rows_in_lag_range(rows, lo, hi)
    assert tmpl.lag_window() == -1
    exp, _, _, _ = LR.expect(oracle, ref, rows[pick], ((lo, hi),))
    check(lag[pick], mv[pick], *exp[(lo, hi)], tag="general %dx%d [%d, %d]" % (M, N, lo, hi))
    assert np.all((lag >= lo) & (lag <= hi))
    # the winner: the record is the group rule applied to the call's own per-row pairs, and its row checks out against the oracle
    k, wl, ws, estate, gap = winner(lag, mv, False)
    assert state == estate == 1 and int(rec["series"]) == k and int(rec["lag"]) == wl and float(rec["score"]) == ws
    ew, _, _, _ = LR.expect(oracle, ref, rows[k:k + 1], ((lo, hi),))
    check(lag[k:k + 1], mv[k:k + 1], *ew[(lo, hi)])
    src = muse.DeviceGroup.from_rows(eng, rows)
    rec2, state2 = tmpl.run_group_rows_in_lag_range(src, np.arange(M)[::-1].copy(), lo, hi)
    assert state2 == 1 and int(rec2["lag"]) == wl and abs(float(rec2["score"]) - ws) <= SCORE_RTOL * abs(ws) + SCORE_ATOL


# ------------------------------------------------------------------ 10. mirrors
@pytest.fixture(scope="module")
def mirror_case(muse, oracle):
    """three label groups of 6 x 2500 and what a Results fed from the oracle Fetches, per range and for today's Run"""
    N, G, K, ranges, maxlag = RL.MIRROR
    ref, rows = RL.mirror_series()
    exp, glag, gmv, n = LR.expect(oracle, ref, rows, ranges)

    def fetch(lag, mv):
        res = muse.NewResults(maxlag, 12, 0.0, muse.SignFilter_ANY)
        for g in range(G):
            k, wl, ws, state, gap = winner(lag[g * K:(g + 1) * K], mv[g * K:(g + 1) * K], False)
            assert state == 1 and gap > 1e-7
            res.Update(muse.Score(muse.NewLabels({"id": str(g * K + k)}), wl, ws))
        return [(s.Labels.labels["id"], s.Lag, s.PercentScore) for s in res.Fetch()[0]]
    want = {k: fetch(exp[k][0], exp[k][1]) for k in ranges}
    want_run = fetch(glag, gmv)
    assert all(len(w) >= 1 and w != want_run for w in want.values())
    return N, G, K, ranges, maxlag, ref, rows, want, want_run


def _assert_fetch(got, want):
    assert [(g[0], g[1]) for g in got] == [(w[0], w[1]) for w in want]
    assert np.allclose([g[2] for g in got], [w[2] for w in want], rtol=SCORE_RTOL, atol=SCORE_ATOL)


def test_python_muse_run_in_lag_range(muse, eng, mirror_case):
    N, G, K, ranges, maxlag, ref, rows, want, want_run = mirror_case
    series = [muse.NewSeries(rows[i], muse.NewLabels({"id": str(i), "graph": "g%d" % (i // K)})) for i in range(G * K)]
    refs = muse.NewSeries(ref, muse.NewLabels({"id": "ref"}))

    def fetched(res):
        return [(s.Labels.labels["id"], s.Lag, s.PercentScore) for s in res.Fetch()[0]]
    res = muse.NewResults(maxlag, 12, 0.0, muse.SignFilter_ANY)
    m = muse.New(refs, res, engine=eng)
    for k in ranges:
        for g in range(G):
            m.RunInLagRange(series[g * K:(g + 1) * K], *k)
        _assert_fetch(fetched(res), want[k])
    for g in range(G):                                          # Run on the same object afterwards is today's
        m.Run(series[g * K:(g + 1) * K])
    _assert_fetch(fetched(res), want_run)
    # the same with the series resident in one group on the engine (scored where they lie), reuse on and off
    comp = muse.NewGroup("all")
    comp.Add(*series)
    muse.NewBatch(refs, comp, muse.NewResults(maxlag, 5, 0.0, muse.SignFilter_ANY), 4, engine=eng).Run(None)
    assert m._resident(series[:K]) is not None
    for on in (True, False):
        eng.reuse_resident_rows(on)
        try:
            for k in ranges:
                for g in range(G):
                    m.RunInLagRange(series[g * K:(g + 1) * K], *k)
                _assert_fetch(fetched(res), want[k])
        finally:
            eng.reuse_resident_rows(True)
    with pytest.raises(muse.MuseError) as e:
        m.RunInLagRange(series[:K], 1, 7)
    assert e.value.status == muse.binding.MUSE_ERR_INVALID


def test_cpp_muse_run_in_lag_range(muse, mirror_case):
    N, G, K, ranges, maxlag, ref, rows, want, want_run = mirror_case
    exe = muse.build.build_rows_lag_range_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rows lag range ok" in r.stdout, r.stdout + r.stderr
    for tag, w in (("narrow", want[ranges[0]]), ("wide", want[ranges[1]]), ("run", want_run)):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(tag + " ")]
        _assert_fetch([(l[1], int(l[2]), float(l[3])) for l in lines], w)
