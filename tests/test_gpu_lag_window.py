"""GPU tests of the lag window (muse_batch_set_lag_window, run with -m gpu on an MI355X): the best match INSIDE +-L lags from the
direct fp64 matrix-product kernel (xcorr_window.hip), through the C ABI.

Expected values never come from the code under test: per series, the definition in include/muse_hip.h applied in numpy
(tests/_window.py) to the correlation slice `oracle.xcorr_with_x` returns; Runs, `oracle.results` fed with those windowed
(lag, mv).  Tolerances are the project's (tests/test_gpu_parity.py): scores 1e-6 relative + 1e-12 absolute,
NaN pattern equal, lags exact except rows whose two largest |cc| INSIDE THE WINDOW lie within 1e-12 relative of each other
(taken from the oracle's cc); such rows may be at most 1 in 1000 of a case's continuous-noise rows.  One length is exempt from
that cap, by arithmetic and not by measurement: at N = 2 a z-normalised series is +-(1, -1) / sqrt 2, so cc[1] = -cc[0] for
EVERY pair of series -- each row is a tie of the two lags the moment the window holds both (L >= 1), in the reference too.
MUSE_TEST_WORST=<file> appends the worst relative score error of every case (profiles/window_parity.txt)."""
import os
import subprocess

import numpy as np
import pytest

import _window as W
from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
SCORE_ATOL = 1e-12
LS = (0, 1, 7, 8, 15, 16, 31, 63) + (32, 40, 48)   # (the last three: the 5-, 6- and 7-tile builds of the kernel)


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


def _record(tag, worst):
    path = os.environ.get("MUSE_TEST_WORST")
    if path:
        with open(path, "a") as f:
            f.write("%s %.3e\n" % (tag, worst))


def check(lag, mv, elag, emv, tie, keep=None, cap_ties=True, tag=None):
    """scores to tolerance, NaN pattern equal, lags exact off the oracle's ties; returns the worst relative score error"""
    lag, mv, elag, emv, tie = map(np.asarray, (lag, mv, elag, emv, tie))
    nan_e = np.isnan(emv)
    assert np.array_equal(np.isnan(mv), nan_e), "NaN pattern: %s vs %s" % (np.nonzero(np.isnan(mv))[0][:8], np.nonzero(nan_e)[0][:8])
    ok = ~nan_e
    err = np.abs(mv[ok] - emv[ok])
    rel = err / np.maximum(np.abs(emv[ok]), 1e-300)
    worst = float(rel[np.abs(emv[ok]) > 0].max()) if (np.abs(emv[ok]) > 0).any() else 0.0
    if tag:
        print("%s: worst score rel err %.3e, ties %d of %d" % (tag, worst, int(tie.sum()), len(tie)))
        _record(tag, worst)
    # (a tie between lags of opposite sign -- N = 2 -- may resolve to either value: compared by magnitude there)
    err = np.where(tie[ok], np.abs(np.abs(mv[ok]) - np.abs(emv[ok])), err)
    assert np.all(err <= SCORE_RTOL * np.abs(emv[ok]) + SCORE_ATOL), "score mismatch: worst rel %.3e" % worst
    bad = (lag != elag) & ~tie
    assert not bad.any(), "lag mismatches at rows %s: %s vs %s" % (np.nonzero(bad)[0][:10], lag[bad][:10], elag[bad][:10])
    if cap_ties:
        plain = tie if keep is None else tie & keep
        assert int(plain.sum()) * 1000 <= len(tie), "%d tied rows of %d" % (int(plain.sum()), len(tie))
    return worst


# ------------------------------------------------------------------ 1. per-series parity
LENGTHS = [512, 1024, 4096, 8192, 65536, 480, 1433, 5000, 20000, 40000, 2, 3, 8, 100, 255]


@pytest.mark.parametrize("N", LENGTHS)
def test_window_parity(muse, eng, oracle, N):
    """every window against the oracle-derived expectation, block counts with partial 16-row blocks, N = n, N < n and tiny
    lengths (L clipped to n / 2); at least a quarter of the rows have their global winner outside the window and a quarter
    inside wherever the window leaves room for both: at every length from 480 on, and from N = 100 on while 8 L < n (below
    that a series has too few lags for a pulse to be placed at will: N = 2 has two, and they tie)"""
    Ms = (1, 15, 16, 17, 1001) if N <= 8192 else (1, 15, 16, 17, 49)
    ref, rows = W.make_case(N, Ms[-1], seed=N)
    exp, glag, gmv, n = W.expect(oracle, ref, rows, LS)
    keep = W.plain_rows(Ms[-1])
    for L in LS:
        if N >= 480 or (N >= 100 and 8 * L < n):
            inside = np.abs(glag) <= min(L, n // 2)
            assert (inside & keep).sum() * 4 >= Ms[-1] and (~inside & keep).sum() * 4 >= Ms[-1], (N, L)
    for M in Ms:
        dg = muse.DeviceGroup.from_rows(eng, rows[:M])
        db = muse.DeviceBatch(eng, dg, ref)
        assert db.n == n
        for L in LS:
            db.set_lag_window(L)
            assert db.lag_window() == L
            lag, mv = db.scores()
            elag, emv, tie = exp[L]
            check(lag, mv, elag[:M], emv[:M], tie[:M], keep[:M], cap_ties=(N != 2 and M >= 1000),
                  tag="parity N=%d M=%d L=%d" % (N, M, L) if M == Ms[-1] else None)
            assert np.all(np.abs(lag) <= min(L, n // 2))
            if N != 2:
                assert not (tie[:M] & keep[:M]).any()      # continuous noise: the oracle by itself yields no tie
        name = eng.kernel_name(db)
        assert name.startswith("xcorr_window_mfma"), name
        db.close()
        dg.close()


# ------------------------------------------------------------------ 2. consistency with today's pass
@pytest.mark.parametrize("N", [480, 4096, 5000])
def test_rows_won_inside_the_window_equal_todays_pass(muse, eng, oracle, N):
    M = 300
    ref, rows = W.make_case(N, M, seed=7 * N)
    exp, glag, gmv, n = W.expect(oracle, ref, rows, LS)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    plain = muse.DeviceBatch(eng, dg, ref)
    plag, pmv = plain.scores()
    db = muse.DeviceBatch(eng, dg, ref)
    for L in LS:
        db.set_lag_window(L)
        lag, mv = db.scores()
        inside = (np.abs(glag) <= L) & ~np.isnan(gmv) & ~exp[L][2]
        assert inside.sum() >= M // 4
        assert np.array_equal(lag[inside], plag[inside])
        assert np.all(np.abs(mv[inside] - pmv[inside]) <= SCORE_RTOL * np.abs(pmv[inside]) + SCORE_ATOL)
    # L >= n / 2: today's result for every row
    if n // 2 <= muse.binding.MUSE_LAG_WINDOW_MAX:
        db.set_lag_window(n // 2)
        lag, mv = db.scores()
        assert np.array_equal(lag, plag)


# ------------------------------------------------------------------ 3. off is off
def test_off_is_off_and_passes_repeat(muse, eng, oracle):
    N, M = 4096, 333
    ref, rows = W.make_case(N, M + 40, seed=99)
    dg = muse.DeviceGroup.from_rows(eng, rows[:M])
    never = muse.DeviceBatch(eng, dg, ref)
    nlag, nmv = never.scores()
    db = muse.DeviceBatch(eng, dg, ref)
    assert db.lag_window() == -1
    db.set_lag_window(15)
    a = db.scores()
    b = db.scores()
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()      # two windowed passes: bit-identical
    assert not np.array_equal(a[0], nlag)                                       # (and not today's result)
    db.set_lag_window(-1)
    assert db.lag_window() == -1
    lag, mv = db.scores()
    assert np.array_equal(lag, nlag) and mv.tobytes() == nmv.tobytes()          # off: bit-identical to a batch that never had one
    assert not eng.kernel_name(db).startswith("xcorr_window")
    # rows appended between two passes are scored
    db.set_lag_window(15)
    db.scores()
    dg.append(rows[M:])
    lag, mv = db.scores()
    assert len(lag) == M + 40
    exp, _, _, _ = W.expect(oracle, ref, rows, (15,))
    check(lag, mv, *exp[15], keep=W.plain_rows(M + 40), cap_ties=False)
    # a batch made like a windowed one does not inherit the window
    like = muse.DeviceBatch.like(db, dg)
    assert like.lag_window() == -1


# ------------------------------------------------------------------ 4. Runs
def _assert_run(got, want):
    idx, lag, score = got[0], got[1], got[2]
    oi, ol, osc = want[0], want[1], want[2]
    assert lag.tolist() == ol.tolist()
    assert np.allclose(score, osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert idx.tolist() == oi.tolist()


@pytest.mark.parametrize("M", [1001, 100_000])
def test_runs_match_oracle_results(muse, eng, oracle, M):
    """muse_batch_run without and with label groups (the small-Run path and, at 100 000 x 480, the general path), _run_groups +
    muse_merge_group_winners, _run_shard + muse_merge_records, sign filters and a threshold"""
    N, L = 480, 15
    ref, rows = W.make_case(N, M, seed=M, scaled=False)
    rng = np.random.default_rng(5)
    rows[rng.random(M) < 0.3] *= -1.0                                           # both signs for the sign filters
    rows[1] = ref
    exp, glag, gmv, n = W.expect(oracle, ref, rows, (L,))
    wlag, wmv, _ = exp[L]
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    db.set_lag_window(L)
    G = M // 7 + 1
    gid = (np.arange(M) % G).astype(np.int32)
    for sign, thr in ((0, 0.0), (1, 0.0), (-1, 0.0), (0, 0.35)):
        got = db.run(None, 0, L, 20, thr, sign, True)
        _assert_run(got, oracle.results(wlag, wmv, None, 0, True, L, 20, thr, sign))
        assert db.last_run_path() == 0                                          # never screened
        got = db.run(gid, G, L, 20, thr, sign, True)
        _assert_run(got, oracle.results(wlag, wmv, gid, G, True, L, 20, thr, sign))
        got = db.run(gid, G, L, 20, thr, sign, False)
        _assert_run(got, oracle.results(wlag, wmv, gid, G, False, L, 20, thr, sign))
    # with the filter-and-refine Run switched on for groups of this size, a windowed batch still scores in float64 (and a plain
    # batch over the same rows does take the screened path: the switch is live)
    if M >= 100_000:
        eng.set_screening(True, 1000)
        try:
            got = db.run(None, 0, L, 20, 0.0, 0, True)
            assert db.last_run_path() == 0
            _assert_run(got, oracle.results(wlag, wmv, None, 0, True, L, 20, 0.0, 0))
            plain = muse.DeviceBatch(eng, dg, ref)
            plain.run(None, 0, L, 20, 0.0, 0, True)
            assert plain.last_run_path() == 1
        finally:
            eng.set_screening(False)
    # the windowed Run keeps series today's Run drops
    today = oracle.results(glag, gmv, None, 0, True, L, M, 0.0, 0)
    now = oracle.results(wlag, wmv, None, 0, True, L, M, 0.0, 0)
    assert len(now[0]) >= len(today[0]) + M // 4
    got = db.run(None, 0, L, M, 0.0, 0, True)
    assert len(got[0]) == len(now[0]) and got[1].tolist() == now[1].tolist()
    # per-group winners + host merge
    rec, state = db.run_groups(gid, G, 0, abs_scores=True)
    wrec, wstate = muse.merge_group_winners(rec[None, :], state[None, :])
    mi, ml, ms, _ = muse.merge_group_records(rec[None, :], state[None, :], L, 20, 0.0, 0)
    _assert_run((mi, ml, ms), oracle.results(wlag, wmv, gid, G, True, L, 20, 0.0, 0))
    assert int((wstate == 1).sum()) > 0
    # shard candidates + host merge (two shards of one device)
    half = M // 2
    recs = []
    for lo, hi in ((0, half), (half, M)):
        sg = muse.DeviceGroup.from_rows(eng, rows[lo:hi])
        sb = muse.DeviceBatch(eng, sg, ref)
        sb.set_lag_window(L)
        recs.append(sb.run_shard(None, 0, lo, L, 20, 0.0, 0, True))
    mi, ml, ms, _ = muse.merge_records(np.concatenate(recs), 20)
    want = oracle.results(wlag, wmv, None, 0, True, L, 20, 0.0, 0)
    assert ml.tolist() == want[1].tolist() and np.allclose(ms, want[2], rtol=SCORE_RTOL, atol=SCORE_ATOL)
    assert sorted(mi.tolist()) == sorted(want[0].tolist())


@pytest.mark.parametrize("sharded", [False, True])
def test_python_batch_run_windowed(muse, eng, oracle, sharded):
    """Batch.RunWindowed(None) and (["graph"]) Fetch what the oracle gives, on one engine and on device 0 listed twice; the
    Run behind it is the Run it was before"""
    N, graphs, hosts, L = 1433, 30, 8, 10
    M = graphs * hosts
    ref_y, rows = W.make_case(N, M, seed=31, scaled=False)
    exp, glag, gmv, n = W.expect(oracle, ref_y, rows, (L,))
    wlag, wmv, _ = exp[L]
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    ref = muse.NewSeries(ref_y, muse.NewLabels({"graph": "ref"}))
    engines = [muse.Engine(0), muse.Engine(0)] if sharded else None
    res = muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY)
    b = muse.NewBatch(ref, comp, res, 8, engine=eng, engines=engines)
    for by, gid, G in ((None, None, 0), (["graph"], (np.arange(M) // hosts).astype(np.int32), graphs)):
        b.RunWindowed(by)
        got, mean = res.Fetch()
        oi, ol, osc, omean = oracle.results(wlag, wmv, gid, G, True, L, 12, 0.0, 0)
        assert len(got) == len(oi) > 0
        assert [s.Lag for s in got] == ol.tolist()
        assert np.allclose([s.PercentScore for s in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
        assert [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
        assert abs(mean - omean) < 1e-9
    b.Run(None)                                                                  # the window is off again
    got, _ = res.Fetch()
    oi, ol, osc, _ = oracle.results(glag, gmv, None, 0, True, L, 12, 0.0, 0)
    assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()


def _lcg_series(N, i):
    """host/muse_window_test.cpp's series(), bit for bit (32-bit LCG, exact arithmetic)"""
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


def test_cpp_batch_run_windowed(muse, oracle):
    """Batch::RunWindowed of the C++ host mirror (host/muse_window_test.cpp) Fetches what the oracle gives"""
    exe = muse.build.build_window_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "window ok" in r.stdout, r.stdout + r.stderr
    N, M, L = 1000, 240, 15
    ref = _lcg_series(N, -1)
    rows = np.stack([_lcg_series(N, i) for i in range(M)])
    exp, glag, gmv, n = W.expect(oracle, ref, rows, (L,))
    wlag, wmv, tie = exp[L]
    assert not tie.any()
    assert (np.abs(glag) > L).sum() * 4 >= M                                     # rows a filter of today's result would drop
    for case, gid, G in (("nil", None, 0), ("graph", (np.arange(M) // 6).astype(np.int32), M // 6)):
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith(case + " ")]
        oi, ol, osc, _ = oracle.results(wlag, wmv, gid, G, True, L, 12, 0.0, 0)
        assert len(lines) == len(oi) == 12
        assert [int(l[1]) for l in lines] == oi.tolist()
        assert [int(l[2]) for l in lines] == ol.tolist()
        assert np.allclose([float(l[3]) for l in lines], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_handles_as_they_were(muse, eng, oracle):
    B = muse.binding
    UNS = B.MUSE_ERR_UNSUPPORTED
    N, M = 1024, 64
    ref, rows = W.make_case(N, M, seed=3)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    base = db.scores()
    exp, _, _, _ = W.expect(oracle, ref, rows, (7,))

    def refused(fn):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == UNS, e.value
        assert e.value.message

    # wider than the cap: refused, the batch unchanged (off stays off, a set window stays)
    refused(lambda: db.set_lag_window(B.MUSE_LAG_WINDOW_MAX + 1))
    assert db.lag_window() == -1
    again = db.scores()
    assert np.array_equal(again[0], base[0]) and again[1].tobytes() == base[1].tobytes()
    db.set_lag_window(7)
    refused(lambda: db.set_lag_window(B.MUSE_LAG_WINDOW_MAX + 1))
    assert db.lag_window() == 7
    check(*db.scores(), *exp[7], cap_ties=False)
    # a windowed batch inside a many-references pass
    other = muse.DeviceBatch(eng, dg, ref[::-1].copy())
    refused(lambda: muse.score_many([db, other]))
    refused(lambda: muse.run_many([other, db], None, 0, 7, 5, 0.0, 0, True))
    # a windowed batch as the template of a Muse.Run
    refused(lambda: db.run_rows(rows[:4]))
    refused(lambda: db.run_row_ptrs([rows[0], rows[1]]))
    refused(lambda: db.run_group_rows(dg, np.arange(4, dtype=np.int64)))
    check(*db.scores(), *exp[7], cap_ties=False)                                  # still scores as before
    db.set_lag_window(-1)
    rec, state = db.run_rows(rows[:4])                                           # and serves as a template again once off
    assert int(state) == 1
    got = other.scores()
    assert len(got[0]) == M
    # float32-storage groups
    g32 = muse.DeviceGroup.from_rows(eng, rows, f32=True)
    b32 = muse.DeviceBatch(eng, g32, ref)
    base32 = b32.scores()
    refused(lambda: b32.set_lag_window(7))
    assert b32.lag_window() == -1
    again = b32.scores()
    assert np.array_equal(again[0], base32[0]) and again[1].tobytes() == base32[1].tobytes()
    # series longer than 65536 samples
    Nh = 70000
    rng = np.random.default_rng(4)
    refh = rng.standard_normal(Nh)
    gh = muse.DeviceGroup.from_rows(eng, rng.standard_normal((3, Nh)))
    bh = muse.DeviceBatch(eng, gh, refh)
    baseh = bh.scores()
    refused(lambda: bh.set_lag_window(7))
    assert bh.lag_window() == -1
    again = bh.scores()
    assert np.array_equal(again[0], baseh[0]) and again[1].tobytes() == baseh[1].tobytes()


# ------------------------------------------------------------------ 6. scale
def test_full_size_1m_x_4096_window_15(muse, eng, oracle):
    """1 M x 4096 with L = 15: sampled rows against the oracle, as the unwindowed full-size test samples them"""
    M, N, L = 1_000_000, 4096, 15
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=0x6D757365)
    db = muse.DeviceBatch(eng, dg, ref)
    db.set_lag_window(L)
    lag, mv = db.scores()
    assert np.all(np.abs(lag) <= L) and np.all(np.abs(mv[~np.isnan(mv)]) <= 1.0 + 1e-9)
    rng = np.random.default_rng(1)
    starts = np.sort(rng.choice(M // 256, 16, replace=False)) * 256
    worst = 0.0
    for s0 in starts:                                       # 16 x 256 = 4096 sampled rows
        rows = dg.read(int(s0), 256)
        exp, _, _, _ = W.expect(oracle, ref, rows, (L,))
        worst = max(worst, check(lag[s0:s0 + 256], mv[s0:s0 + 256], *exp[L], cap_ties=False))
        assert int(exp[L][2].sum()) <= 1
    _record("scale 1Mx4096 L=15", worst)
    zero = mv == 0
    assert 500 < zero.sum() < 1500 and np.all(lag[zero] == 0)            # ~1/1024 constant rows
    ones = np.abs(mv - 1.0) < 1e-12
    assert 500 < ones.sum() < 1500 and np.all(lag[ones] == 0)            # ~1/1024 copies of ref
