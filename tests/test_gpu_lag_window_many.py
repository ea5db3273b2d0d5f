"""GPU tests of the windowed many-references pass (muse_batch_score_many_windowed / _run_many_windowed, run with -m gpu on an
MI355X): R references against one resident group, each series' best match INSIDE +-L lags, the references' windows packed into
the tiles of one fp64 matrix product (xcorr_window_many.hip).

Expected values never come from the code under test: per reference and series, the window definition applied in numpy
(tests/_window.py) to the correlation slice the CPU oracle returns; Runs, `oracle.results` fed with those windowed (lag, mv).
Tolerances are the project's, applied exactly as tests/test_gpu_lag_window.py applies them (scores 1e-6 relative + 1e-12 absolute,
NaN pattern equal, lags exact off the oracle's ties).  On top of that the packed pass must be BIT-IDENTICAL, per batch, to
set_lag_window(L) + scores() on that batch alone.

The references are six recipes on the reference of W.make_case(N, M, seed=N); the inputs were checked on the CPU oracle beforehand:
no continuous-noise row is an oracle-flagged tie for any reference at any of the windows used here (asserted again below)."""
import os
import subprocess

import numpy as np
import pytest

import _window as W
from _load import pkg
from test_gpu_lag_window import SCORE_ATOL, SCORE_RTOL, _assert_run, check

pytestmark = pytest.mark.gpu

LS = (0, 1, 3, 7, 8, 15, 31, 63)
RS = (1, 2, 3, 6)


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


def make_refs(ref, N, seed):
    """the six recipes; the random ones drawn in list order, one standard_normal call each"""
    rng = np.random.default_rng(seed)
    return [ref.copy(),
            np.roll(ref, 5) + 0.05 * rng.standard_normal(N),
            -np.roll(ref, -9) + 0.05 * rng.standard_normal(N),
            ref[::-1].copy(),
            rng.standard_normal(N),
            np.cumsum(rng.standard_normal(N))]


def expectations(oracle, refs, rows, Ls):
    """per reference: ({L: (lag, mv, tie)}, global lag, global mv), n"""
    out, n = [], None
    for rf in refs:
        exp, glag, gmv, n = W.expect(oracle, rf, rows, Ls)
        out.append((exp, glag, gmv))
    return out, n


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def alone(db, L):
    """set_lag_window(L) + scores() on one batch, its own setting put back"""
    before = db.lag_window()
    db.set_lag_window(L)
    try:
        return db.scores()
    finally:
        db.set_lag_window(before)


# ------------------------------------------------------------------ 1. parity and bit-identity
@pytest.mark.parametrize("N", [480, 1024, 1433, 4096, 5000, 40000, 100, 8])
def test_many_windowed_parity_and_bits(muse, eng, oracle, N):
    """scores_many_windowed of the first R references against the oracle-derived expectation per reference, and bit for bit
    against the single-reference pass of each batch, in both orders of doing the two forms; odd N = odd row stride (the 8-byte
    build), even N the WIDE one; block counts with partial 16-row blocks"""
    Mfull = 200 if N >= 5000 else 1001
    ref, rows = W.make_case(N, Mfull, seed=N)
    refs = make_refs(ref, N, 1000 + N)
    exps, n = expectations(oracle, refs, rows, LS)
    keep = W.plain_rows(Mfull)
    if N >= 480:                                   # references 1 - 4: global winners inside and outside the windows
        for exp, glag, gmv in exps[:4]:
            inside = (np.abs(glag) <= 7) & keep
            assert inside.any() and (~inside & keep).any()
    for M in (Mfull, 1, 15, 17):
        dg = muse.DeviceGroup.from_rows(eng, rows[:M])
        dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
        assert dbs[0].n == n
        for R in RS:
            for L in LS:
                first_alone = (R + L) % 2 == 1     # both orders of the two forms
                single = [alone(db, L) for db in dbs[:R]] if first_alone else None
                got = muse.scores_many_windowed(dbs[:R], L)
                if single is None:
                    single = [alone(db, L) for db in dbs[:R]]
                for r in range(R):
                    elag, emv, tie = exps[r][0][L]
                    assert not (tie[:M] & keep[:M]).any()          # continuous noise: the oracle by itself yields no tie
                    check(got[r][0], got[r][1], elag[:M], emv[:M], tie[:M], keep[:M], cap_ties=(M >= 1000),
                          tag="many N=%d M=%d R=%d L=%d ref=%d" % (N, M, R, L, r) if M == Mfull and R == RS[-1] else None)
                    assert np.all(np.abs(got[r][0]) <= min(L, n // 2))
                    assert same_bits(got[r], single[r]), (N, M, R, L, r)
                    assert dbs[r].lag_window() == -1
        for db in dbs:
            db.close()
        dg.close()


# ------------------------------------------------------------------ 2. the packing is taken; several launches
def test_packing_is_really_taken(muse, eng):
    N, M = 1024, 100
    ref, rows = W.make_case(N, M, seed=N)
    refs = make_refs(ref, N, 1000 + N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
    for R, L, tiles in ((6, 3, 3), (4, 7, 4), (2, 15, 4), (6, 1, 2), (4, 15, 8), (3, 16, 7)):
        plan = muse.window_many_plan(R, L)
        assert plan["launches"] < R and plan["launches"] == 1 and int(plan["tiles_of"][0]) == tiles
        muse.score_many_windowed(dbs[:R], L)
        for db in dbs[:R]:
            name = eng.kernel_name(db)
            assert name.startswith("xcorr_window_many_mfma<%d, true>" % tiles), name
            assert db.last_run_path() == 0
    # a window that fills four tiles by itself is not packed: R single passes of the single-reference kernel -- and a plain pass
    # behind a packed one names the plain kernel again
    assert muse.window_many_plan(2, 63)["launches"] == 2 and muse.window_many_plan(2, 31)["launches"] == 2
    muse.score_many_windowed(dbs[:2], 63)
    assert not eng.kernel_name(dbs[0]).startswith("xcorr_window")
    muse.score_many_windowed(dbs[:2], 7)
    assert eng.kernel_name(dbs[0]).startswith("xcorr_window_many_mfma")
    dbs[0].scores()
    assert not eng.kernel_name(dbs[0]).startswith("xcorr_window")
    assert eng.kernel_name(dbs[1]).startswith("xcorr_window_many_mfma")


@pytest.mark.parametrize("N", [1433, 4096])
def test_several_launches(muse, eng, oracle, N):
    """R = 12 references at L = 7 are 180 packed rows: two launches (8 + 4 references); at L = 15 three launches of four, at L = 1
    one launch of twelve.  Parity and bit-identity hold across the cuts.  The second six references are the six recipes again
    with a second seed."""
    M = 1001
    ref, rows = W.make_case(N, M, seed=N)
    refs = make_refs(ref, N, 1000 + N) + make_refs(ref, N, 2000 + N)
    Ls = (7, 1, 15)
    exps, n = expectations(oracle, refs, rows, Ls)
    keep = W.plain_rows(M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
    plan = muse.window_many_plan(12, 7)
    assert plan["launches"] == 2 and plan["launch_of"].tolist() == [0] * 8 + [1] * 4 and plan["tiles_of"].tolist() == [8, 4]
    assert muse.window_many_plan(12, 15)["launches"] == 3
    for L in Ls:
        got = muse.scores_many_windowed(dbs, L)
        for r in range(12):
            elag, emv, tie = exps[r][0][L]
            assert not (tie & keep).any()
            check(got[r][0], got[r][1], elag, emv, tie, keep)
            assert same_bits(got[r], alone(dbs[r], L)), (N, L, r)
        again = muse.scores_many_windowed(dbs, L)
        assert all(same_bits(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------ 3. Runs
def test_run_many_windowed_matches_oracle_results(muse, eng, oracle):
    N, M, L = 1433, 1001, 7
    ref, rows = W.make_case(N, M, seed=N, scaled=False)
    refs = make_refs(ref, N, 1000 + N)
    exps, n = expectations(oracle, refs, rows, (L,))
    keep = W.plain_rows(M)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
    G = (M + 5) // 6
    gid6 = (np.arange(M) // 6).astype(np.int32)
    for gid, Gn in ((None, 0), (gid6, G)):
        for _ in range(2):                                                      # Run(); Run(): the same
            got = muse.run_many_windowed(dbs, gid, Gn, L, 12, 0.0, 0, True)
            assert len(got) == 6
            for r in range(6):
                wlag, wmv, tie = exps[r][0][L]
                assert not (tie & keep).any()
                _assert_run(got[r], oracle.results(wlag, wmv, gid, Gn, True, L, 12, 0.0, 0))
                assert dbs[r].last_run_path() == 0 and dbs[r].lag_window() == -1
    a = muse.run_many_windowed(dbs, gid6, G, L, 12, 0.0, 0, True)
    b = muse.run_many_windowed(dbs, gid6, G, L, 12, 0.0, 0, True)
    for x, y in zip(a, b):
        assert x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() and x[2].tobytes() == y[2].tobytes()
    # every windowed score lies inside MaxLag: the Run keeps series that today's Run over the same rows drops
    today = muse.run_many(dbs, None, 0, L, M, 0.0, 0, True)
    now = muse.run_many_windowed(dbs, None, 0, L, M, 0.0, 0, True)
    assert sum(len(x[0]) for x in now) > sum(len(x[0]) for x in today)


def test_python_run_many_windowed_equals_run_windowed(muse, eng, oracle):
    """RunManyWindowed over the reference-style API gives every batch what its own RunWindowed gives, and what the oracle gives"""
    N, graphs, hosts, L = 1433, 30, 8, 7
    M = graphs * hosts
    ref_y, rows = W.make_case(N, M, seed=N, scaled=False)
    # (rows 1 and 2 are the reference and its negative: |score| 1 twice for the first recipe, an EXACT tie, and the order among
    # exactly tied scores is the one thing the feed of RunMany and the feed of Run do not share -- muse.py, Batch.Run; the C entry
    # point is held to the oracle's order on those rows in test_run_many_windowed_matches_oracle_results)
    rows[2] = -rows[10]
    refs = make_refs(ref_y, N, 1000 + N)[:4]
    exps, n = expectations(oracle, refs, rows, (L,))
    assert not any((e[0][L][2] & W.plain_rows(M)).any() for e in exps)
    labels = [{"graph": "g%02d" % (i // hosts), "host": "h%d" % (i % hosts), "i": str(i)} for i in range(M)]
    comp = muse.NewGroup("comparison")
    comp.Add(*[muse.NewSeries(rows[i], muse.NewLabels(labels[i])) for i in range(M)])
    series = [muse.NewSeries(rf, muse.NewLabels({"graph": "ref%d" % k})) for k, rf in enumerate(refs)]
    for by, gid, G in ((None, None, 0), (["graph"], (np.arange(M) // hosts).astype(np.int32), graphs)):
        many = [muse.NewBatch(s, comp, muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY), 8, engine=eng) for s in series]
        solo = [muse.NewBatch(s, comp, muse.NewResults(L, 12, 0.0, muse.SignFilter_ANY), 8, engine=eng) for s in series]
        muse.RunManyWindowed(many, by)
        for r, (bm, bs) in enumerate(zip(many, solo)):
            bs.RunWindowed(by)
            got, mean = bm.Results.Fetch()
            want, wmean = bs.Results.Fetch()
            assert len(got) == len(want) > 0
            assert [s.Lag for s in got] == [s.Lag for s in want]
            assert [s.Labels.labels["i"] for s in got] == [s.Labels.labels["i"] for s in want]
            assert [s.PercentScore for s in got] == [s.PercentScore for s in want]          # bit-identical passes
            wlag, wmv, _ = exps[r][0][L]
            oi, ol, osc, omean = oracle.results(wlag, wmv, gid, G, True, L, 12, 0.0, 0)
            assert [s.Lag for s in got] == ol.tolist() and [int(s.Labels.labels["i"]) for s in got] == oi.tolist()
            assert np.allclose([s.PercentScore for s in got], osc, rtol=SCORE_RTOL, atol=SCORE_ATOL)
            assert abs(mean - omean) < 1e-9
    # batches that do not share the Results settings are RunWindowed one by one
    odd = [muse.NewBatch(s, comp, muse.NewResults(L + k, 12, 0.0, muse.SignFilter_ANY), 8, engine=eng) for k, s in enumerate(series[:2])]
    muse.RunManyWindowed(odd, None)
    for k, b in enumerate(odd):
        ref_b = muse.NewBatch(series[k], comp, muse.NewResults(L + k, 12, 0.0, muse.SignFilter_ANY), 8, engine=eng)
        ref_b.RunWindowed(None)
        assert [s.Lag for s in b.Results.Fetch()[0]] == [s.Lag for s in ref_b.Results.Fetch()[0]]


def test_cpp_run_many_windowed(muse):
    """Batch::RunManyWindowed of the C++ host mirror (host/muse_window_many_test.cpp): every batch Fetches, bit for bit, what its
    own RunWindowed Fetches"""
    exe = muse.build.build_window_many_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "window many ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ 4. nothing leaks
def test_nothing_leaks(muse, eng, oracle):
    N, M, L = 4096, 333, 7
    ref, rows = W.make_case(N, M + 40, seed=N)
    refs = make_refs(ref, N, 1000 + N)[:4]
    exps, n = expectations(oracle, refs, rows, (L,))
    keep = W.plain_rows(M + 40)
    dg = muse.DeviceGroup.from_rows(eng, rows[:M])
    dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
    plain = [db.scores() for db in dbs]
    dbs[1].set_lag_window(L)                                                    # a batch's own window equal to the pass's is fine
    before = [db.lag_window() for db in dbs]
    assert before == [-1, L, -1, -1]
    own = dbs[1].scores()
    got = muse.scores_many_windowed(dbs, L)
    assert [db.lag_window() for db in dbs] == before                             # the settings read what they read before
    assert same_bits(got[1], own)
    for r in (0, 2, 3):                                                          # a following plain pass: bit-identical
        assert same_bits(dbs[r].scores(), plain[r])
        assert not eng.kernel_name(dbs[r]).startswith("xcorr_window")
    assert same_bits(dbs[1].scores(), own)
    assert same_bits(muse.scores_many_windowed(dbs, L)[0], got[0])
    # plain many-references passes still refuse the batch with a window, and take the others
    with pytest.raises(muse.MuseError):
        muse.score_many(dbs)
    both = muse.scores_many([dbs[0], dbs[2]])
    assert np.array_equal(both[0][0], plain[0][0]) and np.array_equal(both[1][0], plain[2][0])
    # rows appended between two packed passes are scored
    dg.append(rows[M:])
    got = muse.scores_many_windowed(dbs, L)
    for r in range(4):
        assert len(got[r][0]) == M + 40
        elag, emv, tie = exps[r][0][L]
        check(got[r][0], got[r][1], elag, emv, tie, keep, cap_ties=False)
        assert same_bits(got[r], alone(dbs[r], L))


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_handles_as_they_were(muse, eng, oracle):
    B = muse.binding
    N, M = 1024, 64
    ref, rows = W.make_case(N, M, seed=3)
    refs = make_refs(ref, N, 1003)[:3]
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, rf) for rf in refs]
    base = [db.scores() for db in dbs]
    exp7 = muse.scores_many_windowed(dbs, 7)

    def refused(fn, status):
        with pytest.raises(muse.MuseError) as e:
            fn()
        assert e.value.status == status, e.value
        assert e.value.message

    def unchanged(batches, windows):
        assert [db.lag_window() for db in batches] == windows
        for db, b, w in zip(batches, base, windows):
            if w < 0:
                assert same_bits(db.scores(), b)
        assert all(same_bits(a, b) for a, b in zip(muse.scores_many_windowed(batches, 7), exp7))

    # wider than the cap
    refused(lambda: muse.score_many_windowed(dbs, B.MUSE_LAG_WINDOW_MAX + 1), B.MUSE_ERR_UNSUPPORTED)
    refused(lambda: muse.run_many_windowed(dbs, None, 0, B.MUSE_LAG_WINDOW_MAX + 1, 5, 0.0, 0, True), B.MUSE_ERR_UNSUPPORTED)
    unchanged(dbs, [-1, -1, -1])
    refused(lambda: muse.score_many_windowed(dbs, -1), B.MUSE_ERR_INVALID)
    # a batch whose own window is 7 in a pass of 15
    dbs[1].set_lag_window(7)
    refused(lambda: muse.score_many_windowed(dbs, 15), B.MUSE_ERR_INVALID)
    refused(lambda: muse.run_many_windowed(dbs, None, 0, 15, 5, 0.0, 0, True), B.MUSE_ERR_INVALID)
    unchanged(dbs, [-1, 7, -1])
    dbs[1].set_lag_window(-1)
    # the same batch twice
    refused(lambda: muse.score_many_windowed([dbs[0], dbs[1], dbs[0]], 7), B.MUSE_ERR_INVALID)
    # batches of two groups
    dg2 = muse.DeviceGroup.from_rows(eng, rows[:32])
    other = muse.DeviceBatch(eng, dg2, refs[0])
    obase = other.scores()
    refused(lambda: muse.score_many_windowed([dbs[0], other], 7), B.MUSE_ERR_INVALID)
    assert same_bits(other.scores(), obase) and other.lag_window() == -1
    unchanged(dbs, [-1, -1, -1])
    # a float32-storage group
    g32 = muse.DeviceGroup.from_rows(eng, rows, f32=True)
    b32 = [muse.DeviceBatch(eng, g32, rf) for rf in refs[:2]]
    base32 = [b.scores() for b in b32]
    refused(lambda: muse.score_many_windowed(b32, 7), B.MUSE_ERR_UNSUPPORTED)
    assert all(b.lag_window() == -1 for b in b32)
    assert all(same_bits(b.scores(), s) for b, s in zip(b32, base32))
    # series longer than 65536 samples
    Nh = 70000
    rng = np.random.default_rng(4)
    gh = muse.DeviceGroup.from_rows(eng, rng.standard_normal((3, Nh)))
    bh = [muse.DeviceBatch(eng, gh, rng.standard_normal(Nh)) for _ in range(2)]
    baseh = [b.scores() for b in bh]
    refused(lambda: muse.score_many_windowed(bh, 7), B.MUSE_ERR_UNSUPPORTED)
    assert all(same_bits(b.scores(), s) for b, s in zip(bh, baseh))
