"""GPU tests of round 6's cold-path work (run with -m gpu on an MI355X), all through the C ABI and against the CPU oracle:
the context's allocation cache (a reused block never leaks the previous group's rows or guard), the pinned staging
windows (muse_group_stage / muse_group_commit), the row-pointer form of Muse.Run (muse_batch_run_row_ptrs), per-slot
streams under concurrent callers with kernel timing on, and the piecewise flush of per-Series appends."""
import threading

import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
SCORE_ATOL = 1e-12
TIE_GAP = 1e-12


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


def _check(lag, mv, olag, omv, gap):
    lag, mv, olag, omv = map(np.asarray, (lag, mv, olag, omv))
    nan_o = np.isnan(omv)
    assert np.array_equal(np.isnan(mv), nan_o)
    ok = ~nan_o
    err = np.abs(mv[ok] - omv[ok])
    assert np.all(err <= SCORE_RTOL * np.abs(omv[ok]) + SCORE_ATOL), float(err.max())
    tie = (gap < TIE_GAP) & ok
    assert not ((lag != olag) & ~tie & ok).any()


def test_pool_block_reuse_never_leaks_rows_or_guard(muse, eng, oracle):
    """NewGroup -> Add -> NewBatch -> Run -> free, over and over on one context, with shapes that land in the SAME size class
    of the allocation cache: a long-series group full of large values, then a padded short-series group (N < n: the kernels
    read up to n - N samples IN FRONT of a row -- the guard for row 0, the previous row otherwise -- and mask them), whose
    block is the one the first group just handed back.  Every pass is checked row by row against the oracle; the cache is
    observed to hold blocks in between (the reuse happens), and muse_ctx_trim empties it."""
    rng = np.random.default_rng(6001)
    eng.trim()
    assert eng.pool_stats()[0] == 0
    shapes = [(64, 4096, 1e6), (511, 513, 1.0), (256, 1024, 1e-3), (300, 700, 1.0), (64, 4096, 1.0), (37, 5000, 1.0), (181, 1025, 1e3),
              (23, 8000, 1.0), (6, 20000, 1.0)]
    for M, N, scale in shapes:
        ref = rng.standard_normal(N)
        rows = rng.standard_normal((M, N)) * scale
        rows[0] += 3.0 * scale * np.roll(ref, 2)                     # row 0 reads the guard in front of it when N < n
        rows[M // 2] = 7.0 * scale                                   # sigma == 0
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        lag, mv = db.scores()
        olag, omv, gap = oracle.batch_scores(ref, rows)
        _check(lag, mv, olag, omv, gap)
        # the same rows through per-Series appends (the staging pair, flushed piece by piece)
        dg2 = muse.DeviceGroup(eng, N, 0)
        for r in range(M):
            dg2.append(rows[r])
        db2 = muse.DeviceBatch.like(db, dg2)
        lag2, mv2 = db2.scores()
        assert np.array_equal(lag, lag2) and np.array_equal(mv, mv2, equal_nan=True)
        db2.close()
        dg2.close()
        db.close()
        dg.close()
        assert eng.pool_stats()[1] > 0                               # freed blocks are kept ...
    dev_bytes, dev_blocks, host_bytes, host_blocks = eng.pool_stats()
    assert 0 < dev_bytes <= (1 << 30) and host_bytes <= (192 << 20)
    eng.trim()                                                       # ... until asked for
    assert eng.pool_stats() == (0, 0, 0, 0)


@pytest.mark.parametrize("N,M", [(480, 5000), (4096, 300), (513, 70000), (20000, 40)])
def test_staging_windows_match_append(muse, eng, oracle, N, M):
    """muse_group_stage / muse_group_commit (the host packs rows straight into pinned memory, commits piece by piece, in any
    order, from several threads) gives the group muse_group_append gives: rows read back bit for bit, scores identical, and
    equal to the oracle's.  513 x 70000 needs more than one 32 MB window (the two buffers alternate); rows appended the
    ordinary way before and after a window keep their order."""
    rng = np.random.default_rng(6100 + N)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    rows[::5] += 2.0 * np.roll(ref, -3)
    dg = muse.DeviceGroup(eng, N, 0)
    head = 3
    dg.append(rows[:head])                                            # ordinary appends in front of the windows
    i = head
    tail = 2
    while i < M - tail:
        win = dg.stage(M - tail - i)
        k = win.shape[0]
        assert 0 < k <= M - tail - i
        with pytest.raises(muse.MuseError):                           # one window at a time; nothing else on the group meanwhile
            dg.stage(1)
        with pytest.raises(muse.MuseError):
            dg.append(rows[:1])
        pieces = [(lo, min(k, lo + max(1, k // 7))) for lo in range(0, k, max(1, k // 7))]
        order = rng.permutation(len(pieces))                          # commits in any order ...
        errs = []

        def fill(idx):
            try:
                for j in idx:
                    lo, hi = pieces[j]
                    win[lo:hi] = rows[i + lo:i + hi]
                    dg.commit(lo, hi - lo)
            except Exception as e:                                    # noqa: BLE001 (reported below on the main thread)
                errs.append(e)
        th = [threading.Thread(target=fill, args=(order[w::3],)) for w in range(3)]   # ... from three threads
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        with pytest.raises(muse.MuseError):
            dg.commit(0, 1)                                           # the window is closed
        i += k
    dg.append(rows[M - tail:])
    assert dg.M == M
    step = max(1, M // 50)
    for first in range(0, M, step * 10):
        cnt = min(step, M - first)
        assert np.array_equal(dg.read(first, cnt), rows[first:first + cnt])
    assert np.array_equal(dg.read(M - 5, 5), rows[M - 5:])
    db = muse.DeviceBatch(eng, dg, ref)
    lag, mv = db.scores()
    dg_ref = muse.DeviceGroup.from_rows(eng, rows)
    db_ref = muse.DeviceBatch.like(db, dg_ref)
    lag_r, mv_r = db_ref.scores()
    assert np.array_equal(lag, lag_r) and np.array_equal(mv, mv_r)
    sub = np.unique(np.concatenate([np.arange(0, M, max(1, M // 400)), [0, head - 1, head, M - tail - 1, M - tail, M - 1]]))
    olag, omv, gap = oracle.batch_scores(ref, rows[sub])
    _check(lag[sub], mv[sub], olag, omv, gap)
    for h in (db_ref, dg_ref, db, dg):
        h.close()


def test_append_staged_helper_and_f32_refusal(muse, eng):
    rng = np.random.default_rng(6200)
    N, M = 1000, 2500
    series = [rng.standard_normal(N) for _ in range(M)]
    dg = muse.DeviceGroup(eng, N, 0)
    dg.append_staged(series)
    assert dg.M == M and np.array_equal(dg.read(0, M), np.stack(series))
    dg.close()
    g32 = muse.DeviceGroup(eng, N, 0, f32=True)
    with pytest.raises(muse.MuseError) as ei:
        g32.stage(4)
    assert ei.value.status == muse.binding.MUSE_ERR_UNSUPPORTED
    g32.close()


@pytest.mark.parametrize("N", [8, 480, 4096, 5000])
def test_run_row_ptrs_equals_run_rows(muse, eng, N):
    """muse_batch_run_row_ptrs (one pointer per series, gathered into the pinned slot) returns what muse_batch_run_rows returns
    for the same rows packed: one to 300 series, signed and abs, NaN first member, constant member, an empty group, a NULL row."""
    rng = np.random.default_rng(6300 + N)
    ref = rng.standard_normal(N)
    probe = muse.DeviceGroup(eng, N, 0)
    tmpl = muse.DeviceBatch(eng, probe, ref)
    for M in (1, 2, 50, 300):
        rows = rng.standard_normal((M, N))
        rows[::4] += np.roll(ref, 1)
        if M >= 50:
            rows[7] = 0.25
            rows[9] = rows[5]
        for nan_first in (False, True):
            r = rows.copy()
            if nan_first:
                r[0, N // 3] = np.nan
            series = [r[i].copy() for i in range(M)]                  # separate allocations, as the Series of a Muse.Run are
            for abs_scores in (False, True):
                w1, s1 = tmpl.run_rows(r, abs_scores=abs_scores)
                w2, s2 = tmpl.run_row_ptrs(series, abs_scores=abs_scores)
                assert s1 == s2 and w1.tolist() == w2.tolist(), (N, M, nan_first, abs_scores)
    w, s = tmpl.run_row_ptrs([])
    assert s == 0 and int(w["series"]) == -1
    with pytest.raises(muse.MuseError) as ei:
        tmpl.run_row_ptrs([np.zeros(N + 1)])
    assert ei.value.status == muse.binding.MUSE_ERR_LENGTH
    tmpl.close()
    probe.close()


def test_concurrent_run_rows_on_slot_streams_with_timing_on(muse, eng, oracle):
    """Sixteen host threads drive one template (muse_test.go:203-214) while kernel timing is ON (the event list is shared by
    the callers): every call returns the winner the single-threaded call returns, the launch count adds up, groups of
    different sizes and lengths share the slot pool (n = 512 and n = 8192: the latter stays on the context's stream)."""
    rng = np.random.default_rng(6400)
    cases = []
    for N in (480, 5000):
        ref = rng.standard_normal(N)
        probe = muse.DeviceGroup(eng, N, 0)
        tmpl = muse.DeviceBatch(eng, probe, ref)
        groups = []
        for g in range(24):
            M = int(rng.integers(1, 60))
            rows = rng.standard_normal((M, N))
            rows[rng.integers(0, M)] += 2.5 * np.roll(ref, int(rng.integers(-5, 6)))
            groups.append(rows)
        expect = [tmpl.run_rows(r) for r in groups]
        cases.append((tmpl, probe, groups, expect, ref))
    eng.kernel_time()
    eng.kernel_timing(True)
    errs, calls = [], [0] * 16

    def worker(w):
        try:
            for rep in range(6):
                for tmpl, _, groups, expect, _ in cases:
                    for gi in range(w % 3, len(groups), 3):
                        win, st = tmpl.run_rows(groups[gi]) if (rep + gi) % 2 else tmpl.run_row_ptrs([x.copy() for x in groups[gi]])
                        calls[w] += 1
                        if st != expect[gi][1] or win.tolist() != expect[gi][0].tolist():
                            errs.append((w, gi, win.tolist(), expect[gi][0].tolist()))
        except Exception as e:                                        # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(w,)) for w in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    eng.synchronize()
    eng.kernel_timing(False)
    ms, launches = eng.kernel_time()
    assert not errs, errs[:3]
    assert launches == sum(calls) and ms > 0.0
    # the winners against the oracle (one group per length)
    for tmpl, probe, groups, expect, ref in cases:
        rows = groups[0]
        olag, omv, gap = oracle.batch_scores(ref, rows)
        sc = np.clip(omv, -1.0, 1.0)
        best = int(np.argmax(np.abs(sc)))
        win = expect[0][0]
        assert abs(win["score"] - sc[best]) <= SCORE_RTOL * abs(sc[best]) + SCORE_ATOL
        tmpl.close()
        probe.close()


def test_live_batch_grows_every_work_buffer(muse, eng, oracle):
    """One batch walks through the C API's grow-on-demand work buffers, each growth while a pass of the batch may still be
    queued (a bare score() without read-back goes in front of every step): the score buffers and the hand-off list, the
    group grown past its capacity, the selection workspace (more label groups), the screening buffers (screened Runs over
    more rows and more label groups), the many-reference pointer table (a larger R, fp64 and screened).  Every step is
    checked against the oracle: scores row by row, Run records against the oracle's Results over the fp64 scores."""
    rng = np.random.default_rng(6500)
    N, M0, M1, M2 = 4096, 1000, 2600, 4200
    refs = [rng.standard_normal(N) for _ in range(4)]
    rows = rng.standard_normal((M2, N))
    for i in rng.integers(0, M2, size=300):
        rows[i] += rng.uniform(-3, 3) * np.roll(refs[int(rng.integers(0, 4))], int(rng.integers(-50, 50)))
    rows[7, 11] = np.nan                                              # a pair the n = 4096 kernel lists and redoes
    rows[9] = 5.0                                                     # sigma == 0
    dg = muse.DeviceGroup(eng, N, M0)
    dg.append(rows[:M0])
    db = muse.DeviceBatch(eng, dg, refs[0])
    others = []

    def exact(b, ref):
        M = dg.M
        lag, mv = b.read_scores()
        olag, omv, gap = oracle.batch_scores(ref, rows[:M], nthreads=8)
        _check(lag, mv, olag, omv, gap)
        return lag, mv

    def check_run(b, scores, gid, G, screened, top_n=10, got=None):
        lag, mv = scores
        if got is None:
            got = b.run(gid, G, max_lag=15, top_n=top_n)
        exp = oracle.results(lag, mv, gid, G, True, 15, top_n, 0.0, 0)
        assert got[0].tolist() == exp[0].tolist() and got[1].tolist() == exp[1].tolist(), (G, screened)
        np.testing.assert_allclose(got[2], exp[2], rtol=1e-12, atol=0)
        assert b.last_run_info()[0] is screened, G

    try:
        db.score()                                                    # 1. first score buffers, no read-back
        s = exact(db, refs[0])
        db.score()
        dg.append(rows[M0:M1])                                        # 2. past the group's capacity ...
        db.score()                                                    # ... and larger score buffers
        s = exact(db, refs[0])
        for G in (2100, 2500):                                        # 3. more label groups than before (beyond the
            db.score()                                                #    small-Run kernel's: the selection workspace)
            gid = rng.permutation(np.arange(M1) % G).astype(np.int32)
            check_run(db, s, gid, G, False)
        eng.set_screening(True, min_rows=M0)                          # 4. screened Runs ...
        db.score()
        check_run(db, s, None, 0, True)
        dg.append(rows[M1:M2])
        db.score()
        s = exact(db, refs[0])
        db.score()
        check_run(db, s, None, 0, True)                               # ... over more rows, then more label groups
        for G in (40, 900):
            db.score()
            gid = rng.permutation(np.arange(M2) % G).astype(np.int32)
            check_run(db, s, gid, G, True)
        eng.set_screening(False)
        others = [muse.DeviceBatch(eng, dg, r) for r in refs[1:]]
        batches = [db] + others
        db.score()
        muse.score_many(batches[:2])                                  # 5. the pointer table for R = 2 ...
        got = muse.scores_many(batches)                               # ... grown for R = 4
        scores = []
        for b, r, (lag, mv) in zip(batches, refs, got):
            olag, omv, gap = oracle.batch_scores(r, rows, nthreads=8)
            _check(lag, mv, olag, omv, gap)
            scores.append((lag, mv))
        eng.set_screening(True, min_rows=M0)                          # ... and for R = 4 screened (five columns)
        muse.score_many(batches)
        for b, sc, g in zip(batches, scores, muse.run_many(batches, None, 0, max_lag=15, top_n=10)):
            check_run(b, sc, None, 0, True, got=g)
    finally:
        eng.set_screening(False)
        for b in others + [db]:
            b.close()
        dg.close()
