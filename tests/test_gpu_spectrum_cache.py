"""GPU tests of a resident group's spectrum cache (xcorr_r16_cached.hip, capi_batch.hip).  Run with -m gpu on an
MI355X.

The expectation is always the plain kernel with the cache OFF on a fresh group holding the same rows; a pass that builds the
cache (the writer) or reads it (the reader) must give the same lags and, bit for bit, the same scores (NaN included), and list
the same pairs for the rescaling kernel.  The smallest cached group is set to 2 rows so that small groups exercise every path."""
import ctypes
import threading

import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu

PAIR_BYTES = 65536 + 128


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return m


@pytest.fixture()
def eng(muse):
    e = muse.Engine(0)                       # a context of its own: the hooks below never leak into other tests
    e.spectrum_cache_limits(min_rows=2)
    yield e
    e.close()


def _planted(M, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, N)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))
    ref = rng.standard_normal(N)
    x[0] = ref                               # an exact copy of the reference
    x[1] = 3.5                               # a constant row
    if M >= 16:
        x[3, 17] = np.nan
        x[4, 5] = np.inf
        x[5] = 2.0 ** 600                    # a constant whose square overflows
        x[6] *= 1e25                         # a pair with sigmas 1e50 apart
        x[7] *= 1e-25
        x[M - 1, N // 2] = np.nan            # the last row (a single one when M is odd)
    return x, ref


def _same(got, want, what):
    lag, mv = got
    wlag, wmv = want
    assert np.array_equal(lag, wlag), what
    assert np.array_equal(mv.view(np.uint64), wmv.view(np.uint64)), what


def _plain(muse, eng, rows, ref):
    """(lag, mv), sorted redo list of the plain kernel on a fresh group with the cache off"""
    eng.set_spectrum_cache(False)
    try:
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        out = db.scores()
        assert "cached" not in eng.kernel_name(db)
        redo = sorted(db.redo_pairs().tolist())
        assert dg.spectrum_cache() == (0, 0)
        db.close()
        dg.close()
    finally:
        eng.set_spectrum_cache(True)
    return out, redo


# ------------------------------------------------------------------ 1. plain, writer, reader, reader
@pytest.mark.parametrize("M", [2, 3, 1000, 1001, 4097])
def test_four_passes_are_bit_identical(muse, eng, M):
    rows, ref = _planted(M, 4096, M)
    want, want_redo = _plain(muse, eng, rows, ref)
    if M >= 16:
        assert len(want_redo) >= 4
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    assert dg.spectrum_cache() == (0, 0)
    for k in range(4):
        name = eng.kernel_name(db)
        assert name == ("xcorr_cached_n4096<false>" if k >= 2 else "xcorr_fused_n4096_fold<false, false, false>"), (k, name)
        _same(db.scores(), want, "pass %d" % (k + 1))
        assert sorted(db.redo_pairs().tolist()) == want_redo, k
        assert dg.spectrum_cache() == ((0, 0) if k == 0 else (M & ~1, (M // 2) * PAIR_BYTES)), k
    db.close()
    dg.close()


def test_cached_scores_match_the_oracle(muse, eng, oracle):
    M, N = 1000, 4096
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((M, N)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))
    ref = rng.standard_normal(N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for _ in range(3):
        lag, mv = db.scores()
    assert eng.kernel_name(db).startswith("xcorr_cached_n4096") and dg.spectrum_cache()[0] == M
    olag, omv, gap = oracle.batch_scores(ref, dg.read(0, M), nthreads=4)
    tie = gap < 1e-12
    assert int(np.sum((lag != olag) & ~tie)) == 0
    assert np.all(np.abs(mv - omv) <= 1e-6 * np.abs(omv) + 1e-12)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 2. another reference on a cached group
def test_second_batch_reads_the_cache_on_its_first_pass(muse, eng):
    M = 1000
    rows, ref = _planted(M, 4096, 5)
    ref2 = np.random.default_rng(6).standard_normal(4096)
    want2, redo2 = _plain(muse, eng, rows, ref2)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    db.scores()
    db.scores()
    db2 = muse.DeviceBatch(eng, dg, ref2)
    assert eng.kernel_name(db2) == "xcorr_cached_n4096<false>"
    _same(db2.scores(), want2, "second batch")
    assert sorted(db2.redo_pairs().tolist()) == redo2
    for b in (db, db2):
        b.close()
    dg.close()


# ------------------------------------------------------------------ 3. appends behind a valid cache
def test_appends_extend_the_cache(muse, eng):
    N = 4096
    rows, ref = _planted(1000 + 1 + 1 + 2049, N, 11)
    dg = muse.DeviceGroup.from_rows(eng, rows[:1000])
    db = muse.DeviceBatch(eng, dg, ref)
    for _ in range(3):
        db.scores()
    assert dg.spectrum_cache()[0] == 1000
    M = 1000
    for extra in (1, 1, 2049):               # onto an even M, onto an odd M, many rows
        dg.append(rows[M:M + extra])
        M += extra
        want, redo = _plain(muse, eng, rows[:M], ref)
        for k in range(2):
            _same(db.scores(), want, "M = %d pass %d" % (M, k))
            assert sorted(db.redo_pairs().tolist()) == redo
            assert dg.spectrum_cache() == (M & ~1, (M // 2) * PAIR_BYTES)
            assert eng.kernel_name(db) == "xcorr_cached_n4096<false>"
    db.close()
    dg.close()


# ------------------------------------------------------------------ 4. rows rewritten under the cache
def test_fill_synthetic_drops_the_cache(muse, eng):
    M, N = 1000, 4096
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=1)
    db = muse.DeviceBatch(eng, dg, ref)
    for _ in range(3):
        db.scores()
    assert dg.spectrum_cache()[0] == M
    B = muse.binding
    B.check(B.load().muse_group_fill_synthetic(dg._h, 0, M, 0, ctypes.c_uint64(2), ctypes.c_uint32(0), None))
    assert dg.spectrum_cache()[0] == 0
    want, _ = _plain(muse, eng, dg.read(0, M), ref)
    assert eng.kernel_name(db).startswith("xcorr_fused_n4096_fold")
    _same(db.scores(), want, "first pass over the new rows")
    assert dg.spectrum_cache() == (0, 0)
    _same(db.scores(), want, "writer over the new rows")
    assert dg.spectrum_cache()[0] == M
    _same(db.scores(), want, "reader over the new rows")
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. off, declined, dropped
def test_mode_budget_and_drop(muse, eng):
    M = 1000
    rows, ref = _planted(M, 4096, 21)
    want, _ = _plain(muse, eng, rows, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    eng.set_spectrum_cache(False)
    for k in range(3):
        _same(db.scores(), want, "mode 0")
        assert dg.spectrum_cache() == (0, 0)
    eng.set_spectrum_cache(True)
    eng.spectrum_cache_limits(min_rows=2, budget_bytes=0)
    for k in range(3):
        _same(db.scores(), want, "declined")
        assert dg.spectrum_cache() == (0, 0) and eng.kernel_name(db).startswith("xcorr_fused_n4096_fold")
    db.close()
    dg.close()
    eng.spectrum_cache_limits(min_rows=2)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for k in range(3):
        _same(db.scores(), want, "before the drop")
    assert dg.spectrum_cache() == (M, (M // 2) * PAIR_BYTES)
    dg.drop_spectrum_cache()
    assert dg.spectrum_cache() == (0, 0) and eng.kernel_name(db).startswith("xcorr_fused_n4096_fold")
    _same(db.scores(), want, "behind the drop")
    assert dg.spectrum_cache() == (0, 0)
    _same(db.scores(), want, "rebuilt")
    assert dg.spectrum_cache()[0] == M
    _same(db.scores(), want, "read again")
    db.close()
    dg.close()


# ------------------------------------------------------------------ 6. Runs
def test_runs_give_the_same_records(muse, eng):
    M, N = 66000, 4096                       # above 65 536 series: Run(nil) selects on the device
    eng.spectrum_cache_limits()              # the default limits apply to a group of this size
    gid = (np.arange(M) % 97).astype(np.int32)
    outs = []
    for on in (False, True):
        eng.set_spectrum_cache(on)
        dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=3, copies=False)
        db = muse.DeviceBatch(eng, dg, ref)
        db.scores()
        db.scores()
        assert (dg.spectrum_cache()[0] == M) == on
        assert eng.kernel_name(db).startswith("xcorr_cached_n4096" if on else "xcorr_fused_n4096_fold")
        outs.append((db.run(None, 0, 15, 20, 0.0, 0, True), db.run(gid, 97, 15, 20, 0.0, 0, True),
                     db.run_shard(None, 0, 12345, 15, 20, 0.0, 0, True), db.run_shard(gid, 97, 12345, 15, 20, 0.0, 0, True)))
        db.close()
        dg.close()
    eng.set_spectrum_cache(True)
    off, on = outs
    for a, b in zip(off[:2], on[:2]):
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u, v)
        assert a[3] == b[3] or (np.isnan(a[3]) and np.isnan(b[3]))
    for a, b in zip(off[2:], on[2:]):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 7. a leading zero pad
def test_padded_length(muse, eng):
    M, N = 1001, 3000
    rows, ref = _planted(M, N, 31)
    want, redo = _plain(muse, eng, rows, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    for k in range(4):
        _same(db.scores(), want, "pass %d" % (k + 1))
        assert sorted(db.redo_pairs().tolist()) == redo
    assert dg.spectrum_cache() == (M & ~1, (M // 2) * PAIR_BYTES) and eng.kernel_name(db) == "xcorr_cached_n4096<true>"
    db.close()
    dg.close()


# ------------------------------------------------------------------ 8. two host threads across the build
def test_two_threads_two_batches_one_group(muse, eng):
    M = 4097
    rows, ref = _planted(M, 4096, 41)
    refs = [ref, np.random.default_rng(42).standard_normal(4096)]
    wants = [_plain(muse, eng, rows, r)[0] for r in refs]
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, r) for r in refs]
    dbs[0].scores()                          # pass 1: the next one builds
    gate = threading.Barrier(2)
    got, errs = [[], []], []

    def work(i):
        try:
            for _ in range(3):
                gate.wait()
                got[i].append(dbs[i].scores())
        except Exception as e:               # noqa: BLE001 (reported below)
            errs.append(e)
            gate.abort()
    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    for i in range(2):
        for k, g in enumerate(got[i]):
            _same(g, wants[i], "thread %d pass %d" % (i, k))
    assert dg.spectrum_cache() == (M & ~1, (M // 2) * PAIR_BYTES)   # built once
    for b in dbs:
        b.close()
    dg.close()


# ------------------------------------------------------------------ 9. everything goes back
def test_memory_is_returned(muse):
    import torch
    e = muse.Engine(0)
    e.spectrum_cache_limits(min_rows=2)
    e.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    M = 8192
    dg, ref = muse.DeviceGroup.synthetic(e, M, 4096, seed=9)
    db = muse.DeviceBatch(e, dg, ref)
    for _ in range(3):
        db.scores()
    cache_bytes = dg.spectrum_cache()[1]
    assert cache_bytes == (M // 2) * PAIR_BYTES
    assert torch.cuda.mem_get_info(0)[0] <= free0 - cache_bytes
    db.close()
    dg.close()
    e.trim()
    assert e.pool_stats() == (0, 0, 0, 0)
    assert torch.cuda.mem_get_info(0)[0] >= free0 - cache_bytes // 2   # the cache's bytes are gone
    e.close()
