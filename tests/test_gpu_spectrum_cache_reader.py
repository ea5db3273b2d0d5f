"""GPU tests of the spectrum cache's reader at two workgroups per CU (xcorr_cached_n4096 in xcorr_r16_cached.hip; DESIGN.md
4.10).  Run with -m gpu on an MI355X.

The reader keeps the reference's table in registers for the whole launch, requests a pair's spectrum a whole pair ahead and
claims its pairs in chunks of two, two chunks ahead.  For every shape it is compared with the reader at four workgroups per
CU it replaced (test hook muse_test_spectrum_cache_reader) and with the plain kernel with the cache off on a fresh group
holding the same rows: equal lags, scores equal bit for bit (NaN included), the same pairs listed for the rescaling kernel.
The shapes are chosen by what a workgroup of the resident grid G = 2 x CUs gets: half a chunk, one chunk and nothing past it,
exactly one workgroup with a second chunk (of one pair), three or more chunks each (both claim slots and both record
parities reused), a trailing uncached row, a second segment (pair0 > 0), the padded build."""
import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu

NEW, OLD = "xcorr_cached_n4096<%s>", "xcorr_cached_n4096_occ4<%s>"


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
    """as test_gpu_spectrum_cache.py::_planted"""
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
    (lag, mv), redo = got
    (wlag, wmv), wredo = want
    assert np.array_equal(lag, wlag), what
    assert np.array_equal(mv.view(np.uint64), wmv.view(np.uint64)), what
    assert redo == wredo, what


def _pass(db):
    out = db.scores()
    return out, sorted(db.redo_pairs().tolist())


def _plain(muse, eng, rows, ref):
    """the plain kernel on a fresh group with the cache off"""
    eng.set_spectrum_cache(False)
    try:
        dg = muse.DeviceGroup.from_rows(eng, rows)
        db = muse.DeviceBatch(eng, dg, ref)
        out = _pass(db)
        assert "cached" not in eng.kernel_name(db) and dg.spectrum_cache() == (0, 0)
        db.close()
        dg.close()
    finally:
        eng.set_spectrum_cache(True)
    return out


def _both_readers(eng, db, want, padded, what):
    """one pass with each reader over a valid cache: each equal to `want`, and so to each other"""
    for hook, name in ((0, NEW), (1, OLD), (0, NEW)):
        eng.spectrum_cache_reader(hook)
        assert eng.kernel_name(db) == name % padded, what
        _same(_pass(db), want, "%s, reader %d" % (what, hook))
    eng.spectrum_cache_reader(0)


def _shape(eng, case):
    G = 2 * eng.device_info()[1]             # the reader's resident grid
    return {"one pair": 2, "single row": 3, "two pairs": 4, "one second pair": 2 * (G + 1),
            "three pairs each": 2 * (3 * G + 1) + 1,
            # in chunks of two pairs (ZC_CLAIM): G + 1 chunks, the last one of one pair; 3 G chunks and one pair, odd M (~200 MB)
            "one second chunk": 2 * (2 * G + 1), "three chunks each": 2 * (6 * G + 1) + 1}[case]


@pytest.mark.parametrize("case", ["one pair", "single row", "two pairs", "one second pair", "three pairs each",
                                  "one second chunk", "three chunks each"])
def test_readers_and_plain_kernel_agree(muse, eng, case):
    M = _shape(eng, case)
    rows, ref = _planted(M, 4096, M)
    want = _plain(muse, eng, rows, ref)
    if M >= 16:
        assert len(want[1]) >= 4
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    _same(_pass(db), want, "first pass")
    _same(_pass(db), want, "writer")
    assert dg.spectrum_cache()[0] == M & ~1
    _both_readers(eng, db, want, "false", "M = %d" % M)
    db.close()
    dg.close()


@pytest.mark.parametrize("N", [2049, 3000])
def test_padded_lengths(muse, eng, N):
    M = 1001
    rows, ref = _planted(M, N, N)
    want = _plain(muse, eng, rows, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    _pass(db)
    _same(_pass(db), want, "writer")
    _both_readers(eng, db, want, "true", "N = %d" % N)
    db.close()
    dg.close()


def test_second_segment(muse, eng):
    """rows appended behind a valid cache: the reader on the first segment with the writer on the tail, then the reader on both
    segments, the second one with pair0 > 0"""
    rows, ref = _planted(1600, 4096, 3)
    dg = muse.DeviceGroup.from_rows(eng, rows[:1000])
    db = muse.DeviceBatch(eng, dg, ref)
    for _ in range(3):
        _pass(db)
    assert dg.spectrum_cache()[0] == 1000
    dg.append(rows[1000:])
    want = _plain(muse, eng, rows, ref)
    _same(_pass(db), want, "reader + writer over the tail")
    assert dg.spectrum_cache()[0] == 1600
    _both_readers(eng, db, want, "false", "two segments")
    db.close()
    dg.close()


def test_another_reference_on_the_same_cache(muse, eng):
    """the registers a launch keeps come from that batch's table"""
    M = 1000
    rows, ref = _planted(M, 4096, 5)
    ref2 = np.random.default_rng(6).standard_normal(4096)
    want, want2 = _plain(muse, eng, rows, ref), _plain(muse, eng, rows, ref2)
    assert not np.array_equal(want[0][1].view(np.uint64), want2[0][1].view(np.uint64))
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    _pass(db)
    _pass(db)
    db2 = muse.DeviceBatch(eng, dg, ref2)
    assert eng.kernel_name(db2) == NEW % "false"
    _same(_pass(db2), want2, "second batch, first pass")
    _both_readers(eng, db, want, "false", "first batch")
    _both_readers(eng, db2, want2, "false", "second batch")
    db.close()
    db2.close()
    dg.close()


def test_reader_hook_rejects_other_values(muse, eng):
    with pytest.raises(Exception):
        eng.spectrum_cache_reader(2)
    eng.spectrum_cache_reader(0)
