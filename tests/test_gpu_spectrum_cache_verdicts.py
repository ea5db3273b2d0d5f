"""GPU tests of the verdicts the spectrum cache keeps beside its spectra (xcorr_r16_cached.hip, foldk_device.h).
Run with -m gpu on an MI355X.

What does not depend on the reference -- 1 / sigma of a series, "sigma is zero", "the statistics are NaN / Inf", "the pair's
sigmas are too far apart for one shared transform" -- is computed once, by the writer's finalize, and stored in the pair's
statistics record; the two readers only combine.  Every test compares writer and readers with the plain kernel with the cache
off on a fresh group holding the same rows: equal lags, scores equal bit for bit (NaN included), the same pairs listed for the
rescaling kernel.  64 or 65 rows: 32 cached pairs, a fraction of one resident grid -- nothing here depends on the grid."""
import ctypes

import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu

NEW, OLD = "xcorr_cached_n4096<%s>", "xcorr_cached_n4096_occ4<%s>"
KINDS = ["constant", "overflow", "nan", "inf", "tiny", "copy"]
SPREAD_K = [7, 8, 9, 10]   # see test_the_spread_boundary


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


def _noise(M, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, N)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))
    return x, rng.standard_normal(N)


def _plant(x, r, kind, ref):
    if kind == "constant":
        x[r] = 3.5
    elif kind == "overflow":
        x[r] = 2.0 ** 600                    # the squares overflow
    elif kind == "nan":
        x[r, 17] = np.nan
    elif kind == "inf":
        x[r, 5] = np.inf
    elif kind == "tiny":
        x[r] *= 1e-150                       # a tiny variance (and sigmas far apart from the other seat's)
    elif kind == "copy":
        x[r] = ref[:x.shape[1]]              # an exact copy of the reference
    else:
        raise ValueError(kind)


def _planted(M, N, kind, seat, seed):
    """`kind` in seat `seat` of pair 0, a middle pair and the last full pair, and in the trailing single row when M is odd"""
    x, ref = _noise(M, N, seed)
    pairs = M // 2
    for p in (0, pairs // 2, pairs - 1):
        _plant(x, 2 * p + seat, kind, ref)
    if M & 1:
        _plant(x, M - 1, kind, ref)
    return x, ref


def _mixed(M, N, seat, seed):
    """every kind in one group: kind i in seat `seat` of pair 5 i, a NaN in the last full pair and (M odd) in the single row"""
    x, ref = _noise(M, N, seed)
    for i, kind in enumerate(KINDS):
        _plant(x, 2 * (5 * i) + seat, kind, ref)
    _plant(x, 2 * (M // 2 - 1) + seat, "nan", ref)
    if M & 1:
        _plant(x, M - 1, "nan", ref)
    return x, ref


def _same(got, want, what):
    """as test_gpu_spectrum_cache_reader.py::_same"""
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
    """one pass with each reader over a valid cache (hooks 0, 1, 0): each equal to `want`"""
    for hook, name in ((0, NEW), (1, OLD), (0, NEW)):
        eng.spectrum_cache_reader(hook)
        assert eng.kernel_name(db) == name % padded, what
        _same(_pass(db), want, "%s, reader %d" % (what, hook))
    eng.spectrum_cache_reader(0)


def _first_writer_readers(muse, eng, rows, ref, want, padded, what):
    """first pass, writer, then each reader over a fresh group holding `rows`"""
    M = len(rows)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    _same(_pass(db), want, what + ", first pass")
    _same(_pass(db), want, what + ", writer")
    assert dg.spectrum_cache()[0] == M & ~1
    _both_readers(eng, db, want, padded, what)
    db.close()
    dg.close()


def _check_oracle(oracle, rows, ref, got):
    """scores within 1e-6 relative (NaN where the oracle has NaN), lags exact outside the rows the oracle flags as ties"""
    (lag, mv), _ = got
    olag, omv, gap = oracle.batch_scores(ref, rows, nthreads=4)
    nan = np.isnan(omv)
    print("oracle: %d NaN rows, worst relative error %.3g" % (
        int(nan.sum()), float(np.max(np.abs(mv[~nan] - omv[~nan]) / np.maximum(np.abs(omv[~nan]), 1e-300)))))
    assert np.array_equal(np.isnan(mv), nan)
    assert np.all(np.abs(mv[~nan] - omv[~nan]) <= 1e-6 * np.abs(omv[~nan]))
    tie = (gap < 1e-12) | nan
    assert int(np.sum((lag != olag) & ~tie)) == 0


# ------------------------------------------------------------------ 1. every verdict in every seat
@pytest.mark.parametrize("seat", [0, 1], ids=["seat A", "seat B"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [64, 65])
def test_every_verdict_in_every_seat(muse, eng, oracle, M, kind, seat):
    rows, ref = _planted(M, 4096, kind, seat, 100 + 7 * KINDS.index(kind) + seat)
    want = _plain(muse, eng, rows, ref)
    if kind in ("nan", "inf", "tiny"):       # NaN / Inf statistics; 1e-150 against O(1): sigmas too far apart
        assert set(want[1]) >= {0, M // 4, M // 2 - 1}
    _first_writer_readers(muse, eng, rows, ref, want, "false", "M = %d, %s in seat %d" % (M, kind, seat))
    _check_oracle(oracle, rows, ref, want)


# ------------------------------------------------------------------ 2. the spread boundary
def test_the_spread_boundary(muse, eng):
    """sigma_spread_too_wide lists a pair when the exponents of its two variances differ by more than SIGMA_EXP_SPREAD = 32.
    The two rows of a pair are the same noise times 2^k and 2^-k: every sum scales by an exact power of two, so the exponents
    differ by exactly 4 k -- k = 8 (32) is the last that stays, k = 9 (36) the first that goes."""
    M, N = 64, 4096
    rows, ref = _noise(M, N, 200)
    stays, goes = [], []
    for i, k in enumerate(SPREAD_K):
        for order in (0, 1):                 # the larger series in seat A, in seat B
            p = 3 + 4 * (2 * i + order)      # pairs 3, 7, ..., 31 (the last full pair)
            z = rows[2 * p].copy()
            rows[2 * p + order] = np.ldexp(z, k)
            rows[2 * p + 1 - order] = np.ldexp(z, -k)
            (goes if 4 * k > 32 else stays).append(p)
    want = _plain(muse, eng, rows, ref)
    assert len(stays) == 4 and len(goes) == 4
    assert set(goes) <= set(want[1]) and not set(stays) & set(want[1])
    _first_writer_readers(muse, eng, rows, ref, want, "false", "spread boundary")


# ------------------------------------------------------------------ 3. a leading zero pad
@pytest.mark.parametrize("seat", [0, 1], ids=["seat A", "seat B"])
@pytest.mark.parametrize("kind", KINDS)
def test_padded_length(muse, eng, kind, seat):
    M, N = 65, 3000
    rows, ref = _planted(M, N, kind, seat, 300 + 7 * KINDS.index(kind) + seat)
    want = _plain(muse, eng, rows, ref)
    _first_writer_readers(muse, eng, rows, ref, want, "true", "N = %d, %s in seat %d" % (N, kind, seat))


# ------------------------------------------------------------------ 4. verdicts follow the rows
@pytest.mark.parametrize("seat", [0, 1], ids=["seat A", "seat B"])
def test_appended_rows_get_their_own_verdicts(muse, eng, seat):
    """40 rows cached and a single one behind them, 25 appended: the former single row becomes seat A of a new cached pair, and
    the second segment has pair0 > 0"""
    N = 4096
    rows, ref = _noise(66, N, 400 + seat)
    for i, kind in enumerate(KINDS):         # in the appended rows only: pairs 20 (its seat A: the former single row), 22, ..., 30
        _plant(rows, 2 * (20 + 2 * i) + seat, kind, ref)
    dg = muse.DeviceGroup.from_rows(eng, rows[:41])
    db = muse.DeviceBatch(eng, dg, ref)
    want = _plain(muse, eng, rows[:41], ref)
    for k in range(3):
        _same(_pass(db), want, "41 rows, pass %d" % k)
    assert dg.spectrum_cache()[0] == 40
    dg.append(rows[41:])
    want = _plain(muse, eng, rows, ref)
    assert len(want[1]) >= 3
    _same(_pass(db), want, "reader + writer over the tail")
    assert dg.spectrum_cache()[0] == 66
    _same(_pass(db), want, "reader over both segments")
    _both_readers(eng, db, want, "false", "two segments")
    db.close()
    dg.close()


def test_rewritten_rows_get_new_verdicts(muse, eng):
    """rows rewritten below M, by muse_group_fill_synthetic and then by muse_group_slide: the cache is dropped and rebuilt"""
    M, N, k = 64, 4096, 24
    dg, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=1)
    db = muse.DeviceBatch(eng, dg, ref)
    for _ in range(3):
        _pass(db)
    assert dg.spectrum_cache()[0] == M
    B = muse.binding
    B.check(B.load().muse_group_fill_synthetic(dg._h, 0, M, 0, ctypes.c_uint64(2), ctypes.c_uint32(0), None))
    assert dg.spectrum_cache()[0] == 0
    tails = np.random.default_rng(401).standard_normal((M, k))
    tails[0, 3] = np.nan                     # new verdicts: NaN statistics in seat A of pair 0 and seat B of the last pair,
    tails[M - 1, k - 1] = np.inf
    tails[10] *= 2.0 ** 40                   # a series that no longer fits its neighbour's scale
    for step in ("fill_synthetic", "slide"):
        if step == "slide":
            dg.slide(tails)
            assert dg.spectrum_cache()[0] == 0
        want = _plain(muse, eng, dg.read(0, M), ref)
        _same(_pass(db), want, step + ", first pass")
        _same(_pass(db), want, step + ", writer")
        assert dg.spectrum_cache()[0] == M
        _both_readers(eng, db, want, "false", step)
    assert {0, M // 2 - 1} <= set(want[1])
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. the verdicts are shared, the scores are not
@pytest.mark.parametrize("seat", [0, 1], ids=["seat A", "seat B"])
def test_a_second_reference_on_the_same_cache(muse, eng, seat):
    M = 65
    rows, ref = _mixed(M, 4096, seat, 500 + seat)
    ref2 = np.random.default_rng(501).standard_normal(4096)
    want, want2 = _plain(muse, eng, rows, ref), _plain(muse, eng, rows, ref2)
    assert not np.array_equal(want[0][1].view(np.uint64), want2[0][1].view(np.uint64))
    assert want[1] == want2[1] and len(want[1]) >= 4      # which pairs are redone does not depend on the reference
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    _pass(db)
    _pass(db)
    db2 = muse.DeviceBatch(eng, dg, ref2)
    assert eng.kernel_name(db2) == NEW % "false"
    _both_readers(eng, db2, want2, "false", "second reference")
    _both_readers(eng, db, want, "false", "first reference")
    db.close()
    db2.close()
    dg.close()
