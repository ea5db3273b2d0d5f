"""GPU tests of muse_group_slide (row_slide.hip): rows of a resident group moved forward in time, in place in HBM.  Run with
-m gpu on an MI355X.

Expected row contents are computed in numpy -- np.concatenate([rows[:, k:], tails], 1), rounded through float32 for float32
groups -- and compared bit for bit.  Expected scores come from a FRESH group uploaded with those rows through the unchanged
upload path, never from a slid group."""
import ctypes

import numpy as np
import pytest

from _load import pkg

pytestmark = pytest.mark.gpu


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


def _rows(M, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, N)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e-40)   # (1e-40: a denormal once narrowed to float32)


def _planted(M, N, seed):
    """noise with NaN, +-Inf, -0.0 and denormals planted in about one sample in 40 (at least one per array)"""
    x = _rows(M, N, seed)
    rng = np.random.default_rng(seed + 1000003)
    flat = x.reshape(-1)
    at = rng.choice(flat.shape[0], size=max(1, flat.shape[0] // 40), replace=False)
    flat[at] = np.array(SPECIALS)[np.arange(at.shape[0]) % len(SPECIALS)]
    return x


def _stored(x, f32):
    """what a group of that storage type holds for the float64 samples x"""
    with np.errstate(all="ignore"):
        return x.astype(np.float32).astype(np.float64) if f32 else np.array(x, dtype=np.float64)


def _slid(cur, tails, f32, first=0):
    out = cur.copy()
    count, k = tails.shape
    out[first:first + count] = np.concatenate([cur[first:first + count, k:], _stored(tails, f32)], 1)
    return out


def _same_bytes(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def _ks(N):
    ks = []
    for k in (1, 2, 3, 7, 16, N // 2, N - 1, N):
        k = min(max(k, 1), N)
        if k not in ks:
            ks.append(k)
    return ks


# ------------------------------------------------------------------ 1. contents, bit for bit
CONTENT_SHAPES = [(False, N, M) for N in (2, 3, 8, 255, 480, 1433, 4096, 5000) for M in (1, 17, 1001)] + \
                 [(False, N, M) for N in (40000, 70000) for M in (1, 5, 17)] + \
                 [(True, N, M) for N in (480, 1433, 4096, 5000) for M in (1, 17, 1001)]


@pytest.mark.parametrize("f32,N,M", CONTENT_SHAPES)
def test_slide_contents_bit_for_bit(muse, eng, f32, N, M):
    """one group per shape, slid again and again (composition): every unit width, pieces that end inside a row, rows shorter than
    one piece, k larger than a piece, k = N"""
    x = _planted(M, N, 7 * N + M)
    dg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
    cur = _stored(x, f32)
    assert _same_bytes(dg.read(0, M), cur)
    for i, k in enumerate(_ks(N)):
        tails = _planted(M, k, 31 * N + M + i)
        dg.slide(tails)
        cur = _slid(cur, tails, f32)
        got = dg.read(0, M)
        assert _same_bytes(got, cur), (k, np.argwhere(got.view(np.uint64) != cur.view(np.uint64))[:4])
    assert dg.slides == len(_ks(N)) and dg.M == M
    dg.close()


def test_slide_takes_strided_and_non_contiguous_tails(muse, eng):
    N, M, k = 480, 9, 6
    x = _rows(M, N, 1)
    dg = muse.DeviceGroup.from_rows(eng, x)
    wide = _rows(M, 4 * k, 2)
    cur = x
    for tails in (wide[:, k:2 * k], wide[:, ::4], wide[::-1, :k]):   # a row stride above k; a strided last axis; rows backwards
        dg.slide(tails)
        cur = _slid(cur, np.array(tails), False)
        assert _same_bytes(dg.read(0, M), cur)
    dg.close()


# ------------------------------------------------------------------ 2. row ranges
@pytest.mark.parametrize("f32,N,k", [(False, 480, 2), (False, 481, 3), (False, 5000, 1200), (True, 480, 4), (True, 482, 2), (True, 481, 1)])
def test_slide_row_ranges_leave_the_other_rows(muse, eng, f32, N, k):
    M = 40
    x = _planted(M, N, N + k)
    dg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
    cur = _stored(x, f32)
    for i, (first, count) in enumerate(((0, 1), (M - 1, 1), (3, 10), (0, M))):
        tails = _planted(count, k, 50 + i)
        dg.slide(tails, first=first)
        cur = _slid(cur, tails, f32, first)
        assert _same_bytes(dg.read(0, M), cur), (first, count)
    dg.close()


# ------------------------------------------------------------------ 3. neighbours
@pytest.mark.parametrize("f32", [False, True])
def test_slide_then_append_into_the_spare_capacity(muse, eng, f32):
    N, M, k = 1433, 33, 5
    dg = muse.DeviceGroup(eng, N, capacity=M + 8, f32=f32)
    x, more = _rows(M, N, 3), _rows(8, N, 4)
    dg.append(x)
    tails = _rows(M, k, 5)
    dg.slide(tails)
    dg.append(more)
    assert dg.M == M + 8
    want = np.vstack([_slid(_stored(x, f32), tails, f32), _stored(more, f32)])
    assert _same_bytes(dg.read(0, M + 8), want)
    dg.slide(_rows(8, k, 6), first=M)            # the appended rows alone: the slid ones in front of them stay
    want = _slid(want, _rows(8, k, 6), f32, M)
    assert _same_bytes(dg.read(0, M + 8), want)
    dg.close()


@pytest.mark.parametrize("f32", [False, True])
def test_slide_right_behind_single_row_appends(muse, eng, f32):
    """rows still packed in the staging buffer are sent first"""
    N, M, k = 480, 57, 3
    x = _rows(M, N, 8)
    dg = muse.DeviceGroup(eng, N, capacity=0, f32=f32)
    for r in range(M):
        dg.append(x[r])
    tails = _rows(M, k, 9)
    dg.slide(tails)
    cur = _slid(_stored(x, f32), tails, f32)
    assert _same_bytes(dg.read(0, M), cur)
    dg.append(x[0])                               # and the staging state is as the appends left it
    dg.slide(_rows(2, k, 10), first=M - 1)
    cur = _slid(np.vstack([cur, _stored(x[:1], f32)]), _rows(2, k, 10), f32, M - 1)
    assert _same_bytes(dg.read(0, M + 1), cur)
    dg.close()


# ------------------------------------------------------------------ 4. every cache follows
def _scores_match(muse, eng, db, fb, fresh_scores):
    """bit for bit; at the project's tolerance (1e-6 relative + 1e-12 absolute, lags exact) only if the two groups legitimately run
    different kernels -- the spectrum cache's reader is documented bit-identical to the kernel it replaces and counts as the same"""
    a, b = eng.kernel_name(db), eng.kernel_name(fb)
    lag, mv = db.scores()
    flag, fmv = fresh_scores
    assert np.array_equal(lag, flag)
    if a == b or (a.startswith("xcorr_cached_n4096") and b.startswith("xcorr_fused_n4096_fold")):
        assert mv.tobytes() == fmv.tobytes(), (a, b, float(np.nanmax(np.abs(mv - fmv))))
    else:
        print("kernels differ: %s / %s" % (a, b))
        assert np.allclose(mv, fmv, rtol=1e-6, atol=1e-12), (a, b)


CACHE_SHAPES = [(False, 480), (False, 4096), (False, 5000), (False, 40000), (False, 70000), (True, 480), (True, 4096)]


@pytest.mark.parametrize("rng", ["whole", "part"])
@pytest.mark.parametrize("f32,N", CACHE_SHAPES)
def test_every_cache_follows_a_slide(muse, eng, f32, N, rng):
    """the spectrum cache (N = 4096 float64), the kept statistics (N = 70000) and the batches' kernel selection describe the old
    rows: the slid group scores exactly as a fresh group uploaded with the new rows"""
    M, k = 200, 5
    first, count = (0, M) if rng == "whole" else (37, 101)
    cached = N == 4096 and not f32
    if cached:
        eng.spectrum_cache_limits(min_rows=64)
    try:
        x, ref = _rows(M, N, N + 11), _rows(1, N, N + 12)[0]
        dg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
        db = muse.DeviceBatch(eng, dg, ref)
        db.scores()
        db.scores()
        if cached:
            assert dg.spectrum_cache()[0] > 0          # a cache really exists
        tails = _rows(count, k, N + 13)
        dg.slide(tails, first=first)
        assert dg.spectrum_cache()[0] == 0
        want = _slid(_stored(x, f32), tails, f32, first)
        assert _same_bytes(dg.read(0, M), want)
        fresh = muse.DeviceGroup.from_rows(eng, want, f32=f32)
        fb = muse.DeviceBatch(eng, fresh, ref)
        fresh_scores = fb.scores()
        _scores_match(muse, eng, db, fb, fresh_scores)
        _scores_match(muse, eng, db, fb, fresh_scores)
        if cached:
            assert dg.spectrum_cache()[0] > 0          # rebuilt by the second pass over the new rows
        _scores_match(muse, eng, db, fb, fresh_scores)     # (read from the rebuilt cache)
        for h in (db, fb, dg, fresh):
            h.close()
    finally:
        if cached:
            eng.spectrum_cache_limits()


def test_a_group_that_slides_between_passes_never_builds_a_cache(muse, eng):
    N, M = 4096, 128
    eng.spectrum_cache_limits(min_rows=64)
    try:
        dg = muse.DeviceGroup.from_rows(eng, _rows(M, N, 21))
        db = muse.DeviceBatch(eng, dg, _rows(1, N, 22)[0])
        for i in range(4):
            db.scores()
            assert dg.spectrum_cache() == (0, 0)
            dg.slide(_rows(M, 2, 23 + i))
        db.close()
        dg.close()
    finally:
        eng.spectrum_cache_limits()


# ------------------------------------------------------------------ 5. other readers of the rows after a slide
def _same_rec(a, b):
    (ra, sa), (rb, sb) = a, b
    return sa == sb and int(ra["series"]) == int(rb["series"]) and int(ra["lag"]) == int(rb["lag"]) and \
        np.float64(ra["score"]).view(np.uint64) == np.float64(rb["score"]).view(np.uint64)


@pytest.mark.parametrize("N", [480, 4096])
def test_other_readers_see_the_slid_rows(muse, eng, N):
    M, k = 200, 5
    x, ref = _rows(M, N, N + 31), _rows(1, N, N + 32)[0]
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), ref)
    contiguous, scattered = np.arange(20, 90), np.random.default_rng(33).integers(0, M, size=60)
    db.set_lag_window(7)
    db.scores()                                       # every reader has seen the old rows
    tmpl.run_group_rows(dg, contiguous)
    tmpl.run_group_rows(dg, scattered)
    tails = _rows(M, k, N + 34)
    dg.slide(tails)
    fresh = muse.DeviceGroup.from_rows(eng, _slid(x, tails, False))
    fb = muse.DeviceBatch(eng, fresh, ref)
    fb.set_lag_window(7)
    lag, mv = db.scores()
    flag, fmv = fb.scores()
    assert eng.kernel_name(db) == eng.kernel_name(fb)
    assert np.array_equal(lag, flag) and mv.tobytes() == fmv.tobytes()
    for idx in (contiguous, scattered):
        for abs_scores in (0, 1):
            assert _same_rec(tmpl.run_group_rows(dg, idx, abs_scores), tmpl.run_group_rows(fresh, idx, abs_scores)), idx[:4]
    for h in (db, fb, tmpl, dg, fresh):
        h.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_rows_and_cache(muse, eng):
    B = muse.binding
    L = B.load()
    N, M = 4096, 200
    eng.spectrum_cache_limits(min_rows=64)
    try:
        x = _rows(M, N, 41)
        dg = muse.DeviceGroup.from_rows(eng, x)
        db = muse.DeviceBatch(eng, dg, _rows(1, N, 42)[0])
        db.scores()
        db.scores()
        cache = dg.spectrum_cache()
        assert cache[0] > 0
        t = np.ascontiguousarray(_rows(M + 1, 8, 43))
        tp = B.dptr(t)

        def unchanged():
            return _same_bytes(dg.read(0, M), x) and dg.spectrum_cache() == cache

        E = B.MUSE_ERR_INVALID
        cases = [
            ((None, 0, 1, tp, 4, 8), E),              # a NULL group
            ((dg._h, -1, 1, tp, 4, 8), E),            # first < 0
            ((dg._h, 0, -1, tp, 4, 8), E),            # count < 0
            ((dg._h, 0, M + 1, tp, 4, 8), E),         # first + count > M
            ((dg._h, M, 1, tp, 4, 8), E),
            ((dg._h, M + 1, 0, tp, 4, 8), E),
            ((dg._h, 0, 1, tp, -1, 8), E),            # k < 0
            ((dg._h, 0, 1, tp, N + 1, N + 1), E),     # k > N
            ((dg._h, 0, 2, tp, 4, 3), E),             # tail_stride < k
            ((dg._h, 0, 1, None, 4, 8), E),           # NULL tails with something to move
            ((dg._h, 0, M, tp, 0, 8), B.MUSE_OK),     # k == 0
            ((dg._h, 0, M, None, 0, 0), B.MUSE_OK),
            ((dg._h, 5, 0, tp, 4, 8), B.MUSE_OK),     # count == 0
            ((dg._h, M, 0, None, 4, 8), B.MUSE_OK),
        ]
        for i, (args, want) in enumerate(cases):
            assert L.muse_group_slide(*args) == want, (i, args[1:3], args[4:])
            assert unchanged(), i
        assert dg.slides == 0
        with pytest.raises(muse.binding.MuseError):
            dg.slide(np.zeros((1, N + 1)))
        with pytest.raises(ValueError):
            dg.slide(np.zeros(4))
        assert dg.slides == 0
        # an open staging window
        win = dg.stage(1)
        assert win.shape[0] == 1
        assert L.muse_group_slide(dg._h, 0, 1, tp, 4, 8) == E
        assert L.muse_group_slide(dg._h, 0, 1, tp, 0, 8) == E
        win[0, :] = 1.5
        dg.commit(0, 1)
        assert dg.M == M + 1
        assert _same_bytes(dg.read(0, M), x) and dg.spectrum_cache() == cache
        db.close()
        dg.close()
    finally:
        eng.spectrum_cache_limits()


# ------------------------------------------------------------------ 7. the counter and the mirror's homes
def test_slides_counts_and_a_slid_home_goes_back_to_the_host(muse, eng):
    m = muse.muse
    N, M = 480, 12
    x = _rows(M, N, 51)
    ser = [muse.NewSeries(x[i]) for i in range(M)]
    g1 = muse.NewGroup("first")
    g1.Add(*ser)
    dg1 = g1._device_group(eng)
    assert dg1.slides == 0
    assert [m.live_home(s, eng, N) for s in ser] == [(dg1, i) for i in range(M)]
    assert m.plan_rows(ser, eng, N) == [("device", 0, M, dg1, list(range(M)))]
    dg1.slide(np.zeros((M, 0)))
    dg1.slide(np.zeros((0, 3)))
    assert dg1.slides == 0 and m.live_home(ser[0], eng, N) == (dg1, 0)
    dg1.slide(_rows(M, 3, 52))
    dg1.slide(_rows(2, 1, 53), first=4)
    assert dg1.slides == 2
    assert m.plan_rows(ser, eng, N) == [("host", 0, M)]
    g2 = muse.NewGroup("second")
    g2.Add(*ser)
    dg2 = g2._device_group(eng)
    assert _same_bytes(dg2.read(0, M), x)            # the Series' own values, not what the slid rows hold now
    assert [m.live_home(s, eng, N) for s in ser] == [(dg2, i) for i in range(M)]
    dg1.close()
    dg2.close()
