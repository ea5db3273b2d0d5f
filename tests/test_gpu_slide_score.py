"""GPU tests of muse_batch_slide_score_windowed / muse_batch_slide_run_windowed (xcorr_window_slide.hip): a resident group's rows
moved forward in time and scored inside a lag window in one pass.  Run with -m gpu on an MI355X.

Everything is held to BIT IDENTITY against code that does not know the fused kernel: expected rows are the numpy slide
np.concatenate([rows[:, k:], tails], 1); expected scores come from a FRESH group uploaded with those rows, set_lag_window(L),
score(), read_scores()."""
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


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 5e-324, 1e-40)


def _planted(M, N, seed):
    """noise with NaN, +-Inf, -0.0 and denormals planted in about one sample in 40 (at least one per array)"""
    x = _rows(M, N, seed)
    rng = np.random.default_rng(seed + 1000003)
    flat = x.reshape(-1)
    at = rng.choice(flat.shape[0], size=max(1, flat.shape[0] // 40), replace=False)
    flat[at] = np.array(SPECIALS)[np.arange(at.shape[0]) % len(SPECIALS)]
    return x


def _mixed(M, N, seed):
    """rows for the score comparisons: clean noise, every fourth row (1, 5, ...) with specials planted (its score is NaN: compared as
    bytes), every eighth (2, 10, ...) constant (sigma == 0 as long as its tails are the same constant)"""
    x = _rows(M, N, seed)
    sp = _planted(M, N, seed + 7)
    x[1::4] = sp[1::4]
    x[1::4, -1] = np.nan      # (whatever the planting drew: a slid row keeps this one unless k = N, and its tail brings another)
    x[2::8] = 1.5
    return x


def _slid(cur, tails):
    return np.concatenate([cur[:, tails.shape[1]:], tails], 1)


def _same_bytes(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def _diff(got, want):
    return np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:4].tolist()


def _fresh_scores(muse, eng, rows, ref, L):
    """(lag, mv) of the windowed pass as the parent commit computes it: a fresh group, the batch's own window, score()"""
    fresh = muse.DeviceGroup.from_rows(eng, rows)
    fb = muse.DeviceBatch(eng, fresh, ref)
    fb.set_lag_window(L)
    fb.score()
    out = fb.read_scores()
    fb.close()
    fresh.close()
    return out


def _same_scores(got, want):
    (lag, mv), (flag, fmv) = got, want
    return lag.tobytes() == flag.tobytes() and mv.tobytes() == fmv.tobytes()


KS = (1, 2, 3, 7, 16, 63, 64, 65, 255, 256, 257)


def _ks(N):
    ks = []
    for k in KS + (N // 2, N - 1, N):
        k = min(max(k, 1), N)
        if k not in ks:
            ks.append(k)
    return ks


# ------------------------------------------------------------------ 1. rows, bit for bit
ROW_SHAPES = [(N, M) for N in (2, 3, 63, 64, 65, 480, 1023, 1024, 1025, 1433, 4096, 5000) for M in (1, 15, 16, 17, 1001)] + \
             [(N, M) for N in (40000, 65536) for M in (5, 17)]


@pytest.mark.parametrize("N,M", ROW_SHAPES)
def test_rows_bit_for_bit(muse, eng, N, M):
    """one group per shape, slid by every k in turn through the fused call and read back after each (one call, then compositions):
    every load / store width, k below, at and above a piece and a four-piece round, the kept / tail boundary inside a lane's pair,
    partial 16-row blocks, rows shorter than one piece, k = N"""
    x = _planted(M, N, 7 * N + M)
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, _rows(1, N, N + 5)[0])
    cur = x
    ks = _ks(N)
    for i, k in enumerate(ks):
        tails = _planted(M, k, 31 * N + M + i)
        db.slide_score_windowed(tails, 7)
        cur = _slid(cur, tails)
        got = dg.read(0, M)
        assert _same_bytes(got, cur), (k, _diff(got, cur))
    assert dg.slides == len(ks) and dg.M == M
    db.close()
    dg.close()


def test_takes_strided_and_non_contiguous_tails(muse, eng):
    N, M, k = 480, 9, 6
    x = _rows(M, N, 1)
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, _rows(1, N, 3)[0])
    wide = _rows(M, 4 * k, 2)
    cur = x
    for tails in (wide[:, k:2 * k], wide[:, ::4], wide[::-1, :k]):   # a row stride above k; a strided last axis; rows backwards
        db.slide_score_windowed(tails, 7)
        cur = _slid(cur, np.array(tails))
        assert _same_bytes(dg.read(0, M), cur)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 2. scores, bit for bit
# accumulator tiles of a window: ceil((2 L + 1) / 16) -- L = 0, 1, 7: 1; 8, 15: 2; 16: 3; 24: 4; 32: 5; 40: 6; 48: 7; 63: 8
WINDOWS = (0, 1, 7, 8, 15, 16, 24, 32, 40, 48, 63)
# per mapping / load width two shapes: (N, M, k) -- odd N: the narrow mapping; even N, odd k: WIDE with 8-byte loads; even N, even
# k: WIDE with 16-byte loads.  Several chunks (N > 1024), a partial last piece, partial blocks, a tail inside / across pieces
BUILD_SHAPES = [(1433, 17, 7), (1025, 1001, 64), (4096, 17, 3), (480, 1001, 65), (4096, 16, 16), (5000, 1001, 256)]
SCORE_CASES = [(N, M, k, L) for L in WINDOWS for (N, M, k) in BUILD_SHAPES] + \
              [(N, M, k, 7) for N in (2, 3, 63, 64, 65, 480, 1023, 1024, 1025, 1433, 4096, 5000) for M in (15, 17)
               for k in (1, 16, N // 2, N) if 1 <= k <= N and (N, M, k) not in BUILD_SHAPES] + \
              [(N, 5, k, L) for N in (40000, 65536) for (k, L) in ((1, 7), (16, 15), (N, 7))]
SCORE_CASES = list(dict.fromkeys(SCORE_CASES))


@pytest.mark.parametrize("N,M,k,L", SCORE_CASES)
def test_scores_bit_for_bit(muse, eng, N, M, k, L):
    x, ref = _mixed(M, N, 3 * N + M + k), _rows(1, N, N + 17)[0]
    tails = _mixed(M, k, 5 * N + M + k + L)
    want_rows = _slid(x, tails)
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    db.slide_score_windowed(tails, L)
    got = db.read_scores()
    got_rows = dg.read(0, M)
    assert _same_bytes(got_rows, want_rows), _diff(got_rows, want_rows)
    want = _fresh_scores(muse, eng, want_rows, ref, L)
    assert _same_scores(got, want), (np.flatnonzero(got[0] != want[0])[:4], np.flatnonzero(got[1].view(np.uint64) != want[1].view(np.uint64))[:4])
    assert np.isnan(want[1][1])                                   # the comparison saw NaN scores ...
    if N >= 8:
        assert np.isfinite(want[1][0]) and want[1][0] != 0.0      # ... and real ones
    # the later stand-alone pass over the slid rows sums in the same order: the same bits again
    db.set_lag_window(L)
    db.score()
    assert _same_scores(db.read_scores(), want)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. many co-resident workgroups
BIG_M, BIG_N = 5000, 4096


@pytest.fixture(scope="module")
def big():
    return _rows(BIG_M, BIG_N, 901), _rows(1, BIG_N, 902)[0]


@pytest.mark.parametrize("k", [1, 16, 64, 1000])
def test_many_workgroups(muse, eng, big, k):
    """313 workgroups of four waves running side by side: a race between waves or rounds shows here"""
    x, ref = big
    tails = _rows(BIG_M, k, 903 + k)
    want_rows = _slid(x, tails)
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    db.slide_score_windowed(tails, 7)
    got = db.read_scores()
    got_rows = dg.read(0, BIG_M)
    db.close()
    dg.close()
    assert _same_bytes(got_rows, want_rows), _diff(got_rows, want_rows)
    assert _same_scores(got, _fresh_scores(muse, eng, want_rows, ref, 7))


# ------------------------------------------------------------------ 4. slide_run_windowed
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("N,k,L,abs_scores", [(480, 16, 7, True), (1433, 3, 15, False), (4096, 16, 7, False)])
def test_slide_run_windowed_matches_run_on_a_fresh_windowed_batch(muse, eng, N, k, L, abs_scores, grouped):
    M, G = 600, 37
    x, ref = _mixed(M, N, N + 61), _rows(1, N, N + 62)[0]
    tails = _mixed(M, k, N + 63)
    gid = (np.arange(M) * 7 % G).astype(np.int32) if grouped else None
    kw = dict(group_id=gid, G=G if grouped else 0, top_n=10, threshold=0.0, sign_filter=0, abs_scores=abs_scores)
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    got = db.slide_run_windowed(tails, L, **kw)
    assert _same_bytes(dg.read(0, M), _slid(x, tails))
    fresh = muse.DeviceGroup.from_rows(eng, _slid(x, tails))
    fb = muse.DeviceBatch(eng, fresh, ref)
    fb.set_lag_window(L)
    want = fb.run(max_lag=L, **kw)
    assert len(want[0]) > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes()
    assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes()
    assert db.last_run_path() == 0 and db.lag_window() == -1
    for h in (db, fb, dg, fresh):
        h.close()


# ------------------------------------------------------------------ 5. state
def test_window_is_an_argument_and_refusals_leave_the_rows(muse, eng):
    B = muse.binding
    lib = B.load()
    N, M, k = 480, 50, 4
    x, ref = _planted(M, N, 71), _rows(1, N, 72)[0]
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    t = np.ascontiguousarray(_rows(M, k, 73))
    tp = B.dptr(t)

    def unchanged():
        return _same_bytes(dg.read(0, M), x)

    # the batch's own window: off stays off, equal is accepted and stays, different is refused
    assert db.lag_window() == -1
    db.slide_score_windowed(np.zeros((M, 0)), 7)
    assert db.lag_window() == -1 and unchanged() and dg.slides == 0
    db.set_lag_window(5)
    assert lib.muse_batch_slide_score_windowed(db._h, tp, k, k, 7) == B.MUSE_ERR_INVALID
    assert unchanged() and db.lag_window() == 5
    with pytest.raises(B.MuseError):
        db.slide_score_windowed(t, 7)
    assert dg.slides == 0 and unchanged()
    E = B.MUSE_ERR_INVALID
    for args in ((tp, -1, k, 5), (tp, N + 1, N + 1, 5), (tp, k, k - 1, 5), (None, k, k, 5), (tp, k, k, -1)):
        assert lib.muse_batch_slide_score_windowed(db._h, *args) == E, args[1:]
        assert unchanged()
    assert lib.muse_batch_slide_score_windowed(db._h, tp, k, k, 64) == B.MUSE_ERR_UNSUPPORTED
    assert unchanged() and db.lag_window() == 5
    # a refused selection leaves them too
    o_s, o_l, o_v = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int32), np.zeros(4)
    cnt, mean = ctypes.c_int32(0), ctypes.c_double(0)
    rc = lib.muse_batch_slide_run_windowed(db._h, tp, k, k, None, 0, 5, 4, 0.0, 2, 1, B.i64ptr(o_s), B.i32ptr(o_l), B.dptr(o_v),
                                           ctypes.byref(cnt), ctypes.byref(mean))
    assert rc == E and unchanged()
    # an open staging window
    win = dg.stage(1)
    assert win.shape[0] == 1
    assert lib.muse_batch_slide_score_windowed(db._h, tp, k, k, 5) == E
    win[0, :] = 1.5
    dg.commit(0, 1)
    assert dg.M == M + 1 and unchanged()
    # equal: accepted, the setting stays, the rows move (M + 1 of them now)
    t1 = _rows(M + 1, k, 74)
    db.slide_score_windowed(t1, 5)
    assert db.lag_window() == 5 and dg.slides == 1
    assert _same_bytes(dg.read(0, M + 1), _slid(np.vstack([x, np.full((1, N), 1.5)]), t1))
    with pytest.raises(ValueError):
        db.slide_score_windowed(t, 5)             # the whole group slides: M + 1 tails, not M
    db.close()
    dg.close()


def test_f32_groups_are_refused(muse, eng):
    B = muse.binding
    N, M, k = 480, 20, 4
    x = _rows(M, N, 81)
    dg = muse.DeviceGroup.from_rows(eng, x, f32=True)
    db = muse.DeviceBatch(eng, dg, _rows(1, N, 82)[0])
    held = dg.read(0, M)
    t = np.ascontiguousarray(_rows(M, k, 83))
    assert B.load().muse_batch_slide_score_windowed(db._h, B.dptr(t), k, k, 7) == B.MUSE_ERR_UNSUPPORTED
    assert _same_bytes(dg.read(0, M), held) and dg.slides == 0
    db.close()
    dg.close()


def test_caches_follow_and_k0_leaves_them(muse, eng):
    N, M, k, L = 4096, 200, 16, 7
    eng.spectrum_cache_limits(min_rows=64)
    try:
        x, ref = _rows(M, N, 91), _rows(1, N, 92)[0]
        dg = muse.DeviceGroup.from_rows(eng, x)
        db = muse.DeviceBatch(eng, dg, ref)
        db.scores()
        db.scores()
        cache = dg.spectrum_cache()
        assert cache[0] > 0                             # a cache really exists
        db.slide_score_windowed(np.zeros((M, 0)), L)    # k = 0: the windowed pass alone
        assert dg.slides == 0 and dg.spectrum_cache() == cache
        assert _same_scores(db.read_scores(), _fresh_scores(muse, eng, x, ref, L))
        tails = _rows(M, k, 93)
        db.slide_score_windowed(tails, L)
        assert dg.slides == 1 and dg.spectrum_cache()[0] == 0
        want_rows = _slid(x, tails)
        assert _same_scores(db.read_scores(), _fresh_scores(muse, eng, want_rows, ref, L))
        # a later plain (unwindowed) pass scores the slid rows as a fresh group's
        assert db.lag_window() == -1
        fresh = muse.DeviceGroup.from_rows(eng, want_rows)
        fb = muse.DeviceBatch(eng, fresh, ref)
        flag, fmv = fb.scores()
        lag, mv = db.scores()
        assert np.array_equal(lag, flag)
        if eng.kernel_name(db) == eng.kernel_name(fb):
            assert mv.tobytes() == fmv.tobytes()
        else:
            assert np.allclose(mv, fmv, rtol=1e-6, atol=1e-12), (eng.kernel_name(db), eng.kernel_name(fb))
        for h in (db, fb, dg, fresh):
            h.close()
    finally:
        eng.spectrum_cache_limits()


def test_an_empty_group_is_not_an_error(muse, eng):
    dg = muse.DeviceGroup(eng, 480, 0)
    db = muse.DeviceBatch(eng, dg, _rows(1, 480, 95)[0])
    db.slide_score_windowed(np.zeros((0, 4)), 7)
    assert dg.slides == 0 and dg.M == 0
    db.close()
    dg.close()
