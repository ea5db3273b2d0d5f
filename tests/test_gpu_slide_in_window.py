"""GPU tests of muse_batch_slide_score_in_window / _slide_run_in_window / _slide_run: a resident group's rows moved forward in time and
scored inside a lag window of any width (or unwindowed), float64 or float32 storage, in one call -- at FFT length 4096 in ONE pass of
the default kernel (the SLIDE builds of xcorr_fused_n4096_fold).  Run with -m gpu on an MI355X.

Everything is held to BIT IDENTITY against code that does not know the new kernel: expected rows are the numpy slide
np.concatenate([rows[:, k:], tails], 1) (float32 storage: of the narrowed values); expected scores come from a FRESH group uploaded
with those rows, score_in_window(L), read_scores()."""
import ctypes

import numpy as np
import pytest

import _slidein as SI
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


def _mixed(M, N, seed, every=4):
    """rows for the score comparisons: clean noise, every `every`-th row (1, 1 + every, ...) with specials planted (its score is NaN:
    compared as bytes), every 2 `every`-th (2, ...) constant (sigma == 0 as long as its tails are the same constant).  Large groups
    plant sparsely: with a NaN series in more than one pair in eight the pass would learn to hand the rows to the rescaling kernel,
    and the next call would rightly take two steps."""
    x = _rows(M, N, seed)
    sp = _planted(M, N, seed + 7)
    x[1::every] = sp[1::every]
    x[1::every, -1] = np.nan   # (whatever the planting drew: a slid row keeps this one unless k = N, and its tail brings another)
    x[2::2 * every] = 1.5
    return x


def _every(M):
    return 4 if M < 1024 else 64


def _stored(x, f32):
    """what a group of this storage holds of x, as float64"""
    return np.float32(x).astype(np.float64) if f32 else x


def _slid(cur, tails):
    return np.concatenate([cur[:, tails.shape[1]:], tails], 1)


def _same_bytes(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def _diff(got, want):
    return np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:4].tolist()


def _fresh_scores(muse, eng, rows, ref, L, f32=False):
    """(lag, mv) of the pass as the parent commit computes it: a fresh group of these rows, score_in_window(L)"""
    fresh = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
    fb = muse.DeviceBatch(eng, fresh, ref)
    fb.score_in_window(L)
    out = fb.read_scores()
    fb.close()
    fresh.close()
    return out


def _same_scores(got, want):
    (lag, mv), (flag, fmv) = got, want
    return lag.tobytes() == flag.tobytes() and mv.tobytes() == fmv.tobytes()


def _where(got, want):
    return (np.flatnonzero(got[0] != want[0])[:4].tolist(), np.flatnonzero(got[1].view(np.uint64) != want[1].view(np.uint64))[:4].tolist())


# ------------------------------------------------------------------ 1. the fused kernel: rows and scores, bit for bit
def _ks(N):
    return (1, 2, 3, 16, 255, 256, 257, N // 2, N - 1, N)


WINDOWS = {False: (2048, 64, 257, 2047), True: (2048, 64, 257, 2047, 0, 7)}   # n/2: the plain pass; the others: masked
FUSED_CASES = [(N, M, f32, off) for N in (4096, 4095, 3000, 2049) for M in (1, 2, 3, 2501) for f32 in (False, True)
               for off in range(len(WINDOWS[f32]))]


@pytest.mark.parametrize("N,M,f32,off", FUSED_CASES)
def test_fused_rows_and_scores_bit_for_bit(muse, eng, N, M, f32, off):
    """one group per case, slid by every k in turn through the fused call (one call, then compositions; odd and even k; the kept /
    tail boundary inside and across a 256-sample slice; k = N) and read back after each; the window of call i is WINDOWS[i + off], so
    the cases of a shape bring every k together with every window.  M = 2501: more pairs than the resident grid, so workgroups claim
    and prefetch further pairs; an odd M: a single last row.  A twin group takes the same calls with TWO_STEP forced."""
    B = muse.binding
    every = _every(M)
    x = _stored(_mixed(M, N, 7 * N + M, every), f32)
    ref = _rows(1, N, N + 5)[0]
    dg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
    db = muse.DeviceBatch(eng, dg, ref)
    tg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
    tb = muse.DeviceBatch(eng, tg, ref)
    cur = x
    Ls = WINDOWS[f32]
    try:
        for i, k in enumerate(_ks(N)):
            L = Ls[(i + off) % len(Ls)]
            assert muse.slide_in_window_plan(N, f32, L, k) == B.MUSE_SLIDE_IN_WINDOW_FUSED
            tails = _mixed(M, k, 31 * N + M + i, every)
            db.slide_score_in_window(tails, L)
            got = db.read_scores()
            assert db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_FUSED, (k, L)
            name = eng.kernel_name(db)
            assert name == "xcorr_fused_n4096_fold<false, %s, %s, %s, true>" % (
                "true" if N < 4096 else "false", "true" if f32 else "false", "true" if L < 2048 else "false"), name
            cur = _slid(cur, _stored(tails, f32))
            got_rows = dg.read(0, M)
            assert _same_bytes(got_rows, cur), (k, L, _diff(got_rows, cur))
            want = _fresh_scores(muse, eng, cur, ref, L, f32)
            assert _same_scores(got, want), (k, L, _where(got, want))
            if M > 1:
                assert np.isnan(want[1][1])                               # the comparison saw NaN scores ...
            assert np.isfinite(want[1][0]) and want[1][0] != 0.0          # ... and real ones
            # a stand-alone pass over the slid rows: the same bits again
            db.score_in_window(L)
            assert _same_scores(db.read_scores(), want), (k, L)
            assert db.last_slide_path() == 0
            # and the two kernels the fused one replaces
            eng.slide_in_window_force(1)
            tb.slide_score_in_window(tails, L)
            eng.slide_in_window_force(0)
            assert tb.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
            assert _same_scores(tb.read_scores(), want), (k, L)
        assert _same_bytes(tg.read(0, M), cur)
        assert dg.slides == len(_ks(N)) == tg.slides and dg.M == M
    finally:
        eng.slide_in_window_force(0)
        for h in (db, tb, dg, tg):
            h.close()


# ------------------------------------------------------------------ 2. the other paths
@pytest.mark.parametrize("N", [4096, 480])
@pytest.mark.parametrize("L", [0, 7, 63])
def test_narrow_float64_windows_are_slide_score_windowed(muse, eng, N, L):
    B = muse.binding
    M = 37
    x, ref = _mixed(M, N, N + L), _rows(1, N, N + 6)[0]
    dg, tg = muse.DeviceGroup.from_rows(eng, x), muse.DeviceGroup.from_rows(eng, x)
    db, tb = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, tg, ref)
    cur = x
    for i, k in enumerate((1, 16, N)):
        tails = _mixed(M, k, 3 * N + L + i)
        db.slide_score_in_window(tails, L)
        tb.slide_score_windowed(tails, L)
        cur = _slid(cur, tails)
        assert db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_MFMA and db.last_in_window_path() == B.MUSE_IN_WINDOW_MFMA
        assert _same_bytes(dg.read(0, M), cur) and _same_bytes(tg.read(0, M), cur)
        assert _same_scores(db.read_scores(), tb.read_scores())
        assert eng.kernel_name(db).startswith("xcorr_window_mfma<")
    for h in (db, tb, dg, tg):
        h.close()


@pytest.mark.parametrize("N,L,f32", [(480, 256, False), (480, 100, False), (480, 256, True), (480, 7, True), (5000, 4096, False)])
def test_two_step_lengths(muse, eng, N, L, f32):
    B = muse.binding
    M = 201
    x, ref = _stored(_mixed(M, N, N + L + 1), f32), _rows(1, N, N + 7)[0]
    dg = muse.DeviceGroup.from_rows(eng, x, f32=f32)
    db = muse.DeviceBatch(eng, dg, ref)
    cur = x
    for i, k in enumerate((1, 16, N // 2, N)):
        assert muse.slide_in_window_plan(N, f32, L, k) == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
        tails = _mixed(M, k, 5 * N + L + i)
        db.slide_score_in_window(tails, L)
        got = db.read_scores()
        assert db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
        cur = _slid(cur, _stored(tails, f32))
        got_rows = dg.read(0, M)
        assert _same_bytes(got_rows, cur), (k, _diff(got_rows, cur))
        want = _fresh_scores(muse, eng, cur, ref, L, f32)
        assert _same_scores(got, want), (k, _where(got, want))
    assert dg.slides == 4
    db.close()
    dg.close()


def test_forced_variant_and_missing_table_take_two_steps(muse, eng):
    """FUSED is the default kernel's build: with the rescaling kernel forced the call still slides and scores, the long way round"""
    B = muse.binding
    N, M, k, L = 3000, 50, 16, 257
    x, ref = _mixed(M, N, 11), _rows(1, N, 12)[0]
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    tails = _mixed(M, k, 13)
    eng.set_kernel(7)
    try:
        db.slide_score_in_window(tails, L)
        got = db.read_scores()
        assert db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_TWO_STEP
        assert _same_bytes(dg.read(0, M), _slid(x, tails))
        fresh = muse.DeviceGroup.from_rows(eng, _slid(x, tails))
        fb = muse.DeviceBatch(eng, fresh, ref)
        fb.score_in_window(L)
        assert _same_scores(got, fb.read_scores())
        fb.close()
        fresh.close()
    finally:
        eng.set_kernel(0)
    db.close()
    dg.close()


# ------------------------------------------------------------------ 3. the Run forms
def _with_matches(x, ref, k):
    """a strong copy of the reference in two rows of three, shifted so that after a slide by k one of the two matches at a lag of at
    most 3 -- a selection with a small MaxLag keeps records, grouped or not (noise alone peaks at any lag)"""
    x = x.copy()
    for i in range(x.shape[0]):
        if i % 3 < 2:
            x[i] += 4.0 * np.roll(ref, (k if i % 3 == 0 else -k) + i % 7 - 3)
    return x


def _same_records(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes() and
            np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes())


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("N,f32,abs_scores", [(4096, False, True), (3000, True, False), (480, False, True)])
def test_slide_run_is_slide_then_run(muse, eng, N, f32, abs_scores, grouped):
    M, G, k = 600, 37, 16
    ref = _rows(1, N, N + 62)[0]
    x = _stored(_with_matches(_mixed(M, N, N + 61), ref, k), f32)
    tails = _mixed(M, k, N + 63)
    gid = (np.arange(M) * 7 % G).astype(np.int32) if grouped else None
    kw = dict(group_id=gid, G=G if grouped else 0, max_lag=15, top_n=10, threshold=0.0, sign_filter=0, abs_scores=abs_scores)
    dg, tg = muse.DeviceGroup.from_rows(eng, x, f32=f32), muse.DeviceGroup.from_rows(eng, x, f32=f32)
    db, tb = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, tg, ref)
    got = db.slide_run(tails, **kw)
    tg.slide(tails)
    want = tb.run(**kw)
    assert len(want[0]) > 0
    assert _same_records(got, want)
    assert _same_bytes(dg.read(0, M), tg.read(0, M)) and _same_bytes(dg.read(0, M), _slid(x, _stored(tails, f32)))
    assert db.last_run_path() == 0 and db.lag_window() == -1 and dg.slides == 1
    for h in (db, tb, dg, tg):
        h.close()


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("N,f32,L", [(4096, False, 257), (4096, False, 15), (2049, True, 7), (480, False, 100)])
def test_slide_run_in_window_is_slide_then_run_in_window(muse, eng, N, f32, L, grouped):
    M, G, k = 600, 37, 3
    ref = _rows(1, N, N + 72)[0]
    x = _stored(_with_matches(_mixed(M, N, N + 71), ref, k), f32)
    tails = _mixed(M, k, N + 73)
    gid = (np.arange(M) * 7 % G).astype(np.int32) if grouped else None
    kw = dict(group_id=gid, G=G if grouped else 0, top_n=10, threshold=0.0, sign_filter=0, abs_scores=True)
    dg, tg = muse.DeviceGroup.from_rows(eng, x, f32=f32), muse.DeviceGroup.from_rows(eng, x, f32=f32)
    db, tb = muse.DeviceBatch(eng, dg, ref), muse.DeviceBatch(eng, tg, ref)
    got = db.slide_run_in_window(tails, L, **kw)
    tg.slide(tails)
    want = tb.run_in_window(L, **kw)
    assert len(want[0]) > 0
    assert _same_records(got, want)
    assert _same_bytes(dg.read(0, M), tg.read(0, M))
    for h in (db, tb, dg, tg):
        h.close()


# ------------------------------------------------------------------ 4. state
def test_refusals_leave_the_rows_and_the_scores(muse, eng):
    B = muse.binding
    lib = B.load()
    N, M, k, L = 3000, 50, 4, 257
    x, ref = _planted(M, N, 71), _rows(1, N, 72)[0]
    dg = muse.DeviceGroup.from_rows(eng, x)
    db = muse.DeviceBatch(eng, dg, ref)
    db.score_in_window(L)
    held = db.read_scores()
    t = np.ascontiguousarray(_rows(M, k, 73))
    tp = B.dptr(t)

    def unchanged():
        return _same_bytes(dg.read(0, M), x) and _same_scores(db.read_scores(), held) and dg.slides == 0

    E, U = B.MUSE_ERR_INVALID, B.MUSE_ERR_UNSUPPORTED
    # the slide's own arguments, the window, the batch's own window
    for args in ((tp, -1, k, L), (tp, N + 1, N + 1, L), (tp, k, k - 1, L), (None, k, k, L), (tp, k, k, -1)):
        assert lib.muse_batch_slide_score_in_window(db._h, *args) == E, args[1:]
        assert unchanged()
    db.set_lag_window(5)
    assert lib.muse_batch_slide_score_in_window(db._h, tp, k, k, L) == E
    assert unchanged() and db.lag_window() == 5
    o_s, o_l, o_v = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int32), np.zeros(4)
    cnt, mean = ctypes.c_int32(0), ctypes.c_double(0)
    outs = (B.i64ptr(o_s), B.i32ptr(o_l), B.dptr(o_v), ctypes.byref(cnt), ctypes.byref(mean))
    assert lib.muse_batch_slide_run(db._h, tp, k, k, None, 0, 15, 4, 0.0, 0, 1, *outs) == E    # (every lag: the own window must be off)
    assert unchanged()
    db.set_lag_window(-1)
    # a refused selection leaves them too
    assert lib.muse_batch_slide_run_in_window(db._h, tp, k, k, None, 0, L, 4, 0.0, 2, 1, *outs) == E and unchanged()
    assert lib.muse_batch_slide_run(db._h, tp, k, k, None, 0, 15, 4, 0.0, 2, 1, *outs) == E and unchanged()
    gid = np.zeros(M, dtype=np.int32)
    assert lib.muse_batch_slide_run(db._h, tp, k, k, B.i32ptr(gid), -1, 15, 4, 0.0, 0, 1, *outs) == E and unchanged()
    # an open staging window
    win = dg.stage(1)
    assert lib.muse_batch_slide_score_in_window(db._h, tp, k, k, L) == E
    win[0, :] = 1.5
    dg.commit(0, 1)
    assert dg.M == M + 1 and _same_bytes(dg.read(0, M), x)
    with pytest.raises(ValueError):
        db.slide_score_in_window(t, L)             # the whole group slides: M + 1 tails, not M
    db.close()
    dg.close()
    # what muse_batch_score_in_window refuses: a wide window at a length without masked kernels, float32 storage there
    for N2, f32, L2 in ((5000, False, 100), (5000, True, 7), (10000, True, 7)):
        x2 = _stored(_rows(9, N2, 75), f32)
        dg2 = muse.DeviceGroup.from_rows(eng, x2, f32=f32)
        db2 = muse.DeviceBatch(eng, dg2, _rows(1, N2, 76)[0])
        t2 = np.ascontiguousarray(_rows(9, k, 77))
        assert lib.muse_batch_slide_score_in_window(db2._h, B.dptr(t2), k, k, L2) == U, (N2, f32, L2)
        assert lib.muse_batch_score_in_window(db2._h, L2) == U
        assert _same_bytes(dg2.read(0, 9), x2) and dg2.slides == 0
        db2.close()
        dg2.close()


def test_k0_scores_without_moving_and_caches_follow(muse, eng):
    N, M, k, L = 4096, 200, 16, 257
    eng.spectrum_cache_limits(min_rows=64)
    try:
        x, ref = _rows(M, N, 91), _rows(1, N, 92)[0]
        dg = muse.DeviceGroup.from_rows(eng, x)
        db = muse.DeviceBatch(eng, dg, ref)
        db.scores()
        db.scores()
        cache = dg.spectrum_cache()
        assert cache[0] > 0                              # a cache really exists
        db.slide_score_in_window(np.zeros((M, 0)), L)    # k = 0: the pass alone
        assert dg.slides == 0 and dg.spectrum_cache() == cache and db.last_slide_path() == 0
        assert _same_bytes(dg.read(0, M), x)
        assert _same_scores(db.read_scores(), _fresh_scores(muse, eng, x, ref, L))
        tails = _rows(M, k, 93)
        db.slide_score_in_window(tails, L)
        assert dg.slides == 1 and dg.spectrum_cache()[0] == 0      # as after muse_group_slide: dropped with the old rows
        want_rows = _slid(x, tails)
        assert _same_scores(db.read_scores(), _fresh_scores(muse, eng, want_rows, ref, L))
        db.slide_score_in_window(_rows(M, k, 94), 2048)            # the fused pass is not counted towards a new cache
        assert dg.spectrum_cache()[0] == 0
        db.close()
        dg.close()
    finally:
        eng.spectrum_cache_limits()


def test_an_empty_group_is_not_an_error(muse, eng):
    dg = muse.DeviceGroup(eng, 4096, 0)
    db = muse.DeviceBatch(eng, dg, _rows(1, 4096, 95)[0])
    db.slide_score_in_window(np.zeros((0, 4)), 257)
    assert dg.slides == 0 and dg.M == 0
    db.close()
    dg.close()


# ------------------------------------------------------------------ 5. against the oracle
def test_fused_scores_match_the_oracle(muse, eng, oracle):
    """1000 x 4096 float64, k = 16: the scores of the fused call within the project's 1e-6 relative (floor 1e-12) of the CPU oracle
    on the rows read back, the lags exact -- no row excused: the oracle flags no tie on these inputs (asserted here and, without a
    GPU, in tests/test_slide_in_window_cpu.py)"""
    B = muse.binding
    M, N = SI.ORACLE_M, SI.ORACLE_N
    ref, rows, tails, want_rows = SI.oracle_case()
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, ref)
    db.slide_score_in_window(tails, N // 2)
    lag, mv = db.read_scores()
    assert db.last_slide_path() == B.MUSE_SLIDE_IN_WINDOW_FUSED
    back = dg.read(0, M)
    assert _same_bytes(back, want_rows)
    olag, omv, gap = oracle.batch_scores(ref, back, nthreads=8)
    assert not np.isnan(omv).any() and not (gap < 1e-12).any()       # no tie row, nothing excused
    assert np.array_equal(lag, olag)
    err = np.abs(mv - omv)
    assert np.all(err <= 1e-6 * np.abs(omv) + 1e-12), float(np.max(err / np.maximum(np.abs(omv), 1e-300)))
    db.close()
    dg.close()
