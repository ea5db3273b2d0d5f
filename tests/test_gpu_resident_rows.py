"""GPU tests of rows that are already resident (row_gather.hip; muse_group_append_from, muse_batch_run_group_rows; the host
mirrors' reuse of a Series' home).  Run with -m gpu on an MI355X.

A gathered group must hold exactly the bytes of the source rows it names; every Run over it, and Muse.Run over rows named in a
resident group, must give bit for bit what the same rows uploaded from the host give."""
import ctypes
import threading

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
    x = rng.standard_normal((M, N)) * rng.uniform(0.5, 3.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))
    return x


def _lists(M, seed):
    rng = np.random.default_rng(seed)
    return {
        "random_dups": rng.integers(0, M, size=2 * M + 3),
        "reversed": np.arange(M)[::-1].copy(),
        "contiguous": np.arange(M // 3, M),
        "single": np.array([M // 2]),
    }


# ------------------------------------------------------------------ 1. append_from
@pytest.mark.parametrize("N", [8, 480, 4095, 4096, 5000, 100000])
def test_append_from_is_byte_exact(muse, eng, N):
    M = 24 if N >= 100000 else 96
    src = muse.DeviceGroup.from_rows(eng, _rows(M, N, N))
    want = src.read(0, M)
    for name, idx in _lists(M, N + 1).items():
        for d0 in (0, 1):                                     # both parities of the first destination row
            dst = muse.DeviceGroup(eng, N, capacity=1)        # (a list longer than one row grows the group)
            pre = _rows(d0, N, 99) if d0 else np.zeros((0, N))
            if d0:
                dst.append(pre)
            dst.append_from(src, idx)
            assert dst.M == d0 + len(idx)
            got = dst.read(0, dst.M)
            assert np.array_equal(got[:d0], pre), (name, d0)
            assert np.array_equal(got[d0:], want[idx]), (name, d0)
            dst.close()
    src.close()


@pytest.mark.parametrize("N", [480, 4095])
def test_append_from_f32(muse, eng, N):
    M = 64
    src = muse.DeviceGroup.from_rows(eng, _rows(M, N, 5), f32=True)
    want = src.read(0, M)
    for name, idx in _lists(M, 6).items():
        for d0 in (0, 1, 3):
            dst = muse.DeviceGroup(eng, N, capacity=2, f32=True)
            if d0:
                dst.append(_rows(d0, N, 7))
            head = dst.read(0, d0) if d0 else None
            dst.append_from(src, idx)
            got = dst.read(0, dst.M)
            if d0:
                assert np.array_equal(got[:d0], head)
            assert np.array_equal(got[d0:], want[idx]), (name, d0)
            dst.close()
    src.close()


def test_append_from_orders_with_packed_host_rows_and_survives_src_free(muse, eng):
    N, M = 480, 40
    src = muse.DeviceGroup.from_rows(eng, _rows(M, N, 11))
    want = src.read(0, M)
    a, b, c, d = (_rows(1, N, 20 + k) for k in range(4))
    dst = muse.DeviceGroup(eng, N, capacity=0)
    dst.append(a)                     # the first small append goes straight up
    dst.append(b)                     # later ones are packed into the staging buffer and not sent yet
    idx = np.array([39, 0, 7, 7, 12])
    dst.append_from(src, idx)
    src.close()                       # freed right behind the call
    dst.append(c)
    dst.append(d)
    got = dst.read(0, dst.M)
    assert np.array_equal(got, np.vstack([a, b, want[idx], c, d]))
    dst.close()


# --------------------------------------------------------- 2. Runs over a gathered group
@pytest.mark.parametrize("N", [480, 4096])
def test_batch_over_gathered_group(muse, eng, oracle, N):
    M = 300
    src = muse.DeviceGroup.from_rows(eng, _rows(M, N, 31))
    ref = _rows(1, N, 32)[0]
    idx = np.random.default_rng(33).permutation(M)[:200]
    gath = muse.DeviceGroup(eng, N)
    gath.append_from(src, idx)
    rows = gath.read(0, gath.M)
    host = muse.DeviceGroup.from_rows(eng, rows)
    db_g, db_h = muse.DeviceBatch(eng, gath, ref), muse.DeviceBatch(eng, host, ref)
    lag_g, mv_g = db_g.scores()
    lag_h, mv_h = db_h.scores()
    assert np.array_equal(lag_g, lag_h) and np.array_equal(mv_g.view(np.uint64), mv_h.view(np.uint64))
    gid = (np.arange(len(idx)) % 17).astype(np.int32)
    for group_id, G in ((None, 0), (gid, 17)):
        rg = db_g.run(group_id, G, max_lag=N, top_n=10, threshold=0.0, sign_filter=0)
        rh = db_h.run(group_id, G, max_lag=N, top_n=10, threshold=0.0, sign_filter=0)
        for x, y in zip(rg[:3], rh[:3]):
            assert np.array_equal(x, y)
        assert rg[3] == rh[3] or (np.isnan(rg[3]) and np.isnan(rh[3]))
        olag, omv, _ = oracle.batch_scores(ref, rows, nthreads=4)
        oi, ol, osc, omean = oracle.results(olag, omv, group_id, G, True, N, 10, 0.0, 0)
        assert np.allclose(rg[2], osc, rtol=1e-6, atol=1e-12)
    for g in (db_g, db_h, gath, host, src):
        g.close()


# ------------------------------------------------------ 3. run_group_rows == run_rows
def _same(a, b):
    (ra, sa), (rb, sb) = a, b
    return sa == sb and int(ra["series"]) == int(rb["series"]) and int(ra["lag"]) == int(rb["lag"]) and \
        np.float64(ra["score"]).view(np.uint64) == np.float64(rb["score"]).view(np.uint64)


@pytest.mark.parametrize("N", [480, 4096, 100000])
def test_run_group_rows_equals_run_rows(muse, eng, N):
    M = 12 if N == 100000 else 400
    x = _rows(M, N, 41)
    x[3] = 2.5                         # a constant row (sigma == 0)
    x[5, 7] = np.nan                   # a NaN row
    src = muse.DeviceGroup.from_rows(eng, x)
    rows = src.read(0, M)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), _rows(1, N, 42)[0])
    rng = np.random.default_rng(43)
    lists = [np.array([0]), np.array([5]), np.array([5, 0, 1]), np.array([3, 1]), np.arange(2, min(M, 9)),
             rng.integers(0, M, size=min(M, 50)), np.arange(M)]
    for idx in lists:
        for abs_scores in (0, 1):
            want = tmpl.run_rows(rows[idx], abs_scores=abs_scores)
            got = tmpl.run_group_rows(src, idx, abs_scores=abs_scores)
            assert _same(got, want), (idx[:5], abs_scores, got, want)
    st = tmpl.run_group_rows(src, np.array([5, 0]))[1]
    assert st == 2                     # the first member scores NaN
    src.close()
    tmpl.close()


def test_run_group_rows_beyond_the_slot_cap(muse, eng):
    N, M = 4096, 4200                  # 4200 x 4096 samples > the 2^24-sample slot: the general path
    src, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=51)
    rows = src.read(0, M)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), ref)
    for idx in (np.arange(M), np.random.default_rng(52).permutation(M)):
        for abs_scores in (0, 1):
            assert _same(tmpl.run_group_rows(src, idx, abs_scores), tmpl.run_rows(rows[idx], abs_scores))
    src.close()
    tmpl.close()


@pytest.mark.parametrize("N", [480, 4095])
def test_run_group_rows_f32_source(muse, eng, N):
    M = 80
    src = muse.DeviceGroup.from_rows(eng, _rows(M, N, 61), f32=True)
    wide = src.read(0, M)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), _rows(1, N, 62)[0])
    for idx in (np.arange(M), np.arange(10, 20), np.random.default_rng(63).integers(0, M, 33)):
        for abs_scores in (0, 1):
            assert _same(tmpl.run_group_rows(src, idx, abs_scores), tmpl.run_rows(wide[idx], abs_scores))
    src.close()
    tmpl.close()


# ------------------------------------------------------------------ 4. errors
def test_errors_leave_dst_unchanged(muse, eng):
    B = muse.binding
    N = 480
    src = muse.DeviceGroup.from_rows(eng, _rows(10, N, 71))
    dst = muse.DeviceGroup.from_rows(eng, _rows(3, N, 72))
    other_len = muse.DeviceGroup.from_rows(eng, _rows(3, N + 1, 73))
    f32 = muse.DeviceGroup.from_rows(eng, _rows(3, N, 74), f32=True)
    eng2 = muse.Engine(0)
    far = muse.DeviceGroup.from_rows(eng2, _rows(3, N, 75))
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), _rows(1, N, 76)[0])
    L = B.load()
    idx = np.array([0, 1], dtype=np.int64)
    rec = np.zeros(1, dtype=B.RECORD_DTYPE)
    state = ctypes.c_uint8(0)

    def app(d, s, i, count=None):
        i = np.ascontiguousarray(i, dtype=np.int64)
        return L.muse_group_append_from(d, s, B.i64ptr(i), len(i) if count is None else count)

    def run(t, s, i, count=None):
        i = np.ascontiguousarray(i, dtype=np.int64)
        return L.muse_batch_run_group_rows(t, s, B.i64ptr(i), len(i) if count is None else count, 0, B.recptr(rec),
                                           ctypes.byref(state))

    cases = [
        (app(None, src._h, idx), B.MUSE_ERR_INVALID),
        (app(dst._h, None, idx), B.MUSE_ERR_INVALID),
        (app(dst._h, src._h, idx, -1), B.MUSE_ERR_INVALID),
        (app(dst._h, src._h, [0, 10]), B.MUSE_ERR_INVALID),
        (app(dst._h, src._h, [-1]), B.MUSE_ERR_INVALID),
        (app(dst._h, far._h, [0]), B.MUSE_ERR_INVALID),
        (app(dst._h, dst._h, [0]), B.MUSE_ERR_INVALID),
        (app(dst._h, f32._h, [0]), B.MUSE_ERR_INVALID),
        (app(dst._h, other_len._h, [0]), B.MUSE_ERR_LENGTH),
        (app(dst._h, src._h, []), B.MUSE_OK),
        (run(None, src._h, idx), B.MUSE_ERR_INVALID),
        (run(tmpl._h, None, idx), B.MUSE_ERR_INVALID),
        (run(tmpl._h, src._h, idx, -1), B.MUSE_ERR_INVALID),
        (run(tmpl._h, src._h, [10]), B.MUSE_ERR_INVALID),
        (run(tmpl._h, far._h, [0]), B.MUSE_ERR_INVALID),
        (run(tmpl._h, other_len._h, [0]), B.MUSE_ERR_LENGTH),
        (run(tmpl._h, src._h, []), B.MUSE_OK),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, (k, got, want)
    assert state.value == 0 and int(rec[0]["series"]) == -1
    # an open staging window on either group
    win = src.stage(1)
    assert win.shape[0] == 1
    assert app(dst._h, src._h, [0]) == B.MUSE_ERR_INVALID
    assert run(tmpl._h, src._h, [0]) == B.MUSE_ERR_INVALID
    win[0, :] = 1.0
    src.commit(0, 1)
    win = dst.stage(1)
    assert app(dst._h, src._h, [0]) == B.MUSE_ERR_INVALID
    win[0, :] = 2.0
    dst.commit(0, 1)
    assert dst.M == 4 and src.M == 11
    for h in (src, dst, other_len, f32, far, tmpl):
        h.close()
    eng2.close()


# -------------------------------------------------------------- 5. many callers
def test_sixteen_threads_one_template_one_src(muse, eng):
    N, M = 480, 5000
    src, ref = muse.DeviceGroup.synthetic(eng, M, N, seed=81)
    tmpl = muse.DeviceBatch(eng, muse.DeviceGroup(eng, N, 0), ref)
    rng = np.random.default_rng(82)
    lists = [rng.integers(0, M, 50) if k % 3 else np.arange(50 * k, 50 * k + 50) for k in range(64)]
    serial = [tmpl.run_group_rows(src, l) for l in lists]
    out = [None] * (16 * len(lists))
    errs = []

    def work(t):
        try:
            for r in range(3):
                for k, l in enumerate(lists):
                    if (k + t) % 16 == 0 or r == 0:
                        out[t * len(lists) + k] = tmpl.run_group_rows(src, l)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(16)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for t in range(16):
        for k in range(len(lists)):
            assert _same(out[t * len(lists) + k], serial[k]), (t, k)
    src.close()
    tmpl.close()


# ---------------------------------------------------------------- 6. mirrors
def _labelled_group(muse, M, N, seed):
    x = _rows(M, N, seed)
    g = muse.NewGroup("all")
    for i in range(M):
        g.Add(muse.NewSeries(x[i], muse.NewLabels({"id": str(i), "graph": "g%d" % (i % 7), "host": "h%d" % (i % 3)})))
    return g, x


@pytest.mark.parametrize("N", [480, 4096])
def test_python_sub_group_reuse_on_and_off(muse, eng, N):
    big, x = _labelled_group(muse, 210, N, 91)
    ref = muse.NewSeries(_rows(1, N, 92)[0])
    r0 = muse.NewResults(N, 20, 0.0, 0)
    muse.NewBatch(ref, big, r0, 4, engine=eng).Run(["graph"])   # the big group becomes resident: the series' home
    big.indexLabelValues(["host"])
    members = big.FilterByLabelValues(muse.NewLabels({"host": "h1"}))
    assert len(members) == 70
    outs = []
    for on in (True, False):
        eng.reuse_resident_rows(on)
        try:
            sub = muse.NewGroup("h1")
            sub.Add(*members)
            extra = muse.NewSeries(_rows(1, N, 93)[0], muse.NewLabels({"id": "x", "graph": "g1", "host": "h1"}))
            sub.Add(extra)                                            # one series without a home: the host path in between
            res = muse.NewResults(N, 10, 0.0, 0)
            muse.NewBatch(ref, sub, res, 4, engine=eng).Run(["graph"])
            dg = sub._dev[1]
            outs.append((res.Fetch(), dg.read(0, dg.M)))
        finally:
            eng.reuse_resident_rows(True)
    assert eng.reuse_resident_rows() is True
    (f_on, rows_on), (f_off, rows_off) = outs
    assert np.array_equal(rows_on, rows_off)
    assert len(f_on[0]) == len(f_off[0])
    for a, b in zip(f_on[0], f_off[0]):
        assert a.Labels == b.Labels and a.Lag == b.Lag and a.PercentScore == b.PercentScore
    assert f_on[1] == f_off[1] or (np.isnan(f_on[1]) and np.isnan(f_off[1]))


def test_python_muse_run_resident(muse, eng):
    N = 480
    big, x = _labelled_group(muse, 140, N, 95)
    ref = muse.NewSeries(_rows(1, N, 96)[0])
    muse.NewBatch(ref, big, muse.NewResults(N, 5, 0.0, 0), 4, engine=eng).Run(None)
    big.indexLabelValues(["graph"])
    outs = []
    for on in (True, False):
        eng.reuse_resident_rows(on)
        try:
            res = muse.NewResults(N, 7, 0.0, 0)
            m = muse.New(ref, res, engine=eng)
            for g in range(7):
                m.Run(big.FilterByLabelValues(muse.NewLabels({"graph": "g%d" % g})))
            outs.append(res.Fetch())
        finally:
            eng.reuse_resident_rows(True)
    a, b = outs
    assert [(s.Labels, s.Lag, s.PercentScore) for s in a[0]] == [(s.Labels, s.Lag, s.PercentScore) for s in b[0]]
    assert a[1] == b[1]


def test_cpp_mirror_reuse(muse):
    import subprocess
    exe = muse.build.build_resident_test()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "resident ok" in out.stdout
