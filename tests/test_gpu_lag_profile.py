"""GPU tests of the lag profiles (muse_batch_lag_profile / _lag_profile_device, run with -m gpu on an MI355X): the direct product
with the scan replaced by a write-out (xcorr_window_profile_mfma, window_device.h), through the C ABI and its mirrors.

Expected values never come from the code under test.  Every entry of every profile is held to tests/_winsweep.py's long-double table
of the same rows, within that table's derived per-entry rounding bound B -- derived for exactly this product, for any summation order;
nothing is tuned.  The CPU oracle's correlation slice is a second opinion at the project's 1e-6 relative.  Rows: WS.sweep_case(N), one
row per lag in +-63, thirty just outside per side and eight outlier rows -- not a multiple of 16, so the masked tail of the last
workgroup is exercised.

"Same bits as the passes that scan" (test 4) compares with the direct product's scanning passes.  scores_in_lag_band is that pass for
every band but one: at N = 64 the band (-31, 32) is every lag of the length, which the scoring calls hand to the transform kernels
(MUSE_IN_WINDOW_PLAIN).  There the direct product's scan is the batch's own lag window of 32 (muse_batch_set_lag_window), which is
held to byte identity, and scores_in_lag_band to exact lags and the score tolerance."""
import functools
import subprocess

import numpy as np
import pytest

import _lagband as LB
import _winsweep as WS
from _load import pkg

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-6
LENGTHS = (4096, 1433, 480, 64)
BANDS = ((-63, 63), (-7, 7), (0, 15), (1, 16), (1, 17), (-63, -1), (32, 63))
WIDE = ((1433, -100, 100, [(-100, 127), (27, 74)]), (480, -127, 126, [(-127, 127), (0, 127)]))
SENTINEL = -12345.678


def bands_of(N):
    return ((-31, 32),) if N == 64 else BANDS


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


@functools.lru_cache(maxsize=None)
def table(N, lo=None, hi=None):
    """the long-double table of sweep_case(N) over the lags lo .. hi stretched to hold lag 0 (default: the case's own +-Lc, at N = 64
    -31 .. 32); computed once per (N, lags) and never written"""
    case = WS.sweep_case(N)
    if lo is None:
        lo, hi = (-31, 32) if N == 64 else (-WS.LMAX, WS.LMAX)
    lags = np.arange(min(lo, 0), max(hi, 0) + 1)
    t = WS.tables(case.ref, case.rows, case.n, lags=lags)
    t.cc.setflags(write=False)
    t.B.setflags(write=False)
    return t


def columns(t, lo, hi):
    """(cc, B) of the table's columns for the lags lo .. hi"""
    first = int(t.lags[0])
    assert first <= lo and hi <= int(t.lags[-1])
    return t.cc[:, lo - first:hi - first + 1], t.B[:, lo - first:hi - first + 1]


def within_bound(prof, t, lo, hi, tag):
    cc, B = columns(t, lo, hi)
    assert prof.shape == cc.shape, (tag, prof.shape, cc.shape)
    err = np.abs(prof.astype(np.longdouble) - cc).astype(np.float64)
    ratio = err / B
    print("%s: worst err / B %.3f (err %.3e)" % (tag, float(ratio.max()), float(err.max())))
    bad = np.argwhere(~(err <= B))
    assert bad.size == 0, "%s: %d entries outside B, first (row, column) %s" % (tag, len(bad), bad[:5].tolist())


@pytest.fixture(scope="module")
def resident(muse, eng):
    """one resident group and batch per length, shared by the tests"""
    made = {}

    def get(N):
        if N not in made:
            case = WS.sweep_case(N)
            dg = muse.DeviceGroup.from_rows(eng, case.rows)
            made[N] = (case, dg, muse.DeviceBatch(eng, dg, case.ref))
        return made[N]
    yield get
    for _, dg, db in made.values():
        db.close()
        dg.close()


# ------------------------------------------------------------------ 1. element parity
@pytest.mark.parametrize("N", LENGTHS)
def test_every_entry_within_the_derived_bound(muse, resident, oracle, N):
    case, dg, db = resident(N)
    M = case.rows.shape[0]
    assert M % 16 != 0 and db.n == case.n
    t = table(N)
    X, n = oracle.ref_spectrum(case.ref)
    slices = np.array([oracle.xcorr_with_x(X, case.rows[r], n, want_cc=True)[0] for r in range(M)])
    for lo, hi in bands_of(N):
        prof = muse.lag_profile(db, lo, hi)
        assert prof.shape == (M, hi - lo + 1) and prof.dtype == np.float64
        within_bound(prof, t, lo, hi, "N=%d [%d, %d]" % (N, lo, hi))
        want = slices[:, np.arange(lo, hi + 1) % n]
        rel = np.abs(prof - want) / np.abs(want)
        print("N=%d [%d, %d]: worst rel err against the oracle %.3e" % (N, lo, hi, float(rel.max())))
        assert np.all(np.abs(prof - want) <= SCORE_RTOL * np.abs(want)), (N, lo, hi, float(rel.max()))


# ------------------------------------------------------------------ 2. wide bands: more than one launch
@pytest.mark.parametrize("N,lo,hi,plan", WIDE)
def test_wide_bands_take_consecutive_launches(muse, resident, N, lo, hi, plan):
    case, dg, db = resident(N)
    assert muse.lag_profile_plan(N, lo, hi) == plan
    prof = muse.lag_profile(db, lo, hi)
    within_bound(prof, table(N, lo, hi), lo, hi, "wide N=%d [%d, %d]" % (N, lo, hi))


# ------------------------------------------------------------------ 3. the value at a lag does not depend on the band
def test_values_do_not_depend_on_the_band(muse, resident):
    case, dg, db = resident(1433)
    wide = muse.lag_profile(db, -100, 100)
    inner = muse.lag_profile(db, -63, 63)
    assert wide[:, 37:164].tobytes() == inner.tobytes()
    case, dg, db = resident(480)
    a = muse.lag_profile(db, 1, 17)
    b = muse.lag_profile(db, 0, 15)
    assert a[:, 0:15].tobytes() == b[:, 1:16].tobytes()


# ------------------------------------------------------------------ 4. the same bits as the passes that scan
def scan(prof, n, lo, hi):
    """maxAbsIndex over each profile row in the definition's order (tests/_lagband.py: banded -- ascending cc index, strict '>',
    start (0, 0.0)): the row is laid into a slice of length n at its cc indices, which are all that `banded` reads"""
    lag = np.zeros(prof.shape[0], dtype=np.int32)
    mv = np.zeros(prof.shape[0])
    for r in range(prof.shape[0]):
        cc = np.zeros(n)
        cc[np.arange(lo, hi + 1) % n] = prof[r]
        lag[r], mv[r], _ = LB.banded(cc, n, lo, hi, 0)
    return lag, mv


@pytest.mark.parametrize("N", LENGTHS)
def test_same_bits_as_the_scanning_passes(muse, resident, N):
    B = muse.binding
    case, dg, db = resident(N)
    n = case.n
    for lo, hi in bands_of(N):
        slag, smv = db.scores_in_lag_band(lo, hi, 0)
        path = db.last_in_window_path()
        prof = muse.lag_profile(db, lo, hi)
        rlag, rmv = db.read_scores()                                     # the profile call left the score buffers alone
        assert rlag.tobytes() == slag.tobytes() and rmv.tobytes() == smv.tobytes(), (N, lo, hi)
        assert db.last_in_window_path() == path and db.lag_window() == -1
        plag, pmv = scan(prof, n, lo, hi)
        assert np.array_equal(plag, slag), (N, lo, hi, np.nonzero(plag != slag)[0][:8])
        if path == B.MUSE_IN_WINDOW_MFMA:
            assert pmv.tobytes() == smv.tobytes(), (N, lo, hi, np.nonzero(pmv != smv)[0][:8])
            continue
        # every lag of the length: the scoring call took the transform kernels; the direct product's scan is the batch's own window
        assert N == 64 and (lo, hi) == (-31, 32) and path == B.MUSE_IN_WINDOW_PLAIN
        assert np.all(np.abs(pmv - smv) <= SCORE_RTOL * np.abs(smv))
        db.set_lag_window(32)
        try:
            wlag, wmv = db.scores()
        finally:
            db.set_lag_window(-1)
        assert np.array_equal(plag, wlag) and pmv.tobytes() == wmv.tobytes()


# ------------------------------------------------------------------ 5. lists
LIST = [5, 5, 194, 0] + list(range(40, 11, -1))


@pytest.mark.parametrize("K", (1, 16, 17, 33))
def test_listed_rows_are_the_groups_rows(muse, resident, K):
    assert len(LIST) == 33
    case, dg, db = resident(480)
    for lo, hi in ((-7, 7), (1, 17), (-127, 126)):
        whole = muse.lag_profile(db, lo, hi)
        got = muse.lag_profile(db, lo, hi, LIST[:K])
        assert got.shape == (K, hi - lo + 1)
        for k in range(K):
            assert got[k].tobytes() == whole[LIST[k]].tobytes(), (K, k, lo, hi)


def _raw(muse, db, series, K, lo, hi, out, stride):
    B = muse.binding
    idx = None if series is None else np.ascontiguousarray(series, dtype=np.int64)
    return B.load().muse_batch_lag_profile(db._h, None if idx is None else B.i64ptr(idx), K, lo, hi, B.dptr(out), stride)


def test_list_indices_outside_the_group_are_refused(muse, resident):
    B = muse.binding
    case, dg, db = resident(480)
    M = case.rows.shape[0]
    for bad in ([0, -1, 3], [0, 3, M], [M]):
        out = np.full((len(bad), 15), SENTINEL)
        assert _raw(muse, db, bad, len(bad), -7, 7, out, 15) == B.MUSE_ERR_INVALID
        assert np.all(out == SENTINEL)
    out = np.full((M, 15), SENTINEL)
    assert _raw(muse, db, None, M - 1, -7, 7, out, 15) == B.MUSE_ERR_INVALID      # without a list K is 0 or M
    assert _raw(muse, db, None, M, -7, 7, out, 14) == B.MUSE_ERR_INVALID          # out_stride < W
    assert _raw(muse, db, [1, 2], -1, -7, 7, out, 15) == B.MUSE_ERR_INVALID
    assert np.all(out == SENTINEL)
    assert _raw(muse, db, None, M, -7, 7, out, 15) == B.MUSE_OK and not np.any(out == SENTINEL)


# ------------------------------------------------------------------ 6. padding and special rows
def test_padding_and_special_rows(muse, eng):
    B = muse.binding
    N, lo, hi = 480, -7, 11
    W = hi - lo + 1
    case = WS.sweep_case(N)
    rows = case.rows[:21].copy()
    rows[3] = 2.5                                                        # a constant row: sigma == 0
    rows[7, 100] = np.nan
    rows[18, N - 1] = np.inf
    rows[19, 0] = -np.inf
    dg = muse.DeviceGroup.from_rows(eng, rows)
    db = muse.DeviceBatch(eng, dg, case.ref)
    out = np.full((21, W + 3), SENTINEL)
    assert _raw(muse, db, None, 21, lo, hi, out, W + 3) == B.MUSE_OK
    assert np.all(out[:, W:] == SENTINEL)                                # columns W .. out_stride - 1 are never written
    assert np.all(out[3, :W] == 0.0) and not np.signbit(out[3, :W]).any()
    for r in (7, 18, 19):
        assert np.isnan(out[r, :W]).all(), r
    plain = [r for r in range(21) if r not in (3, 7, 18, 19)]
    t = WS.tables(case.ref, rows[plain], case.n, lags=np.arange(lo, hi + 1))
    assert np.all(np.abs(out[plain, :W].astype(np.longdouble) - t.cc).astype(np.float64) <= t.B)
    listed = np.full((3, W + 3), SENTINEL)
    assert _raw(muse, db, [7, 3, 20], 3, lo, hi, listed, W + 3) == B.MUSE_OK
    assert np.isnan(listed[0, :W]).all() and np.all(listed[1, :W] == 0.0) and listed[2, :W].tobytes() == out[20, :W].tobytes()
    assert np.all(listed[:, W:] == SENTINEL)
    # K = 0 with a list, and an empty group: nothing to do, nothing written
    assert muse.lag_profile(db, lo, hi, []).shape == (0, W)
    assert _raw(muse, db, [], 0, lo, hi, listed, W + 3) == B.MUSE_OK and np.all(listed[:, W:] == SENTINEL)
    db.close()
    dg.close()
    dg = muse.DeviceGroup(eng, N, 0)
    db = muse.DeviceBatch(eng, dg, case.ref)
    assert muse.lag_profile(db, lo, hi).shape == (0, W)
    assert _raw(muse, db, None, 0, lo, hi, listed, W) == B.MUSE_OK
    db.close()
    dg.close()


# ------------------------------------------------------------------ 7. the device form
def test_device_form_fills_a_torch_tensor(muse, resident):
    import torch
    case, dg, db = resident(1433)
    M = case.rows.shape[0]
    dev = torch.device("cuda", db.engine.device)
    for lo, hi, series in ((-7, 7, None), (1, 17, None), (-100, 100, None), (-63, 63, LIST), (-100, 100, LIST[:17])):
        K = M if series is None else len(series)
        t = torch.full((K, hi - lo + 1), SENTINEL, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                                         # (torch's fill runs on torch's stream, the profile on the batch's)
        assert muse.lag_profile_into(db, lo, hi, t, series) is t
        torch.cuda.synchronize()
        assert t.cpu().numpy().tobytes() == muse.lag_profile(db, lo, hi, series).tobytes(), (lo, hi, series is None)
    with pytest.raises(muse.MuseError) as e:
        muse.lag_profile_into(db, -7, 7, torch.zeros((M, 14), dtype=torch.float64, device=dev))
    assert e.value.status == muse.binding.MUSE_ERR_INVALID


# ------------------------------------------------------------------ 8. refusals
def _refused(muse, db, fn, status):
    lag, mv = db.read_scores()
    with pytest.raises(muse.MuseError) as e:
        fn()
    assert e.value.status == status and e.value.message, e.value
    lag2, mv2 = db.read_scores()
    assert lag2.tobytes() == lag.tobytes() and mv2.tobytes() == mv.tobytes()


def test_refusals_leave_the_scores(muse, eng, resident):
    B = muse.binding
    case, dg, db = resident(480)
    n = case.n
    db.scores()
    _refused(muse, db, lambda: muse.lag_profile(db, 0, n // 2 + 1), B.MUSE_ERR_INVALID)
    _refused(muse, db, lambda: muse.lag_profile(db, -(n // 2), 0), B.MUSE_ERR_INVALID)
    _refused(muse, db, lambda: muse.lag_profile(db, 3, 2), B.MUSE_ERR_INVALID)
    assert muse.lag_profile(db, -(n // 2 - 1), n // 2, [0]).shape == (1, n)      # the widest: every lag, five launches
    rng = np.random.default_rng(5)
    with np.errstate(over="ignore"):
        rows32 = case.rows[:20].astype(np.float32).astype(np.float64)
    dg32 = muse.DeviceGroup.from_rows(eng, rows32, f32=True)
    db32 = muse.DeviceBatch(eng, dg32, case.ref)
    db32.scores()
    _refused(muse, db32, lambda: muse.lag_profile(db32, -7, 7), B.MUSE_ERR_UNSUPPORTED)
    db32.close()
    dg32.close()
    N = 70000
    long_rows = rng.standard_normal((2, N))
    dgl = muse.DeviceGroup.from_rows(eng, long_rows)
    dbl = muse.DeviceBatch(eng, dgl, rng.standard_normal(N))
    dbl.scores()
    _refused(muse, dbl, lambda: muse.lag_profile(dbl, -7, 7), B.MUSE_ERR_UNSUPPORTED)
    dbl.close()
    dgl.close()


# ------------------------------------------------------------------ 9. the label level
def test_label_level_curves_behind_the_scores(muse, eng):
    N = 480
    rng = np.random.default_rng(480)
    ref = rng.standard_normal(N)
    # series i leads the reference by 2 i + 1 samples (y[t] = ref[t + lead]), so its best match inside 1 .. 15 is positive, at lead
    leads = [1, 3, 5, 7, 9, 11]
    comp = muse.NewGroup("comparison")
    for i, lead in enumerate(leads):
        y = (1.0 + 0.25 * i) * np.roll(ref, -lead) + 0.3 * rng.standard_normal(N)
        comp.Add(muse.NewSeries(y, muse.NewLabels({"graph": "g%d" % i})))
    res = muse.NewResults(15, 6, 0.0, muse.SignFilter_ANY)
    b = muse.NewBatch(muse.NewSeries(ref, muse.NewLabels({"graph": "ref"})), comp, res, 1, engine=eng)
    b.RunInLagBand(["graph"], 1, 15)
    curves = muse.LagProfiles(b, 1, 15)
    assert len(curves) == 6
    seen = 0
    for sc, lags, cc in curves:
        assert np.array_equal(lags, np.arange(1, 16)) and cc.shape == (15,)
        i = int(sc.Labels.labels["graph"][1:])
        assert sc.Lag == leads[i]
        if abs(sc.PercentScore) < 1:
            assert cc[sc.Lag - 1] == sc.PercentScore, (sc, cc)
            seen += 1
    assert seen >= 4
    assert res.Fetch()[0] == []                                           # the default took the Scores as Fetch does
    given = [c[0] for c in curves[:2]]
    again = muse.LagProfiles(b, 1, 15, given)
    assert [a[0] for a in again] == given and all(a[2].tobytes() == c[2].tobytes() for a, c in zip(again, curves))
    with pytest.raises(muse.MuseError):
        muse.LagProfiles(b, 1, 15, [muse.Score(muse.NewLabels({"graph": "nobody"}), 1, 0.5)])
    assert muse.LagProfiles(b, 1, 15, []) == []


# ------------------------------------------------------------------ the C++ mirror
def test_cpp_mirror_lag_profiles(muse):
    """Batch::LagProfile / LagProfiles of the C++ host mirror (host/muse_lag_profile_test.cpp), in a fresh process: every printed entry
    within the long-double table's bound"""
    exe = muse.build.build_lag_profile_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lag-profile ok" in r.stdout, r.stdout + r.stderr
    ref, rows = LB.cpp_case()
    n = WS.LS.fft_len(len(ref))
    t = WS.tables(ref, rows, n, lags=np.arange(-3, 21))
    curves = [l.split() for l in r.stdout.splitlines() if l.startswith("curve ")]
    whole = [l.split() for l in r.stdout.splitlines() if l.startswith("row ")]
    assert len(curves) > 0 and [int(l[1]) for l in whole] == [0, 17, rows.shape[0] - 1]
    for l in curves:
        i, got = int(l[1]), np.array([float(x) for x in l[3:]])
        cc, B = columns(t, 1, 15)
        assert got.shape == (15,) and np.all(np.abs(got.astype(np.longdouble) - cc[i]).astype(np.float64) <= B[i]), l[:3]
    for l in whole:
        i, got = int(l[1]), np.array([float(x) for x in l[2:]])
        assert got.shape == (24,) and np.all(np.abs(got.astype(np.longdouble) - t.cc[i]).astype(np.float64) <= t.B[i]), l[:2]
