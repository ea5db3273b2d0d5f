"""The planted-lag construction of tests/_winsweep.py and its long-double expectation, checked on the CPU alone: what
tests/test_gpu_window_sweep.py takes for granted.  At every length (and for every reference and every slid state) the GPU file uses:

  * the gap condition holds for every row and every window L = 0 .. 63: the two largest |cc| inside the window differ by at
    least 100 (B_first + B_second).  No row is left out;
  * every non-outlier row whose planted lag lies inside the window wins there, with |mv| > 0.9 (before any slide);
  * the long-double table agrees with _lagsweep.ld_score_at entry by entry (a sample), and _window.expect -- the FFT oracle with
    the window definition applied, the expectation of every other windowed test -- agrees with its (lag, mv) at every L within
    _lagsweep.bound(n);
  * a plain float64 numpy restatement of the kernels' arithmetic (first-sample shift, one-pass variance, (S - mean P) / sigma)
    stays inside B on every entry of the table; the worst err / B is printed.

Measured with these seeds (x86-64, 80-bit long double): smallest gap / (B_first + B_second) 7.9e4 (the 25 rows of N = 35841;
2.6e5 ... 1.2e9 elsewhere), restatement err / B between 0.0003 (N = 35841) and 0.08 (N = 64)."""
import numpy as np
import pytest

import _lagsweep as LS
import _window as W
import _winsweep as WS

ALL_LS = tuple(range(WS.LMAX + 1))


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the table needs an extended long double to referee float64 kernels"


def _inside(case, L, i=0):
    """non-outlier rows whose planted lag (against reference i) the window L scans"""
    order = WS.scan_order(case.n, L)
    return ~case.outlier & np.isin(WS.planted(case, i), order)


def _check_construction(tag, case, oracle, refs=None):
    worst_ratio, worst_restated = np.inf, 0.0
    for i in (range(len(case.refs)) if refs is None else refs):
        ref = case.refs[i]
        t = WS.tables(ref, case.rows, case.n)
        ratio = WS.gap_ratio(t)
        assert ratio >= WS.GAP_FACTOR, (tag, i, ratio)
        worst_ratio = min(worst_ratio, ratio)
        # the planted lag wins wherever the window holds it
        pl = WS.planted(case, i)
        for L in ALL_LS:
            lag, mv, B, _ = WS.expect(t, L)
            ins = _inside(case, L, i)
            assert np.array_equal(lag[ins], pl[ins]), (tag, i, L)
            assert np.all(np.abs(lag) <= min(L, case.n // 2))
            if ins.any():
                assert float(np.abs(mv[ins]).min()) > 0.9, (tag, i, L, float(np.abs(mv[ins]).min()))
        # a sample of entries against _lagsweep's single-index statement of the definition
        xs_pad = LS.ld_ref(ref, case.n)
        rng = np.random.default_rng(case.N)
        for r in rng.choice(len(case.rows), min(6, len(case.rows)), replace=False):
            for lag in (-t.Lc if 2 * t.Lc != case.n else -t.Lc + 1, -1, 0, 1, t.Lc):
                want = LS.ld_score_at(ref, case.rows[r], case.n, lag % case.n, xs_pad)
                # (two long-double sums in different orders: each within N 2^-64 of the magnitudes B is built from, 2^-11 of B)
                assert abs(float(t.cc[r, lag + t.Lc] - want)) <= t.B[r, lag + t.Lc] * 2.0 ** -10, (tag, r, lag)
        # the oracle-derived expectation of the existing windowed tests
        exp, _, _, n = W.expect(oracle, ref, case.rows, ALL_LS)
        assert n == case.n
        for L in ALL_LS:
            lag, mv, _, _ = WS.expect(t, L)
            assert np.array_equal(exp[L][0], lag), (tag, i, L)
            assert not exp[L][2].any()
            assert float(np.max(np.abs(exp[L][1] - mv.astype(np.float64)))) <= LS.bound(case.n), (tag, i, L)
        # the kernels' arithmetic in float64
        err = np.abs(WS.kernel_restatement(ref, case.rows, case.n).astype(np.longdouble) - t.cc).astype(np.float64)
        assert np.all(err <= t.B), (tag, i, float((err / t.B).max()))
        worst_restated = max(worst_restated, float((err / t.B).max()))
    print("%s: %d rows, smallest gap / (B1 + B2) %.3g, float64 restatement worst err / B %.4f"
          % (tag, len(case.rows), worst_ratio, worst_restated))


@pytest.mark.parametrize("N", WS.LENGTHS + WS.SPLIT_LENGTHS)
def test_sweep_case(oracle, N):
    case = WS.sweep_case(N)
    _check_construction("N=%d" % N, case, oracle)
    lags = set(WS.planted(case)[~case.outlier].tolist())
    Lc = min(WS.LMAX, case.n // 2)
    assert set(WS.scan_order(case.n, WS.LMAX).tolist()) <= lags          # one row per lag of the widest window
    assert int(case.outlier.sum()) == WS.OUTLIERS
    if N >= 480:
        assert len(case.rows) == 2 * WS.LMAX + 1 + 2 * WS.OUTSIDE + WS.OUTLIERS == 195
        assert int((np.abs(case.lag) > WS.LMAX).sum()) >= 2 * WS.OUTSIDE
    if N == 64:
        assert Lc == 32 and sorted(lags) == list(range(-31, 33))
    lam = LS.first_sample_level(case.rows)
    # far-outlier first samples (lambda is taken against the row's own sigma, which the outlier inflates: 50 sigma of the source row
    # is 7.9 at N = 64 and 39 at N = 4096), and no other row starts on one
    assert np.all(lam[case.outlier] > LS.LEVEL_MAX) and np.all(lam[~case.outlier] < lam[case.outlier].min())


def test_long_case(oracle):
    case = WS.long_case()
    assert case.rows.shape == (17 + WS.OUTLIERS, WS.SPLIT_LONG)
    _check_construction("N=%d" % WS.SPLIT_LONG, case, oracle)


@pytest.mark.parametrize("N", WS.MANY_LENGTHS)
def test_many_case(oracle, N):
    case = WS.many_case(N)
    assert len(case.refs) == 8 and case.offsets[:3] == (0, 5, -11) and max(abs(o) for o in case.offsets) <= 20
    for i in range(8):                                                  # every reference sees every lag of the widest window
        assert set(range(-WS.LMAX, WS.LMAX + 1)) <= set(WS.planted(case, i)[~case.outlier].tolist())
    _check_construction("many N=%d" % N, case, oracle)


@pytest.mark.parametrize("N", WS.SLIDE_LENGTHS)
@pytest.mark.parametrize("k", WS.SLIDE_KS)
def test_slid_states_keep_the_gap(N, k):
    """after each of the four slides by k: the gap condition on the host-rolled rows at the windows the GPU file scores, and the
    rows whose walked lag (planted + calls * k) is still inside the window win there"""
    case = WS.sweep_case(N)
    image = WS.Image(case.ref, case.n)
    worst = np.inf
    for call, (tails, rows) in enumerate(WS.slide_states(case, k), 1):
        assert tails.shape == (len(case.rows), k) and rows.shape == case.rows.shape
        t = WS.tables(case.ref, rows, case.n, image)
        ratio = WS.gap_ratio(t, WS.SLIDE_LS)
        assert ratio >= WS.GAP_FACTOR, (N, k, call, ratio)
        worst = min(worst, ratio)
        walked = case.lag + call * k
        for L in WS.SLIDE_LS:
            lag = WS.expect(t, L)[0]
            ins = np.abs(walked) <= L      # (the outlier copies too: their first sample has slid out)
            assert np.array_equal(lag[ins], walked[ins]), (N, k, call, L)
    print("slide N=%d k=%d: smallest gap / (B1 + B2) over %d calls %.3g" % (N, k, WS.SLIDE_CALLS, worst))


@pytest.mark.parametrize("N", [4096, 1433, 480, 64])
def test_the_check_sees_a_dropped_sample_and_a_lag_off_by_one(N):
    """the sensitivity of the GPU file's three assertions, on the float64 restatement: (a) a kernel that takes the last sample
    of a row for nothing (the masked last piece cut one sample short) leaves B on more than 99 of 100 rows at the winning entry
    of L = 63; (b) a reference image read
    one lag off moves the lag of every row whose planted lag and its neighbour lie inside the window"""
    case = WS.sweep_case(N)
    t = WS.tables(case.ref, case.rows, case.n)
    Lc = t.Lc
    short = np.array(case.rows)
    short[:, -1] = short[:, 0]                                            # d[N - 1] = 0 in the sums and in the product
    cc_short = WS.kernel_restatement(case.ref, short, case.n)
    lag, mv, B, _ = WS.expect(t, WS.LMAX)
    r = np.arange(len(lag))
    err = np.abs(cc_short[r, lag + Lc].astype(np.longdouble) - mv).astype(np.float64)
    seen = err > B
    print("N=%d: a dropped last sample moves the winning score by %.1e ... %.1e (B there %.1e ... %.1e): outside B on %d of %d rows"
          % (N, err.min(), err.max(), B.min(), B.max(), int(seen.sum()), len(seen)))
    assert int(seen.sum()) * 100 > 99 * len(seen)
    loose = err <= 1e-6 * np.abs(mv.astype(np.float64)) + 1e-12
    print("      (1e-6 relative + 1e-12, the other windowed tests' tolerance, passes %d of those rows)" % int(loose.sum()))
    # (b) column c of the shifted table holds lag c - Lc - 1: the scan of window L = 7 over it
    cc = WS.kernel_restatement(case.ref, case.rows, case.n)
    order = WS.scan_order(case.n, 7)
    sub = np.abs(cc[:, order + Lc - 1])
    got = order[np.argmax(sub, axis=1)]
    elag = WS.expect(t, 7)[0]
    pl = WS.planted(case)
    ins = np.isin(pl, order) & np.isin(pl + 1, order) & ~case.outlier        # (the shifted peak is still inside the window)
    assert ins.sum() == 14 and np.array_equal(got[ins], elag[ins] + 1)
