"""The planted-lag construction of tests/_rangesweep.py and its expectations, checked on the CPU alone: what
tests/test_gpu_range_sweep.py takes for granted.

  * the gap condition holds for every row, every range and every sign of the direct-product, panel and many-references cases: the
    two largest keys inside the range differ by at least 100 (B_first + B_second).  No row is left out;
  * every non-outlier row planted inside a range wins there under sign 0, and under the sign of its match on `rows` or on `-rows`:
    one row per lag, so every in-range lag is won under sign 0 and under each sign;
  * the kernels' rules restated in Python -- _lagrange.table_argmax, _rowslagrange.panel_merge, _signed.table_argmax and
    _signed.masked_argmax -- give expect()'s (lag, mv) on the long-double tables: the definition's scan order and the kernels' orders
    agree at every planted lag;
  * on the masked cases (a winner at every output index) the oracle flags no tie on any row of the second tier, the planted index
    is the oracle's winner on every row of the first tier, no second-tier row is expected at its planted lag, and the vectorised
    oracle_expect equals _signed.expect;
  * a default-argument call of the helpers of tests/_winsweep.py that gained a parameter returns what it returned before."""
import hashlib

import numpy as np
import pytest

import _lagrange as LR
import _lagsweep as LS
import _rangesweep as RS
import _rowslagrange as RL
import _signed as SG
import _winsweep as WS


def _sha(*arrays):
    m = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        if a.dtype == np.longdouble:       # exactly, as two float64 halves (the storage of a long double has padding bytes)
            hi = a.astype(np.float64)
            m.update(hi.tobytes())
            a = (a - hi.astype(np.longdouble)).astype(np.float64)
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()[:16]


# recorded from the parent commit's tests/_winsweep.py (x86-64, 80-bit long double)
BEFORE = {480: ("29183abe723194e7", "b51c80c4f0a3a5cc", "8e7b2ab5d1f3536e"), 64: ("a61ad4441b1f419b", "05ef148fc702ddeb", "7c0ccacda10c9071")}
BEFORE_MANY = "1ea2d91ff5457ca4"


@pytest.mark.parametrize("N", sorted(BEFORE))
def test_default_arguments_give_the_arrays_of_before(N):
    c = WS.sweep_case(N)
    im = WS.Image(c.ref, c.n)
    t = WS.tables(c.ref, c.rows, c.n)
    assert _sha(c.ref, c.rows, c.lag, c.outlier) == BEFORE[N][0]
    assert _sha(im.E, im.P, im.Pabs) == BEFORE[N][1]
    assert _sha(t.cc, t.B) == BEFORE[N][2]
    # and the explicit statement of the default: the same columns, the same bits
    Lc = min(WS.LMAX, c.n // 2)
    t2 = WS.tables(c.ref, c.rows, c.n, lags=np.arange(-Lc, Lc + 1))
    assert t2.Lc == t.Lc == Lc and np.array_equal(t2.lags, t.lags)
    assert np.array_equal(t2.cc, t.cc) and np.array_equal(t2.B, t.B)
    mid = WS.make_case(N, seed=WS.case_seed(N), p=(N - WS.code_len(N)) // 2)
    assert np.array_equal(mid.rows, c.rows) and np.array_equal(mid.ref, c.ref)
    if N == 480:
        m = WS.many_case(480)
        assert _sha(*m.refs, m.rows, m.lag) == BEFORE_MANY


def test_a_wider_table_holds_the_narrow_one():
    """columns -126 .. 126 restrict to the columns -63 .. 63 bit for bit, and expect() under sign 0 on a symmetric range is
    _winsweep.expect"""
    c = WS.sweep_case(480)
    t = WS.tables(c.ref, c.rows, c.n)
    w = WS.tables(c.ref, c.rows, c.n, lags=np.arange(-RS.RMAX, RS.RMAX + 1))
    cols = np.arange(-WS.LMAX, WS.LMAX + 1) + w.Lc
    assert np.array_equal(w.cc[:, cols], t.cc) and np.array_equal(w.B[:, cols], t.B)
    for L in (0, 1, 7, 63):
        a, b = WS.expect(t, L), RS.expect(w, -L, L, 0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        if L:
            assert np.array_equal(a[3], b[3])


def _signs_of(case, table):
    """the sign of every row's planted match: of cc at the planted lag (0 where the table does not hold it)"""
    pl = WS.planted(case)
    held = (pl >= table.lags[0]) & (pl <= table.lags[-1])
    col = np.where(held, pl + table.Lc, 0)
    return np.where(held, np.sign(table.cc[np.arange(len(pl)), col].astype(np.float64)), 0).astype(np.int64)


def _check_ranges(tag, case, table, ranges, signs=RS.SIGNS):
    """the gap condition for every range, sign and row group; the planted lag wins wherever the range holds it"""
    worst, won = np.inf, 0
    sgn = _signs_of(case, table)
    pl = WS.planted(case)
    for g, tab in ((1, table), (-1, RS.negated(table))):
        for lo, hi in ranges:
            ins = RS.in_range(case, case.n, lo, hi)
            for s in (signs if g > 0 else [s for s in signs if s]):
                lag, mv, B, ratio = RS.expect(tab, lo, hi, s)
                assert float(ratio.min()) >= RS.GAP_FACTOR, (tag, lo, hi, s, g, float(ratio.min()))
                worst = min(worst, float(ratio.min()))
                clo, chi = LR.clip(case.n, lo, hi)
                assert np.all((lag >= clo) & (lag <= chi))
                mine = ins & ((s == 0) | (sgn * g == s))
                assert np.array_equal(lag[mine], pl[mine]), (tag, lo, hi, s, g)
                if mine.any():
                    assert float(np.abs(mv[mine]).min()) > 0.9 and np.all(s * mv[mine] >= 0)
                    won += int(mine.sum())
                if s:
                    assert np.all(s * mv >= 0) and not np.signbit(mv[mv == 0].astype(np.float64)).any()
    # one row per lag: under sign 0, and under each sign on rows or on -rows, every in-range planted lag is won
    assert np.all(sgn[RS.in_range(case, case.n, int(table.lags[0]), int(table.lags[-1]))] != 0)
    return worst, won


@pytest.mark.parametrize("N", RS.DIRECT_LENGTHS)
def test_direct_cases(N):
    case = RS.direct_case(N)
    table = WS.tables(case.ref, case.rows, case.n, lags=RS.direct_table_lags(case.n))
    lags = set(WS.planted(case)[~case.outlier].tolist())
    assert set(RS.direct_table_lags(case.n).tolist()) <= lags              # one row per lag of the widest range
    if N >= 480:
        assert len(case.rows) == 2 * RS.RMAX + 1 + 2 * RS.OUTSIDE + WS.OUTLIERS
    else:
        assert sorted(lags) == list(range(-31, 33))
    ranges = RS.direct_ranges(N)
    have = set(ranges)
    assert all((-k, 0) in have and (0, k) in have for k in range(RS.RMAX + 1)) and all((lo, lo + RS.RMAX) in have for lo in range(-RS.RMAX, 1))
    assert len(ranges) == 3 * RS.RMAX + 2 + RS.RANDOM_RANGES and all(hi - lo <= RS.RMAX and lo <= 0 <= hi for lo, hi in ranges)
    assert {RS.tiles_of(case.n, *r) for r in ranges} == set(range(1, (8 if case.n >= 256 else 4) + 1))
    assert {-LR.clip(case.n, *r)[0] % 16 for r in ranges} == set(range(16))
    worst, won = _check_ranges("direct N=%d" % N, case, table, ranges)
    print("direct N=%d: %d rows, %d ranges, smallest gap / (B1 + B2) %.3g, %d planted wins" % (N, len(case.rows), len(ranges), worst, won))


@pytest.mark.parametrize("N", RS.PANEL_LENGTHS)
def test_panel_cases(N):
    case = RS.panel_case(N)
    table = WS.tables(case.ref, case.rows, case.n, lags=RS.panel_table_lags())
    ranges = RS.panel_ranges()
    assert sorted({hi - lo + 1 for lo, hi in ranges}) == sorted(RS.PANEL_WIDTHS) and len(ranges) == 3 * len(RS.PANEL_WIDTHS)
    subs = sorted({s for r in ranges for s in RS.sub_ranges(*r)})
    assert all(lo <= a <= 0 <= b <= hi and b - a <= RS.RMAX for lo, hi in ranges for a, b in RS.sub_ranges(lo, hi))
    worst, won = _check_ranges("panels N=%d" % N, case, table, ranges + subs, signs=(0,))
    print("panels N=%d: %d rows, smallest gap / (B1 + B2) %.3g, %d planted wins" % (N, len(case.rows), worst, won))
    # the merge rule of the panel kernels and the direct product's scan on the long-double table, a sample of rows
    rows = np.random.default_rng(N).choice(len(case.rows), 24, replace=False)
    for lo, hi in ranges:
        lag, mv, _, _ = RS.expect(table, lo, hi, 0)
        for r in rows:
            cc = RS.full_cc(table, r)
            assert RL.panel_merge(cc, case.n, lo, hi) == (int(lag[r]), float(mv[r])), (N, lo, hi, r)


@pytest.mark.parametrize("which", [c[0] for c in RS.SIXTEEN])
def test_sixteen_panel_cases(which):
    case, (lo, hi) = RS.sixteen_case(which)
    table = WS.tables(case.ref, case.rows, case.n, lags=np.arange(lo, hi + 1))
    v = set((WS.planted(case)[~case.outlier] - lo).tolist())
    assert {128 * z + d for z in range(17) for d in (-2, -1, 0, 1) if 0 <= 128 * z + d < 2048} | {-1, 0, 2047, 2048} == v
    worst, won = _check_ranges("sixteen panels, " + which, case, table, ((lo, hi),) + RS.sub_ranges(lo, hi), signs=(0,))
    assert won >= 66
    lag, mv, _, _ = RS.expect(table, lo, hi, 0)
    for r in range(len(case.rows)):
        assert RL.panel_merge(RS.full_cc(table, r), case.n, lo, hi) == (int(lag[r]), float(mv[r])), (which, r)
    print("sixteen panels, %s: %d rows, smallest gap / (B1 + B2) %.3g" % (which, len(case.rows), worst))


def test_many_direct_case():
    case = WS.many_case(RS.MANY_N)
    for i, ref in enumerate(case.refs):
        table = WS.tables(ref, case.rows, case.n, lags=RS.many_table_lags())
        worst = np.inf
        pl = WS.planted(case, i)
        for lo, hi in RS.MANY_RANGES:
            lag, mv, B, ratio = RS.expect(table, lo, hi, 0)
            assert float(ratio.min()) >= RS.GAP_FACTOR, (i, lo, hi, float(ratio.min()))
            worst = min(worst, float(ratio.min()))
            ins = RS.in_range(case, case.n, lo, hi, i)
            assert ins.sum() >= 50 and np.array_equal(lag[ins], pl[ins])
        print("many direct reference %d: smallest gap / (B1 + B2) %.3g" % (i, worst))


@pytest.mark.parametrize("N", (480, 64))
def test_the_restated_kernel_rules_give_the_expectation(N):
    """_lagrange.table_argmax, _signed.table_argmax and _signed.masked_argmax on the long-double table's rows against expect(), on
    `rows` and `-rows`: ranges from every kind of the list, a sample of rows that holds the outliers"""
    case = RS.direct_case(N)
    table = WS.tables(case.ref, case.rows, case.n, lags=RS.direct_table_lags(case.n))
    rng = np.random.default_rng(N)
    allr = RS.direct_ranges(N)
    ranges = [(0, 0), (-1, 0), (0, 1), (-126, 0), (0, 126), (-63, 63), (-100, 26), (-16, 0)] + [allr[i] for i in rng.choice(len(allr), 8, replace=False)]
    rows = np.concatenate([rng.choice(len(case.rows) - WS.OUTLIERS, 16, replace=False), np.nonzero(case.outlier)[0][:2]])
    for g, tab in ((1, table), (-1, RS.negated(table))):
        for lo, hi in ranges:
            for s in RS.SIGNS:
                lag, mv, _, _ = RS.expect(tab, lo, hi, s)
                for r in rows:
                    cc = RS.full_cc(tab, r)
                    e = (int(lag[r]), float(mv[r]))
                    if s == 0:
                        assert LR.table_argmax(cc, case.n, lo, hi) == e, (N, lo, hi, r)
                    assert SG.table_argmax(cc, case.n, lo, hi, s) == e, (N, lo, hi, s, r)
                    assert SG.masked_argmax(cc, case.n, lo, hi, s) == e, (N, lo, hi, s, r)


# ------------------------------------------------------------------ the masked cases
def _check_masked(tag, m, ranges, signs=RS.SIGNS, groups=(1, -1)):
    t1, t2 = 0, 0
    for lo, hi in ranges:
        for s in signs:
            for g in (groups if s else (1,)):
                tier1, lag, mv, tie = RS.masked_want(m, lo, hi, s, g)
                assert not tie[~tier1].any(), (tag, lo, hi, s, g, np.nonzero(tie & ~tier1)[0][:4])
                assert np.array_equal(lag[tier1], m.pl[tier1]), (tag, lo, hi, s, g)     # the planted index is the range's winner
                assert np.all(np.abs(mv[tier1]) > 0.9) and np.all(np.abs(mv[tier1] - g * m.ld[tier1].astype(np.float64)) <= LS.bound(m.n))
                none = (mv == 0) if s else np.zeros(len(mv), dtype=bool)
                assert not ((lag == m.pl) & ~tier1 & ~none).any(), (tag, lo, hi, s, g)
                assert np.all(np.abs(mv[~tier1]) < 0.9)
                t1, t2 = t1 + int(tier1.sum()), t2 + int((~tier1).sum())
    return t1, t2


@pytest.mark.parametrize("N,f32", [(N, False) for N in RS.MASKED_LENGTHS] + [(N, True) for N in RS.MASKED_F32])
def test_masked_cases(oracle, N, f32):
    cases = RS.masked_cases(oracle, N, f32)
    n = LS.fft_len(N)
    assert len(cases) == (1 if N == n else 2)
    seen = set()
    for ci, m in enumerate(cases):
        assert np.all(m.sgn != 0) and (m.sgn > 0).sum() > len(m.sgn) // 4 and (m.sgn < 0).sum() > len(m.sgn) // 4
        seen |= set(m.k.tolist())
        t1, t2 = _check_masked("N=%d f32=%d ref %d" % (N, f32, ci), m, RS.masked_ranges(n) + list(RS.FORCED_RANGES))
        print("masked N=%d f32=%d reference %d: %d rows, %d first-tier and %d second-tier expectations, no tie" % (N, f32, ci, len(m.rows), t1, t2))
        # the vectorised expectation against _signed.expect's, and the definition is odd in the rows: a sample
        pick = np.random.default_rng(N).choice(len(m.rows), 6, replace=False)
        keys = [(lo, hi) for lo, hi in RS.masked_ranges(n)[:4] + list(RS.FORCED_RANGES[:2])]
        for g in (1, -1):
            exp, n2 = SG.expect(oracle, m.ref, g * m.rows[pick], keys)
            assert n2 == n
            for lo, hi in keys:
                for s in RS.SIGNS:
                    _, lag, mv, tie = RS.masked_want(m, lo, hi, s, g)
                    e = exp[(lo, hi, s)]
                    assert np.array_equal(lag[pick], e[0]) and np.array_equal(mv[pick], e[1]) and np.array_equal(tie[pick], e[2]), (N, lo, hi, s, g)
    assert seen == set(range(n))                                          # every output index is planted


@pytest.mark.parametrize("N", RS.MANY_MASKED_LENGTHS)
def test_many_masked_cases(oracle, N):
    for i, m in enumerate(RS.many_masked_cases(oracle, N)):
        t1, t2 = _check_masked("many N=%d ref %d" % (N, i), m, RS.MANY_MASKED_RANGES, signs=(0,))
        assert t1 > 0 and t2 > 0


def test_tie_case():
    """every row of the tie case holds its largest |cc| at two lags or more of every range, exactly equal in the long-double table,
    at least 100 x 2 B above every other value; the definition's winner is the first of them in scan order, which is NOT the first in
    table order wherever the range has negative lags -- and the panels' merge rule restated gives it"""
    ref, rows = RS.tie_case()
    n = LS.fft_len(RS.TIE_N)
    t = WS.tables(ref, rows, n, lags=RS.tie_table_lags())
    for lo, hi in RS.TIE_RANGES:
        lag, mv, B, ratio, ties = RS.expect_tied(t, lo, hi)
        assert ties.min() >= 2 and float(ratio.min()) >= RS.GAP_FACTOR, (lo, hi, int(ties.min()), float(ratio.min()))
        assert np.all((lag >= 0) & (lag < RS.TIE_PERIOD)) or hi < RS.TIE_PERIOD - 1
        first_in_table = np.array([int(np.argmax(np.abs(t.cc[r, lo + t.Lc:hi + t.Lc + 1]))) + lo for r in range(len(rows))])
        if lo < -RS.TIE_PERIOD and hi >= RS.TIE_PERIOD:
            assert np.all(first_in_table != lag)
        for r in range(len(rows)):
            assert RL.panel_merge(RS.full_cc(t, r), n, lo, hi) == (int(lag[r]), float(mv[r])), (lo, hi, r)
        print("ties [%d, %d]: %d .. %d tied lags per row, gap to the rest / 2 B %.3g" % (lo, hi, ties.min(), ties.max(), ratio.min()))
