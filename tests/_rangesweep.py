"""Planted-lag construction and long-double expectation for the lag-RANGE kernels, shared by tests/test_range_sweep_cpu.py and
tests/test_gpu_range_sweep.py: tests/_winsweep.py's table and bound carried from "window L" to "range [lo, hi], sign s".  It touches
nothing under test.

TABLE.  _winsweep.tables(..., lags=arange(a, b + 1)): cc[r, lag] and the derived bound B[r, lag] for every lag of a contiguous list,
the same long-double sums and the same B (Higham's gamma_k on the kernel's own quantities; it holds for any summation order, so it
covers split-K and the panels unchanged).  Negating the rows negates cc exactly and leaves B as it is (every term of B is a magnitude):
negated(t) is the table of -rows.

EXPECTATION.  expect(t, lo, hi, sign) -> (lag, mv, B, ratio): the range clipped as the definition clips it (_lagrange.clip), scanned
0 .. hi, then lo .. -1; the key of an entry is |cc| (sign 0) or sign * cc; only keys > 0 can win, the first maximum wins.  Nothing of
the sign: (0, +0.0); sign 0 and nothing above zero: (0, cc[0]).

GAP CONDITION.  A condition of the inputs, not a tolerance: ratio = (key_first - max(key_second, 0)) / (B_first + B_second) >=
_winsweep.GAP_FACTOR for every row, every tested range and every sign (B_second = 0 where the range holds one lag).  Where no key is
above zero the largest key must lie as far BELOW zero: ratio = -key_first / B_first, so a kernel inside B cannot find a value of the
sign either.  No row is excused.

CASES.  _winsweep.make_case(N, seed, lags=...): one row per planted lag, shuffled, plus the 8 copies whose first sample lies 50 sigma
off.  The amplitudes carry random signs, so scoring `rows` and `-rows` makes every planted lag the winner under both signs."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _lagrange as LR
import _lagsweep as LS
import _winsweep as WS

GAP_FACTOR = WS.GAP_FACTOR
SIGNS = (0, 1, -1)
RMAX = 126                 # the widest direct-product range has 127 lags
OUTSIDE = WS.OUTSIDE


def negated(t):
    """the table of -rows: cc negated (exact), B shared"""
    m = WS.Table()
    m.n, m.N, m.Lc, m.lags, m.cc, m.B = t.n, t.N, t.Lc, t.lags, -t.cc, t.B
    return m


def scan_order(n, lo, hi):
    """the lags the definition scans, in order: 0 .. hi, then lo .. -1 (clipped)"""
    lo, hi = LR.clip(n, lo, hi)
    assert lo <= 0 <= hi
    return np.concatenate([np.arange(0, hi + 1), np.arange(lo, 0)]).astype(np.int64)


def expect(t, lo, hi, sign):
    """(lag[M] int32, mv[M] long double, B[M], ratio[M]) of the range [lo, hi] under `sign` from a table that holds its lags"""
    order = scan_order(t.n, lo, hi)
    assert t.lags[0] <= order.min() and order.max() <= t.lags[-1], (lo, hi, int(t.lags[0]), int(t.lags[-1]))
    cols = order + t.Lc
    sub, Bs = t.cc[:, cols], t.B[:, cols]
    key = np.abs(sub) if sign == 0 else (sub if sign > 0 else -sub)
    k = np.argmax(key, axis=1)
    r = np.arange(len(k))
    k1, B1 = key[r, k], Bs[r, k]
    win = k1 > 0
    lag = np.where(win, order[k], 0).astype(np.int32)
    mv = np.where(win, sub[r, k], sub[:, 0] if sign == 0 else np.longdouble(0))
    B = np.where(win, B1, Bs[:, 0])
    if len(order) > 1:
        key2 = key.copy()
        key2[r, k] = -np.inf
        j = np.argmax(key2, axis=1)
        k2, B2 = np.maximum(key2[r, j], 0), Bs[r, j]
    else:
        k2, B2 = np.zeros(len(k), dtype=np.longdouble), np.zeros(len(k))
    ratio = np.where(win, (k1 - k2) / (B1 + B2), -k1 / B1).astype(np.float64)
    return lag, mv, B, ratio


def in_range(case, n, lo, hi, i=0):
    """the non-outlier rows whose planted lag (against reference i) lies inside the clipped range"""
    lo, hi = LR.clip(n, lo, hi)
    pl = WS.planted(case, i)
    return ~case.outlier & (pl >= lo) & (pl <= hi)


def full_cc(t, row):
    """one row of a table as the float64 correlation slice the restated kernel rules take: cc[lag mod n], zero off the table"""
    cc = np.zeros(t.n)
    cc[t.lags % t.n] = t.cc[row].astype(np.float64)
    return cc


# ------------------------------------------------------------------ a. the direct product from any origin
DIRECT_LENGTHS = (1433, 1025, 480, 64)   # odd stride; a last chunk of one sample; less than one chunk; N = n (hi clipped to 32, lo to -31)
RANDOM_RANGES = 200


def direct_lags(N):
    """one row per lag in [-126, 126] and 30 per side just outside, where the code still fits in the row (N = n: folded, each once)"""
    w = WS.code_len(N)
    n, p = LS.fft_len(N), (N - w) // 2
    cand = list(range(-RMAX, RMAX + 1)) + [s * k for k in range(RMAX + 1, RMAX + 1 + OUTSIDE) for s in (1, -1)]
    if N == n:
        out = []
        for lag in WS.fold_lag(cand, n).tolist():
            if lag not in out:
                out.append(lag)
        return np.array(out, dtype=np.int64)
    return np.array([lag for lag in cand if 0 <= p - lag <= N - w], dtype=np.int64)


def direct_case(N):
    return WS.make_case(N, seed=WS.case_seed(N), lags=direct_lags(N))


def direct_table_lags(n):
    lo, hi = LR.clip(n, -RMAX, RMAX)
    return np.arange(lo, hi + 1)


def direct_ranges(N):
    """every one-sided (-k, 0) and (0, k), k = 0 .. 126; the widest range at every origin; 200 seeded random ranges of at most 127
    lags: every tile count 1 .. 8 and every origin residue mod 16.  As asked for: the kernels see them clipped (N = 64)"""
    out = [(0, 0)] + [(-k, 0) for k in range(1, RMAX + 1)] + [(0, k) for k in range(1, RMAX + 1)]
    out += [(lo, lo + RMAX) for lo in range(-RMAX, 1)]
    rng = np.random.default_rng([N, 9])
    while len(out) < 2 * RMAX + 1 + RMAX + 1 + RANDOM_RANGES:
        Wd = int(rng.integers(1, RMAX + 2))
        lo = -int(rng.integers(0, Wd))
        out.append((lo, lo + Wd - 1))
    return out


def tiles_of(n, lo, hi):
    lo, hi = LR.clip(n, lo, hi)
    return (hi - lo + 1 + 15) // 16


# ------------------------------------------------------------------ b. the panel kernels
PANEL = 128
PANEL_LENGTHS = (2049, 2500)             # 3 chunks, the last one sample long, odd stride; even stride
PANEL_SPAN = 180
PANEL_WIDTHS = (128, 129, 255, 256, 257, 300, 361)
PANEL_SLICES = (0, 1, 2, 3)              # 0 = the planner


def panel_case(N):
    return WS.make_case(N, seed=N, lags=np.arange(-PANEL_SPAN, PANEL_SPAN + 1))


def panel_table_lags():
    m = max(PANEL_WIDTHS) - 1
    return np.arange(-m, m + 1)


def panel_ranges():
    """each width from three origins: lo = 0, lo = -W / 2, hi = 0 ((-128, 0) and (0, 128): two panels, the second a single row)"""
    out = []
    for Wd in PANEL_WIDTHS:
        out += [(0, Wd - 1), (-(Wd // 2), Wd - 1 - Wd // 2), (-(Wd - 1), 0)]
    assert (-128, 0) in out and (0, 128) in out
    return out


def sub_ranges(lo, hi):
    """the two sub-ranges of at most 127 lags whose direct product must give the panels' bits on the rows that win inside them:
    (0, min(hi, 126)) for the winners 0 .. 126 and (max(lo, -126), 0) for the winners -126 .. -1"""
    return (0, min(hi, RMAX)), (max(lo, -RMAX), 0)


# sixteen panels at N = 2500 (n = 4096): the code in the middle for (-1023, 1024); the code one sample short of the tail for
# (0, 2047) -- from the very tail no row could carry lag -1, the lag just outside that range's lower end
SIXTEEN_N = 2500
SIXTEEN = (("middle", None, (-1023, 1024)), ("tail", SIXTEEN_N - LS.W - 1, (0, 2047)))
SIXTEEN_SLICES = (0, 1, 2)


def sixteen_lags(lo, hi):
    """table rows v = 128 z + {-2, -1, 0, 1}, z = 0 .. 16, that fall inside the range (v = lag - lo), both ends among them, and one
    lag just outside each end"""
    Wd = hi - lo + 1
    vs = sorted({128 * z + d for z in range(17) for d in (-2, -1, 0, 1) if 0 <= 128 * z + d < Wd} | {0, Wd - 1})
    return np.array([lo - 1] + [v + lo for v in vs] + [hi + 1], dtype=np.int64)


def sixteen_case(which):
    name, p, (lo, hi) = [c for c in SIXTEEN if c[0] == which][0]
    return WS.make_case(SIXTEEN_N, seed=SIXTEEN_N + (0 if p is None else 1), lags=sixteen_lags(lo, hi), p=p), (lo, hi)


# ------------------------------------------------------------------ d. many references on the direct packed pass
MANY_N = 480
MANY_RANGES = ((-126, 0), (0, 126), (-100, 26))


def many_table_lags():
    return np.arange(-RMAX, RMAX + 1)


# ------------------------------------------------------------------ c. the masked transform kernels
# Every output index is planted once (_lagsweep.sweep_cases(N, None)); the expectation has two tiers.  A row planted INSIDE the
# range, and of the sign, must come back at its planted lag with _lagsweep.ld_score_at's long-double score within
# _lagsweep.row_bounds (the mask adds no arithmetic).  Every other row has its 0.9 peak outside the range or of the other sign -- a
# leaking mask would report it -- and is compared with the definition applied to the oracle's correlation (oracle_expect: _signed's
# expect, vectorised over the rows; the CPU file shows the two agree), at the project's 1e-6 / 1e-12, lag exact, no tie allowed.
MASKED_LENGTHS = (512, 280, 1024, 2048, 4096, 3000)      # 280: n = 512 with head and tail references, the c1 table in use
MASKED_F32 = (1024, 4096)
FORCED_RANGES = ((0, 0), (-1, 0), (0, 1), (-16, 0))      # sent through the transform by the test hook
SCORE_RTOL, SCORE_ATOL = 1e-6, 1e-12
TIE_GAP = LR.TIE_GAP
THREADS = 8                # of the CPU oracle's transforms
MANY_MASKED_LENGTHS = (4096, 1024)
MANY_MASKED_RANGES = ((-257, 0), (-255, 256), (-1000, 70))


def masked_ranges(n):
    h = n // 2
    return [(-257, 0), (-256, 255), (-255, 256), (0, h), (-(h - 1), 0), (-(h - 1), h), (-64, 300), (-1000, 70)]


def every_lag(n, lo, hi):
    return LR.clip(n, lo, hi) == (-(n // 2 - 1), n // 2)


class Masked:
    """one reference's rows: C[M, n] the oracle's correlation, pl[M] the planted lag, ld[M] the long-double score at the planted
    index, sgn[M] its sign, bounds[M] _lagsweep.row_bounds"""


def masked_case(oracle, ref, rows, ks, f32=False):
    """f32: the rows as a float32-storage group holds them"""
    rows = np.asarray(rows, dtype=np.float64)
    if f32:
        rows = rows.astype(np.float32).astype(np.float64)
    m = Masked()
    M, N = rows.shape
    X, n = oracle.ref_spectrum(ref)
    assert n == LS.fft_len(N)
    m.ref, m.rows, m.n, m.N, m.f32 = ref, rows, n, N, f32
    m.C = np.empty((M, n))

    def fill(r):                               # (one oracle transform per row; the C oracle runs outside the interpreter lock)
        m.C[r] = oracle.xcorr_with_x(X, rows[r], n)[0]
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(fill, range(M)))
    assert np.all(np.isfinite(m.C))
    m.k = np.asarray(ks, dtype=np.int64)
    m.pl = LS.fold(m.k, n).astype(np.int64)
    m.ld = LS.ld_scores(ref, rows, n, m.k)
    m.sgn = np.sign(m.ld.astype(np.float64)).astype(np.int64)
    m.bounds, _ = LS.row_bounds(n, rows, ref)
    for a in (m.rows, m.C, m.pl, m.ld, m.sgn, m.bounds):
        a.setflags(write=False)
    m.want = {}
    return m


def prepare(m, ranges, signs=SIGNS):
    """fills m.want for every range and sign at once (the wide ranges cost a pass over all of C each: a few at a time)"""
    keys = [(lo, hi, s) for lo, hi in ranges for s in signs if (lo, hi, s) not in m.want]
    with ThreadPoolExecutor(4) as pool:
        for key, got in zip(keys, pool.map(lambda k: oracle_expect(m.C, m.n, *k), keys)):
            m.want[key] = got
    return m


def masked_cases(oracle, N, f32=False):
    n = LS.fft_len(N)
    return [prepare(masked_case(oracle, ref, rows, ks, f32), masked_ranges(n) + list(FORCED_RANGES)) for ref, rows, ks in LS.sweep_cases(N, None)]


def oracle_expect(C, n, lo, hi, sign):
    """_signed.signed_ranged_fast over all rows of a finite C at once: (lag[M], mv[M], tie[M])"""
    idx = LR.range_indices(n, lo, hi)
    sub = C[:, idx]
    key = np.abs(sub) if sign == 0 else (sub if sign > 0 else -sub)
    r = np.arange(C.shape[0])
    j = np.argmax(key, axis=1)
    k1 = key[r, j].copy()
    win = k1 > 0
    mi = np.where(win, idx[j], 0)
    lag = np.where(mi <= n // 2, mi, mi - n).astype(np.int32)
    mv = np.where(win, C[r, mi], C[:, 0] if sign == 0 else 0.0)
    tie = np.zeros(len(r), dtype=bool)
    if len(idx) > 1:
        if key is sub:
            key = sub.copy()
        key[r, j] = -np.inf
        k2 = key.max(axis=1)
        tie = win & (k2 > 0) & ((k1 - k2) <= TIE_GAP * k1)
    return lag, mv, tie


def masked_want(m, lo, hi, sign, g=1):
    """the expectation of range and sign on the rows (g = 1) or the negated rows (g = -1: the definition is odd in the rows, so the
    sign and the values swap): (tier1[M], lag[M], mv[M], tie[M]) -- tier1 rows: lag = planted, value g * ld"""
    key = (lo, hi, sign * g)
    if key not in m.want:
        m.want[key] = oracle_expect(m.C, m.n, lo, hi, sign * g)
    lag, mv, tie = m.want[key]
    clo, chi = LR.clip(m.n, lo, hi)
    tier1 = (m.pl >= clo) & (m.pl <= chi) & ((sign == 0) | (m.sgn * g == sign))
    return tier1, lag, mv * g if g < 0 else mv, tie


def masked_name(n, N, f32, sign, occ4=False):
    """the instantiation's name (muse_batch_kernel_name)"""
    padded, f = "true" if N < n else "false", "true" if f32 else "false"
    if sign:
        neg = "true" if sign < 0 else "false"
        if n == 4096:
            return "xcorr_fused_n4096_%s_signed<%s, %s, %s>" % ("occ4" if occ4 else "fold", padded, f, neg)
        return "xcorr_fused_small_signed<%d, %s, %s, %s>" % (n.bit_length() - 1, padded, f, neg)
    if n == 4096:
        return ("xcorr_fused_n4096_occ4<%s, 3, false, %s, true>" if occ4 else "xcorr_fused_n4096_fold<false, %s, %s, true>") % (padded, f)
    return "xcorr_fused_small<%d, %s, false, %s, true>" % (n.bit_length() - 1, padded, f)


def many_masked_name(n, N):
    padded = "true" if N < n else "false"
    if n == 4096:
        return "xcorr_fused_n4096_fold_multi<%s, false, true>" % padded
    return "xcorr_fused_small<%d, %s, true, false, true>" % (n.bit_length() - 1, padded)


def many_masked_cases(oracle, N):
    refs, rows, ks = LS.many_refs_case(N)
    return [prepare(masked_case(oracle, ref, rows, k), MANY_MASKED_RANGES, (0,)) for ref, k in zip(refs, ks)]


# ------------------------------------------------------------------ exact ties across panels
# The gap condition above leaves the tie-break of the panels' merge (equal |val|: the smaller scan position wins) unused, so it has a
# case of its own.  The reference repeats a block of TIE_PERIOD samples exactly; a row is +amp at sample a, -amp at sample b and
# zero elsewhere.  Then sum d == 0 exactly, the mean term vanishes and cc[lag] is (e[a + lag] - e[b + lag]) amp / sigma: the SAME
# operands in the same places at lag and lag + TIE_PERIOD, so the kernels' values there are equal bit for bit (as are the
# long-double table's), whatever the slices and panels.  The definition takes the first of them in scan order.
TIE_N, TIE_PERIOD, TIE_ROWS = 2500, 30, 20
TIE_RANGES = ((-200, 50), (-128, 0), (0, 128), (-1023, 1024))
TIE_SLICES = (0, 1, 2, 3)


def tie_case():
    """(ref, rows): impulses far enough inside the row that every lag of TIE_RANGES keeps them on the reference"""
    rng = np.random.default_rng([TIE_N, 11])
    ref = np.tile(rng.standard_normal(TIE_PERIOD), TIE_N // TIE_PERIOD + 1)[:TIE_N]
    rows = np.zeros((TIE_ROWS, TIE_N))
    for r in range(TIE_ROWS):
        a = int(rng.integers(1100, 1300))
        amp = float(rng.uniform(0.5, 1.5))
        rows[r, a], rows[r, a + int(rng.integers(1, TIE_PERIOD))] = amp, -amp
    for x in (ref, rows):
        x.setflags(write=False)
    return ref, rows


def tie_table_lags():
    return np.arange(min(r[0] for r in TIE_RANGES), max(r[1] for r in TIE_RANGES) + 1)


def expect_tied(t, lo, hi):
    """(lag, mv, B, ratio, ties): the first maximum of |cc| in scan order; ties[r]: how many lags of the range hold exactly that
    |cc|; ratio: (the maximum - the largest |cc| below it) / (2 max B) -- the gap condition between the tied group and the rest"""
    order = scan_order(t.n, lo, hi)
    cols = order + t.Lc
    sub, Bs = t.cc[:, cols], t.B[:, cols]
    key = np.abs(sub)
    k = np.argmax(key, axis=1)
    r = np.arange(len(k))
    top = key[r, k]
    ties = (key == top[:, None]).sum(axis=1)
    below = np.where(key < top[:, None], key, 0).max(axis=1)
    ratio = ((top - below) / (2 * Bs.max(axis=1))).astype(np.float64)
    return order[k].astype(np.int32), sub[r, k], Bs[r, k], ratio, ties
