"""The signed best match (include/muse_hip.h, muse_batch_score_signed_in_lag_range) applied in numpy to the correlation slice the
CPU oracle returns, and the inputs tests/test_signed_lag_range_cpu.py and tests/test_gpu_signed_lag_range.py share.  Nothing here
touches the code under test: the CPU test checks, on exactly these inputs, that the oracle by itself flags no tie the GPU tests
could hide behind and that the rows show what filtering could not."""
import numpy as np

import _lagrange as LR
import _window as W

TIE_GAP = W.TIE_GAP
SIGNS = (1, -1)


def signed_ranged(cc, n, lo, hi, sign):
    """(lag, mv, tie) of one series, the plain loop: from (0, 0.0), index i of the range's scan order is taken when sign * cc[i] >
    sign * best (strict: the first index wins, only values of the sign can win, NaN never); nothing of the sign: (0, +0.0).  cc
    None = the reference's (nil, 0, 0); a slice of nothing but NaN = a NaN / Inf series: (0, NaN), as the unsigned pass gives.  tie:
    the two largest values OF THE SIGN inside the range lie within TIE_GAP relative of each other.  sign 0: tests/_lagrange.py's
    ranged."""
    if sign == 0:
        return LR.ranged(cc, n, lo, hi)
    if cc is None:
        return 0, 0.0, False
    if np.isnan(cc).all():
        return 0, float("nan"), False
    s = 1.0 if sign > 0 else -1.0
    mi, best = 0, 0.0
    for i in LR.range_indices(n, lo, hi):
        if s * cc[i] > s * best:        # (NaN compares false: never taken)
            best, mi = cc[i], int(i)
    if not s * best > 0.0:
        return 0, 0.0, False
    k = [s * cc[i] for i in LR.range_indices(n, lo, hi) if s * cc[i] > 0.0]
    k.sort(reverse=True)
    tie = bool(len(k) >= 2 and (k[0] - k[1]) <= TIE_GAP * k[0])
    return (mi if mi <= n // 2 else mi - n), float(best), tie


def signed_ranged_fast(cc, n, lo, hi, sign):
    """the same, vectorised (np.argmax returns the first maximum = strict '>' in scan order)"""
    if sign == 0:
        return LR.ranged_fast(cc, n, lo, hi)
    if cc is None:
        return 0, 0.0, False
    if np.isnan(cc).all():
        return 0, float("nan"), False
    idx = LR.range_indices(n, lo, hi)
    k = (1.0 if sign > 0 else -1.0) * cc[idx]
    k = np.where(np.isnan(k), -1.0, k)
    j = int(np.argmax(k))
    if not k[j] > 0.0:
        return 0, 0.0, False
    mi = int(idx[j])
    u = k[k > 0.0]
    tie = False
    if len(u) >= 2:
        top = np.partition(u, len(u) - 2)[-2:]
        tie = bool((top[1] - top[0]) <= TIE_GAP * top[1])
    return (mi if mi <= n // 2 else mi - n), float(cc[mi]), tie


def expect(oracle, ref, rows, ranges, signs=(0, 1, -1)):
    """{(lo, hi, sign): (lag[M], mv[M], tie[M])} by the definition, and n.  One oracle transform per row."""
    rows = np.asarray(rows, dtype=np.float64)
    M = rows.shape[0]
    X, n = oracle.ref_spectrum(ref)
    keys = [(lo, hi, s) for lo, hi in ranges for s in signs]
    out = {k: (np.zeros(M, dtype=np.int32), np.zeros(M), np.zeros(M, dtype=bool)) for k in keys}
    for r in range(M):
        cc = oracle.xcorr_with_x(X, rows[r], n)[0]
        for k in keys:
            out[k][0][r], out[k][1][r], out[k][2][r] = signed_ranged_fast(cc, n, *k)
    return out, n


# ---- the kernels' rules, restated in numpy
def _key(v, sign):
    return abs(v) if sign == 0 else v if sign > 0 else -v


def table_argmax(cc, n, lo, hi, sign):
    """the direct product's scan (tests/_lagrange.py's table_argmax) with the key |v|, v or -v in place of |v|; nothing found: the
    unsigned scan reads row `origin` (cc[0]), the signed one returns +0.0; a NaN / Inf series (the kernel knows it by its statistics,
    here: a slice of nothing but NaN) is (0, NaN) in front of either.  -> (lag, mv)"""
    if np.isnan(cc).all():
        return 0, float("nan")
    lo, hi = LR.clip(n, lo, hi)
    origin, Wd = -lo, hi - lo + 1
    table = np.array([cc[(v - origin) % n] for v in range(Wd)])
    best_key, best_val, best_pos = 0.0, 0.0, -1
    for pos in range(Wd):
        v = (pos if pos <= hi else pos - 1 - hi + lo) + origin
        if _key(table[v], sign) > best_key:
            best_key, best_val, best_pos = _key(table[v], sign), table[v], pos
    if best_pos < 0:
        return 0, (0.0 if sign else float(table[origin]))
    return (best_pos if best_pos <= hi else best_pos - 1 - hi + lo), float(best_val)


def masked_argmax(cc, n, lo, hi, sign):
    """the WIN kernels' rule with the sign in the mask: every entry outside the range, and inside it every entry that is not > 0
    (sign +1) / < 0 (sign -1), replaced by +0.0; then the unrestricted maxAbsIndex, the cc[0] fallback (of the MASKED values), the
    lag unwrap; a NaN / Inf series (by its statistics; here: a slice of nothing but NaN) is (0, NaN).  -> (lag, mv)"""
    if np.isnan(cc).all():
        return 0, float("nan")
    lo, hi = LR.clip(n, lo, hi)
    i = np.arange(n)
    keep = (i <= hi) | (i >= n + lo)
    with np.errstate(invalid="ignore"):
        if sign > 0:
            keep &= cc > 0.0
        elif sign < 0:
            keep &= cc < 0.0
    m = np.where(keep, cc, 0.0)
    a = np.abs(m)
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    mi = k if a[k] > 0 else 0
    return (mi if mi <= n // 2 else mi - n), float(m[mi])


# ---- the shared inputs
SPECIAL_ROWS = 1 + W.SPECIALS   # row 0 and the eight specials of tests/_window.py's make_case
MAX_SHIFT = 40


def make_case(N, M, seed, scaled=True, max_shift=MAX_SHIFT):
    """(ref, rows).  Rows 0 .. 8 are tests/_window.py's make_case(N, 9, seed): a plain row and its eight specials (a copy of the
    reference, a negated copy, a constant row, a NaN row, an Inf row, mean 1e6 with sigma 1, scaled by 1e-100 and by 1e100).  Row
    r >= 9, by r % 4:
      0, 1, 2 -- a * shift(ref, d1) - b * shift(ref, d2) + noise, d1 != d2, both inside +-max_shift: a correlated copy at one lag and an
                 anti-correlated one at another; 0: a > b (the positive peak is the larger one by magnitude), 1: a < b (the
                 negative one is), 2: b = 0 (no planted negative peak);
      3       -- pure noise.
    _window.make_case's rows correlate positively almost everywhere: they cannot show a best match of the other sign."""
    ref, head = W.make_case(N, SPECIAL_ROWS, seed, scaled=scaled)
    rng = np.random.default_rng(seed + 77)
    rows = np.zeros((M, N))
    rows[:min(M, SPECIAL_ROWS)] = head[:min(M, SPECIAL_ROWS)]
    for r in range(SPECIAL_ROWS, M):
        cls = r % 4
        noise = 0.3 * rng.standard_normal(N) + rng.standard_normal()
        if cls == 3:
            rows[r] = noise
            continue
        d1 = int(rng.integers(-max_shift, max_shift + 1))
        d2 = d1
        while d2 == d1:
            d2 = int(rng.integers(-max_shift, max_shift + 1))
        big, small = 1.0 + rng.random(), 0.35 + 0.3 * rng.random()
        a, b = ((big, small), (small, big), (big, 0.0))[cls]
        rows[r] = a * np.roll(ref, d1) - b * np.roll(ref, d2) + noise
    return ref, rows


def planted_rows(M):
    """the rows of make_case with planted matches: the rows of classes 0 .. 2"""
    r = np.arange(M)
    return (r >= SPECIAL_ROWS) & (r % 4 != 3)


def plain_rows(M):
    """the rows of make_case that are no copies of the reference, constants, NaN / Inf rows (tests/_window.py's plain_rows).  The two
    copies are left out of the tie conditions as they are there, and here for a reason of their own: the autocorrelation is even,
    cc[k] == cc[-k], so under the sign the copy does NOT match with (+1 for -ref, -1 for ref) its best value is an exact tie
    between two mirror lags by construction, whatever the seed.  The oracle flags them; the GPU tests compare such rows by value."""
    return W.plain_rows(M)


PARITY_M = LR.PARITY_M


def mfma_case(N):
    return make_case(N, PARITY_M, seed=13000 + N)


def masked_case(N, f32):
    ref, rows = make_case(N, PARITY_M, seed=14000 + N)
    if f32:
        with np.errstate(over="ignore"):
            rows = rows.astype(np.float32).astype(np.float64)
    return ref, rows


# edges: tests/_lagrange.py's edge_case with the planted code negated on every second row
def edge_case(N, lo, hi):
    """(ref, rows, n, planted lag of every row, sign of every row's planted match)"""
    ref, rows, n, planted = LR.edge_case(N, lo, hi)
    # the rows' amplitudes have random signs (tests/_lagsweep.py, make_rows): the sign of a row's planted match is the sign of its
    # circular correlation with the reference where that is largest by magnitude (the planted code: the rest is low noise)
    F = np.fft.rfft(ref - ref.mean())
    cc = np.fft.irfft(np.conj(F)[None, :] * np.fft.rfft(rows - rows.mean(axis=1, keepdims=True), axis=1), n=N, axis=1)
    have = np.sign(cc[np.arange(len(rows)), np.argmax(np.abs(cc), axis=1)]).astype(np.int64)
    sgn = np.where(np.arange(rows.shape[0]) % 2 == 0, 1, -1)      # rows 0, 2, ... match positively, rows 1, 3, ... negatively
    return ref, rows * (sgn * have)[:, None], n, planted, sgn


# the Run form: label groups of 3
RUN_NS, RUN_RANGES, RUN_M, RUN_GROUP = LR.RUN_NS, LR.RUN_RANGES, LR.RUN_M, 3


def run_case(N):
    """shifts of up to 12 samples: either way round, about half of them lie inside the narrow range of RUN_RANGES"""
    return make_case(N, RUN_M, seed=16000 + N, scaled=False, max_shift=12)


def run_groups():
    return (np.arange(RUN_M) // RUN_GROUP).astype(np.int32), RUN_M // RUN_GROUP


# the C++ program's series (host/muse_signed_lag_range_test.cpp): tests/_lagrange.py's, series i negated when i % 4 == 1
CPP_RANGES = LR.CPP_RANGES
CPP_SIGNED_MAXLAG = 40


def cpp_case():
    ref, rows = LR.cpp_case()
    rows[1::4] *= -1.0
    return ref, rows
