"""The lag-band definition (include/muse_hip.h, muse_batch_score_in_lag_band) applied in numpy to the correlation slice the CPU
oracle returns, and the inputs tests/test_lag_band_cpu.py and tests/test_gpu_lag_band.py share.  Nothing here touches the code
under test: the CPU test checks, on exactly these inputs, that the oracle by itself flags no tie, so that the GPU tests may demand
exact lags on every row."""
import numpy as np

import _lagrange as LR
import _lagsweep as LS
import _signed as SG
import _window as W

TIE_GAP = W.TIE_GAP
SIGNS = (0, 1, -1)


def clip(n, lo, hi):
    """the band as the definition clips it: hi to n / 2, lo to -(n / 2 - 1); None when nothing of it is left"""
    lo, hi = max(int(lo), -(n // 2 - 1)), min(int(hi), n // 2)
    return (lo, hi) if lo <= hi else None


def holds_zero(lo, hi):
    return lo <= 0 <= hi


def band_indices(n, lo, hi):
    """the indices a band WITHOUT lag 0 scans, ascending: lo .. hi above zero, n + lo .. n + hi below"""
    lo, hi = clip(n, lo, hi)
    assert not holds_zero(lo, hi)
    return np.arange(lo, hi + 1, dtype=np.int64) if lo > 0 else np.arange(n + lo, n + hi + 1, dtype=np.int64)


def _key(v, sign):
    return abs(v) if sign == 0 else v if sign > 0 else -v


def banded(cc, n, lo, hi, sign):
    """(lag, mv, tie) of one series, the plain loop.  A band that holds lag 0 is tests/_signed.py's signed_ranged.  Otherwise: from
    (0, 0.0), index i of the band in ascending order is taken when key(cc[i]) > key(best), strict, key = |v|, v, -v for sign 0, +1,
    -1 -- so only keys > 0 can win and a NaN never does; nothing wins: (0, +0.0), whatever cc[0] is.  cc None = the reference's
    (nil, 0, 0); a slice of nothing but NaN = a NaN / Inf series: (0, NaN).  tie: the two largest keys > 0 of the band lie within
    TIE_GAP relative of each other."""
    clo, chi = clip(n, lo, hi)
    if holds_zero(clo, chi):
        return SG.signed_ranged(cc, n, lo, hi, sign)
    if cc is None:
        return 0, 0.0, False
    if np.isnan(cc).all():
        return 0, float("nan"), False
    mi, best, bkey = -1, 0.0, 0.0
    for i in band_indices(n, lo, hi):
        if _key(cc[i], sign) > bkey:        # (NaN compares false: never taken)
            bkey, best, mi = _key(cc[i], sign), cc[i], int(i)
    if mi < 0:
        return 0, 0.0, False
    k = sorted((_key(cc[i], sign) for i in band_indices(n, lo, hi) if _key(cc[i], sign) > 0.0), reverse=True)
    tie = bool(len(k) >= 2 and (k[0] - k[1]) <= TIE_GAP * k[0])
    return (mi if mi <= n // 2 else mi - n), float(best), tie


def banded_fast(cc, n, lo, hi, sign):
    """the same, vectorised (np.argmax returns the first maximum = strict '>' in ascending order)"""
    clo, chi = clip(n, lo, hi)
    if holds_zero(clo, chi):
        return SG.signed_ranged_fast(cc, n, lo, hi, sign)
    if cc is None:
        return 0, 0.0, False
    if np.isnan(cc).all():
        return 0, float("nan"), False
    idx = band_indices(n, lo, hi)
    v = cc[idx]
    k = np.abs(v) if sign == 0 else v if sign > 0 else -v
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


def expect(oracle, ref, rows, bands, signs=SIGNS, fn=banded_fast):
    """{(lo, hi, sign): (lag[M], mv[M], tie[M])} by the definition for the bands that are not empty at this length, and n.  One
    oracle transform per row."""
    rows = np.asarray(rows, dtype=np.float64)
    M = rows.shape[0]
    X, n = oracle.ref_spectrum(ref)
    keys = [(lo, hi, s) for lo, hi in bands if clip(n, lo, hi) for s in signs]
    out = {k: (np.zeros(M, dtype=np.int32), np.zeros(M), np.zeros(M, dtype=bool)) for k in keys}
    for r in range(M):
        cc = oracle.xcorr_with_x(X, rows[r], n)[0]
        for k in keys:
            out[k][0][r], out[k][1][r], out[k][2][r] = fn(cc, n, *k)
    return out, n


def slices(oracle, ref, rows):
    """the oracle's correlation slice of every row (None: sigma == 0), and n"""
    X, n = oracle.ref_spectrum(ref)
    return [oracle.xcorr_with_x(X, np.asarray(r, dtype=np.float64), n)[0] for r in rows], n


# ---- the kernels' rules, restated in numpy (bands without lag 0)
def table_scan(cc, n, lo, hi, sign):
    """the direct product's band scan: a table whose row v is lag lo + v (origin = -lo), position pos is row pos, strict '>' from
    0.0 on the key; nothing found: (0, +0.0) -- no row is read; the lag of position pos is pos - origin.  -> (lag, mv)"""
    if np.isnan(cc).all():
        return 0, float("nan")
    lo, hi = clip(n, lo, hi)
    origin, Wd = -lo, hi - lo + 1
    table = np.array([cc[(v - origin) % n] for v in range(Wd)])
    best_key, best_val, best_pos = 0.0, 0.0, -1
    for pos in range(Wd):
        if _key(table[pos], sign) > best_key:
            best_key, best_val, best_pos = _key(table[pos], sign), table[pos], pos
    if best_pos < 0:
        return 0, 0.0
    return best_pos - origin, float(best_val)


def interval_mask_argmax(cc, n, lo, hi, sign):
    """the band builds of the transform kernels: every entry outside the ONE index interval a <= i <= b (a = lo, b = hi above zero;
    a = n + lo, b = n + hi below), and inside it every entry that has not the sign, replaced by +0.0; then the unchanged maxAbsIndex
    with its fallback to entry 0 of the MASKED values (+0.0: index 0 is never inside) and the lag unwrap.  -> (lag, mv)"""
    if np.isnan(cc).all():
        return 0, float("nan")
    lo, hi = clip(n, lo, hi)
    a, b = (lo, hi) if lo > 0 else (n + lo, n + hi)
    i = np.arange(n)
    keep = (i >= a) & (i <= b)
    with np.errstate(invalid="ignore"):
        if sign > 0:
            keep &= cc > 0.0
        elif sign < 0:
            keep &= cc < 0.0
    m = np.where(keep, cc, 0.0)
    av = np.abs(m)
    av = np.where(np.isnan(av), -1.0, av)
    k = int(np.argmax(av))
    mi = k if av[k] > 0 else 0
    return (mi if mi <= n // 2 else mi - n), float(m[mi])


# ---- 1. the direct product
MFMA_NS = (64, 100, 480, 1025, 1100)
MFMA_BANDS = ((1, 1), (-1, -1), (1, 7), (-7, -1), (1, 16), (2, 18), (-17, -1), (1, 127), (-127, -1), (5, 131), (20, 40), (-40, -20),
              (100, 226), (-226, -100), (200, 230), (-255, -200))
FAR_BANDS = ((100, 226), (-226, -100), (200, 230), (-255, -200))     # empty at n = 64 and 128
PARITY_M = 35
SMALL_MS = (1, 15, 17)
SMALL_M_N = 480


def mfma_case(N, M=PARITY_M):
    return W.make_case(N, M, seed=3000 + N)


# ---- 2. the masked transform pass
MASKED_NS = (480, 1000, 1433, 3000, 4096)
MASKED_FORCED = ((1, 7), (-17, -1), (20, 40), (-40, -20))            # narrow bands under muse_test_in_window_force_transform


def masked_bands(n):
    return [(1, 200), (-200, -1), (100, 300), (-1000, -70), (1, n // 2), (-(n // 2 - 1), -1), (n // 2, n // 2), (255, 256), (256, 511),
            (257, 510), (-512, -257), (6, 133)]


def masked_case(N, f32):
    ref, rows = W.make_case(N, PARITY_M, seed=4000 + N)
    if f32:
        with np.errstate(over="ignore"):
            rows = rows.astype(np.float32).astype(np.float64)
    return ref, rows


# ---- 4. edges: a code planted at the lags around both ends of a band and around zero
EDGE_CASES = ((4096, (3, 40)), (4096, (-40, -3)), (4096, (100, 300)), (4096, (-300, -100)), (512, (5, 60)), (512, (-60, -5)),
              (512, (100, 200)), (512, (-200, -100)))


def edge_case(N, lo, hi):
    """(ref, rows, n, planted lag of every row): tests/_lagrange.py's edge_case for a band -- the lags lo-1, lo, lo+1, hi-1, hi,
    hi+1, -1, 0, 1 (each once), rows shuffled"""
    return LR.edge_case(N, lo, hi)


# ---- 6. a band of exact zeros (tests/_rowslagrange.py's zeros_case: the reference is zero wherever the last row's two spikes reach)
ZEROS_N = 2500
ZEROS_BANDS = ((1, 50), (-127, -1), (10, 40), (-150, -30))           # inside -200 .. 50, at most 127 lags: the direct product; forced: the masked pass


def zeros_case():
    rng = np.random.default_rng(7700)
    ref = np.zeros(ZEROS_N)
    ref[1000:1040] = 2.0
    ref[1100:1140] = -2.0
    rows = np.zeros((6, ZEROS_N))
    for r in range(6):
        rows[r] = (0.5 + rng.random()) * np.roll(ref, int(rng.integers(-180, 40))) + 0.3 * rng.standard_normal(ZEROS_N)
    rows[5] = 0.0
    rows[5, 100] = 1.0          # ref[100 + lag] and ref[2300 + lag] are zero for every lag in -200 .. 50
    rows[5, 2300] = -1.0
    return ref, rows, 5


# ---- 7. the Run form
RUN_NS = (480, 3000)
RUN_BANDS = ((1, 15), (-300, -20))
RUN_M = 60
RUN_GROUP = 3


def run_case(N):
    return W.make_case(N, RUN_M, seed=6000 + N, scaled=False)


def run_groups():
    return (np.arange(RUN_M) // RUN_GROUP).astype(np.int32), RUN_M // RUN_GROUP


# the C++ program's series (host/muse_lag_band_test.cpp)
CPP_BANDS = ((1, 15), (-300, -20))


def cpp_case():
    """tests/_signed.py's: the LCG series, series i negated when i % 4 == 1"""
    return SG.cpp_case()
