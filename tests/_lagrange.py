"""The lag-range definition (include/muse_hip.h, muse_batch_score_in_lag_range) applied in numpy to the correlation slice the CPU
oracle returns, and the inputs tests/test_lag_range_cpu.py and tests/test_gpu_lag_range.py share.  Nothing here touches the code
under test: the CPU test checks, on exactly these inputs, that the oracle by itself flags no tie the GPU tests could hide behind."""
import numpy as np

import _lagsweep as LS
import _window as W

TIE_GAP = W.TIE_GAP


def clip(n, lo, hi):
    """the range as the definition clips it: hi to n / 2, lo to -(n / 2 - 1)"""
    return max(int(lo), -(n // 2 - 1)), min(int(hi), n // 2)


def range_indices(n, lo, hi):
    """the indices maxAbsIndex scans, in scan order: 0 .. hi, then n + lo .. n - 1 (none when lo == 0)"""
    lo, hi = clip(n, lo, hi)
    assert lo <= 0 <= hi
    return np.concatenate([np.arange(0, hi + 1), np.arange(n + lo, n)]).astype(np.int64)


def ranged(cc, n, lo, hi):
    """(lag, mv, tie) of one series, the plain loop: maxAbsIndex (start (0, 0.0), strict '>') over the range's indices of cc; cc
    None = the reference's (nil, 0, 0).  tie: the two largest |cc| inside the range lie within TIE_GAP relative of each other."""
    if cc is None:
        return 0, 0.0, False
    idx = range_indices(n, lo, hi)
    mi, mval = 0, 0.0
    for i in idx:
        if abs(cc[i]) > abs(mval):      # (NaN compares false: never taken)
            mval, mi = cc[i], int(i)
    a = np.abs(cc[idx])
    a = np.sort(a[np.isfinite(a)])[::-1]
    tie = bool(len(a) >= 2 and a[0] > 0 and (a[0] - a[1]) <= TIE_GAP * a[0])
    return (mi if mi <= n // 2 else mi - n), float(cc[mi]), tie


def ranged_fast(cc, n, lo, hi):
    """the same, vectorised (np.argmax returns the first maximum = strict '>' in scan order)"""
    if cc is None:
        return 0, 0.0, False
    idx = range_indices(n, lo, hi)
    a = np.abs(cc[idx])
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    mi = int(idx[k]) if a[k] > 0 else 0
    u = a[np.isfinite(a) & (a >= 0)]
    tie = False
    if len(u) >= 2:
        top = np.partition(u, len(u) - 2)[-2:]
        tie = bool(top[1] > 0 and (top[1] - top[0]) <= TIE_GAP * top[1])
    return (mi if mi <= n // 2 else mi - n), float(cc[mi]), tie


def expect(oracle, ref, rows, ranges, Ls=()):
    """per (lo, hi) in ranges: (lag[M], mv[M], tie[M]) by the definition; per L in Ls the symmetric window's (tests/_window.py);
    plus the oracle's unwindowed (lag[M], mv[M]) and n.  One oracle transform per row."""
    rows = np.asarray(rows, dtype=np.float64)
    M = rows.shape[0]
    X, n = oracle.ref_spectrum(ref)
    out = {k: (np.zeros(M, dtype=np.int32), np.zeros(M), np.zeros(M, dtype=bool)) for k in list(ranges) + list(Ls)}
    glag, gmv = np.zeros(M, dtype=np.int32), np.zeros(M)
    for r in range(M):
        cc, lag, mv, _ = oracle.xcorr_with_x(X, rows[r], n)
        glag[r], gmv[r] = lag, mv
        for k in ranges:
            out[k][0][r], out[k][1][r], out[k][2][r] = ranged_fast(cc, n, k[0], k[1])
        for L in Ls:
            out[L][0][r], out[L][1][r], out[L][2][r] = W.windowed_fast(cc, n, L)
    return out, glag, gmv, n


# ---- the kernels' rules, restated in numpy
def table_argmax(cc, n, lo, hi):
    """the direct product's scan over a table whose row v is lag v - origin, origin = -lo: scan position pos <= hi is lag pos, later
    positions are the lags lo .. -1; strict '>', start (0, 0.0), the fallback reads row `origin`.  -> (lag, mv)"""
    lo, hi = clip(n, lo, hi)
    origin, Wd = -lo, hi - lo + 1
    table = np.array([cc[(v - origin) % n] for v in range(Wd)])
    best_abs, best_val, best_pos = 0.0, 0.0, -1
    for pos in range(Wd):
        v = (pos if pos <= hi else pos - 1 - hi + lo) + origin
        if abs(table[v]) > best_abs:
            best_abs, best_val, best_pos = abs(table[v]), table[v], pos
    if best_pos < 0:
        return 0, float(table[origin])
    return (best_pos if best_pos <= hi else best_pos - 1 - hi + lo), float(best_val)


def masked_argmax(cc, n, lo, hi):
    """the WIN kernels' rule with two independent bounds: every entry outside (i <= hi) | (i >= n + lo) replaced by +0.0, then the
    unrestricted maxAbsIndex, the cc[0] fallback, the lag unwrap.  -> (lag, mv)"""
    lo, hi = clip(n, lo, hi)
    i = np.arange(n)
    m = np.where((i <= hi) | (i >= n + lo), cc, 0.0)
    a = np.abs(m)
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    mi = k if a[k] > 0 else 0
    return (mi if mi <= n // 2 else mi - n), float(m[mi])


# ---- 1. the direct product
MFMA_NS = (64, 100, 480, 1025, 1100)
MFMA_RANGES = ((0, 0), (-1, 0), (0, 1), (-7, 0), (0, 7), (-15, 0), (-16, 0), (0, 63), (-63, 0), (-126, 0), (0, 126), (-3, 40),
               (-40, 3), (-100, 26))
PARITY_M = 35


def mfma_case(N):
    return W.make_case(N, PARITY_M, seed=3000 + N)


# ---- 2. the masked transform pass
MASKED_NS = (480, 1000, 1433, 3000, 4096)


def masked_ranges(n, f32):
    r = [(-200, 0), (0, 200), (-64, 300), (-1000, 70), (-256, 255), (-255, 256), (-257, 0), (0, n // 2), (-(n // 2 - 1), 0)]
    if f32:
        r += [(-7, 0), (0, 0)]
    return r


def masked_case(N, f32):
    ref, rows = W.make_case(N, PARITY_M, seed=4000 + N)
    if f32:
        with np.errstate(over="ignore"):
            rows = rows.astype(np.float32).astype(np.float64)
    return ref, rows


# ---- 3. edges: a code planted at the lags around both ends of a range and around zero
EDGE_CASES = ((4096, (-40, 3)), (4096, (-300, 100)), (512, (-5, 60)), (512, (-100, 200)))   # (N = n, range): MFMA, MASKED, MFMA, MASKED


def edge_case(N, lo, hi):
    """(ref, rows, n, planted lag of every row): the lags lo-1, lo, lo+1, -1, 0, 1, hi-1, hi, hi+1 (each once), rows shuffled"""
    n = LS.fft_len(N)
    assert n == N
    lags = sorted({lo - 1, lo, lo + 1, -1, 0, 1, hi - 1, hi, hi + 1})
    idx = np.array([l % n for l in lags], dtype=np.int64)
    p = N // 3
    shifts, planted = LS.shifts_for(idx, N, p, seed=N + hi)
    ref, rows, _ = LS.make_case(N, shifts, p, seed=N + hi)
    return ref, rows, n, LS.fold(planted, n)


# ---- 6. the Run form
RUN_NS = (480, 3000)
RUN_RANGES = ((-15, 0), (-300, 20))
RUN_M = 60


def run_case(N):
    return W.make_case(N, RUN_M, seed=6000 + N, scaled=False)


# the C++ program's series (host/muse_lag_range_test.cpp: host/muse_window_test.cpp's generator, 32-bit LCG, exact arithmetic)
CPP_N, CPP_M, CPP_RANGES = 1000, 240, ((-15, 0), (-100, 300))


def lcg_series(N, i):
    s = (12345 + 977 * i) & 0xFFFFFFFF

    def lcg():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        return s
    shift = 0 if i < 0 else (0 if i % 3 == 0 else int(lcg() % 241) - 120)
    amp = 1.0 + 2.0 * (((lcg() >> 8) / 16777216.0 - 0.5) + 0.5)
    y = np.zeros(N)
    for t in range(N):
        u = t - shift
        y[t] = (amp if N // 2 - 12 <= u < N // 2 + 12 else 0.0) + 0.5 * ((lcg() >> 8) / 16777216.0 - 0.5)
    return y


def cpp_case():
    return lcg_series(CPP_N, -1), np.stack([lcg_series(CPP_N, i) for i in range(CPP_M)])
