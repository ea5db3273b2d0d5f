"""Inputs and the numpy statement of the masking rule shared by tests/test_in_window_cpu.py and tests/test_gpu_in_window.py
(muse_batch_score_in_window).  Nothing here touches the code under test: the CPU test checks, on exactly these inputs, that the
oracle by itself flags no tie the GPU tests could hide behind."""
import numpy as np

import _lagsweep as LS
import _window as W

# ---- 1. parity: make_case rows (the eight specials included), an odd row count
PARITY_NS = (512, 480, 1024, 1000, 2048, 1433, 4096, 3000)
PARITY_M = 37


def parity_Ls(n):
    """the issue's windows, clipped below n / 2 (at n / 2 the window is every lag and the plain pass runs): edges inside a lane
    range, on a 256-index register block and on a wave boundary"""
    return sorted({min(L, n // 2 - 1) for L in (64, 65, 100, 255, 256, 257, n // 4, n // 2 - 1)})


def parity_case(N):
    return W.make_case(N, PARITY_M, seed=1000 + N)


# ---- 2. window edges from planted winners
EDGE_NS = (4096, 512)


def edge_Ls(n):
    return [L for L in (64, 255, 256, 1000) if L < n // 2]


def edge_case(N):
    """(ref, rows, n, {L: (row indices, planted lags)}): for every L six rows with the code planted at the lags -(L+1), -L, -(L-1),
    L-1, L, L+1, all in one group (rows shuffled with the seed, so pair partners carry unrelated lags)"""
    n = LS.fft_len(N)
    assert n == N
    lags = []
    for L in edge_Ls(n):
        lags += [-(L + 1), -L, -(L - 1), L - 1, L, L + 1]
    idx = np.array([l % n for l in lags], dtype=np.int64)
    p = N // 3
    shifts, planted = LS.shifts_for(idx, N, p, seed=N)
    ref, rows, _ = LS.make_case(N, shifts, p, seed=N)
    where = {}
    for L in edge_Ls(n):
        want = [l % n for l in (-(L + 1), -L, -(L - 1), L - 1, L, L + 1)]
        r = np.array([int(np.nonzero(planted == k)[0][0]) for k in want], dtype=np.int64)
        where[L] = (r, LS.fold(planted[r], n))
    return ref, rows, n, where


# ---- 4. the redo paths at n = 4096: every second row scaled by 1e30 (class "g" of tests/_seq.py): a dense hand-off list
REDO_N, REDO_M, REDO_L = 4096, 2100, 100


def redo_case():
    ref, rows = W.make_case(REDO_N, REDO_M, seed=77)
    rows[1::2] *= 1e30
    return ref, rows


# ---- 5. float32 storage: the rows as the group holds them
F32_NS = (480, 4096)
F32_LS = (7, 64, 300)
F32_M = 37


def f32_case(N):
    ref, rows = W.make_case(N, F32_M, seed=2000 + N)
    with np.errstate(over="ignore"):
        stored = rows.astype(np.float32).astype(np.float64)
    return ref, stored


# ---- 7. the Run form
RUN_N, RUN_M, RUN_G, RUN_L = 1000, 300, 7, 100


def run_case():
    return W.make_case(RUN_N, RUN_M, seed=555, scaled=False)


# ---- the masking rule of the WIN kernels, in numpy
def masked_argmax(cc, n, L):
    """(lag, mv): every entry of cc outside the window replaced by +0.0, then the UNRESTRICTED maxAbsIndex (xcorr.go:39-50: start
    (0, 0.0), strict '>', ascending index) over all n entries, the cc[0] fallback, the lag unwrap.  cc None: (nil, 0, 0)."""
    if cc is None:
        return 0, 0.0
    L = min(int(L), n // 2)
    lpos, lneg = L, (L - 1 if 2 * L == n else L)
    i = np.arange(n)
    m = np.where((i <= lpos) | (i >= n - lneg), cc, 0.0)        # a select: a NaN outside the window does not survive
    mi, mval = 0, 0.0
    for k in range(n):
        if abs(m[k]) > abs(mval):
            mval, mi = m[k], k
    return (mi if mi <= n // 2 else mi - n), float(m[mi])


def masked_argmax_fast(cc, n, L):
    if cc is None:
        return 0, 0.0
    L = min(int(L), n // 2)
    lpos, lneg = L, (L - 1 if 2 * L == n else L)
    i = np.arange(n)
    m = np.where((i <= lpos) | (i >= n - lneg), cc, 0.0)
    a = np.abs(m)
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    mi = k if a[k] > 0 else 0
    return (mi if mi <= n // 2 else mi - n), float(m[mi])
