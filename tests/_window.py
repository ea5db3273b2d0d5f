"""The lag-window definition (include/muse_hip.h, muse_batch_set_lag_window) applied in numpy to the correlation slice the CPU
oracle returns: what the windowed tests expect.  Nothing here touches the code under test."""
import numpy as np

TIE_GAP = 1e-12


def window_indices(n, L):
    """the indices maxAbsIndex scans, in scan order: 0 .. L, then n-L .. n-1 (L clipped to n/2; at L = n/2 index n/2 comes
    twice, which a strict '>' never notices)"""
    L = min(int(L), n // 2)
    return np.concatenate([np.arange(0, L + 1), np.arange(n - L, n)]).astype(np.int64)


def windowed(cc, n, L):
    """(lag, mv, tie) of one series: maxAbsIndex (xcorr.go:39-50: start (0, 0.0), strict '>') over the window of cc; cc None =
    the reference's (nil, 0, 0).  tie: the two largest |cc| inside the window lie within TIE_GAP relative of each other."""
    if cc is None:
        return 0, 0.0, False
    idx = window_indices(n, L)
    mi, mval = 0, 0.0
    for i in idx:
        if abs(cc[i]) > abs(mval):      # (NaN compares false: never taken)
            mval, mi = cc[i], int(i)
    mv = cc[mi]
    a = np.abs(cc[np.unique(idx)])
    a = np.sort(a[np.isfinite(a)])[::-1]
    tie = bool(len(a) >= 2 and a[0] > 0 and (a[0] - a[1]) <= TIE_GAP * a[0])
    return (mi if mi <= n // 2 else mi - n), float(mv), tie


def windowed_fast(cc, n, L):
    """the same, vectorised (np.argmax returns the first maximum = strict '>' in scan order)"""
    if cc is None:
        return 0, 0.0, False
    idx = window_indices(n, L)
    sub = cc[idx]
    a = np.abs(sub)
    a = np.where(np.isnan(a), -1.0, a)
    k = int(np.argmax(a))
    mi = int(idx[k]) if a[k] > 0 else 0
    mv = float(cc[mi])
    u = np.abs(cc[np.unique(idx)])
    u = u[np.isfinite(u)]
    tie = False
    if len(u) >= 2:
        top = np.partition(u, len(u) - 2)[-2:]
        tie = bool(top[1] > 0 and (top[1] - top[0]) <= TIE_GAP * top[1])
    return (mi if mi <= n // 2 else mi - n), mv, tie


def expect(oracle, ref, rows, Ls):
    """per L in Ls: (lag[M], mv[M], tie[M]) by the definition, plus the oracle's unwindowed (lag[M], mv[M]); one oracle
    transform per row"""
    rows = np.asarray(rows, dtype=np.float64)
    M, N = rows.shape
    X, n = oracle.ref_spectrum(ref)
    out = {L: (np.zeros(M, dtype=np.int32), np.zeros(M), np.zeros(M, dtype=bool)) for L in Ls}
    glag, gmv = np.zeros(M, dtype=np.int32), np.zeros(M)
    for r in range(M):
        cc, lag, mv, _ = oracle.xcorr_with_x(X, rows[r], n)
        glag[r], gmv[r] = lag, mv
        for L in Ls:
            l, v, t = windowed_fast(cc, n, L)
            out[L][0][r], out[L][1][r], out[L][2][r] = l, v, t
    return out, glag, gmv, n


SPECIALS = 8   # rows 1 .. 8 of make_case (from M = 9 on)


def make_case(N, M, seed, scaled=True):
    """(ref, rows): rect + noise.  Row r >= 9 is the reference moved by a shift of one of three classes (r % 3) plus continuous
    noise: 0 -- not moved (the global winner is lag 0: inside every window); 1 -- moved by more than 64 samples where the
    length allows it (the global winner lies outside every window up to 63, so a build that filters today's result fails);
    2 -- moved by up to 70 samples either way.  Rows 1 .. 8 (when M > 8): an exact copy of the reference, a negated copy, a
    constant row, a NaN row, an Inf row, a row with mean 1e6 and sigma 1, rows scaled by 1e-100 and by 1e100 (copies of row 0:
    their scores equal row 0's to rounding, so the Run tests, which compare the ORDER of the selected series, leave them out:
    scaled=False)."""
    rng = np.random.default_rng(seed)
    w = max(1, N // 20)
    ref = np.zeros(N)
    ref[N // 2 - w // 2:N // 2 - w // 2 + w] = 2.0
    ref += 0.1 * rng.standard_normal(N)
    rows = np.zeros((M, N))
    far_lo, far_hi = (64, max(65, min(N // 4, 500))) if N >= 480 else (0, max(1, N // 2))
    for r in range(M):
        cls = r % 3
        if cls == 0:
            shift, noise = 0, 0.02
        elif cls == 1:
            shift, noise = int(rng.integers(far_lo, far_hi + 1)) * (1 if rng.random() < 0.5 else -1), 0.3
        else:
            shift, noise = int(rng.integers(-70, 71)) if N >= 480 else int(rng.integers(-(N // 2), N // 2 + 1)), 0.3
        rows[r] = (0.5 + rng.random()) * np.roll(ref, shift) + noise * rng.standard_normal(N) + rng.standard_normal()
    if M > SPECIALS:
        rows[1] = ref
        rows[2] = -ref
        rows[3] = 3.25
        rows[4] = rows[0]
        rows[4, N // 3] = np.nan
        rows[5] = rows[0]
        rows[5, N // 2] = np.inf
        z = rng.standard_normal(N)
        rows[6] = 1e6 + (z - z.mean()) / z.std()
        if scaled:
            rows[7] = 1e-100 * rows[0]
            rows[8] = 1e100 * rows[0]
    return ref, rows


def plain_rows(M):
    """the rows of make_case that are continuous-noise rows (not planted copies, constants, NaN / Inf)"""
    keep = np.ones(M, dtype=bool)
    if M > SPECIALS:
        keep[1:6] = False
    return keep
