"""The inputs tests/test_rows_lag_range_cpu.py and tests/test_gpu_rows_lag_range.py share (Muse.Run inside a lag range:
muse_batch_run_rows_in_lag_range and its siblings), the dispatch table and the panel kernels' merge rule restated in Python.  Nothing
here touches the code under test: the CPU test checks, on exactly these inputs, that the oracle by itself flags no tie inside any
tested range, so the GPU tests compare the lag of EVERY row."""
import numpy as np

import _lagrange as LR

TIE_GAP = LR.TIE_GAP
WIN_KC = 1024             # samples per chunk (xcorr_kernels.h)
PANEL = 128               # table rows of a panel (WIN_PANEL_ROWS)
RANGE_MAX = 2048          # MUSE_RUN_ROWS_LAG_RANGE_MAX
FULL_SPLIT, MIN_CHUNKS = 16, 2   # WIN_ROWS_FULL_SPLIT, WIN_ROWS_MIN_CHUNKS
UNSUPPORTED, PLAIN, WINDOW, SPLIT, PANELS = 0, 1, 2, 3, 4   # MUSE_ROWS_LAG_RANGE_* (muse_hip_test.h)
SPECIALS = 4              # the rows make_case appends to its M continuous-noise rows


def fft_len(N):
    n = 1
    while n < N:
        n *= 2
    return n


# ---- the dispatch table of include/muse_hip.h, restated
PANEL_BALANCE = 10        # WIN_PANEL_BALANCE


def rows_plan_S(M, N, cus):
    """window_rows_plan's rule (the windowed Muse.Run)"""
    wgs = (M + 15) // 16
    chunks = (N + WIN_KC - 1) // WIN_KC
    if wgs >= cus:
        return 1
    return max(1, min(cus // wgs, min(chunks, max(FULL_SPLIT, chunks // MIN_CHUNKS))))


def panels_plan_S(M, N, cus, panels):
    """window_panels_plan's rule: sqrt(PANEL_BALANCE chunks / panels) rounded -- the largest S <= chunks with (2 S - 1)^2 panels <=
    4 PANEL_BALANCE chunks -- at most CUs / (blocks x panels); 1 whenever blocks x panels >= CUs"""
    wgs = (M + 15) // 16 * panels
    chunks = (N + WIN_KC - 1) // WIN_KC
    if wgs >= cus:
        return 1
    S = max(s for s in range(1, chunks + 1) if s == 1 or (2 * s - 1) ** 2 * panels <= 4 * PANEL_BALANCE * chunks)
    return max(1, min(S, cus // wgs))


def plan(M, N, cus, lo, hi):
    """(path, panels, S) of the table: every lag -> PLAIN; W <= 127 -> the window kernels (SPLIT iff the rows planner says S > 1);
    W <= 2048 -> PANELS with ceil(W / 128) panels; series longer than 65536 samples or more lags -> UNSUPPORTED"""
    n = fft_len(N)
    lo, hi = LR.clip(n, lo, hi)
    W = hi - lo + 1
    if hi == n // 2 and lo == -(n // 2 - 1):
        return PLAIN, 0, 0
    if n > 65536 or W > RANGE_MAX:
        return UNSUPPORTED, 0, 0
    if W <= 127:
        S = rows_plan_S(M, N, cus)
        return (SPLIT if S > 1 else WINDOW), 1, S
    panels = (W + PANEL - 1) // PANEL
    return PANELS, panels, panels_plan_S(M, N, cus, panels)


PLAN_NS = (2, 200, 300, 2500, 4096, 5000, 40000, 65536, 70000)
PLAN_MS = (1, 17, 100, 5000)
PLAN_RANGES = ((-63, 63), (-7, 7), (-126, 0), (-127, 0), (-128, 0), (-100, 155), (0, 2047), (0, 2048), (-5000, 5000), (0, 0), (-7, 0),
               (0, 63), (-1024, 1023), (-1023, 1024), (-1, 1 << 30), (-(1 << 30), 1 << 30), (-(1 << 30), 0), (-32767, 32768), (-300, 20))


# ---- the panel kernels' merge rule, restated
def panel_merge(cc, n, lo, hi):
    """window_panels_finish in numpy: the table's rows v = 0 .. W - 1 (lag v + lo) visited in TABLE order, panel after panel; a
    candidate replaces the best iff |val| > best.abs, or |val| == best.abs and pos < best.pos, with pos = lag >= 0 ? lag :
    hi + 1 + (lag - lo); NaN never wins; nothing above zero leaves (0, cc[0]).  -> (lag, mv)"""
    lo, hi = LR.clip(n, lo, hi)
    W = hi - lo + 1
    best_abs, best_val, best_pos = 0.0, 0.0, -1
    for z in range((W + PANEL - 1) // PANEL):
        for v in range(z * PANEL, min(W, (z + 1) * PANEL)):
            lag = v + lo
            val = cc[lag % n]
            pos = lag if lag >= 0 else hi + 1 + (lag - lo)
            a = abs(val)
            if a > best_abs or (a == best_abs and pos < best_pos):
                best_abs, best_val, best_pos = a, val, pos
    if best_pos < 0:
        return 0, float(cc[0])
    return (best_pos if best_pos <= hi else best_pos - 1 - hi + lo), float(best_val)


# ---- the inputs of the GPU tests
def make_case(N, M, seed, span=None):
    """(ref, rows): a rectangular pulse plus noise, and M + SPECIALS rows -- M continuous-noise copies of the reference moved by a
    shift drawn from -span .. span (default: a quarter of the length, at most 2200: winners inside and outside every tested range, on
    both sides), then a NaN row, a constant row, a quiet row (two opposite unit impulses: sum d == 0 exactly, the correlation
    inside a range is the difference of two reference samples) and a row that starts 50 sigma off (d = y - y[0]: every other sample
    is 50 sigma away from the shift point)."""
    rng = np.random.default_rng(seed)
    w = max(1, N // 20)
    ref = np.zeros(N)
    ref[N // 2 - w // 2:N // 2 - w // 2 + w] = 2.0
    ref += 0.1 * rng.standard_normal(N)
    if span is None:
        span = min(N // 4, 2200)
    rows = np.zeros((M + SPECIALS, N))
    for r in range(M + SPECIALS):
        shift = 0 if r % 5 == 0 else int(rng.integers(-span, span + 1))
        rows[r] = (0.5 + rng.random()) * np.roll(ref, shift) + 0.3 * rng.standard_normal(N) + rng.standard_normal()
    rows[M, N // 3] = np.nan
    rows[M + 1] = 3.25
    rows[M + 2] = 0.0
    rows[M + 2, N // 5] = 1.0
    rows[M + 2, N // 5 + 2 + N // 7] = -1.0
    rows[M + 3, 0] += 50.0 * rows[M + 3].std()
    return ref, rows


def plain_rows(M):
    """the rows of make_case whose score is a number above zero (not the NaN row, not the constant row)"""
    keep = np.ones(M + SPECIALS, dtype=bool)
    keep[M:M + 2] = False
    return keep


# (N, M, ranges, forced slice counts: 0 = the planner): the parity cases of the scores hook
PARITY = (
    (300, 17, ((-128, 0),), (0,)),                               # two panels, the second one row; a partial last block; one chunk
    (200, 17, ((-127, 100),), (0,)),                             # n = 256: a length with no masked pass
    (2500, 5, ((-100, 155), (-300, 20), (0, 2047)), (1, 2, 3)),
    (4999, 5, ((-200, 50),), (0, 1)),                            # odd: the narrow mapping
    (5000, 5, ((-1000, 1047),), (0,)),
    (40000, 3, ((-500, 500),), (0, 2)),
)
NARROW_NS = (2500, 40000)
NARROW_M = 5
NARROW_RANGES = ((-7, 0), (0, 63), (-126, 0))
NARROW_L = 63
ACROSS = (2500, 40, (-200, 50), (-100, 26))                      # the same bits across panels: N, M, the wide range, the narrow one
WINNER = (2500, 30, ((-200, 50), (-7, 0)))
CACHE = (2500, 12, ((-200, 50), (-50, 200), (-7, 0)))
CALLERS = (2500, 12, ((-200, 50), (-50, 200), (-7, 0), (-300, 20)))
GENERAL = (4096, 4097, (-200, 50), 48)                           # N, M (4097 x 4096 > 2^24 elements: the smallest), the range, rows compared
MIRROR = (2500, 3, 6, ((-15, 0), (-300, 20)), 400)               # N, label groups, series per group, ranges, Results.MaxLag


def parity_seed(N):
    return 7000 + N


_CASES = {}


def case(oracle, key, N, M, seed, ranges, Ls=()):
    """(ref, rows, exp, n): exp[(lo, hi)] / exp[L] = (lag, mv, tie) by the definition on the oracle's cc; computed once, never changed"""
    if key not in _CASES:
        ref, rows = make_case(N, M, seed)
        exp, _, _, n = LR.expect(oracle, ref, rows, tuple(ranges), tuple(Ls))
        for a in (ref, rows):
            a.setflags(write=False)
        _CASES[key] = (ref, rows, exp, n)
    return _CASES[key]


def parity_case(oracle, N):
    for n_, M, ranges, _ in PARITY:
        if n_ == N:
            return case(oracle, ("parity", N), N, M, parity_seed(N), ranges)
    raise KeyError(N)


def narrow_case(oracle, N):
    return case(oracle, ("narrow", N), N, NARROW_M, 7100 + N, NARROW_RANGES, (NARROW_L,))


def across_case(oracle):
    N, M, wide, narrow = ACROSS
    return case(oracle, "across", N, M, 7200, (wide, narrow))


def winner_case(oracle):
    N, M, ranges = WINNER
    return case(oracle, "winner", N, M, 7300, ranges)


def cache_case(oracle, which):
    N, M, ranges = CACHE
    return case(oracle, ("cache", which), N, M, 7400 + which, ranges)


def callers_case(oracle):
    N, M, ranges = CALLERS
    return case(oracle, "callers", N, M, 7500, ranges)


def general_case():
    """(ref, rows, pick): make_case without its NaN row and its constant row; pick: the rows the test compares with the oracle"""
    N, M, _, K = GENERAL
    ref, rows = make_case(N, M - 2, 7600, span=300)          # (the NaN row and the constant row go: M rows stay)
    keep = plain_rows(M - 2)
    rows = np.ascontiguousarray(rows[keep])
    pick = np.sort(np.random.default_rng(9).choice(rows.shape[0], K, replace=False))
    return ref, rows, pick


# the exact-zero case: a reference that is exactly zero outside two opposite pulses (mean exactly 0), and a row of two opposite unit
# impulses far from them -- inside the range the direct product is a sum of exact zeros, so the definition's "a window of zeros
# gives (0, cc[0])" applies; the transform oracle's cc there is rounding noise, which the CPU test bounds
ZEROS = (2500, (-200, 50))


def zeros_case():
    N, _ = ZEROS
    rng = np.random.default_rng(7700)
    ref = np.zeros(N)
    ref[1000:1040] = 2.0
    ref[1100:1140] = -2.0
    rows = np.zeros((6, N))
    for r in range(6):
        rows[r] = (0.5 + rng.random()) * np.roll(ref, int(rng.integers(-180, 40))) + 0.3 * rng.standard_normal(N)
    rows[5] = 0.0
    rows[5, 100] = 1.0          # ref[100 + lag] and ref[2300 + lag] are zero for every lag in -200 .. 50
    rows[5, 2300] = -1.0
    return ref, rows, 5


# the C++ program's series (host/muse_rows_lag_range_test.cpp: 32-bit LCG, exact arithmetic)
def mirror_series():
    N, G, K, _, _ = MIRROR
    return LR.lcg_series(N, -1), np.stack([LR.lcg_series(N, i) for i in range(G * K)])
