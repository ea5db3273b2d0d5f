"""Inputs shared by tests/test_many_lag_range_cpu.py and tests/test_gpu_many_lag_range.py (muse_batch_score_many_in_lag_range):
the rows of W.make_case(N, M, seed=N), twelve references (the six recipes of tests/test_gpu_lag_window_many.py with two seeds), the
ranges, and the expectations -- per reference and row tests/_lagrange.py's definition on the oracle's correlation.  Nothing here
touches the code under test: the CPU test checks, on exactly these inputs, that the oracle by itself flags no tie on a
continuous-noise row, so the GPU tests have no tie to hide behind."""
import functools

import numpy as np

import _lagrange as LR
import _lagsweep as LS
import _window as W

# ---- 1. the direct product: ranges of W = 2 .. 48 rows are packed, wider ones take one launch per reference
PACKED_RANGES = ((-1, 0), (0, 1), (-3, 0), (-7, 0), (0, 7), (-15, 0), (0, 15), (-3, 12), (-31, 0), (-40, 3), (-47, 0))
SINGLE_RANGES = ((-48, 0), (0, 63), (-100, 26))
RANGES = PACKED_RANGES + SINGLE_RANGES
WIDE_RANGES = ((-200, 0), (0, 200), (-64, 300), (-1000, 70))   # N = 100 only: FFT length 128 clips them to at most 127 lags
PARITY_NS = (100, 480, 1024, 1433, 4096, 5000)
PARITY_MS = (200, 1, 15, 17)
PARITY_RS = (1, 2, 3, 6)
CPU_RANGES_SYM = (63,)


def full_M(N):
    return 1001 if N < 4096 else 200


def make_refs(ref, N, seed):
    """the six recipes of tests/test_gpu_lag_window_many.py::make_refs (the random ones drawn in list order)"""
    rng = np.random.default_rng(seed)
    return [ref.copy(),
            np.roll(ref, 5) + 0.05 * rng.standard_normal(N),
            -np.roll(ref, -9) + 0.05 * rng.standard_normal(N),
            ref[::-1].copy(),
            rng.standard_normal(N),
            np.cumsum(rng.standard_normal(N))]


def ranges_of(N):
    return RANGES + (WIDE_RANGES if N == 100 else ())


@functools.lru_cache(maxsize=None)
def case(N, M=None):
    """(ref, rows, the twelve references)"""
    ref, rows = W.make_case(N, full_M(N) if M is None else M, seed=N)
    return ref, rows, make_refs(ref, N, 1000 + N) + make_refs(ref, N, 2000 + N)


def third_refs(ref, N):
    """references 13 .. 16 of the R = 16 case: the first four recipes with a third seed"""
    return make_refs(ref, N, 3000 + N)[:4]


def expectations(oracle, refs, rows, ranges, Ls=()):
    """per reference: ({(lo, hi): (lag, mv, tie)}, global lag, global mv), and n"""
    out, n = [], None
    for rf in refs:
        exp, glag, gmv, n = LR.expect(oracle, rf, rows, ranges, Ls=Ls)
        out.append((exp, glag, gmv))
    return out, n


# ---- 2. the masked pass: LR.masked_case rows, the six recipes with seed 1000 + N, four of them used
MASKED_R = 4


def masked_case(N, f32):
    ref, rows = LR.masked_case(N, f32)
    return ref, rows, make_refs(ref, N, 1000 + N)


# ---- 3. edges
EDGE_CASES = ((4096, (-40, 3)), (512, (-5, 60)))
EDGE_ROLLS = (0, 1, -1)   # a roll of the reference by s moves every lag by +s

# ---- 4. Runs
RUN_NS = LR.RUN_NS
RUN_RANGES = LR.RUN_RANGES
RUN_M = LR.RUN_M
RUN_R = 3


def run_case(N):
    ref, rows = LR.run_case(N)
    return ref, rows, make_refs(ref, N, 1000 + N)[:RUN_R]


# the C++ program's series (host/muse_many_lag_range_test.cpp: host/muse_window_test.cpp's generator, 32-bit LCG, exact arithmetic)
CPP_N, CPP_M, CPP_R, CPP_RANGES = 1000, 240, 3, ((-15, 0), (-300, 20))


def cpp_series(N, i):
    s = (12345 + 977 * i) & 0xFFFFFFFF

    def lcg():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        return s
    shift = 45 * (-i - 1) if i < 0 else (0 if i % 3 == 0 else int(lcg() % 241) - 120)
    amp = 1.0 + 2.0 * (((lcg() >> 8) / 16777216.0 - 0.5) + 0.5)
    y = np.zeros(N)
    for t in range(N):
        u = t - shift
        y[t] = (amp if N // 2 - 12 <= u < N // 2 + 12 else 0.0) + 0.5 * ((lcg() >> 8) / 16777216.0 - 0.5)
    return y


def cpp_case():
    rows = np.stack([cpp_series(CPP_N, i) for i in range(CPP_M)])
    return [cpp_series(CPP_N, -1 - r) for r in range(CPP_R)], rows


# ---- the table of include/muse_hip.h (muse_batch_score_many_in_lag_range), restated
UNSUPPORTED, PLAIN, MFMA, MASKED, MASKED_EACH = 0, 1, 2, 3, 4


def plan_table(N, f32, lo, hi, R):
    n = LS.fft_len(N)
    lo, hi = LR.clip(n, lo, hi)
    if hi == n // 2 and lo == -(n // 2 - 1):
        return PLAIN
    if not f32 and hi - lo + 1 <= 127 and n <= 65536:
        return MFMA
    if n not in (512, 1024, 2048, 4096):
        return UNSUPPORTED
    return MASKED if R >= 2 and (n == 4096 or not f32) else MASKED_EACH


# ---- the planner of xcorr_window_many.hip in the rows W of a reference's table, restated from its constants
MAX_TILES, PACK_MAX_ROWS, IMG_DOUBLES, KC = 8, 48, 4608, 1024


def plan_img(Wd, kc):
    img = kc + Wd - 1
    while img % 32 != (Wd + 2) % 32:
        img += 1
    return img


def plan_max_refs(Wd):
    if Wd > PACK_MAX_ROWS:
        return 1
    return max(1, min(16 * MAX_TILES // Wd, IMG_DOUBLES // plan_img(Wd, 256)))


def plan_kc(Wd, refs):
    kc = KC
    while kc > 256 and refs * plan_img(Wd, kc) > IMG_DOUBLES:
        kc //= 2
    return kc


def plan_rows(R, Wd):
    """[(references, tiles) per launch]"""
    per = plan_max_refs(Wd)
    return [(min(per, R - r0), (min(per, R - r0) * Wd + 15) // 16) for r0 in range(0, R, per)]


def launch_lds_bytes(refs, Wd):
    """the dynamic LDS of a packed launch (launch_window_many): image / tile region, the waves' statistics, the scan candidates"""
    img = plan_img(Wd, plan_kc(Wd, refs))
    tiles = (refs * Wd + 15) // 16
    parts = max(1, 16 // refs)
    return 8 * (max(refs * img, tiles * 256) + 128 + refs * parts * 16 * 3)


# the issue's table: (W, R) -> [(references, tiles)]; a launch of one reference is the single-reference kernel's
PLAN_TABLE = {(2, 6): [(6, 1)], (8, 8): [(8, 4)], (8, 16): [(16, 8)], (16, 4): [(4, 4)], (16, 12): [(8, 8), (4, 4)],
              (32, 2): [(2, 4)], (32, 8): [(4, 8), (4, 8)], (48, 2): [(2, 6)], (49, 2): [(1, 4), (1, 4)]}
