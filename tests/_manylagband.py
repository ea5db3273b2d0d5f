"""Inputs shared by tests/test_many_lag_band_cpu.py and tests/test_gpu_many_lag_band.py (muse_batch_score_many_in_lag_band): the rows
and the twelve references of tests/_manylagrange.py's case(N, 35), the bands, and the expectations -- per reference and row
tests/_lagband.py's definition on the oracle's correlation.  Nothing here touches the code under test: the CPU test checks, on
exactly these inputs, that the oracle by itself flags no tie, so the GPU tests may demand exact lags on every row."""
import _lagband as LB
import _lagsweep as LS
import _manylagrange as MLR

SIGNS = LB.SIGNS
M = 35

# W = 1, 2, 7, 8, 16, 17, 32, 48 (the packing maximum), 49 (one reference per launch) and 127, bands far from zero, two that hold lag 0
BANDS = ((1, 1), (-1, -1), (1, 2), (1, 7), (-7, -1), (1, 8), (-8, -1), (1, 16), (-16, -1), (2, 18), (5, 36), (-32, -1), (1, 48), (-48, -1),
         (20, 40), (49, 97), (1, 127), (-127, -1), (100, 226), (200, 230), (-255, -200), (-3, 12), (-7, 0))
NARROW_BANDS = ((1, 1), (1, 2))                      # R = 16 and 17: sixteen references' rows in one tile (W = 1), in two (W = 2)
CUT_BANDS = ((1, 16), (-32, -1))                     # R = 12: two launches (8 + 4), three launches of four
DIRECT_NS = (100, 480, 1025, 1100)
DIRECT_RS = (1, 2, 3, 6)
SMALL_MS = (1, 15, 17)
SMALL_M_N = 480
TIE_RS = 6                                            # the CPU test's first check: the first six references

# the masked pass
MASKED_NS = LB.MASKED_NS
MASKED_RS = (2, 4)


def case(N, m=M):
    """(ref, rows, the twelve references)"""
    return MLR.case(N, m)


def masked_case(N, f32):
    """(ref, rows, six references; four are used)"""
    return MLR.masked_case(N, f32)


def expectations(oracle, refs, rows, bands, signs=SIGNS):
    """per reference {(lo, hi, sign): (lag, mv, tie)} (the bands that are not empty at this length), and n"""
    out, n = [], None
    for rf in refs:
        exp, n = LB.expect(oracle, rf, rows, bands, signs)
        out.append(exp)
    return out, n


# ---- the dispatch of include/muse_hip.h (muse_batch_score_many_in_lag_band), restated
UNSUPPORTED, PLAIN, MFMA, MASKED, MASKED_EACH = 0, 1, 2, 3, 4


def plan_table(N, f32, lo, hi, sign, R):
    n = LS.fft_len(N)
    c = LB.clip(n, lo, hi)
    assert c is not None
    lo, hi = c
    if sign == 0 and lo <= 0 <= hi:
        return MLR.plan_table(N, f32, lo, hi, R)
    masked_len = n in (512, 1024, 2048, 4096)
    every_lag = hi == n // 2 and lo == -(n // 2 - 1)
    if every_lag:                                     # (under a sign: the masked pass with both bounds at their widest)
        p = MASKED if masked_len else UNSUPPORTED
    elif not f32 and hi - lo + 1 <= 127 and n <= 65536:
        p = MFMA
    else:
        p = MASKED if masked_len else UNSUPPORTED
    if p != MASKED:
        return p
    return MASKED if R >= 2 and (n == 4096 or not f32) else MASKED_EACH
