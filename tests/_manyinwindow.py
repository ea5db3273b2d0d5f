"""Inputs shared by tests/test_many_in_window_cpu.py and tests/test_gpu_many_in_window.py (muse_batch_score_many_in_window): the
cases of tests/_inwindow.py with several references, each np.roll(ref0, s) -- a roll by s moves every global lag by +s, so each
reference sees different rows inside and outside the window, and a kernel that applies reference 0's spectrum, table or result
buffer to all references fails on almost every row.  Nothing here touches the code under test: the CPU test checks, on exactly
these inputs, that the oracle by itself flags no tie the GPU tests could hide behind."""
import numpy as np

import _inwindow as IW
import _lagsweep as LS
import _window as W

# ---- 1. parity: IW.parity_case rows (37 rows, 8 specials, an odd count), four references
PARITY_ROLLS = (0, 45, -90, 170)


def parity_Ls(n):
    """the issue's windows, clipped below n / 2 as IW.parity_Ls clips"""
    return sorted({min(L, n // 2 - 1) for L in (64, 100, 256, 257, n // 2 - 1)})


# ---- 2. window edges from planted winners: IW.edge_case, three references
EDGE_ROLLS = (0, 1, -1)

# ---- 3. workgroups that loop, one case per kernel family: at least three iterations per resident workgroup on 256 CUs, an odd M
LOOP_CASES = ((4096, 3073), (512, 24577), (1024, 12289), (2048, 6145))
LOOP_L = 100
ROLLS3 = (0, 45, -90)   # (cases 3, 4, 5, 8)


def loop_case(N, M):
    return W.make_case(N, M, seed=7000 + N)


# ---- 5. float32 storage: one masked pass at FFT length 4096, single masked passes below
F32_ONE_PASS_NS = (4096, 3000)
F32_EACH_N = 480

# ---- 6. identities
IDENT_NS = (1024, 4096)
IDENT_M = 101


def ident_case(N):
    return W.make_case(N, IDENT_M, seed=9 + N)


def refs_of(ref0, rolls):
    return [np.roll(ref0, s) for s in rolls]


# ---- 8. the C++ program (host/muse_many_in_window_test.cpp), bit for bit (32-bit LCG, exact arithmetic)
CPP_N, CPP_M, CPP_L, CPP_R = 1000, 240, 100, 3


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
    refs = [cpp_series(CPP_N, -1 - r) for r in range(CPP_R)]
    return refs, rows


# ---- the table of include/muse_hip.h (muse_batch_score_many_in_window), restated
UNSUPPORTED, PLAIN, MFMA, MASKED, MASKED_EACH = 0, 1, 2, 3, 4


def plan_table(N, f32, max_lag, R):
    n = LS.fft_len(N)
    L = min(max_lag, n // 2)
    if L == n // 2:
        return PLAIN
    if not f32 and L <= 63 and N <= 65536:
        return MFMA
    if n not in (512, 1024, 2048, 4096):
        return UNSUPPORTED
    one_pass = R >= 2 and (n == 4096 or not f32)
    return MASKED if one_pass else MASKED_EACH


# ---- the many-references n = 4096 kernel's form of the mask (r16_device.h, mask_window_quot): register m of thread `base` holds index
# base + step m and stays iff m <= floor((lpos - base) / step) or m >= ceil((nl - base) / step)
def quotient_rule(n, step, L):
    """bool[n]: the indices the quotient form keeps"""
    L = min(int(L), n // 2)
    lpos, nl = L, n - (L - 1 if 2 * L == n else L)
    sh = step.bit_length() - 1
    base = np.arange(step, dtype=np.int64)[:, None]
    m = np.arange(n // step, dtype=np.int64)[None, :]
    a = (lpos - base) >> sh
    b = (nl - base + step - 1) >> sh
    keep = (m <= a) | (m >= b)
    out = np.zeros(n, dtype=bool)
    out[(base + step * m).ravel()] = keep.ravel()
    return out
