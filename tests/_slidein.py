"""Inputs tests/test_gpu_slide_in_window.py and tests/test_slide_in_window_cpu.py share: the oracle case of the fused slide-and-score
kernel (1000 x 4096 float64, k = 16), built once per process."""
import functools

import numpy as np

ORACLE_M, ORACLE_N, ORACLE_K = 1000, 4096, 16


@functools.lru_cache(maxsize=1)
def oracle_case():
    """(ref, rows, tails, slid rows): pulse plus noise, as tests/test_gpu_parity.py builds its rows (without its constant row: every
    row has a score), and noise tails; read-only"""
    M, N, k = ORACLE_M, ORACLE_N, ORACLE_K
    rng = np.random.default_rng(4242)
    ref = rng.standard_normal(N)
    rows = rng.standard_normal((M, N))
    for i in range(0, M, 5):
        rows[i] += rng.uniform(-2, 2) * np.roll(ref, int(rng.integers(-N // 3, N // 3)))
    rows[2] = 2.5 * ref - 7  # perfect match
    rows[3] = -ref           # perfect anti-match
    tails = np.random.default_rng(4243).standard_normal((M, k))
    slid = np.concatenate([rows[:, k:], tails], 1)
    for a in (ref, rows, tails, slid):
        a.setflags(write=False)
    return ref, rows, tails, slid
