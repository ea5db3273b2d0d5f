"""The planted-lag construction of tests/_lagsweep.py, checked on the CPU oracle alone (no GPU): what tests/test_gpu_lag_sweep.py
takes for granted.

For every length below, over every output index of the small transforms and a structured index set of the large ones:

  * the oracle returns the PLANTED index for every row -- a code moved by +s in the row gives lag -s, folded at n / 2; the sign
    convention is asserted here once, so the GPU tests take "planted" as expected without calling the oracle;
  * no ties: every row's top-two gap is at least 0.1, so "lags exact, no tie excused" is a fair condition for a kernel;
  * the fully swept lengths cover all n output indices between their references;
  * the oracle's own error against the long-double sum at the winning index, E_o(n) = max |oracle mv - ld_score_at|, stays inside
    K_ORACLE * log2(n) * 2^-53.  K_ORACLE (tests/_lagsweep.py) is the smallest integer for which that held at every length here when
    it was measured (see MEASURED below); the GPU tests' score bound is 4 x that, so it rests on a checked property of the reference.

This also takes the oracle's long-double check (tests/test_oracle_golden.py::test_oracle_exactness_vs_long_double_direct, N <= 1000:
the O(n^2) direct correlation) to n = 2^20, at the indices that matter."""
import math

import numpy as np
import pytest

import _lagsweep as L

FULL = [512, 480, 1000, 4096, 3000]
# (N, budget of index_set): at most 16 rows above 65536 (the oracle takes ~1 s per row at n = 2^20)
SPARSE = [(65536, 48), (40000, 48), (131072, 16), (100000, 16), (1048576, 16), (1000003, 16)]

# E_o(n) / (log2(n) 2^-53) measured with this construction (x86-64, 80-bit long double, gcc -O2 oracle):
MEASURED = {512: 1.72, 480: 1.99, 1000: 3.50, 4096: 4.40, 3000: 3.92, 65536: 9.20, 40000: 5.21, 131072: 5.81, 100000: 5.90,
            1048576: 12.55, 1000003: 7.69}            # -> K_ORACLE = 13


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "ld_score_at needs an extended long double to referee float64 kernels"


def _sweep(oracle, N, budget):
    n = L.fft_len(N)
    covered, worst, min_gap, rows_total = set(), 0.0, np.inf, 0
    for ref, rows, ks in L.sweep_cases(N, budget, seed=N):
        lag, mv, gap = oracle.batch_scores(ref, rows, nthreads=4)
        assert n == oracle.next_pow2(N)
        # planted index and sign convention
        assert np.array_equal(lag, L.fold(ks, n)), "rows %s" % np.nonzero(lag != L.fold(ks, n))[0][:10]
        assert np.all(lag[ks > n // 2] < 0) and np.all(lag[ks <= n // 2] == ks[ks <= n // 2])
        # no ties, and no row left out: none is constant
        assert np.all(mv != 0.0) and float(gap.min()) >= 0.1, float(gap.min())
        assert float(np.abs(mv).min()) > 0.85              # the 1 / sqrt(N) noise keeps the planted score high at every length
        ld = L.ld_scores(ref, rows, n, ks)
        worst = max(worst, float(np.max(np.abs(mv - ld))))
        min_gap = min(min_gap, float(gap.min()))
        covered |= set(ks.tolist())
        rows_total += len(ks)
    ratio = worst / (math.log2(n) * L.U)
    print("N = %d -> n = %d: %d rows, %d indices, smallest gap %.2f, E_o = %.2e = %.2f log2(n) 2^-53"
          % (N, n, rows_total, len(covered), min_gap, worst, ratio))
    assert ratio <= L.K_ORACLE, "the oracle's error left K_ORACLE: %.2f" % ratio
    return covered, n


@pytest.mark.parametrize("N", FULL)
def test_full_sweep_plants_every_index(oracle, N):
    covered, n = _sweep(oracle, N, None)
    assert covered == set(range(n))                        # union coverage: head and tail references together when N < n


@pytest.mark.parametrize("N,budget", SPARSE)
def test_index_set_sweep(oracle, N, budget):
    covered, n = _sweep(oracle, N, budget)
    must = {0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1}
    assert must <= covered and len(covered) <= budget


def test_head_code_off_the_first_sample(oracle):
    """the third reference of the GPU file's padded lengths above 65536: the code at p = 1 plants the head reference's indices,
    untied, and neither it nor (but for the one row whose code lies on sample 0) its rows start on an outlier"""
    N = 1000003                              # (the seed of the GPU file's case: its head code starts on a sample of ~100 sigma)
    n = L.fft_len(N)
    cases = L.sweep_cases(N, 16, seed=N, head_off_first=True)
    assert len(cases) == 3
    ref, rows, ks = cases[2]
    assert set(ks.tolist()) <= set(cases[0][2].tolist()) and len(ks) >= len(cases[0][2]) - 1
    lag, mv, gap = oracle.batch_scores(ref, rows, nthreads=4)
    assert np.array_equal(lag, L.fold(ks, n)) and float(gap.min()) >= 0.1
    assert float(np.max(np.abs(mv - L.ld_scores(ref, rows, n, ks)))) <= L.K_ORACLE * math.log2(n) * L.U
    assert L.first_sample_level(ref) < L.LEVEL_MAX and L.first_sample_level(cases[0][0]) > L.LEVEL_MAX
    assert int(L.row_bounds(n, rows, ref)[1].sum()) <= 1 and bool(L.row_bounds(n, cases[0][1], cases[0][0])[1].all())
    assert not L.row_bounds(n, cases[0][1], cases[0][0], shifted=False)[1].any()


def test_three_references_share_one_group(oracle):
    """the many-references case of the GPU file: one row set, the code at the head, at the tail and in the middle of three
    references; each reference's winner is its own planted index, untied"""
    for N in (1024, 3000):
        for refs, rows, ks in [L.many_refs_case(N, seed=5 * N)]:
            n = L.fft_len(N)
            for ref, k in zip(refs, ks):
                lag, mv, gap = oracle.batch_scores(ref, rows, nthreads=4)
                assert np.array_equal(lag, L.fold(k, n)) and float(gap.min()) >= 0.1
                assert float(np.max(np.abs(mv - L.ld_scores(ref, rows, n, k)))) <= L.K_ORACLE * math.log2(n) * L.U


def test_index_set_is_structured_and_reachable():
    for N, budget in ((8192, 1024), (5000, 1024), (65536, 512), (40000, 512), (1048576, 96), (1000003, 96)):
        n = L.fft_len(N)
        idx = L.index_set(N, n, budget)
        assert len(idx) == len(set(idx.tolist())) <= budget and idx.min() == 0 and idx.max() == n - 1
        assert {n // 2 - 1, n // 2, n // 2 + 1} <= set(idx.tolist())
        if N < n:
            head, tail = L.split_head_tail(idx, N)
            assert np.all(L.reachable(head, N, 0)) and np.all(L.reachable(tail, N, N - L.W)) and len(head) + len(tail) == len(idx)
            assert {N - L.W, n - (N - L.W), n - N, N - 1} <= set(idx.tolist())
    small = L.index_set(8192, 8192, 1024)
    for j in range(1, 13):
        assert {(1 << j) - 1, 1 << j, (1 << j) + 1, 8192 - (1 << j)} <= set(small.tolist())
