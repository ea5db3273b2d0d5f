"""GPU lag sweep of the one-sided scoring path (muse_batch_scores / muse_batch_run and every kernel behind them).  Run with -m gpu on
an MI355X.

That path returns only (lag, mv) per series, so the other GPU files check its kernels at the one index where a row's maximum
happens to fall.  Here the winner is PLANTED (tests/_lagsweep.py): every output index of the transforms up to n = 4096, a structured
index set of the larger ones (the fold at n / 2, the ends, powers of two, tile multiples, the pad edges), for N == n and for zero-padded
lengths (where the batch's per-lag correction table c1 is in use), through the automatic and the forced kernels, the cached reader,
float32-storage groups, the many-references pass and the screened Run.  Expected, with no oracle call and no FFT:

  * the lag is the planted one, exact, for EVERY row (tests/test_lag_sweep_cpu.py shows the construction leaves no ties);
  * |mv - ld_score_at| <= 4 * K_ORACLE * log2(n) * 2^-53, absolute (scores are O(1)): ld_score_at is the long-double sum at that
    single lag, K_ORACLE the oracle's own measured error constant (asserted in the CPU file).  4 x: the kernels have the oracle's
    stage count and differ in radix, operation order, pair packing with power-of-two rescaling and the real-series post-pass.

One kind of row has a documented bound of its own (derived in tests/_lagsweep.py above row_bounds): a row whose planted code lies on
its FIRST sample (about 24 of a full sweep's rows; n > 65536: every row of a reference whose code does).  The tuned kernels shift a
series by its first sample instead of its mean, so a far-outlier first sample (lambda = |x[0] - mean| / sigma of 10 ... 100 here)
enlarges what is transformed by sqrt(1 + lambda^2) and makes the one-pass variance cancel: measured 1e-14 ... 4e-13 on exactly those
rows and below 1e-15 on all others.  Their lags are held exact like everyone's; the common bound is not widened for any other row.

MUSE_TEST_WORST=<file> appends every case's measured worst error (profiles/lag_sweep_parity.txt is such a run)."""
import os

import numpy as np
import pytest

import _lagsweep as L
from _load import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def muse():
    m = pkg()
    m.build.build()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return m


@pytest.fixture(scope="module")
def eng(muse):
    e = muse.Engine(0)                       # a context of its own: the hooks set below never leak into other test files
    yield e
    e.close()


def _check(tag, n, lag, mv, ks, want, bounds=None):
    """every lag the planted one; every score inside the bound of the long-double value; the worst error is printed and recorded
    before anything is asserted.  bounds: (per-row bound, far-first-sample mask) of _lagsweep.row_bounds"""
    lag, mv, ks = np.asarray(lag), np.asarray(mv, dtype=np.float64), np.asarray(ks)
    assert lag.shape == ks.shape == mv.shape == want.shape
    err = np.abs(mv.astype(np.longdouble) - want).astype(np.float64)
    err[~np.isfinite(err)] = np.inf
    rb, far = bounds if bounds is not None else (np.full(err.shape, L.bound(n)), np.zeros(err.shape, dtype=bool))
    assert np.all(rb[~far] == L.bound(n))
    worst = float(err[~far].max()) if not far.all() else 0.0
    line = "%s n=%d rows=%d worst=%.3e bound=%.3e" % (tag, n, len(ks), worst, L.bound(n))
    if far.any():
        line += " | %d rows with a far first sample: worst=%.3e, of their bound %.3f" % (
            int(far.sum()), float(err[far].max()), float(np.max(err[far] / rb[far])))
    print(line)
    path = os.environ.get("MUSE_TEST_WORST")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    bad = np.nonzero(lag != L.fold(ks, n))[0]
    assert bad.size == 0, "%s: %d lags off the planted index, first at output indices %s (got lags %s)" % (
        tag, bad.size, ks[bad[:8]].tolist(), lag[bad[:8]].tolist())
    over = np.nonzero(err > rb)[0]
    assert over.size == 0, "%s: %d scores outside their bound, first at output indices %s: errors %s, bounds %s" % (
        tag, over.size, ks[over[:8]].tolist(), err[over[:8]].tolist(), rb[over[:8]].tolist())
    return worst


def _expected_kernel(n, variant, f32=False):
    """prefix of the name muse_batch_kernel_name must report for this FFT length under test hook `variant` (capi_batch.hip,
    choose_kernel: a forced kernel whose tables are missing falls through to the generic one -- that must not pass for a sweep of it)"""
    logn = n.bit_length() - 1
    if variant == 1:
        return "xcorr_fused_generic"
    if n == 4096:
        return {0: "xcorr_fused_n4096_fold<", 10: "xcorr_fused_n4096_fold<", 7: "xcorr_fused_n4096_occ4"}[variant]
    real = "xcorr_fused_real32k_split<" if n == 32768 else "xcorr_fused_real%dk<" % (n // 1024)
    return {0: "xcorr_fused_small<%d," % logn if (f32 or n <= 2048) else real,
            11: "xcorr_fused_stk_4step" if n >= 8192 else "xcorr_fused_stockham",
            12: "xcorr_fused_small<%d," % logn,
            13: "xcorr_fused_long<%d," % logn,
            14: "xcorr_fused_real%dk<" % (n // 1024),
            15: "xcorr_fused_real32k_split<"}[variant]


class _Case:
    """one reference and its rows resident on the device, with the expectation"""

    def __init__(self, muse, eng, ref, rows, ks, f32=False):
        self.eng, self.f32 = eng, f32
        self.dg = muse.DeviceGroup.from_rows(eng, rows, f32=f32)
        if f32:                              # the expectation is computed on the float32-rounded rows, rounded HERE; the group holds the same
            rows = rows.astype(np.float32).astype(np.float64)
            assert np.array_equal(self.dg.read(0, rows.shape[0]), rows)
        self.db = muse.DeviceBatch(eng, self.dg, ref)
        self.n, self.ks = self.db.n, ks
        assert self.n == L.fft_len(len(ref))
        self.want = L.ld_scores(ref, rows, self.n, ks)
        self.bounds = L.row_bounds(self.n, rows, ref)
        self.bounds_centred = L.row_bounds(self.n, rows, ref, shifted=False)   # the generic kernel: the common bound on every row

    def check(self, tag, variant=0, cached=False):
        """sets test hook `variant`, asserts that the kernel it names is the one that will run, scores and checks"""
        self.eng.set_kernel(variant)
        name = self.eng.kernel_name(self.db)
        want_name = "xcorr_cached_n4096<" if cached else _expected_kernel(self.n, variant, self.f32)
        assert name.startswith(want_name), (tag, variant, name, want_name)
        lag, mv = self.db.scores()
        return _check("%s variant=%d (%s)" % (tag, variant, name), self.n, lag, mv, self.ks, self.want,
                      self.bounds_centred if variant == 1 else self.bounds)

    def close(self):
        self.db.close()
        self.dg.close()


def _sweep_variants(muse, eng, N, budget, variants, seed, f32_too=False, head_off_first=False):
    """the cases of length N, each resident once and scored by every variant"""
    for i, (ref, rows, ks) in enumerate(L.sweep_cases(N, budget, seed=seed, head_off_first=head_off_first)):
        c = _Case(muse, eng, ref, rows, ks)
        try:
            for v in variants:
                c.check("N=%d ref=%d" % (N, i), v)
        finally:
            eng.set_kernel(0)
            c.close()
        if f32_too:
            c = _Case(muse, eng, ref, rows, ks, f32=True)
            try:
                c.check("N=%d ref=%d float32-storage" % (N, i))
            finally:
                c.close()


# ------------------------------------------------------------------ a. n = 4096: every index
@pytest.mark.parametrize("N", [4096, 3000])
def test_n4096_every_index(muse, eng, N):
    """M = 4096 rows at N = 4096; head and tail references with 2977 rows each at N = 3000 (c1 in use): the default kernel, the
    generic one (1), the rescaling one (7), the default forced (10), then the group's spectrum cache -- writer and reader"""
    eng.set_spectrum_cache(False)            # passes 1 ... 4 run the plain kernels whatever the group's size
    try:
        for i, (ref, rows, ks) in enumerate(L.sweep_cases(N, None, seed=N)):
            c = _Case(muse, eng, ref, rows, ks)
            try:
                for v in (0, 1, 7, 10):
                    c.check("N=%d ref=%d" % (N, i), v)
                eng.set_kernel(0)
                eng.set_spectrum_cache(True)
                eng.spectrum_cache_limits(min_rows=2)
                for k in range(2):           # plain, then the writer
                    c.check("N=%d ref=%d cache pass %d" % (N, i, k + 1))
                assert c.dg.spectrum_cache()[0] == len(ks) & ~1
                c.check("N=%d ref=%d cache pass 3" % (N, i), cached=True)      # the reader, by name
                c.check("N=%d ref=%d cache pass 4" % (N, i), cached=True)
            finally:
                eng.set_kernel(0)
                eng.set_spectrum_cache(False)
                c.close()
    finally:
        eng.set_kernel(0)
        eng.spectrum_cache_limits()
        eng.set_spectrum_cache(True)


@pytest.mark.parametrize("N", [4096, 3000])
def test_n4096_every_index_float32_storage(muse, eng, N):
    """the same construction in a float32-storage group; expected values computed on the rows rounded to float32 by numpy, which the
    group must read back unchanged"""
    for i, (ref, rows, ks) in enumerate(L.sweep_cases(N, None, seed=N + 1)):
        c = _Case(muse, eng, ref, rows, ks, f32=True)
        try:
            c.check("N=%d ref=%d float32-storage" % (N, i))
        finally:
            c.close()


# ------------------------------------------------------------------ b. n = 512, 1024, 2048: every index
@pytest.mark.parametrize("n", [512, 1024, 2048])
@pytest.mark.parametrize("padded", [False, True])
def test_small_lengths_every_index(muse, eng, n, padded):
    """N = n, and the shortest N whose head and tail references still cover all n indices (N = n / 2 + W + 1): automatic selection, the
    Stockham kernels (11), the half-round kernels (12), the generic one (1); a float32-storage group at n = 1024"""
    N = n // 2 + L.W + 1 if padded else n
    _sweep_variants(muse, eng, N, None, (0, 11, 12, 1), seed=7 * N, f32_too=(n == 1024))


# ------------------------------------------------------------------ c. n = 8192 ... 65536: the index set
@pytest.mark.parametrize("N", [8192, 5000, 16384, 10000, 32768, 20000, 65536, 40000])
def test_long_lengths_index_set(muse, eng, N):
    """the variants tests/test_gpu_parity.py::test_stockham_kernels_match_oracle_and_generic lists for each length, on planted
    winners at the fold, the ends, the powers of two, the tile multiples and the pad edges"""
    n = L.fft_len(N)
    small = n in (8192, 16384)
    variants = ((0, 11, 12, 1) if small else (0, 11, 1)) + ((13,) if n >= 16384 else ()) + ((14,) if n >= 8192 else ()) + \
        ((15,) if n == 32768 else ())
    _sweep_variants(muse, eng, N, 1024 if n <= 16384 else 512, variants, seed=3 * N)


# ------------------------------------------------------------------ d. n = 2^17, 2^20: the four-step kernels
@pytest.mark.parametrize("N", [131072, 100000, 1048576, 1000003])
def test_huge_lengths_index_set(muse, eng, N):
    """no oracle here: the planted lag and ld_score_at are the expectation.  95 winners per length (row bytes limit it), so the one
    reference of N == n and one of the head and tail references of N < n score an odd row count: the last series then has no pair
    partner.  N < n: a third reference, its code at p = 1, plants the head reference's indices once more (tests/_lagsweep.py, row_bounds)"""
    n = L.fft_len(N)
    odd = 0
    common = 0
    for i, (ref, rows, ks) in enumerate(L.sweep_cases(N, 95, seed=N, head_off_first=True)):
        odd += len(ks) & 1
        c = _Case(muse, eng, ref, rows, ks)
        try:
            name = eng.kernel_name(c.db)
            assert c.n == n and name.startswith("huge_rows"), name
            lag, mv = c.db.scores()
            _check("N=%d ref=%d (%s)" % (N, i, name), n, lag, mv, ks, c.want, c.bounds)
            common += int((~c.bounds[1]).sum())
        finally:
            c.close()
    assert odd >= 1
    # (N < n: the head reference's own first sample is an outlier, so its rows have the derived bound; the reference with the code
    # at p = 1 plants the same indices on the common bound)
    assert common >= 90


# ------------------------------------------------------------------ e. many references, one pass
@pytest.mark.parametrize("N", [4096, 3000, 1024])
def test_many_references_every_index(muse, eng, N):
    """muse.score_many: the head-code, the tail-code and a middle-code reference against ONE resident group holding the code at every
    position; each batch's read_scores() against its own planted indices"""
    refs, rows, ks = L.many_refs_case(N, seed=11 * N)
    n = L.fft_len(N)
    dg = muse.DeviceGroup.from_rows(eng, rows)
    dbs = [muse.DeviceBatch(eng, dg, r) for r in refs]
    try:
        eng.kernel_time()                    # (clears the sums)
        eng.kernel_timing(True)
        muse.score_many(dbs)
        eng.synchronize()
        eng.kernel_timing(False)
        # ONE bracketed launch for the three references: the one-pass kernel, not three single-reference passes one after the other
        assert eng.kernel_time()[1] == 1
        for i, (db, ref, k) in enumerate(zip(dbs, refs, ks)):
            lag, mv = db.read_scores()
            _check("N=%d score_many reference %d" % (N, i), n, lag, mv, k, L.ld_scores(ref, rows, n, k), L.row_bounds(n, rows, ref))
    finally:
        eng.kernel_timing(False)
        for db in dbs:
            db.close()
        dg.close()


# ------------------------------------------------------------------ f. the screened Run
SCREEN_ROWS = 256                            # TOPN_DEVICE_MAX: the largest top_n the filter-and-refine Run is taken for


@pytest.mark.parametrize("N,budget", [(4096, None), (1024, None), (16384, 512)])
def test_screened_run_every_index(muse, eng, N, budget):
    """eng.set_screening(True, 2), then run(None, 0, max_lag=n, top_n=M, 0.0, 0, True): a record per row.  The screened path is
    built for top_n <= 256, so the sweep is cut into resident groups of at most 256 rows (the last ones odd), each with a batch of
    its own on the shared reference spectrum; last_run_path() == 1 proves the fp32 screen and its fp64 refinement ran.  Lags exact;
    scores to the common bound, since the records are fp64 results."""
    n = L.fft_len(N)
    try:
        eng.set_screening(True, 2)
        for i, (ref, rows, ks) in enumerate(L.sweep_cases(N, budget, seed=13 * N)):
            want = L.ld_scores(ref, rows, n, ks)
            M = len(ks)
            cuts = list(range(0, M, SCREEN_ROWS - 1))     # 255 rows per group: every group's last series has no pair partner
            lag, mv = np.zeros(M, dtype=np.int32), np.full(M, np.nan)
            first, dg, db = None, None, None
            try:
                for lo in cuts:
                    hi = min(M, lo + SCREEN_ROWS - 1)
                    dg = muse.DeviceGroup.from_rows(eng, rows[lo:hi])
                    db = muse.DeviceBatch(eng, dg, ref) if first is None else muse.DeviceBatch.like(first[1], dg)
                    idx, l2, sc, _ = db.run(None, 0, n, hi - lo, 0.0, 0, True)
                    assert db.last_run_path() == 1 and db.last_run_info()[0] is True, (N, lo)
                    assert sorted(idx.tolist()) == list(range(hi - lo)), (N, lo)      # a record per row
                    lag[lo + idx], mv[lo + idx] = l2, sc
                    if first is None:
                        first = (dg, db)     # the template lives until the last group is done
                    else:
                        db.close()
                        dg.close()
                    dg, db = None, None
            finally:
                for h in (db, dg) + ((first[1], first[0]) if first else ()):
                    if h is not None:
                        h.close()
            # (Batch.Run with abs_scores reports |score|: scores.go / muse_batch.go; the sign is swept by every other case)
            _check("N=%d ref=%d screened Run, %d groups" % (N, i, len(cuts)), n, lag, mv, ks, np.abs(want), L.row_bounds(n, rows, ref))
    finally:
        eng.set_screening(False)
