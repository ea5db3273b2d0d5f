"""Planted-lag construction and long-double expectation for the lag-window kernels, shared by tests/test_window_sweep_cpu.py and
tests/test_gpu_window_sweep.py.  It touches nothing under test.

The windowed kernels (xcorr_window.hip, _split, _many, _slide) return, per series, maxAbsIndex over the lags -Lneg .. L of the
correlation.  To pin every scan position and every accumulator-tile element, a case holds one row PER LAG: the reference carries
a code of w Gaussian samples at p = (N - w) // 2 and row r the same code at p - lag[r] (tests/_lagsweep.py's generators: low
noise, amplitude +-[0.5, 1.5], a constant offset), so its correlation has one dominant entry, at lag[r].  The rows of a case:

  * one per lag in [-63, 63];
  * 30 on each side just outside, |lag| = 64 .. 93: their best match inside any window is one of the code's autocorrelation
    sidelobes (or, with no overlap left, code against noise) -- a definite value with a definite sign at a non-peak lag;
  * shuffled with the seed; then 8 copies of the first rows with 50 sigma(row) added to sample 0: the kernels shift a row by its
    first sample (d = y - y[0]) and take the variance in one pass, and these rows make that as hard as it gets.

N < n: only lags whose code stays inside the row.  N == n (the shift is circular): lags folded at n / 2, each once -- at N = 64
that is -31 .. +32, every lag of the clipped window L = 32, Lneg = 31.

EXPECTATION.  tables(): cc[r, lag] for every lag in [-Lc, Lc], Lc = min(63, n / 2), by the definition _lagsweep.ld_ref /
ld_score_at state (leading zero pads, zNormalize with divisor N - 1), in np.longdouble throughout, no FFT and no oracle call: one
long-double product of the centred rows with the matrix of shifted references.  expect(): per L the (lag, mv) of maxAbsIndex over
that table in the definition's scan order -- 0 .. L, then -Lneg .. -1, strict '>', start (0, 0.0); Lneg = L - 1 when the clipped L
equals n / 2 (_window.window_indices' order).  The planted lag is a property of the construction that the CPU file checks; it is not
the expectation: outside rows and outlier rows do not win at it.

SCORE BOUND.  Derived, not tuned; it holds for any summation order.  With u = 2^-53, g(k) = k u / (1 - k u) (Higham, Accuracy and
Stability of Numerical Algorithms, Lemma 3.1), and the kernel's own quantities in long double -- d = y - y[0], e[t] = the reference
under sample t at that lag, t1 = sum d, t2 = sum d^2, S = sum d e, P = sum e, var = (t2 - t1^2 / N) / (N - 1):

    dS   = g(N+2) sum|d||e|      dt1 = g(N) sum|d|      dt2 = g(N+1) t2      dP = g(N) sum|e|
    dvar = (dt2 + 2 |t1| dt1 / N + 3u (t2 + t1^2 / N)) / (N - 1)
    dnum = dS + dt1 |P| / N + |t1 / N| dP + 3u (|S| + |t1 P / N|)
    B    = dnum / sqrt(var) + |cc| (dvar / (2 var) + 3u)

N + 2 counts the rounding of d, of the product and N - 1 additions (a fused MFMA only rounds less, which leaves room for the one
rounding of the float64 reference table).  The first-sample shift needs no special case: an outlier y[0] enlarges sum|d||e|, t2
and t1 by itself.  The long-double sums behind the expectation err by at most N 2^-64 of the same magnitudes: 2^-11 of B.

GAP CONDITION.  A condition of the construction, asserted before any comparison; it is not a tolerance.  For every row and every L
the two largest |cc| inside the window differ by at least GAP_FACTOR (B_first + B_second), so a kernel inside B cannot pick another
lag.  No row is excused."""
import numpy as np

import _lagsweep as LS

LMAX = 63                 # MUSE_LAG_WINDOW_MAX
OUTSIDE = 30              # rows just outside the widest window, per side
OUTLIERS = 8
OUTLIER_SIGMAS = 50.0
GAP_FACTOR = 100.0
U = 2.0 ** -53
MANY_OFFSETS = (0, 5, -11, 3, -7, 13, -17, 20)   # code positions of the many-references case, relative to p


def code_len(N):
    return 8 if N <= 128 else LS.W


def fold_lag(lag, n):
    """a circular shift as the lag the definition reports: index (lag mod n) folded at n / 2 (index n / 2 is lag +n/2)"""
    return LS.fold(np.asarray(lag, dtype=np.int64) % n, n).astype(np.int64)


def planted_lags(N, w):
    """the lags a case plants, in ascending-|lag| order: [-63, 63], then |lag| = 64 .. 93"""
    n, p = LS.fft_len(N), (N - w) // 2
    cand = list(range(-LMAX, LMAX + 1)) + [s * k for k in range(LMAX + 1, LMAX + 1 + OUTSIDE) for s in (1, -1)]
    if N == n:
        out = []
        for lag in fold_lag(cand, n).tolist():
            if lag not in out:
                out.append(lag)
        return np.array(out, dtype=np.int64)
    return np.array([lag for lag in cand if 0 <= p - lag <= N - w], dtype=np.int64)


class Case:
    """ref / refs, rows, the planted lag of every row (for refs[0]; refs[i]: + offsets[i], folded), the outlier mask"""


def make_case(N, seed=0, lags=None, offsets=(0,), p=None):
    """the case of length N.  lags: the planted lags instead of planted_lags() (the outlier copies are appended either way);
    offsets: one reference per entry, the code at p + offset over noise of its own; p: the reference's code position instead of
    the middle of the row"""
    w = code_len(N)
    n, p = LS.fft_len(N), ((N - w) // 2 if p is None else int(p))
    lags = planted_lags(N, w) if lags is None else np.asarray(lags, dtype=np.int64)
    lags = lags[np.random.default_rng([seed, 7]).permutation(len(lags))]
    ref, rows, n2 = LS.make_case(N, -lags, p, w, seed)
    assert n2 == n
    k = min(OUTLIERS, len(lags))
    far = rows[:k].copy()
    far[:, 0] += OUTLIER_SIGMAS * rows[:k].std(axis=1, ddof=1)
    c = Case()
    c.N, c.n, c.w, c.p, c.seed = N, n, w, p, seed
    c.rows = np.ascontiguousarray(np.vstack([rows, far]))
    c.lag = np.concatenate([lags, lags[:k]])
    c.outlier = np.concatenate([np.zeros(len(lags), dtype=bool), np.ones(k, dtype=bool)])
    code = LS.make_code(seed, w)
    c.offsets = tuple(offsets)
    assert c.offsets[0] == 0
    c.refs = [ref] + [LS.make_ref(N, p + off, code, seed + 100 * i) for i, off in enumerate(c.offsets) if i > 0]
    c.ref = c.refs[0]
    for a in [c.rows, c.lag, c.outlier] + c.refs:
        a.setflags(write=False)
    return c


def planted(case, i=0):
    """the planted lag of every row against reference i"""
    lag = case.lag + case.offsets[i]
    return fold_lag(lag, case.n) if case.N == case.n else lag


# ------------------------------------------------------------------ the long-double table and its bound
def _g(k):
    k = np.longdouble(k)
    return k * U / (1 - k * U)


class Table:
    """cc[M, 2 Lc + 1] (long double) and B[M, 2 Lc + 1] (float64) for lags -Lc .. Lc (column c: lag lags[c] = c - Lc)"""


class Image:
    """the matrix of shifted references of one reference, [lag][t] contiguous: E[lag + Lc, t] = the (normalised, zero-padded)
    reference under sample t at that lag, in long double; computed once per reference"""

    def __init__(self, ref, n, lags=None):
        """lags: a contiguous ascending lag list in place of -Lc .. Lc (tests/_rangesweep.py); Lc is then the column of lag 0"""
        N = len(ref)
        self.N, self.n, self.Lc = N, n, min(LMAX, n // 2)
        if lags is None:
            lags = np.arange(-self.Lc, self.Lc + 1)
        else:
            lags = np.asarray(lags, dtype=np.int64)
            assert lags[0] <= 0 <= lags[-1] and np.array_equal(lags, np.arange(lags[0], lags[-1] + 1))
            self.Lc = -int(lags[0])
        self.lags = lags
        xs_pad = LS.ld_ref(ref, n)
        self.E = np.ascontiguousarray(xs_pad[(n - N + lags[:, None] + np.arange(N)[None, :]) % n])
        self.Eabs = np.abs(self.E)
        self.P = self.E.sum(axis=1)[None, :]
        self.Pabs = self.Eabs.sum(axis=1)[None, :]


def tables(ref, rows, n, image=None, lags=None):
    """the Table of `rows` against `ref` (image: its Image, when the caller keeps one; lags: Image's, for a table of other columns)"""
    ld = np.longdouble
    rows = np.asarray(rows, dtype=np.float64)
    M, N = rows.shape
    im = Image(ref, n, lags) if image is None else image
    assert im.N == N and im.n == n
    Y = rows.astype(ld)
    mean = Y.sum(axis=1) / N
    Dm = Y - mean[:, None]
    sigma = np.sqrt((Dm * Dm).sum(axis=1) / (N - 1))
    t = Table()
    t.n, t.N, t.Lc, t.lags = n, N, im.Lc, im.lags
    Sm = np.dot(Dm, im.E.T)                                               # one long-double dot per (row, lag)
    t.cc = Sm / sigma[:, None]
    # the bound, from the kernel's quantities
    D = Y - Y[:, :1]
    Dabs = np.abs(D)
    t1 = D.sum(axis=1)[:, None]
    t2 = (D * D).sum(axis=1)[:, None]
    P = im.P
    S = Sm + (mean - Y[:, 0])[:, None] * P                                # = D @ E (D = Dm + (mean - y[0]) 1)
    A = np.dot(Dabs, im.Eabs.T)
    var = (t2 - t1 * t1 / N) / (N - 1)
    dS = _g(N + 2) * A
    dt1 = _g(N) * Dabs.sum(axis=1)[:, None]
    dt2 = _g(N + 1) * t2
    dP = _g(N) * im.Pabs
    dvar = (dt2 + 2 * np.abs(t1) * dt1 / N + 3 * U * (t2 + t1 * t1 / N)) / (N - 1)
    dnum = dS + dt1 * np.abs(P) / N + np.abs(t1 / N) * dP + 3 * U * (np.abs(S) + np.abs(t1 * P / N))
    t.B = (dnum / np.sqrt(var) + np.abs(t.cc) * (dvar / (2 * var) + 3 * U)).astype(np.float64)
    assert np.all(np.isfinite(t.B)) and np.all(t.B > 0)
    return t


def scan_order(n, L):
    """the lags maxAbsIndex scans, in order: 0 .. L, then -Lneg .. -1 (L clipped to n / 2; Lneg = L - 1 there)"""
    L = min(int(L), n // 2)
    Lneg = L - 1 if 2 * L == n else L
    return np.concatenate([np.arange(0, L + 1), np.arange(-Lneg, 0)]).astype(np.int64)


def expect(t, L):
    """(lag[M], mv[M] long double, B[M], ratio[M]) for window L: maxAbsIndex over the table in scan order (np.argmax returns the
    first maximum = strict '>'; an all-zero window leaves (0, 0.0)); ratio = (|first| - |second|) / (B_first + B_second) inside
    the window, inf when the window holds one lag"""
    order = scan_order(t.n, L)
    cols = order + t.Lc
    sub, Bs = t.cc[:, cols], t.B[:, cols]
    a = np.abs(sub)
    k = np.argmax(a, axis=1)
    r = np.arange(len(k))
    win = a[r, k] > 0
    lag = np.where(win, order[k], 0).astype(np.int32)
    mv = np.where(win, sub[r, k], np.longdouble(0))
    B = np.where(win, Bs[r, k], Bs[:, 0])
    if len(order) == 1:
        return lag, mv, B, np.full(len(k), np.inf)
    a2 = a.copy()
    a2[r, k] = -1
    k2 = np.argmax(a2, axis=1)
    ratio = ((a[r, k] - a[r, k2]) / (Bs[r, k] + Bs[r, k2])).astype(np.float64)
    return lag, mv, B, ratio


def gap_ratio(t, Ls=None):
    """the smallest ratio of expect() over all rows and the windows Ls (default: every L in 0 .. 63)"""
    return min(float(expect(t, L)[3].min()) for L in (range(LMAX + 1) if Ls is None else Ls))


def kernel_restatement(ref, rows, n):
    """the kernels' arithmetic restated in plain float64 numpy, for every lag of the table: d = y - y[0], one-pass variance,
    (S - mean P) / sigma with the float64 reference image.  -> cc64[M, 2 Lc + 1]"""
    rows = np.asarray(rows, dtype=np.float64)
    M, N = rows.shape
    Lc = min(LMAX, n // 2)
    lags = np.arange(-Lc, Lc + 1)
    x = np.asarray(ref, dtype=np.float64)
    xd = x - x.mean()
    xs = np.zeros(n)
    xs[n - N:] = xd / np.sqrt((xd * xd).sum() / (N - 1)) / (N - 1)
    E = xs[(n - N + np.arange(N)[:, None] + lags[None, :]) % n]
    D = rows - rows[:, :1]
    t1 = D.sum(axis=1)
    t2 = (D * D).sum(axis=1)
    var = (t2 - t1 * t1 * (1.0 / N)) * (1.0 / (N - 1))
    mean = t1 * (1.0 / N)
    return ((D @ E) - mean[:, None] * E.sum(axis=0)[None, :]) * (1.0 / np.sqrt(var))[:, None]


# ------------------------------------------------------------------ the cases of the two test files
# lengths of the single-reference sweep: even stride and whole pieces; N < n with a partial last piece; odd stride; odd stride with
# a last chunk of one sample; less than one chunk; two pieces; N = n = 64 (L clipped at 32, Lneg = 31, one piece)
LENGTHS = (4096, 3000, 1433, 1025, 480, 128, 64)
SPLIT_LENGTHS = (2049, 5000)      # 3 chunks, the last one sample long; 5 chunks
SPLIT_LONG = 35841                # 35 chunks plus one sample
MANY_LENGTHS = (4096, 1433, 480)
SLIDE_LENGTHS = (4096, 1433)
SLIDE_KS = (1, 16, 64)
SLIDE_CALLS = 4
SLIDE_LS = (7, 8, 23, 24, 63)


def case_seed(N):
    """N, but for N = 64: a code of 8 samples has an energy that depends much on the draw, and the construction wants the weakest
    row (amplitude 0.5) to score above 0.9 -- seed 65's code does (tests/test_window_sweep_cpu.py asserts it)"""
    return {64: 65}.get(N, N)


def sweep_case(N):
    return make_case(N, seed=case_seed(N))


def long_case():
    """17 rows at lags spread over [-63, 63] and their outlier copies, at SPLIT_LONG samples"""
    return make_case(SPLIT_LONG, seed=SPLIT_LONG, lags=np.round(np.linspace(-LMAX, LMAX, 17)).astype(np.int64))


def many_case(N):
    """one row set, eight references with the code at p + MANY_OFFSETS[i] (R = 3: the first three)"""
    return make_case(N, seed=case_seed(N) + 1, offsets=MANY_OFFSETS)


def slide_states(case, k, calls=SLIDE_CALLS):
    """[(tails, rows after the call)] of `calls` slides by k, starting from the case's rows: the planted lag walks by +k per call"""
    out, cur = [], case.rows
    for i in range(calls):
        tails = slide_tails(cur, k, case.seed + i)
        cur = slid(cur, tails)
        out.append((tails, cur))
    return out


# ------------------------------------------------------------------ the slide
def slide_tails(rows, k, seed):
    """noise tails of the rows' own level and sigma: median(row) + sigma(row) * standard normal, (M, k)"""
    rng = np.random.default_rng([seed, 8, k])
    return np.median(rows, axis=1)[:, None] + rows.std(axis=1, ddof=1)[:, None] * rng.standard_normal((rows.shape[0], k))


def slid(rows, tails):
    return np.ascontiguousarray(np.concatenate([rows[:, tails.shape[1]:], tails], axis=1))
