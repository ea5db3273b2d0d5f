"""Planted-lag construction shared by tests/test_lag_sweep_cpu.py and tests/test_gpu_lag_sweep.py.  It touches nothing under test.

The one-sided scoring path returns (lag, mv) per series -- the argmax of the correlation, never the correlation itself.  To check it
at a CHOSEN output index, the reference carries a short code of W Gaussian samples at position p and the row the same code at
position q, over low noise: the correlation then has one dominant entry, at

    k = (p - q) mod n          (lag = k folded at n / 2: a code moved by +s in the row gives lag -s),

and its value there is compared with ld_score_at(): the definition (oracle_xcorr_direct_ld in oracle/muse_oracle.c: leading zero
pads, xs = zNormalize(ref) / (N - 1)) restated in numpy long double for that single index -- mean, variance and dot product all in
long double, no FFT anywhere.  Sweeping q over every position is an element-wise check of cc through the public interface.

N == n: the shift is circular and one reference reaches every index.  N < n: the shift is linear (0 <= q <= N - W), a reference with
the code at its head (p = 0) reaches k = 0 and k >= n - (N - W), one with the code at its tail (p = N - W) reaches k <= N - W; the
two together cover all n indices when N >= n / 2 + W."""
import math

import numpy as np

W = 24            # samples of the planted code
CODE_SIGMA = 3.0  # of the code's samples; the noise has sigma NOISE / sqrt(N): the planted score stays above ~0.9 at every length
NOISE = 2.0
U = 2.0 ** -53

# The oracle's own error, MEASURED by tests/test_lag_sweep_cpu.py against ld_score_at and asserted there at every length it lists:
#     max |oracle mv - long double| <= K_ORACLE * log2(n) * 2^-53.
# The GPU tests allow 4x that (bound(n)): the kernels have the oracle's stage count and differ in radix, operation order, pair
# packing with power-of-two rescaling and the real-series post-pass -- the constant of the rounding error, not its growth.
K_ORACLE = 13
GPU_MARGIN = 4


def bound(n, margin=GPU_MARGIN):
    """absolute score bound at FFT length n (scores are O(1))"""
    return margin * K_ORACLE * math.log2(n) * U


# The one documented exception (found by this sweep).  The tuned kernels read a row once, so they cannot centre it
# on its mean before transforming: they shift it by its FIRST SAMPLE, d = x - x[0], transform d, and take the mean out afterwards
# (DC bin, the c1 table, or one-pass sums); sigma comes from sum d^2 - (sum d)^2 / N.  With lambda = |x[0] - mean| / sigma,
#     d = (x - mean) + (mean - x[0]) 1,      ||d||_2 = ||x - mean||_2 sqrt(1 + lambda^2 N / (N - 1)),
# so (a) the transform's rounding error, proportional to the norm of what is transformed, grows by sqrt(1 + lambda^2): the common
# bound times that factor (which leaves these rows exactly the slack every other row has: measured / bound ~0.02 for both); and
# (b) the variance is the difference of sum d^2 ~ N (sigma^2 + c^2) and (sum d)^2 / N ~ N c^2 (c = mean - x[0]), each rounded along
# a chain of at most SHIFT_CHAIN additions (16 sequential fma per thread, then a tree over up to 2^20 / 16 partial sums).  The
# worst case is a relative error SHIFT_CHAIN u (1 + 2 lambda^2) of the variance; independent roundings accumulate as the square
# root of the chain (Higham & Mary, SIAM J. Sci. Comput. 41 (2019): sqrt(k) u with a constant of order 1), taken here with a factor 2:
# 2 sqrt(SHIFT_CHAIN) u (1 + 2 lambda^2) for the variance, half that for 1 / sigma, and |score| <= 1.
# For a first sample like any other (lambda <= LEVEL_MAX: every row here whose code does not lie on sample 0) nothing is added: the
# common bound holds as it is.  A row whose planted code covers sample 0 has lambda = 10 ... 100; it is held to the lag, exactly, and to
#     bound(n) sqrt(1 + lambda^2) + sqrt(SHIFT_CHAIN) u (1 + 2 lambda^2).
# The generic kernel (test hook 1) centres on the mean: the tests hold it to the common bound on EVERY row (shifted=False).
# Above n = 65536 the REFERENCE goes through the same first-sample shift (huge_reference), so there a head-code reference's lambda
# counts for each of its rows -- and a second head reference with the code at p = 1 sweeps the same indices on the common bound; up
# to 65536 the reference is centred on its mean and its lambda is of no concern (measured).
LEVEL_MAX = 4.0
SHIFT_CHAIN = 32


def first_sample_level(x):
    """lambda = |x[0] - mean| / sigma of a series, or of every row of a matrix"""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x[..., 0] - x.mean(axis=-1)) / x.std(axis=-1, ddof=1)


def row_bounds(n, rows, ref=None, shifted=True):
    """(score bound of every row, mask of the rows off the common bound): bound(n), except -- for a kernel that shifts by the first
    sample -- where the first sample of the row (n > 65536: or of `ref`) is a far outlier"""
    lam2 = first_sample_level(rows) ** 2
    if ref is not None and n > 65536:
        lam2 = lam2 + first_sample_level(ref) ** 2
    b = np.full(lam2.shape, bound(n))
    far = (lam2 > LEVEL_MAX ** 2) & bool(shifted)
    b[far] = bound(n) * np.sqrt(1.0 + lam2[far]) + math.sqrt(SHIFT_CHAIN) * U * (1.0 + 2.0 * lam2[far])
    return b, far


def fft_len(N):
    return 1 << (int(N) - 1).bit_length()


def fold(k, n):
    """output index -> lag (xcorr.go:192-194)"""
    k = np.asarray(k, dtype=np.int64)
    return np.where(k > n // 2, k - n, k).astype(np.int32)


def planted_index(p, q, n):
    return (int(p) - np.asarray(q, dtype=np.int64)) % n


# ------------------------------------------------------------------ the construction
def make_code(seed, w=W):
    return CODE_SIGMA * np.random.default_rng([seed, 1]).standard_normal(w)


def make_ref(N, p, code, seed):
    """low noise plus the code at [p, p + w)"""
    assert 0 <= p <= N - len(code)
    ref = NOISE / math.sqrt(N) * np.random.default_rng([seed, 2]).standard_normal(N)
    ref[p:p + len(code)] += code
    return ref


def make_rows(N, q, code, seed):
    """row r: low noise plus amp[r] * code at position q[r] (wrapping past the end when N is a power of two, i. e. N == n), amp in
    +-[0.5, 1.5], plus a constant offset of up to 3 row-sigmas (so the mean correction -- the batch's c1 table when N < n -- is far
    from negligible)"""
    rng = np.random.default_rng([seed, 3])
    q = np.asarray(q, dtype=np.int64)
    M, w = len(q), len(code)
    circular = fft_len(N) == N
    assert circular or (q.min(initial=0) >= 0 and q.max(initial=0) <= N - w)
    rows = rng.standard_normal((M, N))
    rows *= NOISE / math.sqrt(N)
    amp = rng.uniform(0.5, 1.5, M) * rng.choice([-1.0, 1.0], M)
    idx = (q[:, None] + np.arange(w)[None, :]) % N
    rows[np.arange(M)[:, None], idx] += amp[:, None] * code[None, :]
    sigma = np.sqrt((amp * amp * float(code @ code) + NOISE * NOISE) / N)
    rows += (rng.uniform(-3.0, 3.0, M) * sigma)[:, None]
    return rows


def make_case(N, shifts, p, w=W, seed=0):
    """(ref, rows, n): the reference's code at p, row r's at p + shifts[r]; the planted index of row r is (-shifts[r]) mod n.  The
    row order is the order of `shifts`: take them from sweep_shifts() / shifts_for(), which shuffle with the seed (two series share
    one complex transform in most kernels, so pair partners carry unrelated lags and signs, not adjacent ones)."""
    n = fft_len(N)
    code = make_code(seed, w)
    shifts = np.asarray(shifts, dtype=np.int64)
    q = p + shifts
    if N == n:
        q = q % N
    return make_ref(N, p, code, seed), make_rows(N, q, code, seed), n


def sweep_shifts(N, p, w=W, seed=0):
    """every shift a code at p allows, shuffled: all n circular ones when N == n, else the N - w + 1 linear ones"""
    n = fft_len(N)
    s = np.arange(n) if N == n else np.arange(-p, N - w - p + 1)
    return np.random.default_rng([seed, 4]).permutation(s)


def heads_and_tails(N, w=W):
    """code positions of the references a full sweep needs: one when N == n, head and tail when N < n"""
    return [N // 3] if fft_len(N) == N else [0, N - w]


def row_pos(k, N, p, w=W):
    """position q of the row's code that makes index k the winner against a code at p: (p - q) mod n == k; -1 where no position
    inside the row does (N < n: 0 <= q <= N - w)"""
    n = fft_len(N)
    k = np.asarray(k, dtype=np.int64)
    if N == n:
        return (p - k) % n
    q = np.where(p - k >= 0, p - k, p - k + n)
    return np.where((q >= 0) & (q <= N - w), q, -1)


def reachable(k, N, p, w=W):
    """can a reference with its code at p make index k the winner?"""
    return row_pos(k, N, p, w) >= 0


def shifts_for(indices, N, p, w=W, seed=0):
    """(shifts, indices), shuffled together: the shift that plants each index with the code at p (indices must be reachable)"""
    k = np.asarray(indices, dtype=np.int64)
    q = row_pos(k, N, p, w)
    assert np.all(q >= 0), "index not reachable from p = %d" % p
    perm = np.random.default_rng([seed, 5]).permutation(len(k))
    return (q - p)[perm], k[perm]


def index_set(N, n, budget, w=W, seed=0):
    """at most `budget` winners for a transform too large to sweep fully, sorted: the fold and the ends, every power of two with
    its neighbours and their negatives, multiples of 256 and of 4096 with their neighbours, (N < n) the edges of what the head and
    the tail code reach and of the pad; indices no code of w samples can reach at this N are dropped.  Above the budget the
    power-of-two and multiple families are thinned evenly (the ends, the fold and the pad edges stay); below it seeded random
    indices fill up."""
    rng = np.random.default_rng([seed, 6, N])
    keep = [0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1]
    if N < n:
        for e in (N - w, n - (N - w), n - N, N - 1, N):
            keep += [e - 1, e, e + 1]
    fam = []
    for j in range(1, n.bit_length() - 1):
        for d in (-1, 0, 1):
            fam += [(1 << j) + d, -((1 << j) + d)]
    for step in (256, 4096):
        cnt = n // step
        if cnt > 2:
            for k in np.unique(np.linspace(1, cnt - 1, min(cnt - 1, max(2, budget // 16))).astype(np.int64)):
                fam += [int(k) * step - 1, int(k) * step, int(k) * step + 1]

    def clean(v, seen):
        out = []
        for k in v:
            k = int(k) % n
            if k not in seen and (reachable(k, N, 0, w) or reachable(k, N, N - w, w)):
                seen.add(k)
                out.append(k)
        return out
    seen = set()
    keep = clean(keep, seen)
    fam = clean(fam, seen)
    room = max(budget - len(keep), 0)
    if len(fam) > room:
        fam = [fam[i] for i in np.unique(np.linspace(0, len(fam) - 1, room).astype(np.int64))] if room else []
        seen = set(keep) | set(fam)
    out = keep[:budget] + fam
    while len(out) < min(budget, n):
        out += clean(rng.integers(0, n, budget - len(out)), seen)
    return np.array(sorted(out), dtype=np.int64)


def split_head_tail(indices, N, w=W):
    """N < n: which of the indices the head-code reference (p = 0) plants and which the tail-code one (p = N - w); an index both
    reach goes to them in turn.  -> (head indices, tail indices)"""
    head, tail, turn = [], [], 0
    for k in np.asarray(indices, dtype=np.int64):
        h, t = bool(reachable(k, N, 0, w)), bool(reachable(k, N, N - w, w))
        assert h or t
        if h and t:
            (head if turn else tail).append(int(k))
            turn ^= 1
        else:
            (head if h else tail).append(int(k))
    return np.array(head, dtype=np.int64), np.array(tail, dtype=np.int64)


def sweep_cases(N, budget=None, w=W, seed=0, head_off_first=False):
    """the cases that sweep length N: a list of (ref, rows, planted indices).  budget None: every index (one case when N == n; head
    and tail, each with every shift it allows, when N < n); else index_set(N, n, budget) dealt to one or two references.
    head_off_first (N < n, with a budget): a third reference with the code at p = 1 plants the head reference's indices again --
    its first sample is no outlier (row_bounds)."""
    n = fft_len(N)
    out = []
    if budget is None:
        for i, p in enumerate(heads_and_tails(N, w)):
            s = sweep_shifts(N, p, w, seed + i)
            ref, rows, _ = make_case(N, s, p, w, seed + i)
            out.append((ref, rows, (-s) % n))
        return out
    idx = index_set(N, n, budget, w, seed)
    parts = [(N // 3, idx)] if N == n else list(zip((0, N - w), split_head_tail(idx, N, w)))
    if N < n and head_off_first:             # the head reference's indices once more, from a code that starts on sample 1
        parts.append((1, parts[0][1][reachable(parts[0][1], N, 1, w)]))
    for i, (p, ks) in enumerate(parts):
        if len(ks) == 0:
            continue
        s, k = shifts_for(ks, N, p, w, seed + i)
        ref, rows, _ = make_case(N, s, p, w, seed + i)
        out.append((ref, rows, k))
    return out


# ------------------------------------------------------------------ the long-double expectation
def ld_ref(ref, n):
    """xs = zNormalize(ref) / (N - 1) behind its leading zero pad, in long double"""
    x = np.asarray(ref, dtype=np.float64).astype(np.longdouble)
    N = len(x)
    d = x - x.sum() / N
    xs = d / np.sqrt((d * d).sum() / (N - 1)) / (N - 1)
    pad = np.zeros(n, dtype=np.longdouble)
    pad[n - N:] = xs
    return pad


def ld_score_at(ref, y, n, k, xs_pad=None):
    """cc[k] = sum_j yz_pad[j] * xs_pad[(j + k) mod n] for the single index k (oracle_xcorr_direct_ld's definition): yz = zNormalize(y)
    (divisor N - 1), both behind leading zero pads; everything in long double, no FFT.  xs_pad: ld_ref(ref, n) when the caller has it."""
    if xs_pad is None:
        xs_pad = ld_ref(ref, n)
    yl = np.asarray(y, dtype=np.float64).astype(np.longdouble)
    N = len(yl)
    d = yl - yl.sum() / N
    a = (n - N + int(k)) % n                   # padded index of the x sample under y[0]
    first = min(N, n - a)
    acc = (d[:first] * xs_pad[a:a + first]).sum()
    if first < N:
        acc += (d[first:] * xs_pad[:N - first]).sum()
    return acc / np.sqrt((d * d).sum() / (N - 1))   # (1 / sigma_y taken out of the sum: one long-double division, not N)


def ld_scores(ref, rows, n, ks):
    """ld_score_at for row r at index ks[r], as long double"""
    xs_pad = ld_ref(ref, n)
    return np.array([ld_score_at(ref, rows[r], n, ks[r], xs_pad) for r in range(len(ks))], dtype=np.longdouble)


def many_refs_case(N, w=W, seed=0):
    """([head ref, tail ref, middle ref], rows, [their planted indices]): ONE row set -- the code at every position a row allows,
    shuffled -- against three references that carry the same code at p = 0, N - w and N // 2 over different noise: for
    reference i row r's winner is (p_i - q[r]) mod n"""
    n = fft_len(N)
    code = make_code(seed, w)
    q = np.random.default_rng([seed, 4]).permutation(n if N == n else N - w + 1)
    rows = make_rows(N, q, code, seed)
    ps = [0, N - w, N // 2]
    refs = [make_ref(N, p, code, seed + 1 + i) for i, p in enumerate(ps)]
    return refs, rows, [planted_index(p, q, n) for p in ps]
