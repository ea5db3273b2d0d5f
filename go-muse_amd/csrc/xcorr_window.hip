// xcorr_window.hip -- the lag-window pass (muse_batch_set_lag_window): the best match INSIDE +-L lags, computed directly.
//
// For a window of L lags no transform is needed: with e[v] = xp[(pad + v - L) mod n] (xp = the batch's padded time-domain
// reference, FusedParams::xs; pad = n - N) the correlation slice of xCorrWithX (xcorr.go:160-187) at lag v - L is
//     cc[v] = (S[v] - mean(d) P[v]) / sigma(d),   S[v] = sum_t d[t] e[t + v],   P[v] = sum_t e[t + v],   t = 0 .. N-1,
// d = y - y[0] (the shift every kernel here uses against cancellation).  S is a (2L+1 x N) by (N x M) matrix product between
// shifted copies of the reference and the rows as they lie in HBM: one pass over the rows, any N, on the fp64 matrix pipe
// (v_mfma_f64_16x16x4_f64: lags on the 16 A rows, 16 series on the B columns); mean and sigma come out of the same pass on
// the vector unit.
//
// One 256-thread workgroup scores 16 series.  The samples are cut into chunks of WIN_KC; per chunk the workgroup stages
// e[T0 .. T0 + WIN_KC + 2 L_max) in LDS and its four waves take the chunk's 64-sample pieces in turn (K split across the
// waves).  In a piece, lane (r = lane & 15, q = lane >> 4) loads sample T + 4 m + q of row r for m = 0 .. 15 (B[k = q][col r] of
// k-step m: per load instruction 16 rows x 32 contiguous bytes, four consecutive instructions use a 128-byte line up) and reads
// A[row r][k = q] = e[T + 4 m + q + 16 tile + r] from the LDS image (consecutive doubles: no bank conflict).  Rows that are
// 16-byte aligned (even stride) take the WIDE build: the k order inside a piece is free as long as A follows it, so a lane
// loads two consecutive samples at once (16 rows x 64 contiguous bytes per instruction, half the load instructions).  The four waves'
// accumulator tiles are summed through LDS in wave order (deterministic), then 16 threads per series scan the window in the
// order of the definition -- lags 0, 1 .. L, then -L .. -1, strict '>', first index wins (xcorr.go:39-50) -- and are merged
// in that order.
#include "window_device.h"

namespace muse {

// e[v], v < len: the reference at padded index (pad + v - origin) mod n for v < N + W - 1 (row v of the W rows of the product is lag
// v - origin; the symmetric window: origin = L, W = 2 L + 1), zero behind (the last chunk reads on)
__global__ __launch_bounds__(256) void window_table_e(const double *__restrict__ xs, int N, int n, int origin, int W, long long len,
                                                      double *__restrict__ e)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= len)
        return;
    double x = 0.0;
    if (v < (long long)N + W - 1) {
        long long idx = ((long long)(n - N) + v - origin) % n;
        if (idx < 0)
            idx += n;
        x = xs[idx];
    }
    e[v] = x;
}

// pw[v] = sum_t e[t + v], t < N: one workgroup per v, fixed summation order
__global__ __launch_bounds__(256) void window_table_p(const double *__restrict__ e, int N, double *__restrict__ pw)
{
    __shared__ double part[256];
    const int v = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < N; i += 256)
        s += e[i + v];
    part[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0)
        pw[v] = part[0];
}

// the two launches for a table of 1 <= W <= 2 MUSE_LAG_WINDOW_MAX + 1 rows at ANY integer origin (window_table_e takes the index mod n):
// the callers below and launch_window_tables_band (xcorr_window_band.hip: a negative origin or one beyond the rows) check theirs
hipError_t launch_window_tables_at(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw, hipStream_t stream)
{
    if (W < 1 || W > 2 * MUSE_LAG_WINDOW_MAX + 1) // (pw holds 2 MUSE_LAG_WINDOW_MAX + 1 sums, a chunk's image WIN_E_TAIL more samples)
        return hipErrorInvalidValue;
    window_table_e<<<dim3((unsigned)((e_len + 255) / 256)), dim3(256), 0, stream>>>(xs, N, n, origin, W, e_len, e);
    window_table_p<<<dim3((unsigned)W), dim3(256), 0, stream>>>(e, N, pw);
    return hipGetLastError();
}

hipError_t launch_window_tables(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw, hipStream_t stream)
{
    if (origin < 0 || W < origin + 1) // (a table that holds lag 0: a band's is launch_window_tables_band's)
        return hipErrorInvalidValue;
    return launch_window_tables_at(xs, N, n, origin, W, e, e_len, pw, stream);
}

template <int TILES, bool WIDE>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_mfma(const WindowParams p)
{
    __shared__ double lds[WindowLds<TILES>::SIZE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); nothing of them is written
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];

    v4d acc[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0, s2 = 0.0;

    // This loop is written out -- the staging, the piece's loads and the k-loop that the other kernels take from window_device.h
    // (window_stage_e, window_load_piece, window_mac_piece; the same expressions, on the same window_k / window_a).  Through
    // those functions the 4- and 8-tile builds of this kernel measured 2 ... 3 % slower, with the k-loop alone written out still
    // 2.5 %: profiles/window_refactor.txt.  A change to the mapping or to the k-loop is made here as well.
    for (int T0 = 0; T0 < N; T0 += WIN_KC) {
        if (T0 > 0)
            __syncthreads();
        for (int v = t; v < WIN_ELDS; v += WIN_THREADS) // (the table is padded with zeros to whole chunks)
            lds[v] = p.e[T0 + v];
        __syncthreads();
        for (int s = wave; s < WIN_KC / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            // WIDE: k-step m = 2 mp + h <-> sample T + 8 mp + 2 q + h (one 16-byte load per two k-steps: 16 rows x 64 contiguous
            // bytes per instruction); else k-step m <-> sample T + 4 m + q (8-byte loads: rows of any alignment)
            double d[16];
            if (WIDE && T + 64 <= N) {
#pragma unroll
                for (int mp = 0; mp < 8; mp++) {
                    const double2 v = *reinterpret_cast<const double2 *>(y + T + window_a<true>(2 * mp) + window_k<true>(0, q));
                    d[2 * mp] = v.x - y0;
                    d[2 * mp + 1] = v.y - y0;
                }
            } else if (T + 64 <= N) {
#pragma unroll
                for (int m = 0; m < 16; m++)
                    d[m] = y[T + window_k<false>(m, q)] - y0;
            } else {
#pragma unroll
                for (int m = 0; m < 16; m++) {
                    const int tt = T + window_k<WIDE>(m, q);
                    d[m] = tt < N ? y[tt] - y0 : 0.0;
                }
            }
            const double *a = lds + 64 * s + window_k<WIDE>(0, q) + r;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                s1 += d[m];
                s2 = fma(d[m], d[m], s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[window_a<WIDE>(m) + 16 * i], d[m], acc[i], 0, 0, 0);
            }
        }
    }
    window_finish<TILES>(lds, acc, s1, s2, p, row0, t, wave, r, q);
}

hipError_t launch_window(const WindowParams &p, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    if (window_launch_check(p, &blocks) != hipSuccess)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
    window_with_tiles(window_tiles(p), [&](auto tiles) {
        if (wide)
            xcorr_window_mfma<tiles(), true><<<grid, block, 0, stream>>>(p);
        else
            xcorr_window_mfma<tiles(), false><<<grid, block, 0, stream>>>(p);
    });
    return hipGetLastError();
}

// The signed best match (muse_batch_score_signed_in_lag_range): the product of xcorr_window_mfma -- the same pieces on the same waves
// in the same order, from the functions of window_device.h, so S, the statistics and every cc are its bits -- with the scan's key val
// (SGN = +1) or -val (SGN = -1) in place of |val| (window_key).  A kernel of its own: xcorr_window_mfma and its symbols stay as they are.
template <int TILES, bool WIDE, int SGN>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_signed_mfma(const WindowParams p)
{
    static_assert(SGN == 1 || SGN == -1, "the unsigned scan is xcorr_window_mfma's");
    __shared__ double lds[WindowLds<TILES>::SIZE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); nothing of them is written
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];

    v4d acc[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = 0; T0 < N; T0 += WIN_KC) {
        if (T0 > 0)
            __syncthreads();
        window_stage_e(lds, p.e + T0, t);
        __syncthreads();
        for (int s = wave; s < WIN_KC / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            double d[16];
            window_load_piece<WIDE>(d, y, y0, T, N, q);
            window_mac_piece<TILES, WIDE>(acc, s1, s2, [&](int m) { return d[m]; }, lds, s, r, q);
        }
    }
    window_finish<TILES, SGN>(lds, acc, s1, s2, p, row0, t, wave, r, q);
}

hipError_t launch_window_signed(const WindowParams &p, int sign, hipStream_t stream)
{
    if (sign == 0)
        return launch_window(p, stream);
    if (sign != 1 && sign != -1)
        return hipErrorInvalidValue;
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    if (window_launch_check(p, &blocks) != hipSuccess)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    window_with_tiles(window_tiles(p), [&](auto tiles) {
        with_bools([&](auto wide, auto neg) {
            xcorr_window_signed_mfma<decltype(tiles)::value, decltype(wide)::value, decltype(neg)::value ? -1 : 1><<<grid, block, 0, stream>>>(p);
        }, window_wide(p.rows, p.stride), sign < 0);
    });
    return hipGetLastError();
}

} // namespace muse
