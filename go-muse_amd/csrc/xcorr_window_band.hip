// xcorr_window_band.hip -- the direct product over a lag band (muse_batch_score_in_lag_band): the best match inside lags lo .. hi that
// do NOT hold lag 0 -- 0 < lo <= hi, "which series lead the reference by lo .. hi samples", or lo <= hi < 0 -- from a table whose
// row v is lag lo + v: W = hi - lo + 1 <= 2 MUSE_LAG_WINDOW_MAX + 1 rows, ceil(W / 16) accumulator tiles, wherever the band lies.
//
// The tables are xcorr_window.hip's (window_table_e / window_table_p) with the origin -lo: e[v] = xs[(n - N + v + lo) mod n], so that
// S[v] = sum_t d[t] e[t + v] is the correlation at lag lo + v.  The product, the statistics and every cc are xcorr_window_signed_mfma's
// -- the same pieces on the same waves in the same k order, from the functions of window_device.h -- so a lag's cc has the bits the
// direct product of a range gives at that lag when its table puts the lag on the same row arithmetic (the same e values in the same
// order: a row's sum does not depend on which row of which tile it is).  The scan is the band's own (window_device.h, BAND): row by
// row in ascending cc index, strict '>', first index wins, key |val| / val / -val for SGN = 0 / +1 / -1, and (lag 0, +0.0) where
// nothing wins -- index 0 is not in the band.
#include "window_device.h"

namespace muse {

template <int TILES, bool WIDE, int SGN>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_band_mfma(const WindowParams p)
{
    static_assert(SGN >= -1 && SGN <= 1, "the key of the scan: |val|, val or -val");
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
    window_finish<TILES, SGN, true>(lds, acc, s1, s2, p, row0, t, wave, r, q);
}

// the tables of a band lo .. lo + W - 1 at FFT length n: launch_window_tables with the origin -lo (row v is lag lo + v)
hipError_t launch_window_tables_band(const double *xs, int N, int n, int lo, int W, double *e, long long e_len, double *pw, hipStream_t stream)
{
    const long long hi = (long long)lo + W - 1;
    // lag 0 outside, every lag inside -(n / 2 - 1) .. n / 2; pw holds 2 MUSE_LAG_WINDOW_MAX + 1 sums, a chunk's image WIN_E_TAIL more samples
    if (W < 1 || W > 2 * MUSE_LAG_WINDOW_MAX + 1 || (lo <= 0 && hi >= 0) || lo < -(n / 2 - 1) || hi > n / 2 || e_len < window_e_len(N))
        return hipErrorInvalidValue;
    return launch_window_tables_at(xs, N, n, -lo, W, e, e_len, pw, stream);
}

hipError_t launch_window_band(const WindowParams &p, int sign, hipStream_t stream)
{
    if (sign < -1 || sign > 1)
        return hipErrorInvalidValue;
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    if (window_launch_check_band(p, &blocks) != hipSuccess)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    window_with_tiles((p.L + p.Lneg + 1 + 15) / 16, [&](auto tiles) {
        with_bools([&](auto wide) {
            with_sign(sign, [&](auto sgn) {
                xcorr_window_band_mfma<decltype(tiles)::value, decltype(wide)::value, decltype(sgn)::value><<<grid, block, 0, stream>>>(p);
            });
        }, window_wide(p.rows, p.stride));
    });
    return hipGetLastError();
}

} // namespace muse
