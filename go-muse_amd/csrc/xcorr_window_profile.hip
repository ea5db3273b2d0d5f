// xcorr_window_profile.hip -- the lag profile (muse_batch_lag_profile): every cc of the lags lo .. hi of a series, written out, not
// scanned: out[k][v] = cc[(lo + v) mod n], v = 0 .. W - 1, W = hi - lo + 1 <= 2 MUSE_LAG_WINDOW_MAX + 1 rows per launch, whether or not
// the lags hold lag 0.
//
// The tables are the band's (launch_window_tables_at with the origin -lo: row v is lag lo + v), and the product, the statistics and
// every cc are xcorr_window_band_mfma's -- the same pieces on the same waves in the same k order, from the functions of
// window_device.h -- so the value at a lag has the bits the band, range and signed passes scan at that lag (a row's sum does not
// depend on which row of which tile it is, xcorr_window_band.hip), whatever band it was asked in and wherever the planner cut.
//
// The epilogue replaces the scan.  The summed tiles lie in LDS as [row v][16 series] (v 16 + c doubles).  Thread t takes series
// c = t >> 4 and the rows v = (t & 15), (t & 15) + 16, ... below W: a wave stores four series' runs of 16 consecutive doubles (128
// bytes each) per step.  Its LDS reads then go across the rows: the dword bank of (v, c) is (32 v + 2 c) mod 64, so the 32 lanes of a
// ds_read_b64 group -- 16 rows of 2 series -- fall on 4 bank pairs, an 8-way conflict: 16 LDS cycles per wave instruction where 2
// would do, at most TILES such reads per thread, 64 TILES LDS cycles per workgroup against 16 TILES ceil(N / 64) matrix instructions.
// The layout is window_sum_tiles' own and stays.  (The loop over v is a loop, not TILES unrolled steps: unrolled, the 5-tile
// 8-byte build and the 7-tile 16-byte build took two registers more than xcorr_window_band_mfma's and lost a wave per SIMD.)
//
// LISTED: series r of the workgroup is series[blockIdx.x 16 + r] (an int64 list in device memory, any order, duplicates allowed,
// checked by the host) and output row k belongs to list entry k; otherwise output row k is row k of p.rows.
#include "window_device.h"

namespace muse {

template <int TILES, bool WIDE, bool LISTED>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_profile_mfma(const WindowProfileParams p)
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
    if (LISTED)
        row = p.series[row];
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
    constexpr int STAT = WindowLds<TILES>::STAT;
    window_sum_tiles<TILES>(lds, STAT, acc, s1, s2, wave, r, q);

    // the write-out: series c of the workgroup, rows vl, vl + 16, ... of the table; window_outcome's rules for a row of NaN / sigma == 0
    const int c = t >> 4;
    if (row0 + c >= p.M)
        return;
    const WindowStats st = window_stats(window_wave_sum(lds, STAT, 2 * c), window_wave_sum(lds, STAT, 2 * c + 1), p.invN, p.invNm1);
    double *__restrict__ o = p.out + (row0 + c) * p.out_stride;
    for (int v = t & 15; v < p.W; v += 16)
        o[v] = st.nan ? __builtin_nan("") : st.zero ? 0.0 : window_score(lds, 0, v, c, st, p.pw);
}

hipError_t launch_window_profile(const WindowProfileParams &p, hipStream_t stream)
{
    if (p.W < 1 || p.W > 2 * MUSE_LAG_WINDOW_MAX + 1 || p.N < 2 || p.out_stride < p.W || p.M < 0)
        return hipErrorInvalidValue;
    if (p.M == 0)
        return hipSuccess;
    const long long blocks = (p.M + 15) / 16;
    if (blocks > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    window_with_tiles((p.W + 15) / 16, [&](auto tiles) {
        with_bools([&](auto wide, auto listed) {
            xcorr_window_profile_mfma<decltype(tiles)::value, decltype(wide)::value, decltype(listed)::value><<<grid, block, 0, stream>>>(p);
        }, window_wide(p.rows, p.stride), p.series != nullptr);
    });
    return hipGetLastError();
}

// the planner, a pure host function: lags lo .. hi cut into consecutive launches of up to 2 MUSE_LAG_WINDOW_MAX + 1 table rows, the
// last one taking what is left; lo_of / rows_of: each launch's first lag and its rows (filled up to cap entries).  The launch count.
int window_profile_plan(int lo, int hi, int *lo_of, int *rows_of, int cap)
{
    constexpr int ROWS = 2 * MUSE_LAG_WINDOW_MAX + 1;
    const long long W = (long long)hi - lo + 1;
    const int launches = (int)((W + ROWS - 1) / ROWS);
    for (int j = 0; j < launches && j < cap; j++) {
        if (lo_of)
            lo_of[j] = lo + j * ROWS;
        if (rows_of)
            rows_of[j] = (int)std::min<long long>(ROWS, W - (long long)j * ROWS);
    }
    return launches;
}

} // namespace muse
