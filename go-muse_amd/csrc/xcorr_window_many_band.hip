// xcorr_window_many_band.hip -- the packed lag-window pass for MANY references under a sign or over a lag band
// (muse_batch_score_many_in_lag_band): xcorr_window_many.hip's product -- one read of the rows, the table rows of all references of a
// launch packed into the accumulator tiles of one matrix product -- with the scan and the outcome of the signed and the band kernels
// (xcorr_window_signed_mfma, xcorr_window_band_mfma; window_device.h: window_scan_pos<SGN, BAND>, window_outcome<SGN, BAND>).
//
// A kernel of its own, so that xcorr_window_many_mfma keeps its symbols and its code.  The body is that kernel's: the staged images
// `img` doubles apart, a lane's A offset of tile i from (packed row) / W, the k-loop written out on the same mapping, the waves'
// tiles summed by window_sum_tiles, the scan of a reference cut into `parts`.  A band lo .. hi has the shape origin = Lneg = -lo,
// L = hi, so W = origin + L + 1 = hi - lo + 1 is the rows of its table and L + 1 + Lneg its scan positions, as for every window: the
// planner, the image stride and the bank argument of xcorr_window_many.hip's header hold for it unchanged (they ask nothing of W
// but its value), and so does the LDS layout.
//
// Bit-identity with the single kernels: an accumulator element sees the same A and B values in the same k slots of the same k-steps
// in the same order (as argued in xcorr_window_many.hip), the statistics, the score of a position, the key and the outcome are the
// single kernels' functions, and how the scan is cut into parts is invisible to strict '>' with the first position winning.  So a
// batch's packed result has the bits of its own muse_batch_score_in_lag_band / _score_signed_in_lag_range.
#include "window_device.h"

namespace muse {

constexpr int WINMB_STAGE = 3; // image samples per thread and reference in one batch of staging loads (xcorr_window_many.hip's)

template <int TILES, bool WIDE, int SGN, bool BAND>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_many_signed_mfma(const WindowManyParams p)
{
    static_assert(SGN >= -1 && SGN <= 1, "the key of the scan: |val|, val or -val");
    static_assert(SGN != 0 || BAND, "by magnitude inside a window that holds lag 0: xcorr_window_many_mfma");
    // [max(R img, TILES 256)] the e images, then the summed tiles [tile][row][series] | [4 waves][16 series][2] | [R parts][16 series][3]
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N, R = p.R, L = p.L, Lneg = p.Lneg, origin = p.origin, Wv = origin + L + 1, kc = p.kc, img = p.img, elen = kc + Wv - 1;
    const int STAT = p.buf, CAND = STAT + 128;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); nothing of them is written
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];

    v4d acc[TILES];
    int aoff[TILES]; // this lane's A row of tile i: image base of its reference + table row + the lane's k slot
#pragma unroll
    for (int i = 0; i < TILES; i++) {
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
        int rr = 16 * i + r;
        if (rr >= R * Wv) // the empty rows behind the last reference compute the last row again (one LDS address: a broadcast); nothing of them is read
            rr = R * Wv - 1;
        const int ref = rr / Wv;
        aoff[i] = ref * img + (rr - ref * Wv) + window_k<WIDE>(0, q);
    }
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = 0; T0 < N; T0 += kc) {
        if (T0 > 0)
            __syncthreads();
        // (the tables are padded with zeros to whole chunks of WIN_KC, which kc divides; four references' loads in flight together)
        for (int ref0 = 0; ref0 < R; ref0 += 4) {
            const double *__restrict__ e[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                e[u] = p.e[ref0 + u < R ? ref0 + u : ref0] + T0;
            for (int v0 = t; v0 < elen; v0 += WINMB_STAGE * WIN_THREADS) {
                double x[4][WINMB_STAGE];
#pragma unroll
                for (int j = 0; j < WINMB_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS < elen ? v0 + j * WIN_THREADS : v0;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        x[u][j] = e[u][v];
                }
#pragma unroll
                for (int j = 0; j < WINMB_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (v < elen && ref0 + u < R)
                            lds[(ref0 + u) * img + v] = x[u][j];
                }
            }
        }
        __syncthreads();
        for (int s = wave; s < kc / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            double d[16];
            window_load_piece<WIDE>(d, y, y0, T, N, q);
            // (the k-loop of window_mac_piece, written out as in xcorr_window_many_mfma)
            const double *a = lds + 64 * s;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                s1 += d[m];
                s2 = fma(d[m], d[m], s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[window_a<WIDE>(m) + aoff[i]], d[m], acc[i], 0, 0, 0);
            }
        }
    }
    window_sum_tiles<TILES>(lds, STAT, acc, s1, s2, wave, r, q);

    // the scan per (series, reference) under the sign / over the band: the positions of a reference cut into `parts` consecutive parts
    // of `plen` positions, one (reference, part) item per 16 threads at a time
    const int c = t & 15;
    const int parts = p.parts, plen = (L + 1 + Lneg + parts - 1) / parts;
    const WindowStats st = window_stats(window_wave_sum(lds, STAT, 2 * c), window_wave_sum(lds, STAT, 2 * c + 1), p.invN, p.invNm1);
    for (int item = t >> 4; item < R * parts; item += 16) {
        const int ref = item / parts, part = item - ref * parts;
        const double *__restrict__ pw = p.pw[ref];
        WindowBest best;
        for (int k = 0; k < plen; k++)
            window_scan_pos<SGN, BAND>(best, lds, ref * Wv, part * plen + k, c, L, Lneg, origin, st, pw);
        window_put_best(lds + CAND + (item * 16 + c) * 3, best);
    }
    __syncthreads();
    if (row0 + c < p.M) {
        for (int ref = t >> 4; ref < R; ref += 16) {
            int lag;
            p.mv[ref][row0 + c] = window_outcome<SGN, BAND>(lds, CAND, ref * parts, parts, ref * Wv, c, L, Lneg, origin, st, p.pw[ref], &lag);
            p.lag[ref][row0 + c] = lag;
        }
    }
}

// sign = 0 / +1 / -1; the shape says whether it is a band (one of L, Lneg negative).  sign == 0 over a window that holds lag 0 is
// launch_window_many.  The launch is sized by xcorr_window_many.hip's planner, as that launcher sizes its own.
hipError_t launch_window_many_signed(WindowManyParams p, int sign, hipStream_t stream)
{
    if (sign < -1 || sign > 1)
        return hipErrorInvalidValue;
    const bool band = p.L < 0 || p.Lneg < 0;
    if (sign == 0 && !band)
        return launch_window_many(p, stream);
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    const int W = p.origin + p.L + 1;
    if ((band ? window_launch_check_band(p, &blocks) : window_launch_check(p, &blocks)) != hipSuccess || W < 1 || p.R < 1 ||
        p.R > window_many_max_refs(W))
        return hipErrorInvalidValue;
    const int tiles = (p.R * W + 15) / 16;
    p.kc = window_many_kc(W, p.R);
    p.img = window_many_img(W, p.kc);
    p.buf = std::max(p.R * p.img, tiles * 256);
    p.parts = std::max(1, 16 / p.R);
    const size_t lds_bytes = (size_t)(p.buf + 128 + p.R * p.parts * 16 * 3) * sizeof(double);
    if (tiles > WINM_MAX_TILES || lds_bytes > 64 * 1024)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    window_with_tiles(tiles, [&](auto T) {
        with_bools([&](auto wide, auto bnd) {
            with_sign(sign, [&](auto sgn) {
                if constexpr (decltype(sgn)::value != 0 || decltype(bnd)::value)
                    xcorr_window_many_signed_mfma<decltype(T)::value, decltype(wide)::value, decltype(sgn)::value, decltype(bnd)::value>
                        <<<grid, block, lds_bytes, stream>>>(p);
            });
        }, window_wide(p.rows, p.stride), band);
    });
    return hipGetLastError();
}

} // namespace muse
