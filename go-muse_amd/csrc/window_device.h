// window_device.h -- what the single-reference lag-window kernels share (xcorr_window.hip: xcorr_window_mfma; xcorr_window_slide.hip:
// xcorr_window_slide_mfma): the LDS layout of a workgroup and everything behind the product -- the statistics, the four waves'
// accumulator tiles summed through LDS in wave order, the scan of the window and the write-out.  Used verbatim by both kernels, so
// that the same rows give the same bits whichever of them scored them.
#pragma once
#include "xcorr_kernels.h"

namespace muse {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int WIN_THREADS = 256;
static_assert(2 * MUSE_LAG_WINDOW_MAX + 1 <= 8 * 16, "at most eight accumulator tiles of 16 lags");
constexpr int WIN_ELDS = WIN_KC + WIN_E_TAIL; // doubles of e staged per chunk

template <int TILES> struct WindowLds {
    static constexpr int RED = TILES * 256;                     // the summed accumulator tiles: [tile][lag row][series]
    static constexpr int BUF = WIN_ELDS > RED ? WIN_ELDS : RED; // (the e image is dead when the tiles are summed: one region)
    static constexpr int STAT = BUF;                            // [4 waves][16 series][2]
    static constexpr int CAND = STAT + 128;                     // [16 parts][16 series][3]
    static constexpr int SIZE = CAND + 16 * 16 * 3;
};

// acc: the wave's share of S (its pieces of every chunk); s1 / s2: the lane's share of sum d and sum d^2.  Every thread of the
// workgroup calls it, behind its last piece; row0: the workgroup's first series; t = threadIdx.x, wave = t >> 6 (uniform), lane
// (r, q) = (t & 15, (t & 63) >> 4) as in the kernels.
template <int TILES>
__device__ __forceinline__ void window_finish(double *lds, const v4d (&acc)[TILES], double s1, double s2, const WindowParams &p,
                                              const long long row0, const int t, const int wave, const int r, const int q)
{
    constexpr int STAT = WindowLds<TILES>::STAT;
    constexpr int CAND = WindowLds<TILES>::CAND;
    // statistics: the four k-lanes of a series, then (below) the four waves
    s1 += __shfl_xor(s1, 16);
    s2 += __shfl_xor(s2, 16);
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 32);
    if (q == 0) {
        lds[STAT + wave * 32 + 2 * r] = s1;
        lds[STAT + wave * 32 + 2 * r + 1] = s2;
    }
    __syncthreads(); // every wave is done with the e image
    // C/D of v_mfma_f64_16x16x4_f64: register j of lane (r, q) = [row q + 4 j][column r]
    for (int w = 0; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < TILES; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int at = i * 256 + (q + 4 * j) * 16 + r;
                    lds[at] = w == 0 ? acc[i][j] : lds[at] + acc[i][j];
                }
        }
        __syncthreads();
    }

    // the windowed maxAbsIndex: scan position pos = 0 .. W-1 <-> lag 0 .. L, -Lneg .. -1
    const int c = t & 15, part = t >> 4;
    const int L = p.L, Lneg = p.Lneg, W = L + 1 + Lneg;
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        t1 += lds[STAT + w * 32 + 2 * c];
        t2 += lds[STAT + w * 32 + 2 * c + 1];
    }
    const double var = (t2 - t1 * t1 * p.invN) * p.invNm1;
    const bool nan = !__builtin_isfinite(var);
    const bool zero = !nan && !(var > 0.0);
    const double mean = t1 * p.invN;
    const double inv_sigma = 1.0 / sqrt(var);
    double best_abs = 0.0, best_val = 0.0, best_pos = -1.0;
#pragma unroll
    for (int k = 0; k < TILES; k++) {
        const int pos = part * TILES + k;
        if (pos < W) {
            const int v = pos <= L ? pos + L : pos - 1 - Lneg; // lag + L
            const double S = lds[(v >> 4) * 256 + (v & 15) * 16 + c];
            const double val = (S - mean * p.pw[v]) * inv_sigma;
            if (fabs(val) > best_abs) {
                best_abs = fabs(val);
                best_val = val;
                best_pos = (double)pos;
            }
        }
    }
    lds[CAND + (part * 16 + c) * 3] = best_abs;
    lds[CAND + (part * 16 + c) * 3 + 1] = best_val;
    lds[CAND + (part * 16 + c) * 3 + 2] = best_pos;
    __syncthreads();
    if (t < 16 && row0 + t < p.M) {
        double ba = 0.0, bv = 0.0;
        int bp = -1;
        for (int k = 0; k < 16; k++) {
            const double a = lds[CAND + (k * 16 + c) * 3];
            if (a > ba) {
                ba = a;
                bv = lds[CAND + (k * 16 + c) * 3 + 1];
                bp = (int)lds[CAND + (k * 16 + c) * 3 + 2];
            }
        }
        int lag = 0;
        double mv;
        if (nan) {
            mv = __builtin_nan("");
        } else if (zero) {
            mv = 0.0; // sigma == 0: (nil, 0, 0), xcorr.go:165-168
        } else if (bp < 0) { // only zeros or NaN in the window: index 0 stands
            mv = (lds[(L >> 4) * 256 + (L & 15) * 16 + c] - mean * p.pw[L]) * inv_sigma;
        } else {
            mv = bv;
            lag = bp <= L ? bp : bp - 1 - Lneg - L;
        }
        p.mv[row0 + t] = mv;
        p.lag[row0 + t] = lag;
    }
}

} // namespace muse
