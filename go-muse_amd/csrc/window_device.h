// window_device.h -- the one home of what the four lag-window kernels share (xcorr_window.hip: xcorr_window_mfma;
// xcorr_window_slide.hip: xcorr_window_slide_mfma; xcorr_window_split.hip: xcorr_window_split_partial / window_split_finish;
// xcorr_window_many.hip: xcorr_window_many_mfma): the lane -> sample mapping of a 64-sample piece, the load of a piece, its k-loop on
// the matrix pipe, the staging of the e image, the four waves' accumulator tiles summed through LDS in wave order, the pieces of the
// scan of the window with its outcome rules, and the launch checks.  The kernels call these functions, so the same rows give the same
// bits whichever of them scored them.  The exceptions, all measured (see window_mac_piece): xcorr_window_mfma keeps its loop over the
// pieces written out (staging, loads, k-loop), xcorr_window_many_mfma and xcorr_window_slide_mfma the k-loop alone; all of them on
// window_k / window_a, so the mapping itself is spelled here only.
#pragma once
#include "xcorr_kernels.h"

#include <type_traits>

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

// ---- the mapping.  Lane (r, q) = (lane & 15, lane >> 4) of a wave holds series r on k-lane q.  In the piece that starts at sample T,
// k-step m of k-lane q is sample T + window_k(m, q).  WIDE (rows 16-byte aligned): k-step m = 2 mp + h <-> sample 8 mp + 2 q + h, two
// consecutive samples per lane (one 16-byte load per two k-steps: 16 rows x 64 contiguous bytes per instruction); else k-step m <->
// sample 4 m + q (8-byte loads: rows of any alignment).  The A operand follows it: e[T + window_k(m, q) + lag row].
template <bool WIDE> __device__ __forceinline__ constexpr int window_k(int m, int q)
{
    return WIDE ? 8 * (m >> 1) + 2 * q + (m & 1) : 4 * m + q;
}
// window_k is a sum of an m part and a q part: a lane forms image + 64 piece + window_k(0, q) + (its lag row) once and reads the A operand
// of k-step m at window_a(m) behind it
template <bool WIDE> __device__ __forceinline__ constexpr int window_a(int m) { return window_k<WIDE>(m, 0); }

// ---- one piece of row y, whole or partial, as d = y - y0 in k-step order: 16-byte loads, 8-byte loads, or the masked tail (0.0 behind N)
template <bool WIDE>
__device__ __forceinline__ void window_load_piece(double (&d)[16], const double *y, const double y0, const int T, const int N,
                                                  const int q)
{
    const double *yp = y + T + window_k<WIDE>(0, q); // the lane's k slot of the piece: k-step m at yp[window_a(m)]
    if (WIDE && T + 64 <= N) {
#pragma unroll
        for (int mp = 0; mp < 8; mp++) {
            const double2 v = *reinterpret_cast<const double2 *>(yp + window_a<true>(2 * mp));
            d[2 * mp] = v.x - y0;
            d[2 * mp + 1] = v.y - y0;
        }
    } else if (T + 64 <= N) {
#pragma unroll
        for (int m = 0; m < 16; m++)
            d[m] = yp[window_a<WIDE>(m)] - y0;
    } else {
#pragma unroll
        for (int m = 0; m < 16; m++)
            d[m] = T + window_k<WIDE>(m, q) < N ? yp[window_a<WIDE>(m)] - y0 : 0.0;
    }
}

// ---- a piece's 16 k-steps: the lane's share of sum d and sum d^2, and TILES products on v_mfma_f64_16x16x4_f64 (lags on the 16 A
// rows, 16 series on the B columns).  d_of(m): d of k-step m (an array filled by window_load_piece, or formed from the raw sample
// at use).  The lane's A operand of tile i is lds[a + window_a(m) + tile_off[i]]: a = the piece in the staged
// image(s) (+ window_k(0, q) + r with one reference), tile_off[i] = what selects the lane's row of tile i (one reference: 16 i).
// (lds and an index, not a pointer into it: the compiler then addresses LDS as it does from the kernel's own body.)
// Used by xcorr_window_split_partial.  xcorr_window_mfma, xcorr_window_many_mfma and xcorr_window_slide_mfma keep this loop in
// their own bodies: through this function the 4- and 8-tile builds of the first two ran 2 ... 3 % slower than before (the compiler
// spreads the accumulator copies through the MFMA run) and four shapes of the slide kernel 1 ... 2 %; xcorr_window_mfma was still
// 2.5 % slower with the loop alone written out, so that kernel keeps its loads and staging too (profiles/window_refactor.txt).
// A change to the loop is made in those four places.
template <int TILES, bool WIDE, class D>
__device__ __forceinline__ void window_mac_piece(v4d (&acc)[TILES], double &s1, double &s2, const D d_of, const double *lds, const int a,
                                                 const int (&tile_off)[TILES])
{
#pragma unroll
    for (int m = 0; m < 16; m++) {
        const double d = d_of(m);
        s1 += d;
        s2 = fma(d, d, s2);
#pragma unroll
        for (int i = 0; i < TILES; i++)
            acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(lds[a + window_a<WIDE>(m) + tile_off[i]], d, acc[i], 0, 0, 0);
    }
}
// one reference: piece s of the chunk's image, tile i = lags 16 i .. 16 i + 15 of it
template <int TILES, bool WIDE, class D>
__device__ __forceinline__ void window_mac_piece(v4d (&acc)[TILES], double &s1, double &s2, const D d_of, const double *lds, const int s,
                                                 const int r, const int q)
{
    int tile_off[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        tile_off[i] = 16 * i;
    window_mac_piece<TILES, WIDE>(acc, s1, s2, d_of, lds, 64 * s + window_k<WIDE>(0, q) + r, tile_off);
}

// ---- a chunk's image of ONE reference: e[0 .. WIN_ELDS) into lds (the table is padded with zeros to whole chunks); barriers are the caller's
__device__ __forceinline__ void window_stage_e(double *lds, const double *__restrict__ e, const int t)
{
    for (int v = t; v < WIN_ELDS; v += WIN_THREADS)
        lds[v] = e[v];
}

// ---- behind the last piece, every thread of the workgroup: the statistics of the four k-lanes of a series into lds[STAT ..) per wave
// ([4 waves][16 series][2]), then the four waves' accumulator tiles summed into lds[0 .. TILES 256) in wave order (deterministic).
// t = threadIdx.x, wave = t >> 6 (uniform), lane (r, q) as above.  Ends behind a barrier: the sums are there for every thread.
template <int TILES>
__device__ __forceinline__ void window_sum_tiles(double *lds, const int STAT, const v4d (&acc)[TILES], double s1, double s2, const int wave,
                                                 const int r, const int q)
{
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
}
// entry i of [16 series][2] summed over the four waves, in wave order
__device__ __forceinline__ double window_wave_sum(const double *lds, const int STAT, const int i)
{
    double u = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++)
        u += lds[STAT + w * 32 + i];
    return u;
}

// ---- the pieces of the scan: the windowed maxAbsIndex in the order of the definition, scan position pos = 0 .. W-1 <-> lag 0 .. L,
// -Lneg .. -1, strict '>', first index wins (xcorr.go:39-50).  How the positions are cut into parts is each kernel's own: strict '>'
// with the first index winning cannot see the cut.  Row v of the summed tiles and of pw is lag v - origin (WindowShape::origin: L for
// a symmetric window, Lneg for a lag range whose table starts at its lowest lag); L and Lneg are independent of each other.
struct WindowStats {
    double mean, inv_sigma;
    bool nan, zero;
};
__device__ __forceinline__ WindowStats window_stats(const double t1, const double t2, const double invN, const double invNm1)
{
    const double var = (t2 - t1 * t1 * invN) * invNm1;
    const bool nan = !__builtin_isfinite(var);
    return WindowStats{t1 * invN, 1.0 / sqrt(var), nan, !nan && !(var > 0.0)};
}
// cc at window row v (= lag + origin) of series c; row0: the first of the reference's rows in the summed tiles (one reference: 0)
__device__ __forceinline__ double window_score(const double *lds, const int row0, const int v, const int c, const WindowStats &st,
                                               const double *__restrict__ pw)
{
    const int rr = row0 + v;
    return (lds[(rr >> 4) * 256 + (rr & 15) * 16 + c] - st.mean * pw[v]) * st.inv_sigma;
}
struct WindowBest { // (pos as a double: the candidates lie in LDS as three doubles)
    double abs = 0.0, val = 0.0, pos = -1.0;
};
// SGN (muse_batch_score_signed_in_lag_range; xcorr_window_signed_mfma alone): the key of the scan is |val| (0, what every other
// kernel takes), val (+1: the best positive value) or -val (-1: the best negative one).  A key is compared with strict '>' against
// 0.0 first, so a value of the other sign, a zero and a NaN never win; the candidates' merge compares keys as they are.
template <int SGN> __device__ __forceinline__ double window_key(const double val) { return SGN == 0 ? fabs(val) : SGN > 0 ? val : -val; }
// BAND (muse_batch_score_in_lag_band; xcorr_window_band_mfma alone): the lags lo .. hi do not hold lag 0, origin = Lneg = -lo, L = hi
// (one of L, Lneg is negative; W = L + 1 + Lneg as ever).  The scan runs over the cc indices of the band in ascending order, which is
// the table's own: position pos is row pos, lag pos - origin -- no zig-zag -- and with nothing above 0.0 the outcome is (lag 0, +0.0)
// for every SGN: index 0 is not in the band, so there is no row `origin` to read.
template <int SGN = 0, bool BAND = false>
__device__ __forceinline__ void window_scan_pos(WindowBest &best, const double *lds, const int row0, const int pos, const int c, const int L,
                                                const int Lneg, const int origin, const WindowStats &st, const double *__restrict__ pw)
{
    if (pos < L + 1 + Lneg) {
        const int v = BAND ? pos : (pos <= L ? pos : pos - 1 - Lneg - L) + origin; // lag + origin
        const double val = window_score(lds, row0, v, c, st, pw);
        if (window_key<SGN>(val) > best.abs) {
            best.abs = window_key<SGN>(val);
            best.val = val;
            best.pos = (double)pos;
        }
    }
}
__device__ __forceinline__ void window_put_best(double *cand, const WindowBest &best)
{
    cand[0] = best.abs;
    cand[1] = best.val;
    cand[2] = best.pos;
}
// parts slot0 .. slot0 + parts - 1 of series c merged in their order, and the outcome: the value, and through *lag its lag
// (SGN != 0: no value of the sign in the window is (lag 0, +0.0), not cc[0], which would have the other sign)
template <int SGN = 0, bool BAND = false>
__device__ __forceinline__ double window_outcome(const double *lds, const int CAND, const int slot0, const int parts, const int row0,
                                                 const int c, const int L, const int Lneg, const int origin, const WindowStats &st,
                                                 const double *__restrict__ pw, int *lag)
{
    double ba = 0.0, bv = 0.0;
    int bp = -1;
    for (int k = 0; k < parts; k++) {
        const int at = CAND + ((slot0 + k) * 16 + c) * 3;
        const double a = lds[at];
        if (a > ba) {
            ba = a;
            bv = lds[at + 1];
            bp = (int)lds[at + 2];
        }
    }
    *lag = 0;
    if (st.nan)
        return __builtin_nan("");
    if (st.zero)
        return 0.0; // sigma == 0: (nil, 0, 0), xcorr.go:165-168
    if (bp < 0) // only zeros or NaN in the window: index 0 stands
        return SGN != 0 || BAND ? 0.0 : window_score(lds, row0, origin, c, st, pw);
    *lag = BAND ? bp - origin : bp <= L ? bp : bp - 1 - Lneg - L;
    return bv;
}

// ---- the scan and the write-out of the single-reference kernels: the summed tiles in lds[0 .. TILES 256), (t1, t2) = series (t & 15)'s
// sum d and sum d^2; 16 parts of TILES positions per series, candidates in lds[CAND ..).  Every thread of the workgroup calls it.
template <int TILES, int SGN = 0, bool BAND = false>
__device__ __forceinline__ void window_scan_write(double *lds, const int CAND, const double t1, const double t2, const WindowParams &p,
                                                  const long long row0, const int t)
{
    const int c = t & 15, part = t >> 4;
    const WindowStats st = window_stats(t1, t2, p.invN, p.invNm1);
    WindowBest best;
#pragma unroll
    for (int k = 0; k < TILES; k++)
        window_scan_pos<SGN, BAND>(best, lds, 0, part * TILES + k, c, p.L, p.Lneg, p.origin, st, p.pw);
    window_put_best(lds + CAND + (part * 16 + c) * 3, best);
    __syncthreads();
    if (t < 16 && row0 + t < p.M) {
        int lag;
        p.mv[row0 + t] = window_outcome<SGN, BAND>(lds, CAND, 0, 16, 0, c, p.L, p.Lneg, p.origin, st, p.pw, &lag);
        p.lag[row0 + t] = lag;
    }
}

// acc: the wave's share of S (its pieces of every chunk); s1 / s2: the lane's share of sum d and sum d^2.  Every thread of the
// workgroup calls it, behind its last piece; row0: the workgroup's first series
template <int TILES, int SGN = 0, bool BAND = false>
__device__ __forceinline__ void window_finish(double *lds, const v4d (&acc)[TILES], const double s1, const double s2, const WindowParams &p,
                                              const long long row0, const int t, const int wave, const int r, const int q)
{
    constexpr int STAT = WindowLds<TILES>::STAT;
    window_sum_tiles<TILES>(lds, STAT, acc, s1, s2, wave, r, q);
    const int c = t & 15;
    window_scan_write<TILES, SGN, BAND>(lds, WindowLds<TILES>::CAND, window_wave_sum(lds, STAT, 2 * c), window_wave_sum(lds, STAT, 2 * c + 1), p, row0, t);
}

// ---- the launch side: the checks every launch makes on a window's shape, and the tile count as a compile-time constant
inline hipError_t window_launch_check(const WindowShape &p, long long *blocks)
{
    // rows origin - Lneg .. origin + L of the table: inside the eight tiles, pw and the staged image's tail (2 MUSE_LAG_WINDOW_MAX + 1 rows)
    if (p.L < 0 || p.Lneg < 0 || p.L + p.Lneg > 2 * MUSE_LAG_WINDOW_MAX || p.origin < p.Lneg || p.origin + p.L > 2 * MUSE_LAG_WINDOW_MAX || p.N < 2)
        return hipErrorInvalidValue;
    *blocks = (p.M + 15) / 16;
    return *blocks > 0x7fffffffLL ? hipErrorInvalidValue : hipSuccess;
}
// the same for a band (WindowShape: origin = Lneg = -lo, L = hi, lag 0 outside): rows 0 .. W - 1 = L + Lneg of the table
inline hipError_t window_launch_check_band(const WindowShape &p, long long *blocks)
{
    if ((p.L >= 0 && p.Lneg >= 0) || p.origin != p.Lneg || p.L + p.Lneg < 0 || p.L + p.Lneg > 2 * MUSE_LAG_WINDOW_MAX || p.N < 2)
        return hipErrorInvalidValue;
    *blocks = (p.M + 15) / 16;
    return *blocks > 0x7fffffffLL ? hipErrorInvalidValue : hipSuccess;
}
// f(std::integral_constant<int, TILES>) for tiles = 1 .. 8 accumulator tiles of 16 lags (the checks have bounded it)
template <class F> inline void window_with_tiles(const int tiles, F &&f)
{
    switch (tiles) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}
inline int window_tiles(int L) { return (2 * L + 1 + 15) / 16; } // lag + L runs up to 2 L whichever side the window drops
inline int window_tiles(const WindowShape &p) { return (p.origin + p.L + 1 + 15) / 16; } // rows 0 .. origin + L (symmetric: the line above)

} // namespace muse
