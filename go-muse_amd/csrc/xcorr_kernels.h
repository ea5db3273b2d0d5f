// xcorr_kernels.h -- host-visible launch interface of the device code
// (internal to libmuse_hip.so; the public ABI is include/muse_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "muse_hip.h"

namespace muse {

enum { KERNEL_GENERIC = 0, KERNEL_R16_OCC3 = 6, KERNEL_STOCKHAM = 10, KERNEL_R16_FOLD = 11, KERNEL_SMALL = 12, KERNEL_LONG = 13, KERNEL_REAL = 14, KERNEL_REAL_SPLIT = 15 };

struct FusedParams {
    const double *rows; // M x N row-major, row stride `stride` elements (float64 groups)
    const float *rows32; // the same for float32-storage groups (muse_group_create_f32); exactly one of the two is set
    long long M;
    long long stride;
    long long npairs; // ceil(M/2): one workgroup pass handles two series
    int N;            // series length
    int n;            // FFT length (power of two >= N)
    int logn;
    int normalize_y;     // 1: zNormalize each series (xCorrWithX, xCorr normalize=true)
    const double2 *xc;   // n entries: conj(X_full[f]) * scale
    const double2 *tw1;  // [16][256] W_4096^(k*t)      (tuned kernel)
    const double2 *tw2;  // [16][16]  W_256^(k*c)       (tuned kernel)
    const double2 *xcp;  // [16][256] xc[256*k + (t>>4) + 16*(t&15)]     (xcorr_r16_fold.hip: xc in lane order)
    // xcorr_r16_fold.hip: the eight per-thread factors of a generalised 16-point pass (fold_device.h), delta = u / 256
    const double2 *g2;   // [8][16]  pass 2: u = 16 j
    const double2 *g3a;  // [8][256] first transform, pass 3: u = (t >> 4) + 16 (t & 15)
    const double2 *g3b;  // [8][256] second transform, pass 3: u = t
    const double2 *gsmall; // [8][n/16] xcorr_small.hip (n = 512, 1024, 2048): last-pass factors, delta = j / (n/16), lane-ordered
    // xcorr_real.hip, the 16384-point transform as 16 x 1024 (wave-local 1024-point transforms around ONE workgroup transpose):
    const double2 *gsmall_b; // [8][64]: the 1024-point transform's last-pass factors (the context's table for n = 1024)
    const double2 *wsplit;   // [15][1024] W_16384^(j k1), k1 = 1 .. 15: the twiddles between the register pass and the wave-local transforms
    const double2 *xcw;      // [2][8][1024] xc at the bins of a thread's lower eight registers, k = w + 16 c + 1024 r (j = 64 w + c), and at M - k
    const double2 *twl;  // [4096] W_n^(m2): the base of the sweeps' twiddles W_n^(m2 k1) of the long-series kernel (xcorr_long.hip forms the powers)
    const double *c1;    // [n] (n = 4096 and the long-series kernel) N < n: correlation of the valid-sample indicator with the reference (xcorr_r16_fold.hip)
    // many references in one pass (xcorr_fused_n4096_multi): device arrays of R pointers
    int R;
    const double2 *const *xcp_many; // R lane-ordered spectrum tables
    double *const *mv_many;         // R result vectors (M doubles each)
    int *const *lag_many;           // R lag vectors (M ints each)
    const double *const *c1_many;   // N < 4096: R indicator-correlation tables
    const float2 *const *xcf_many;  // screening pass for R references: R fp32 spectrum tables
    unsigned *const *flags_many;    //   R flag vectors
    double *const *var_many;        //   R variance vectors
    double2 *zscratch;              // zslots x 4096 complex: one parked spectrum per (resident) workgroup
    int zslots;
    const double2 *twm;  // [32768]   W_65536^k         (generic kernel; half period)
    double2 *gscratch;   // n > 8192: one n-element complex work buffer per workgroup (global, L2-resident)
    double *mv;          // out: M signed max values
    int *lag;            // out: M lags
    double *cc_out;      // optional (generic kernel only): M x n correlations
    int *nil_out;        // optional (generic kernel only): M flags, 1 = sigma == 0 -> (nil,0,0)
    unsigned long long *dbg; // diagnostic builds only (tools/ablate): per-workgroup phase cycle sums
    // fp32 screening kernel (xcorr_r16_screen.hip)
    const float2 *twmf;  // [32768]   W_65536^k, fp32 (screening pass, n = 512 .. 2048)
    const float2 *tw1f;  // [16][256] W_4096^(k*t), fp32
    const float2 *tw2f;  // [16][16]  W_256^(k*c), fp32
    const float2 *xcf;   // n entries: conj(X_full[f]) / n, fp32
    const double *xs;    // n entries: zeroPad(zNormalize(ref)/(N-1), n), time domain, fp64
    double screen_delta; // candidate window below the fp32 maximum (scaled units, max |cc| <= 1)
    unsigned *scr_flags; // screening pass (xcorr_screen_pass_n4096): per-row SCR_* bits, OR-ed in
    double *scr_var;     // screening pass: per-row sample variance (the estimate in mv is cc32 * 2^e: score = mv / sqrt(var))
    int scr_max_lag;     // screening pass: the Run's MaxLag (classifies the possible argmax lags)
    int scr_need_sign;   // screening pass (n = 4096): 0 = the Run's filters never look at the sign of a score
    int *ovf_count;      // pairs with too many candidates: redone by the fp64 kernel
    int *work_counter;   // dynamic pair hand-out (xcorr_r16_fold.hip): zeroed before the launch
    long long *ovf_list;
    // optional indirection for the fp64 kernels: process pair_list[0 .. *pair_count)
    const long long *pair_list;
    const int *pair_count;
    long long dense_total; // xcorr_r16_occ4.hip behind the default n = 4096 kernel: > 0 and *pair_count * 8 > dense_total -> redo ALL dense_total pairs
    long long gscratch_slices; // n-element slices `gscratch` holds: a kernel that works in it launches no more workgroups than fit
    // two-sided xCorr (xcorr_two_sided.hip): pair i = (x_i = xrows + i xstride, length Nx; y_i = rows + i stride, length N)
    const double *xrows;
    long long xstride;
    int Nx;
    // 1 / N and 1 / (N - 1), formed on the host by the launchers (with_reciprocals): as kernel arguments they live in scalar
    // registers; formed by the kernel (N is a run-time value in the builds for zero-padded series) they come out of the vector
    // divider, and wave-uniform values in vector registers were what those builds parked in scratch
    double invN, invNm1;
    // masked argmax (the WIN builds of xcorr_r16_fold.hip, xcorr_r16_occ4.hip and xcorr_small.hip; muse_batch_score_in_window): win != 0 ->
    // index i of cc takes part in maxAbsIndex iff i <= win_lpos || i >= n - win_lneg (WindowParams::L / ::Lneg; the two bounds are
    // independent: 0 <= win_lpos <= n / 2, 0 <= win_lneg <= n / 2 - 1, muse_batch_score_in_lag_range); every other value
    // is replaced by +0.0 in front of the argmax.  Last in the structure: the offsets of everything above are what they were.
    int win, win_lpos, win_lneg;
    // the slide fused into the n = 4096 pass (the SLIDE builds of xcorr_r16_fold.hip; muse_batch_slide_score_in_window): slide_tails != 0 ->
    // the kernel scores the rows moved forward by 1 <= slide_k <= N samples -- old row[slide_k .. N) followed by slide_tails[r * slide_k + 0 .. slide_k),
    // a dense M x slide_k device image in the group's storage type, 256-byte aligned -- and stores them in place on the way (rows and
    // rows32 are written).  Behind everything else, for the same reason as the window.
    const void *slide_tails;
    int slide_k;
    // the signed masked argmax (muse_batch_score_signed_in_lag_range; the SIGNED kernels of xcorr_r16_fold.hip, xcorr_r16_occ4.hip and
    // xcorr_small.hip): win != 0 and win_sign = +1 / -1 -> a value inside the window that is not > 0 / < 0 becomes +0.0 as well.  Read
    // by the launchers alone (the sign is a template argument of those kernels); 0: the kernels above.  Behind everything else again.
    int win_sign;
    // the band mask (muse_batch_score_in_lag_band; the BAND kernels of the same three files): win != 0 and win_band != 0 -> index i of cc
    // takes part iff win_a <= i <= win_b, one interval on one side of lag 0 (1 <= win_a <= win_b <= n / 2, or n / 2 + 1 <= win_a <= win_b
    // <= n - 1); win_lpos / win_lneg are not read, win_sign is as above and may be 0.  win_band is read by the launchers alone.  Behind
    // everything else again.
    int win_band, win_a, win_b;
};
inline FusedParams with_reciprocals(FusedParams p)
{
    p.invN = 1.0 / (double)p.N;
    p.invNm1 = 1.0 / (double)(p.N - 1);
    return p;
}
// the band mask's interval at FFT length n: on one side of lag 0, index 0 outside
inline bool band_bounds_ok(const FusedParams &p, int n)
{
    return p.win && p.win_a >= 1 && p.win_a <= p.win_b && p.win_b <= n - 1 && (p.win_b <= n / 2 || p.win_a > n / 2);
}
// the masked argmax's window as the n = 4096 launchers accept it (no window: nothing to check)
inline bool window_bounds_ok(const FusedParams &p)
{
    return (!p.win || (p.win_lpos >= 0 && p.win_lneg >= 0 && p.win_lpos <= 2048 && p.win_lneg <= 2047)) && (!p.win_band || band_bounds_ok(p, 4096));
}
// run-time booleans -> template arguments: with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...),
// so a launcher names its kernel once, with decltype(flag)::value for each flag, and every combination is instantiated
template <typename F>
inline void with_bools(F f)
{
    f();
}
// the same for a sign of -1 .. 1: f(std::integral_constant<int, sign>{})
template <typename F>
inline void with_sign(int sign, F f)
{
    if (sign > 0)
        f(std::integral_constant<int, 1>{});
    else if (sign < 0)
        f(std::integral_constant<int, -1>{});
    else
        f(std::integral_constant<int, 0>{});
}
template <typename F, typename... Rest>
inline void with_bools(F f, bool b, Rest... rest)
{
    if (b)
        with_bools([&](auto... flags) { f(std::true_type{}, flags...); }, rest...);
    else
        with_bools([&](auto... flags) { f(std::false_type{}, flags...); }, rest...);
}

hipError_t launch_fused(const FusedParams &p, int variant, int num_cus, hipStream_t stream);
hipError_t launch_fused_occ4(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_r16_occ4.hip (rescaling / pair-list kernel)
hipError_t launch_screen_pass(const FusedParams &p, int num_cus, hipStream_t stream);  // xcorr_r16_screen.hip (filter-and-refine Run)
hipError_t launch_screen_pass_many(const FusedParams &p, int num_cus, hipStream_t stream); // the same for R references in one pass
hipError_t launch_screen_pass_stk(const FusedParams &p, int num_cus, hipStream_t stream);  // xcorr_screen_stk.hip: n = 512, 1024, 2048
// per-row flags of the screening pass
enum : unsigned { SCR_IN = 1u, SCR_OUT = 2u, SCR_POS = 4u, SCR_NEG = 8u, SCR_REFINE = 16u, SCR_NAN = 32u };
hipError_t launch_fused_fold(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_r16_fold.hip (n == 4096, default)
hipError_t launch_fused_multi(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_r16_fold.hip (R references)
// xcorr_r16_cached.hip: a resident float64 group's spectrum cache at n = 4096.  One segment covers the pairs [pair0, pair0 + zpairs)
// of the group: zc[(pair - pair0)][16][256] double2, zstat[(pair - pair0)][ZC_STAT] double.  Both launchers process the pairs
// [pair0, pair0 + p.npairs) (p.M, p.mv, p.lag, p.ovf_list: the whole group's), ADD to *p.ovf_count and want *p.work_counter zero.
constexpr int ZC_STAT = 16;                                       // doubles per pair: 8 sum-of-squares partials, 2 sums, the verdict, 3 unused
constexpr int ZC_VERDICT = 10;                                    // the pair's verdict (foldk_device.h): 1 / sigma of series A and of B, then one word of bits (the low word of the slot)
constexpr long long ZC_PAIR_BYTES = 4096 * 16 + ZC_STAT * 8;      // 64 KB + 128 B
struct SpectrumCacheArgs {
    double2 *zc;
    double *zstat;
    long long pair0;
    long long zpairs;
};
hipError_t launch_cache_fill(const FusedParams &p, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream); // from the rows; the first c.zpairs pairs into the cache
hipError_t launch_cached(const FusedParams &p, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream, bool occ4 = false); // from the cache (occ4: the four-workgroup reader, a test hook)
hipError_t launch_fused_small(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_small.hip (n = 512, 1024, 2048: default)
hipError_t launch_fused_stockham(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_stockham.hip (n = 512 .. 2048, 8192 .. 65536)
hipError_t launch_fused_long(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_long.hip (n = 65536: default; 16384, 32768)
hipError_t launch_real_split_tables(const double2 *xc, double2 *out, hipStream_t stream); // xcorr_real.hip: FusedParams::xcw for n = 32768
hipError_t launch_real8k_tables(const double2 *xc, double2 *out, hipStream_t stream); // xcorr_real.hip: n = 8192, xc at the threads' bins, lane-ordered ([16][256])
hipError_t launch_two_sided_real(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_real.hip: the two-sided xCorr at n = 32768
hipError_t launch_fused_real_split(const FusedParams &p, int num_cus, hipStream_t stream); // the same, the 16384-point transform as 16 x 1024 (test hook 15)
hipError_t launch_fused_real(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_real.hip (n = 32768: one real series per workgroup on the 16384-point transform)
hipError_t launch_two_sided(const FusedParams &p, int num_cus, hipStream_t stream);
// the same for n = 512 ... 2048, 8192, 16384 on xcorr_small.hip's transforms (called by launch_two_sided)
hipError_t launch_two_sided_small(const FusedParams &p, int num_cus, hipStream_t stream); // xcorr_two_sided.hip (xCorr, n = 512 .. 65536)
// out[4096 k1 + 256 k + t] = in[k1 + R1 (256 k + (t >> 4) + 16 (t & 15))]: the spectrum rows of the long-series kernel in lane order
hipError_t launch_lane_order_rows(const double2 *in, double2 *out, int R1, hipStream_t stream);
// out[256 k + t] = in[256 k + (t >> 4) + 16 (t & 15)], k < 16: a 4096-entry table in the lane order of xcorr_r16_fold.hip
hipError_t launch_lane_order(const double2 *in, double2 *out, hipStream_t stream);
// c1[k] = sum_{j >= pad} xs[(j + k) mod n]: what a series of ones at the valid (non-pad) positions correlates to
hipError_t launch_indicator_corr(const double *xs, int n, int pad, double *c1, hipStream_t stream);
hipError_t launch_ref_spectrum(const double *ref_dev, int N, int n, int logn, int normalize, double x_scale,
                               double xc_scale, const double2 *twm, double2 *X, double2 *xc, float2 *xcf, double *xs,
                               double2 *gscratch, int *status, hipStream_t stream);
constexpr int SMALL_MAX_N = 16384;       // largest FFT length of xcorr_small.hip (it reads n - N samples in front of a row unclamped:
                                         // FusedParams::rows must carry that many readable elements in front of row 0, capi_group.hip GROUP_GUARD)
constexpr int GENERIC_LDS_MAX_N = 8192;  // larger n: the radix-2 passes run in gscratch
constexpr int GENERIC_MAX_N = 65536;
constexpr int GENERIC_GLOBAL_WGS_PER_CU = 2;
constexpr int STOCKHAM_GLOBAL_WGS_PER_CU = 2; // xcorr_fused_stk_4step (the long series' redo kernel): resident workgroups per CU, one n-element slice each
constexpr int LONG_WGS_PER_CU = 4;            // xcorr_long.hip and xcorr_two_sided_long: resident workgroups per CU, one n-element slice each
// n-element complex slices of the context's scratch buffer per CU (capi_batch.hip, ensure_gscratch): every kernel that works in it
// launches at most this many workgroups per CU times the slices each of them uses, and checks FusedParams::gscratch_slices
constexpr int GSCRATCH_SLICES_PER_CU = 4;
static_assert(LONG_WGS_PER_CU <= GSCRATCH_SLICES_PER_CU && GENERIC_GLOBAL_WGS_PER_CU <= GSCRATCH_SLICES_PER_CU &&
                  2 * STOCKHAM_GLOBAL_WGS_PER_CU <= GSCRATCH_SLICES_PER_CU,
              "the scratch buffer is sized for GSCRATCH_SLICES_PER_CU slices per CU");
// ---- the lag-window pass (xcorr_window.hip): the best match inside +-L lags from a direct matrix product, no transform
constexpr int WIN_KC = 1024;    // samples per chunk of the reference image a workgroup stages in LDS
constexpr int WIN_E_TAIL = 128; // >= 2 * MUSE_LAG_WINDOW_MAX + 2: what a chunk's image holds behind its WIN_KC samples
static_assert(2 * MUSE_LAG_WINDOW_MAX + 2 <= WIN_E_TAIL, "the staged image covers every lag of the widest window");
struct WindowShape {    // what every lag-window kernel takes: the rows and the window (capi_window.hip: window_params fills it)
    const double *rows; // M x N row-major float64, row stride `stride` elements
    long long M, stride;
    int N;
    int L, Lneg;        // lags -Lneg .. L (a symmetric window: Lneg = L, or L - 1 when L == n / 2: index n / 2 is lag +n/2 only)
    double invN, invNm1;
    int origin;         // row v of the product table is lag v - origin, Lneg <= origin: L for a symmetric window (rows L - Lneg .. 2 L),
                        // Lneg for a lag range (muse_batch_score_in_lag_range: rows 0 .. L + Lneg).  Last: the offsets above are what they were.
                        // A band (launch_window_band alone): lags lo .. hi without lag 0 as L = hi, Lneg = origin = -lo, one of them negative
};
struct WindowParams : WindowShape {
    const double *e;    // [window_e_len(N)] e[v] = xs[(n - N + v - origin) mod n], zero from N + origin + L on
    const double *pw;   // [origin + L + 1] pw[v] = sum_t e[t + v]
    double *mv;         // out: M signed values
    int *lag;           // out: M lags
};
inline bool window_wide(const double *rows, long long stride) { return stride % 2 == 0 && ((uintptr_t)rows & 15) == 0; } // every row 16-byte aligned
inline long long window_e_len(int N) { return (long long)((N + WIN_KC - 1) / WIN_KC) * WIN_KC + WIN_E_TAIL; }
// the tables of a window whose row v is lag v - origin, rows 0 .. W - 1 (a symmetric window +-L: origin = L, W = 2 L + 1)
hipError_t launch_window_tables(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw, hipStream_t stream);
hipError_t launch_window(const WindowParams &p, hipStream_t stream);
// the signed best match (muse_batch_score_signed_in_lag_range): sign = +1 / -1 the largest positive / the most negative value inside
// the window, (lag 0, +0.0) where there is none (xcorr_window_signed_mfma); sign = 0 is launch_window
hipError_t launch_window_signed(const WindowParams &p, int sign, hipStream_t stream);
// ---- the same over a lag band lo .. hi that does not hold lag 0 (xcorr_window_band.hip; muse_batch_score_in_lag_band): a table whose
// row v is lag lo + v, W = hi - lo + 1 <= 2 MUSE_LAG_WINDOW_MAX + 1 rows (launch_window_tables_band: -(n / 2 - 1) <= lo, hi <= n / 2),
// and the shape L = hi, Lneg = origin = -lo (one of L, Lneg negative).  sign = 0 / +1 / -1: the best by magnitude / the largest positive
// / the most negative value of the band, (lag 0, +0.0) where nothing wins (xcorr_window_band_mfma)
hipError_t launch_window_tables_at(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw, hipStream_t stream);
hipError_t launch_window_tables_band(const double *xs, int N, int n, int lo, int W, double *e, long long e_len, double *pw, hipStream_t stream);
hipError_t launch_window_band(const WindowParams &p, int sign, hipStream_t stream);
// ---- the lag profile (xcorr_window_profile.hip; muse_batch_lag_profile): the band's product with the scan replaced by a write-out,
// out[k * out_stride + v] = cc at lag lo + v of output row k, v = 0 .. W - 1 <= 2 MUSE_LAG_WINDOW_MAX (tables: launch_window_tables_at
// with the origin -lo, lag 0 inside or not); columns W .. out_stride - 1 are never written.  series == nullptr: output row k is row k
// of `rows`; otherwise row series[k] (M entries in device memory, each inside the rows, any order, duplicates allowed)
struct WindowProfileParams {
    const double *rows;      // row-major float64, row stride `stride` elements
    long long M, stride;     // M output rows
    int N, W;
    double invN, invNm1;
    const double *e;         // WindowParams::e / ::pw of the table
    const double *pw;
    const long long *series; // [M] or nullptr
    double *out;
    long long out_stride;    // >= W
};
hipError_t launch_window_profile(const WindowProfileParams &p, hipStream_t stream);
// the planner (pure host function): lags lo .. hi in consecutive launches of up to 2 MUSE_LAG_WINDOW_MAX + 1 table rows; returns the
// launch count and fills lo_of / rows_of (each launch's first lag and its rows) up to cap entries
int window_profile_plan(int lo, int hi, int *lo_of, int *rows_of, int cap);
// ---- the same while the rows slide (xcorr_window_slide.hip; muse_batch_slide_score_windowed): xcorr_window_mfma over the NEW rows
// -- old row[k .. N) followed by tails[r * k + 0 .. k), a dense M x k device buffer, 16-byte aligned -- which are stored in place on
// the way: one read and one write of the rows instead of launch_row_slide's pair plus launch_window's read, the same bits as the two.
// Dense rows (stride == N), 1 <= k <= N.  slide_score_plan (pure host function): the widths the kernel moves in -- 16-byte loads
// iff the rows are wide (window_wide) and k is even, 16-byte stores iff they are wide, 8 bytes otherwise
void slide_score_plan(int N, int k, bool wide, int *load_bytes, int *store_bytes);
hipError_t launch_window_slide(const WindowParams &p, const double *tails, int k, hipStream_t stream);
// ---- the same for few rows of long series (xcorr_window_split.hip; muse_batch_run_rows_windowed): K split across workgroups.
// window_rows_plan (pure host function): the slice count S for M rows of N samples on num_cus CUs -- the largest S with blocks x S
// (blocks = ceil(M / 16)) within the CUs and S <= min(chunks, max(WIN_ROWS_FULL_SPLIT, chunks / WIN_ROWS_MIN_CHUNKS)): one chunk of
// WIN_KC samples per slice up to WIN_ROWS_FULL_SPLIT slices, at least WIN_ROWS_MIN_CHUNKS chunks per slice beyond (slice s = chunks
// [s chunks / S, (s + 1) chunks / S)); *chunks_per_slice = the largest slice.  S == 1: launch_window, untouched.
// Measured (tools/window_rows_bench.py part (b), profiles/window_rows_bench.txt, one box): at every shape with blocks < CUs
// every S > 1 beat S = 1 by 1.35 x or more; the fastest S was chunks at 4 and 16 chunks, chunks / 2 at 40 and 64 chunks (the
// finish kernel adds a block's slabs one after the other: 40 / 64 one-chunk slices lost 10 ... 35 % against 20 / 32).
constexpr int WIN_ROWS_FULL_SPLIT = 16;        // up to this many slices a slice may be a single chunk
constexpr int WIN_ROWS_MIN_CHUNKS = 2;         // beyond: chunks per slice at least
constexpr bool WIN_ROWS_SPLIT_ENABLED = true;  // false: the planner returns 1 everywhere
int window_rows_plan(long long M, int N, int num_cus, int *chunks_per_slice);
long long window_split_slab_doubles(const WindowShape &p); // doubles of one (block, slice) slab: tiles x 256 + 32, tiles = ceil((origin + L + 1) / 16)
// S >= 2 slices (<= chunks) into slabs[blocks x S x window_split_slab_doubles(p)], summed in slice order, scanned into p.mv / p.lag
hipError_t launch_window_split(const WindowParams &p, int S, double *slabs, hipStream_t stream);
// ---- the same for few rows and MANY lags (xcorr_window_panels.hip; muse_batch_run_rows_in_lag_range): a table of W = origin + L + 1
// rows, 128 < W <= WIN_PANEL_MAX_ROWS, cut into panels of WIN_PANEL_ROWS rows (one workgroup's eight accumulator tiles); a grid of
// blocks x S x panels workgroups, then one finish kernel that merges the panels.
constexpr int WIN_PANEL_ROWS = 128;        // table rows of a panel: eight accumulator tiles, the most one workgroup holds
constexpr int WIN_PANEL_MAX_ROWS = 2048;   // = MUSE_RUN_ROWS_LAG_RANGE_MAX: at most 16 panels
static_assert(WIN_PANEL_MAX_ROWS == MUSE_RUN_ROWS_LAG_RANGE_MAX && WIN_PANEL_ROWS + 2 <= WIN_E_TAIL + 2, "a panel's image is a chunk's");
int window_panels(int W);                  // ceil(W / WIN_PANEL_ROWS)
// the tables of such a window: e[window_panels_e_len(N, W)] (a chunk's image per panel runs on 128 (panels - 1) entries behind the
// narrow table's; zero from N + W - 1 on) and pw[W], each entry summed in window_table_p's order
long long window_panels_e_len(int N, int W);
hipError_t launch_window_tables_wide(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw, hipStream_t stream);
// window_panels_plan (pure host function): the slice count S for M rows of N samples and W table rows on num_cus CUs; *panels =
// ceil(W / WIN_PANEL_ROWS).  Lags supply parallelism here, and the finish kernel adds a block's panels x S slabs one after the other
// while the partial kernel's time falls as chunks / S: S = the largest S <= chunks with (2 S - 1)^2 panels <= 4 WIN_PANEL_BALANCE
// chunks (sqrt(WIN_PANEL_BALANCE chunks / panels), rounded), at most CUs / (blocks x panels), at least 1 (S = 1 whenever
// blocks x panels >= CUs).
// Measured (tools/rows_lag_range_bench.py part (b), profiles/rows_lag_range_bench.txt, one box): over 16 / 100 rows x 4096,
// 16384, 40000, 65536 samples x 255, 1025, 2048 lags the fastest S hardly depends on the blocks and follows that square root with a
// constant of 8 ... 10; window_rows_plan's own rule with blocks x panels workgroups (where this planner started) picked 2 ... 8 x
// too many slices for one block of long series (16 x 65536, 1025 lags: 603 us at S = 28 against 309 us at S = 8).
constexpr int WIN_PANEL_BALANCE = 10;
int window_panels_plan(long long M, int N, int num_cus, int W, int *panels);
long long window_panels_slab_doubles();    // doubles of one (block, panel, slice) slab: 8 x 256 + 32
// 1 <= S <= chunks slices into slabs[blocks x panels x S x window_panels_slab_doubles()]; p.e / p.pw: launch_window_tables_wide's
hipError_t launch_window_panels(const WindowParams &p, int S, double *slabs, hipStream_t stream);
// ---- the same for many references in one pass (xcorr_window_many.hip): the references' windows packed into the tiles of one product
constexpr int WINM_MAX_TILES = 8;       // accumulator tiles of a launch: 128 packed (reference, lag) rows
constexpr int WINM_PACK_MAX_ROWS = 48;   // wider windows (four tiles per reference) are not packed: one launch per reference
constexpr int WINM_IMG_DOUBLES = 4608;  // LDS budget of a launch's staged reference images (36 KB: four workgroups per CU)
struct WindowManyParams : WindowShape {
    int R;                    // references of this launch: R W <= 16 WINM_MAX_TILES, W = origin + L + 1 the rows of each one's table
    const double *const *e;   // [R] each reference's WindowParams::e   (the four tables: device memory)
    const double *const *pw;  // [R] each reference's WindowParams::pw
    double *const *mv;        // [R] out: each reference's M signed values
    int *const *lag;          // [R] out: each reference's M lags
    int kc, img, buf, parts;  // filled in by launch_window_many: chunk length, image stride, doubles of the image / tile region, scan parts per reference
};
// the planner (pure host functions) in the rows W of a reference's table (a window +-L: 2 L + 1; a lag range: its lags): image
// stride for W rows and chunk length kc; the most references one launch takes; the chunk length of a launch of `refs` references;
// the cut of R references into consecutive launches (returns their number; launch_of[R], tiles_of[launches <= R])
int window_many_img(int W, int kc);
int window_many_max_refs(int W);
int window_many_kc(int W, int refs);
int window_many_plan(int R, int W, int *launch_of, int *tiles_of);
// (every reference's table has the shape's origin and rows: origin + L <= 2 MUSE_LAG_WINDOW_MAX, Lneg <= origin)
hipError_t launch_window_many(WindowManyParams p, hipStream_t stream);
// ---- the packed pass under a sign or over a lag band (xcorr_window_many_band.hip; muse_batch_score_many_in_lag_band): the same
// product, planner and launch sizes with the scan of launch_window_signed / launch_window_band (xcorr_window_many_signed_mfma).  A band
// is the shape L = hi, Lneg = origin = -lo with one of L, Lneg negative; sign = 0 over a window that holds lag 0 is launch_window_many
hipError_t launch_window_many_signed(WindowManyParams p, int sign, hipStream_t stream);
// ---- the packed pass with a lag range, band and sign PER REFERENCE (xcorr_window_many_each.hip; muse_batch_score_many_in_lag_bands):
// the same product, each reference's table under its own origin and row count, its scan and outcome chosen at run time from the six
// builds of window_scan_pos / window_outcome (xcorr_window_many_each_mfma).  What is per reference is a descriptor in device memory
struct WindowEachRef {
    int L, Lneg, origin, W; // the reference's shape (WindowShape's; a band: one of L, Lneg negative); W = origin + L + 1 table rows
    int sign, band;         // -1 / 0 / +1; 1: lag 0 is outside
    int row0;               // its first row in the launch's packed A rows: the sum of the W in front of it
    int img0;               // the LDS offset of its staged image (window_each_place)
};
struct WindowEachParams {
    const double *rows;       // M x N row-major float64, row stride `stride` elements (WindowShape's)
    long long M, stride;
    int N;
    double invN, invNm1;
    int R;                    // references of this launch
    const double *const *e;   // [R] each reference's WindowParams::e   (the four tables and the descriptors: device memory)
    const double *const *pw;  // [R] each reference's WindowParams::pw
    double *const *mv;        // [R] out: each reference's M signed values
    int *const *lag;          // [R] out: each reference's M lags
    const WindowEachRef *ref; // [R]
    int total;                // packed rows: the sum of the W
    int kc, buf, parts;       // chunk length, doubles of the image / tile region, scan parts per reference
};
// the planner (pure host functions).  window_each_place: img0[0 .. m) of m references with W[j] table rows at chunk length kc --
// img0[0] = 0, img0[j + 1] the smallest offset >= img0[j] + kc + W[j] - 1 with img0[j + 1] - img0[j] = W[j] + 2 (mod 32); returns the
// offset behind the last image, placed by the same rule (the launch's image doubles).  window_each_plan: R references, W[r] table rows
// each (W[r] <= 0: not on the direct product, launch_of[r] = -1), cut into launches in list order: a reference of more than
// WINM_PACK_MAX_ROWS rows has a launch to itself, the others join the open launch until one more would pass 16 WINM_MAX_TILES rows or,
// at kc = 256, WINM_IMG_DOUBLES image doubles.  Launches are numbered by their first member.  Returns their number; tiles_of / kc_of
// [launches <= R] (a reference alone in its launch: the single-reference kernel's tiles and WIN_KC), img0[R] (alone: 0)
int window_each_place(const int *W, int m, int kc, int *img0);
int window_each_plan(int R, const int *W, int *launch_of, int *tiles_of, int *kc_of, int *img0);
// ref_host: the launch's descriptors as uploaded to p.ref (the launcher checks every one of them and sizes the launch from them)
hipError_t launch_window_many_each(WindowEachParams p, const WindowEachRef *ref_host, hipStream_t stream);
hipError_t launch_direct(const double *x, int lenx, const double *y, int leny, int n, int normalize_x,
                         int normalize_y, double x_scale, double cc_scale, double *cc, int *lag, double *mv,
                         int *status, hipStream_t stream);
// two-sided xCorr, pairs whose statistics overflowed (xcorr_kernels.hip): what the reference's arithmetic gives for each listed
// pair (code 0 NaN stands / 1 every cc zero / 2 recompute on copies scaled by (scale.x, scale.y)), and those copies
hipError_t launch_two_sided_rescue(const double *xrows, long long xstride, int Nx, const double *yrows, long long ystride, int Ny,
                                   int n, int normalize, const long long *list, int count, int *code, double2 *scale,
                                   hipStream_t stream);
hipError_t launch_scale_listed_rows(const double *src, long long stride, int N, const long long *list, const double2 *g, int which,
                                    int count, double *dst, hipStream_t stream);
hipError_t launch_synth(double *rows, long long stride, long long first, long long count, long long global_first,
                        int N, unsigned long long seed, unsigned flags, hipStream_t stream);
hipError_t launch_synth_f32(float *rows, long long stride, long long first, long long count, long long global_first,
                            int N, unsigned long long seed, unsigned flags, hipStream_t stream);
hipError_t launch_synth_ref(double *ref, int N, unsigned long long seed, hipStream_t stream);
// row_gather.hip: dst row i = src row idx[i] (i < count; rows N elements apart, idx in memory the device reads), float64 or
// float32 rows, float32 -> float64 widened exactly; nontemporal: the stores bypass the caches
hipError_t launch_row_gather(const void *src, bool src_f32, void *dst, bool dst_f32, const long long *idx, long long count,
                             int N, int num_cus, bool nontemporal, hipStream_t stream);
// row_slide.hip: rows [0, count) behind `rows` (N elements apart, float64 or float32) move forward by 1 <= k <= N samples in place:
// row r <- old row r [k .. N) followed by tails[r * k + 0 .. k) (a dense count x k device buffer of the rows' type, 256-byte
// aligned).  One wave owns a row; nothing outside the count rows is stored to.  slide_unit_bytes (pure host function): the vector
// unit the kernel moves in -- the widest of 16 / 8 (/ 4 for float32) bytes that divides both N x elem and k x elem
int slide_unit_bytes(int N, int k, bool f32);
hipError_t launch_row_slide(void *rows, bool f32, long long count, int N, int k, const void *tails, int num_cus,
                            hipStream_t stream);

// measurement hook (diag_kernels.hip): one wave sampling delta s_memtime / delta s_memrealtime in windows of window_ms for total_ms
hipError_t launch_clock_probe(unsigned long long *out, int *count, int max_windows, double window_ms, double total_ms,
                              hipStream_t stream);
// unit-test hook: foldk::wave_argmax_store on 2 x 4096 given values (diag_kernels.hip); out24 = 4 waves x {max, value, index} x 2 series
hipError_t launch_wave_argmax_probe(const double *ccA, const double *ccB, double *out24, hipStream_t stream);

// ---- group max / filter / top-N (reduce_kernels.hip)
constexpr int TOPN_CHUNK = 4096;    // groups per workgroup in the selection pass
constexpr int TOPN_DEVICE_MAX = 256; // larger top_n: winners are copied to the host instead
constexpr int EXACT_FEED_MAX_GROUPS = 65536; // up to this many groups a Run feeds the top-N heap one Score per group in group order (the reference's feed)

struct GroupWork {
    unsigned long long *key; // [G] max of bits(|score|) over members (atomicMax)
    long long *first;        // [G] lowest member index (atomicMin)
    long long *win;          // [G] lowest member index attaining key (atomicMin)
};

struct SelectParams {
    const double *mv;
    const int *lag;
    long long M;
    const int *group_id; // device, or nullptr: every series its own group
    int G;
    int abs_scores;
    int max_lag;
    double threshold;
    int sign_filter;
    long long series_offset;
    const unsigned char *include; // optional: rows that may be selected (filter-and-refine Run); nullptr = all
    // 1: this device holds ONE SHARD of a group whose label groups may continue on other shards (muse_batch_run_groups):
    // rec[g] = the winner among the shard's members whose score is a number (series -1 if there is none), nothing is
    // filtered, and selkey[g] = the group's state on this shard: 0 no member, 1 members and the first one's score is a
    // number, 2 the first member's score is NaN (if it is the group's first member overall the group's score is NaN:
    // x > NaN never replaces it, muse_batch.go:87)
    int partial;
};

// filter-and-refine Run: what the screening pass left per row, the Run's filters and the error bound of the estimate
struct ScreenSelect {
    const double *mv;      // fp32 estimate of the signed value at the fp32 argmax, times sigma
    const double *var;     // sample variance (score estimate = mv / sqrt(var))
    const unsigned *flags; // SCR_* bits
    long long M;
    double threshold;
    int sign_filter;
    int abs_scores;
    double E;              // |estimate - exact| <= E (score units)
    const int *group_id;   // label groups (device), or nullptr: every series its own group
    int G;
};
// per-group scratch of the grouped filter-and-refine selection (G entries each)
struct ScreenGroupWork {
    long long *first;
    unsigned long long *glo, *gmay, *gkplus;
    int *gcert;
};
// pessimistic keys -> the top_n-th best of them (the cut) -> pairs whose optimistic key reaches it (pair_list,
// *pair_count, include[row] = 1); keys: screen_select_scratch(M, top_n) entries of scratch
long long screen_select_scratch(long long G, int top_n);
// run-time guard of the bound: estimates of the listed rows saved before the fp64 kernel overwrites them, then the largest
// | |estimate| - |fp64 score| | over those rows (as the bits of a non-negative double, atomicMax)
// guard sample: appends one pair in 1024 (hash of pair and salt) to the list and marks its rows re-evaluated
hipError_t launch_screen_sample(long long npairs, long long M, unsigned long long salt, long long *pair_list, int *pair_count,
                                unsigned char *include, hipStream_t stream);
hipError_t launch_screen_save(const ScreenSelect &q, const long long *pair_list, const int *pair_count, double *est_save,
                              hipStream_t stream);
hipError_t launch_screen_check(const double *mv, long long M, const long long *pair_list, const int *pair_count,
                               const double *est_save, unsigned long long *err_bits, hipStream_t stream);
hipError_t launch_screen_select(const ScreenSelect &q, int top_n, unsigned long long *selkey, unsigned long long *keys,
                                const ScreenGroupWork &gw, long long *pair_list, int *pair_count, unsigned char *include,
                                hipStream_t stream);

// per-group winners -> rec[G] (+ selection keys selkey[G]: 0 = filtered out)
hipError_t launch_group_reduce(const SelectParams &sp, const GroupWork &gw, muse_record *rec,
                               unsigned long long *selkey, hipStream_t stream);
// small Runs in one launch (reduce_kernels.hip, small_groups_kernel): what launch_group_reduce computes, one 32-byte slot of pinned
// host memory per label group, each with its own stamp (= token) stored last
constexpr int SMALL_GROUPS_MAX_G = 2048;        // label groups (three 8-byte work arrays in LDS)
constexpr long long SMALL_GROUPS_MAX_M = 32768; // series
constexpr int SMALL_UNGROUPED_MAX = 32768;      // series of a Run without a label map (one slot each, no work arrays)
struct SmallSlot {
    long long series; // muse_record::series, ::score, ::lag of group g (::group = g)
    double score;
    int lag;
    unsigned key;     // the selection key: 0 not selectable / empty; partial mode: the group's state 0 / 1 / 2
    unsigned long long stamp;
};
static_assert(sizeof(SmallSlot) == 32, "one slot = one 32-byte block");
hipError_t launch_small_groups(const SelectParams &sp, SmallSlot *out, unsigned long long token, hipStream_t stream);
// Run(nil) over many series: per chunk of TOPN_CHUNK series the best K candidates (what group_final_kernel + topn_kernel select,
// in the same order) written into pinned slots cand[chunk * K + r], their number into cnt[chunk] (each with its stamp)
constexpr int SMALL_DIRECT_MAX_SLOTS = 131072;  // 4 MB of pinned slots
struct CountSlot {
    unsigned long long count;
    unsigned long long stamp;
};
hipError_t launch_topn_ungrouped(const SelectParams &sp, int K, SmallSlot *cand, CountSlot *cnt, unsigned long long token,
                                 hipStream_t stream);
// one label group in one launch (Muse.Run): the winner record and the group's state (reduce_kernels.hip)
struct SingleGroupOut {
    muse_record rec;
    unsigned long long state;
};
hipError_t launch_single_group(const double *mv, const int *lag, long long M, int abs_scores, long long series_offset,
                               SingleGroupOut *out, hipStream_t stream);
// per-chunk top-K extraction: cand[nblocks*K], cnt[nblocks]
hipError_t launch_topn(const muse_record *rec, const unsigned long long *selkey, int G, int K, muse_record *cand,
                       int *cnt, hipStream_t stream);

} // namespace muse
