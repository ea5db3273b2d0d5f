// xcorr_r16_fold.hip -- the default n = 4096 fp64 kernel (2048 < N <= 4096), round 2.
//
// Mathematics: xCorrWithX, /root/reference/xcorr.go:160-197 (z-normalise, leading zero pad, forward
// transform, multiply by the conjugate reference spectrum, inverse transform, 1/n, global argmax of |cc|),
// two series per complex transform as in xcorr_r16_fast.hip, whose data flow this kernel keeps: 256 threads x
// 16 points, three radix-16 passes per transform, four LDS transposes per pair of which two stay inside a
// wave, nine workgroup barriers, statistics off the DC bin, a resident grid with dynamic pair hand-out,
// NaN/Inf and sigma-spread pairs handed to the rescaling kernel.
//
// What is new is the ARITHMETIC (fold_device.h).  The round-1 kernel was bound by fp64 VALU issue
// (1 456 v_*_f64 per wave per pair).  n = 16^3, input index j = 256 a + 16 b + c, output f = k1 + 16 k2 + 256 k3:
//     X[f] = sum_c W_16^(c (k3 + (k1 + 16 k2)/256))  sum_b W_16^(b (k2 + k1/16))  sum_a W_16^(a k1) x[j]
// i.e. a plain 16-point DFT followed by two GENERALISED 16-point DFTs whose per-thread phase shift delta
// (k1/16 for pass 2, (k1 + 16 k2)/256 for pass 3) carries what used to be 2 x 15 twiddle multiplications per
// thread; each generalised pass is 32 butterflies of 6 FMAs (192 instead of 160 + 60), the plain pass 148
// instead of 160, and the multiplication by the reference spectrum is folded into the first stage of the second
// transform's plain pass (196 instead of 64 + 160).  Per thread and pair: 532 + 580 instead of 2 x 600 + 64
// fp64 instructions in the transforms, and 8 + 16 + 8 table loads from L2 instead of 15 + 16 + 15
// (fold_device.h: every stage's twiddles are one of eight per-thread constants times 1 or -i).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

#include "n4096_pair_device.h"

namespace muse {

// PADDED (2048 < N < 4096, leading zero pad): as in xcorr_r16_fast.hip -- the transforms run on d, sum d is read
// off the DC bin and the 16 values a lane ends with are corrected by -m c1[index] before the argmax.
// F32: float32-storage group (half the HBM bytes; samples widened exactly on consumption, same float64 arithmetic)
// WIN: masked argmax (muse_batch_score_in_window): the values outside the lag window p.win_lpos / p.win_lneg are replaced by +0.0
// right in front of the argmax (behind the PADDED correction); everything else is the kernel as it is
// SLIDE: the slide of the group's rows fused into the pass (muse_batch_slide_score_in_window): the loaders read the NEW row -- old
// row[slide_k .. N) followed by the row's tail samples (p.slide_tails), on the lane-to-column mapping of the stand-alone build, so the
// scores are its bits -- and every thread stores the raw values it loaded back to the same positions of the row: one read and one
// write of the rows where launch_row_slide and this kernel move them three times.  Everything behind the loads is the kernel as it
// is.  A shift inside a row overlaps its own source; the rules that keep it free of races (as row_slide.hip and
// xcorr_window_slide.hip state theirs):
//   1. A pair's rows are touched by ONE workgroup, ONCE: the pair hand-out gives every pair to exactly one workgroup.
//   2. Every load of a pair by every thread of the workgroup has RETURNED before any store to that pair: an explicit
//      s_waitcnt vmcnt(0) lgkmcnt(0) (not the per-register waits in front of a store's operand; a row's first sample may come through
//      the scalar cache), then a workgroup barrier, then the stores.
//   3. That barrier is an extra one, in front of d = x - K: the raw pair is consumed there (128 registers: it cannot live on to one
//      of the transposes' barriers).
//   4. The prefetch of the next pair reads another pair's rows and tails: nothing to order.
//   5. The last iteration's dummy prefetch of pair 0 is only loaded: the stores sit at the head of an iteration, which a
//      workgroup enters for a pair it has claimed (pair < npairs) and for nothing else.
//   6. With M odd the last pair's row B is a clamped copy of row A: loaded, never stored (hasB).
//   7. Stores go to samples 0 <= j < N of rows r < M only: a pad position (PADDED, j < 0) is loaded from the row's first sample and
//      never stored; the guard in front of row 0 and the rows behind the last one are never written.
//   8. The rescaling launch over ovf_list runs behind this kernel on the stream and reads the slid rows, as it is.
template <bool TIMING = false, bool PADDED = false, bool F32 = false, bool WIN = false, bool SLIDE = false>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_fused_n4096_fold(const FusedParams p)
{
    foldk::pair_loop_from_rows<TIMING, PADDED, F32, WIN, SLIDE>(p, foldk::NoTap{});
}
// The WIN build with the signed mask (muse_batch_score_signed_in_lag_range; FusedParams::win_sign): NEG false / true = the largest
// positive / the most negative value inside the window.  A kernel of its own, so that the ones above keep their symbols.
template <bool PADDED, bool F32, bool NEG>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_fused_n4096_fold_signed(const FusedParams p)
{
    foldk::pair_loop_from_rows<false, PADDED, F32, true, false, foldk::NoTap, NEG ? -1 : 1>(p, foldk::NoTap{});
}
// The WIN build with the band mask (muse_batch_score_in_lag_band; FusedParams::win_band): the argmax over the one index interval
// p.win_a .. p.win_b, by magnitude (SGN = 0) or over the values of one sign (+-1).  A kernel of its own again.
template <bool PADDED, bool F32, int SGN>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_fused_n4096_fold_band(const FusedParams p)
{
    foldk::pair_loop_from_rows<false, PADDED, F32, true, false, foldk::NoTap, SGN, true>(p, foldk::NoTap{});
}

// ============================================================================
// Many references against one resident group in ONE pass over the rows
// (the README use case iterates references over a fixed set of
// series).  Each pair of series is read from HBM and forward-transformed once; its
// spectrum Z (DC bin zeroed) STAYS IN REGISTERS for the R references, each of which costs one
// spectrum multiply, one transform and one argmax.  Per (series, reference) that is
// (1 + R) / (2 R) of the single-reference transform work and 1/R of the HBM bytes.
// (Round 2 parked Z in a 64 KB slice of global scratch per resident workgroup: 67 MB against
// 4 MB of L2 per XCD, i.e. 9 x the row bytes through the memory side,
// profiles/r01_many_refs_rocprof_summary.txt; that traffic is gone.)
//
// Two workgroups per CU with 256 registers per lane and 72 KB of LDS each (measured against three at
// 168 registers with a quarter of Z in LDS: +4 %, profiles/r03_many_references.txt), spent on what
// hides latency at that occupancy: every transpose goes through a FULL 16 x 272 buffer (two barriers
// instead of five), the next reference's sixteen spectrum factors are requested one iteration ahead,
// the eight pass-3 factors travel under the transpose in front of the pass (R = 8, 400 000 x 4096:
// 1.64 -> 1.70 -> 1.76 -> 1.86e8 series-references/s step by step, profiles/r03_many_references.txt).  The last reference of
// a pair is peeled out of the reference loop: Z dies in its first stage, and its registers take the
// next pair's rows, requested right behind that stage.
namespace foldk {

constexpr int MSTAT = 12; // per pair: [0,8) sum d^2 partials (2*wave + series), [8,10) sum d, [10] first row, [11] has second row
constexpr int MTRIP = 26; // per iteration: [0,24) argmax partials, [24] reference index (< 0: nothing to write), [25] pair parity

__device__ __forceinline__ bool finalize_multi(const double *tr, const double *st, const int series, const double invN,
                                               const double invNm1, double *mv_out, int *lag_out)
{
    double m[4], s[4], ix[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        m[w] = tr[6 * w + 3 * series];
        s[w] = tr[6 * w + 3 * series + 1];
        ix[w] = tr[6 * w + 3 * series + 2];
    }
    const double s2 = (st[series] + st[2 + series]) + (st[4 + series] + st[6 + series]);
    const Stat stt{st[8 + series], s2};
    double best = m[0], bsv = s[0], bidx = ix[0];
#pragma unroll
    for (int w = 1; w < 4; w++) {
        if (m[w] > best || (m[w] == best && ix[w] < bidx)) {
            best = m[w];
            bsv = s[w];
            bidx = ix[w];
        }
    }
    bool zero, nan;
    const double var = variance(stt, invN, invNm1, zero, nan);
    const int idx = (best > 0.0) ? (int)bidx : 0;
    double y = __builtin_amdgcn_rsq(var);
    y = y * fma(-0.5 * var * y, y, 1.5);
    y = y * fma(-0.5 * var * y, y, 1.5);
    double mv = ((best > 0.0) ? bsv : s[0]) * y;
    int lag = idx > 2048 ? idx - 4096 : idx;
    if (zero) { mv = 0.0; lag = 0; }
    if (nan) { mv = __builtin_nan(""); lag = 0; }
    *mv_out = mv;
    *lag_out = lag;
    bool redo = nan;
    if (series == 0 && st[11] != 0.0) { // sigmas too far apart for one shared transform?
        const Stat sb{st[9], (st[1] + st[3]) + (st[5] + st[7])};
        bool zb, nb;
        const double varb = variance(sb, invN, invNm1, zb, nb);
        redo = redo || (!nb && sigma_spread_too_wide(var, varb));
    }
    return redo;
}

// the previous iteration's results, written behind the first barrier of the current one
// (a free function on purpose: a by-reference lambda with two call sites is not inlined and
// drags the kernel argument struct into private memory)
__device__ __forceinline__ void finalize_prev_multi(const double *trip, const double *stats, const int cur_ip,
                                                    const int t, const double invN, const double invNm1,
                                                    double *const *mv_many, int *const *lag_many, int *ovf_count,
                                                    long long *ovf_list)
{
    const double *const tr = trip + MTRIP * (cur_ip ^ 1);
    const int series = t >> 6; // lane 0 of waves 0 / 1 writes one series' result each
    if ((t & 63) == 0 && series < 2 && tr[24] >= 0.0) {
        const double *const st = stats + MSTAT * (int)tr[25];
        if (series == 0 || st[11] != 0.0) {
            const int r = (int)tr[24];
            const long long row = (long long)st[10] + series;
            if (finalize_multi(tr, st, series, invN, invNm1, mv_many[r] + row, lag_many[r] + row) && r == 0) {
                const int slot = atomicAdd(ovf_count, 1);
                ovf_list[slot] = row >> 1;
            }
        }
    }
}

} // namespace foldk

constexpr int MULTI_WGS_PER_CU = 2;

// PADDED (2048 < N < 4096): the spectrum keeps its DC bin and every reference's results are corrected by
// -m c1_r[index] (FusedParams::c1_many) before the argmax.
// F32: float32-storage group (rows widened as they are consumed, float64 arithmetic)
// TIMING: the phase-stamped build of tools/ablate/multi_phases.hip (FusedParams::dbg); the product kernel below is <.., false>.
// WIN: masked argmax (muse_batch_score_many_in_window): every reference's values outside the ONE lag window p.win_lpos / p.win_lneg
// are replaced by +0.0 right in front of its argmax (behind the PADDED correction), as in xcorr_fused_n4096_fold
// SGN / BAND (with WIN; muse_batch_score_many_in_lag_band): the sign and / or the one index interval p.win_a .. p.win_b in the mask
// (mask_window_quot_band); 0 / false is the build above, its mask call unchanged
template <bool PADDED, bool F32, bool TIMING, bool WIN = false, int SGN = 0, bool BAND = false>
__device__ __forceinline__ void fold_multi_body(const FusedParams &p)
{
    using namespace occ4;
    using namespace fold;
    using namespace foldk;
    __shared__ double2 xbuf[OCC_XBUF_FULL];
    __shared__ double2 g2s[128];
    __shared__ double stats[2 * MSTAT];
    __shared__ double trip[2 * MTRIP];
    __shared__ int next_s[2];
    const PairThread th = pair_prologue<PADDED>(p, g2s, trip + 24, MTRIP);
    const int t = th.t, lane = th.lane, wave = th.wave;
    const double invN = th.invN, invNm1 = th.invNm1;
    double2 *const xw = xbuf + 1088 * wave;
    const int pad = PADDED ? 4096 - p.N : 0;
    const int R = p.R;
    PhaseClock<TIMING> clk;
    __syncthreads();
    clk.start();

    int ip = 0, pp = 0;
    const long long total = p.npairs;
    RawPair raw;
    constexpr bool WIDE = !PADDED && !F32;
    request_rows<PADDED, F32>(raw, p, blockIdx.x < total ? (long long)blockIdx.x : 0ll, t, pad);
    // reference r's sixteen spectrum factors of this thread (lane-ordered table, L2): requested one iteration ahead
    const auto request_spectrum = [&](double2 (&xf)[16], const int r) __attribute__((always_inline)) {
        const XcFetch xr{uniform_ptr(p.xcp_many[r]), t}; // the table pointer is wave-uniform: kept in SGPRs
#pragma unroll
        for (int j = 0; j < 16; j++)
            xf[j] = xr(j);
    };

    // one reference: V = Z conj(X_r) / n (factors xf, requested earlier), cc = FFT(V), argmax -> trip[ip]; `v` holds Z on entry.
    // `ahead()` runs in front of the last stage of the last pass: the place to request what the NEXT iteration needs.
    // `early()` runs right behind the spectrum multiply (the last reference: Z is dead there, its registers can take the next pair's rows).
    // `g3_first`: pass 3's factors are requested IN FRONT of early() -- loads return in order, so a factor requested behind the
    // next pair's rows could only be used once those rows (HBM latency) have arrived.
    const auto correlate = [&](double2 (&v)[16], const double2 (&xf)[16], const int r, const double *st, auto g3_first, auto early, auto ahead) __attribute__((always_inline)) {
        double *const tr = trip + MTRIP * ip;
        clk.template stamp<13>();
        xc_stage1_pre(v, xf);
        fence();
        double2 g3[8];
        if (decltype(g3_first)::value) {
#pragma unroll
            for (int q = 0; q < 8; q++)
                g3[q] = G3Fetch{p.g3b, t}(q);
            fence();
        }
        early();
        fence();
        clk.template stamp<6>();
        dft16_rn_s234(v);
        clk.template stamp<7>();
        exchange_local_full<0>(v, xw, t);
        clk.template stamp<8>();
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        if (!decltype(g3_first)::value) { // pass 3's factors travel under the transpose
#pragma unroll
            for (int q = 0; q < 8; q++)
                g3[q] = G3Fetch{p.g3b, t}(q);
        }
        fence();
        clk.template stamp<9>();
        exchange_cross_full<1, 1>(v, xbuf, t);
        if (r > 0) // (r == 0: the previous iteration's results went out behind the forward transform's first barriers)
            finalize_prev_multi(trip, stats, ip, t, invN, invNm1, p.mv_many, p.lag_many, p.ovf_count, p.ovf_list);
        clk.template stamp<10>();
        gdft16_nr_s12(v, g3[0], g3[1]); // cc index t + 256 m3 at v[BR16(m3)]
        gdft16_nr_s3(v, g3[2], g3[3]);
        fence();
        ahead();
        fence();
        gdft16_nr_s4(v, g3[4], g3[5], g3[6], g3[7]);
        if (PADDED) // with reference r's table
            correct_padded<4>(v, uniform_ptr(p.c1_many[r]), t, st[8] * invN, st[9] * invN);
        if constexpr (WIN && (SGN != 0 || BAND)) // cc index t + 256 m3 at v[BR16(m3)]
            mask_window_quot_band<true, 256, SGN, BAND>(v, tl<true>(t), BAND ? p.win_b : p.win_lpos, BAND ? p.win_a : 4096 - p.win_lneg);
        else if (WIN)
            mask_window_quot<true, 256>(v, tl<true>(t), p.win_lpos, 4096 - p.win_lneg);
        clk.template stamp<11>();
        wave_argmax_store(v, wave, lane, tr + 6 * wave);
        if (wave == 0 && lane == 0) {
            tr[24] = (double)r;
            tr[25] = (double)pp;
        }
        ip ^= 1;
        clk.template stamp<12>();
    };

    long long nextpair = 0;
#pragma clang loop unroll(disable)
    for (long long pair = blockIdx.x; pair < total; pair = nextpair) {
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const st = stats + MSTAT * pp;
        if (t == 0) // claim the pair after this one (read at the last reference, many barriers later)
            next_s[pp] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
        // ---------- rows -> Z = FFT(dA + i dB), as in xcorr_fused_n4096_fold
        double2 Z[16];
        MUSE_CONSUME_ROWS(WIDE, raw, Z, st, t, lane, wave, rA, hasB)
        double2 xf[16];
        fence();
        clk.template stamp<0>();
        request_spectrum(xf, 0); // (the rows' registers are free again: the first reference's factors travel under the forward transform)
        fence();
        dft16_nr(Z);
        clk.template stamp<1>();
        exchange_cross_full<0, 1>(Z, xbuf, t, WIDE ? wide_column(t) : -1);
        finalize_prev_multi(trip, stats, ip, t, invN, invNm1, p.mv_many, p.lag_many, p.ovf_count, p.ovf_list);
        clk.template stamp<2>();
        gdft16_nr(Z, G2Fetch{g2s, t >> 4});
        {
            double2 g3[8]; // pass 3's factors travel under the transpose
#pragma unroll
            for (int q = 0; q < 8; q++)
                g3[q] = G3Fetch{p.g3a, t}(q);
            fence();
            clk.template stamp<3>();
            exchange_local_full<1>(Z, xw, t);
            clk.template stamp<4>();
            gdft16_nr_s12(Z, g3[0], g3[1]); // Z[hi + 16 lo + 256 k3] at Z[BR16(k3)]
            gdft16_nr_s3(Z, g3[2], g3[3]);
            gdft16_nr_s4(Z, g3[4], g3[5], g3[6], g3[7]);
        }
        {
            double s1a, s1b;
            take_dc<PADDED>(Z, t, s1a, s1b);
            if (wave == 0 && lane == 0) { // (PADDED: every lane needs the means before each argmax of this pair: many barriers away)
                st[8] = s1a;
                st[9] = s1b;
            }
        }
        clk.template stamp<5>();
#pragma clang loop unroll(disable)
        for (int r = 0; r + 1 < R; r++) {
            double2 v[16], xn[16];
#pragma unroll
            for (int k = 0; k < 16; k++)
                v[k] = Z[k];
            correlate(v, xf, r, st, std::false_type{}, [&]() __attribute__((always_inline)) {}, [&]() __attribute__((always_inline)) { request_spectrum(xn, r + 1); });
#pragma unroll
            for (int k = 0; k < 16; k++)
                xf[k] = xn[k];
        }
        {   // the last reference: Z dies in its first stage and the next pair's rows are requested right behind it -- a whole
            // reference iteration (~ 5 us) ahead of their use
            nextpair = __builtin_amdgcn_readfirstlane(next_s[pp]);
            const long long nxt = nextpair < total ? nextpair : 0; // nothing left: pair 0 (L2-resident dummy)
            if (WIN) { // (the spectrum as the loop left it: nothing derived from it for this stage -- nine negated components -- is formed
                       // in front of the reference loop and carried across it; with the mask's registers they went to scratch)
#pragma unroll
                for (int k = 0; k < 16; k++)
                    asm volatile("" : "+v"(Z[k].x), "+v"(Z[k].y));
            }
            correlate(Z, xf, R - 1, st, std::true_type{}, [&]() __attribute__((always_inline)) { request_rows<PADDED, F32>(raw, p, nxt, t, pad); }, [&]() __attribute__((always_inline)) {});
        }
        pp ^= 1;
    }
    lds_barrier();
    finalize_prev_multi(trip, stats, ip, t, invN, invNm1, p.mv_many, p.lag_many, p.ovf_count, p.ovf_list);
    if (TIMING && p.dbg && lane == 0) {
#pragma unroll
        for (int i = 0; i < NPHASE; i++)
            p.dbg[((long long)blockIdx.x * 4 + wave) * NPHASE + i] = clk.acc[i];
    }
}

template <bool PADDED = false, bool F32 = false, bool WIN = false>
__global__ __launch_bounds__(OCC_THREADS, MULTI_WGS_PER_CU) void xcorr_fused_n4096_fold_multi(const FusedParams p)
{
    fold_multi_body<PADDED, F32, false, WIN>(p);
}

// the WIN build with the signed and / or the band mask (muse_batch_score_many_in_lag_band; FusedParams::win_sign / ::win_band): one
// sign and one window or band for every reference; a kernel of its own, so that xcorr_fused_n4096_fold_multi keeps its symbols
template <bool PADDED, bool F32, int SGN, bool BAND>
__global__ __launch_bounds__(OCC_THREADS, MULTI_WGS_PER_CU) void xcorr_fused_n4096_fold_multi_band(const FusedParams p)
{
    static_assert(SGN != 0 || BAND, "by magnitude inside a window that holds lag 0: xcorr_fused_n4096_fold_multi<PADDED, F32, true>");
    fold_multi_body<PADDED, F32, false, true, SGN, BAND>(p);
}

// R >= 1 references, n == 4096 (N < 4096: p.c1_many); p.ovf_count and p.work_counter zeroed; a resident grid
// (pairs are handed out dynamically)
hipError_t launch_fused_multi(const FusedParams &p_in, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    const long long grid = std::min<long long>(p.npairs, (long long)num_cus * MULTI_WGS_PER_CU);
    if (!p.work_counter || p.R < 1 || !p.g2 || !p.g3a || !p.g3b || !p.xcp_many || !p.mv_many || !p.lag_many)
        return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(OCC_THREADS);
    if ((p.N < 4096 && !p.c1_many) || !window_bounds_ok(p)) // (one window for every reference: muse_batch_score_many_in_window)
        return hipErrorInvalidValue;
    if (p.win_sign || p.win_band) { // one sign and one window or band for every reference (muse_batch_score_many_in_lag_band)
        if (!p.win || p.win_sign < -1 || p.win_sign > 1)
            return hipErrorInvalidValue;
        with_bools([&](auto padded, auto f32, auto band) {
            with_sign(p.win_sign, [&](auto sgn) {
                if constexpr (decltype(sgn)::value != 0 || decltype(band)::value)
                    hipLaunchKernelGGL((xcorr_fused_n4096_fold_multi_band<decltype(padded)::value, decltype(f32)::value, decltype(sgn)::value, decltype(band)::value>),
                                       g, b, 0, stream, p);
            });
        }, p.N < 4096, p.rows32 != nullptr, p.win_band != 0);
        return hipGetLastError();
    }
    with_bools([&](auto padded, auto f32, auto win) {
        hipLaunchKernelGGL((xcorr_fused_n4096_fold_multi<decltype(padded)::value, decltype(f32)::value, decltype(win)::value>), g, b, 0, stream, p);
    }, p.N < 4096, p.rows32 != nullptr, p.win != 0);
    return hipGetLastError();
}

// n == 4096 (N < 4096: p.c1 required); p.ovf_count / work_counter must be zeroed and p.ovf_list hold 2*npairs entries;
// a resident grid, pairs handed out by the atomic counter
hipError_t launch_fused_fold(const FusedParams &p_in, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    if (!p.work_counter || !p.g2 || !p.g3a || !p.g3b || !p.xcp)
        return hipErrorInvalidValue;
    const long long grid = std::min<long long>(p.npairs, (long long)num_cus * 4);
    if (p.N < 4096 && !p.c1) // leading zero pad: needs the batch's correction table
        return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(OCC_THREADS);
    if (!window_bounds_ok(p)) // (the masked argmax: muse_batch_score_in_window)
        return hipErrorInvalidValue;
    // the slide fused into the pass (muse_batch_slide_score_in_window): the rows are rewritten in place.  Every pair is claimed once
    // (pair_list / dense_total belong to the rescaling kernel); the rows are dense float64 pairs of 16-byte aligned rows where the
    // kernel moves them in 16-byte units
    if (p.slide_tails && (p.slide_k < 1 || p.slide_k > p.N || p.N <= 2048 || p.N > 4096 || p.stride < p.N || p.pair_list || p.npairs != (p.M + 1) / 2 ||
                          (p.N == 4096 && !p.rows32 && !window_wide(p.rows, p.stride))))
        return hipErrorInvalidValue;
    if (p.win_band) { // the band mask: a window, a sign of -1 .. 1, no slide
        if (!p.win || p.win_sign < -1 || p.win_sign > 1 || p.slide_tails)
            return hipErrorInvalidValue;
        with_bools([&](auto padded, auto f32) {
            with_sign(p.win_sign, [&](auto sgn) {
                hipLaunchKernelGGL((xcorr_fused_n4096_fold_band<decltype(padded)::value, decltype(f32)::value, decltype(sgn)::value>), g, b, 0, stream, p);
            });
        }, p.N < 4096, p.rows32 != nullptr);
        return hipGetLastError();
    }
    if (p.win_sign) { // the signed masked argmax: a window, a sign of +-1, no slide
        if (!p.win || (p.win_sign != 1 && p.win_sign != -1) || p.slide_tails)
            return hipErrorInvalidValue;
        with_bools([&](auto padded, auto f32, auto neg) {
            hipLaunchKernelGGL((xcorr_fused_n4096_fold_signed<decltype(padded)::value, decltype(f32)::value, decltype(neg)::value>), g, b, 0, stream, p);
        }, p.N < 4096, p.rows32 != nullptr, p.win_sign < 0);
        return hipGetLastError();
    }
    with_bools([&](auto padded, auto f32, auto win, auto slide) {
        hipLaunchKernelGGL((xcorr_fused_n4096_fold<false, decltype(padded)::value, decltype(f32)::value, decltype(win)::value, decltype(slide)::value>), g, b, 0, stream, p);
    }, p.N < 4096, p.rows32 != nullptr, p.win != 0, p.slide_tails != nullptr);
    return hipGetLastError();
}

} // namespace muse

#undef MUSE_CONSUME_ROWS // (n4096_pair_device.h: this file is its last user)
