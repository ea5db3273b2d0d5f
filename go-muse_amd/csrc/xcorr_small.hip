// xcorr_small.hip -- fp64 kernels for the FFT lengths n = 512, 1024, 2048, 8192, 16384 (every config-5 length whose pair of
// series fits one workgroup's registers; n = 4096 has its own kernel, xcorr_r16_fold.hip), round 2.
//
// Mathematics: xCorrWithX, /root/reference/xcorr.go:160-197, two series per complex transform, radix-16 Stockham
// passes as in xcorr_stockham.hip (n = R1 * 16^(P-1): P = 3 with R1 = 2, 4, 8 for n <= 2048, P = 4 with R1 = 2, 4 for
// n = 8192, 16384; every thread owns the 16 points x[j + i S], S = n / 16; S threads per pair).  What is different from
// the round-1 kernels of these lengths:
//   * Occupancy.  Round 1 kept a full padded work buffer per pair (n complex = 69.6 KB per 256-thread workgroup):
//     two workgroups = 8 waves per CU, and every profile said the kernels were bound by that, not by arithmetic
//     (profiles/r01_sizes_*: 24-27 % of the HBM roofline).  Here every transpose runs in TWO HALF ROUNDS through a
//     buffer of n / 2 points (8.7 KB per wave: 16 waves per CU at 128 VGPRs for every length), and in all transposes
//     EVERY lane reads eight values per round (no idle half as in the n = 4096 kernel's wave-local transposes):
//       A (after the radix-R1 pass): writer j, output (m, r) -> position (j + m S) R1 + r; reader j reads j + i S.
//         Round h carries the positions [8 S h, 8 S (h + 1)): the outputs m in [h Q1/2, (h+1) Q1/2) of every lane, read
//         back as the inputs i in [8 h, 8 h + 8) of every lane.
//       B (between radix-16 passes, Ns -> 16 Ns): writer j = g Ns + m, output r -> position g 16 Ns + r Ns + m.
//         Round h: the lower / upper half of the columns write all sixteen outputs; every lane reads its inputs
//         i in [8 h, 8 h + 8).  Where both halves sit in one wave (n = 512, 1024) they first trade eight registers
//         (v_permlane16/32_swap) so that every lane stores eight values in each round (level()).
//   * No workgroup barrier for n <= 1024: a pair lives inside one wave (n = 512: two pairs per wave) and LDS
//     operations of one wave execute in order.  n >= 2048: a pair spans 2, 8 or 16 waves = the workgroup, the half rounds
//     are separated by workgroup barriers; its reductions share one exchange and one barrier per kind (pair_sum4 ...).
//   * Arithmetic: every radix-16 pass is a generalised 16-point transform with the twiddles folded into the
//     butterflies (fold_device.h: 192 instructions and eight table entries per pass instead of 264 and four), and the
//     second transform is the forward algorithm again (xcorr_stockham.hip, lds_transforms).
//   * Tables: pass 2's 8 x R1 factors from an LDS copy (a broadcast read; gathered per lane out of the W_65536 table they
//     were the longest stall of the kernel), the later passes' from lane-ordered per-length tables (coalesced).
//   * Lanes are relabelled to columns so that LDS read groups and write groups meet no bank conflicts (column_of_lane()).
//   * MULTI: R references in one pass (muse_batch_score_many): the pair's spectrum stays in registers (n <= 8192: 256 VGPRs, half
//     the resident waves; round 2 parked it in global scratch: x 1.4 per reference at R = 8, now x 1.5 - 1.8) or is parked per
//     workgroup (n = 16384), and every reference takes product, second transform and argmax from there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "fold_device.h"
#include "r16_device.h"
#include "small_device.h"
#include "two_device.h"

namespace muse {

// PADDED: N < n (leading zero pad); N == n needs no per-sample validity masks
// Workgroup: 256 threads (n <= 1024: pairs never leave a wave, the workgroup is only a scheduling unit) or the 128 threads
// of ONE pair (n = 2048: the barriers of the half rounds then couple the pair's two waves and nobody else).
// MULTI: R references against the group in one pass (muse_batch_score_many): rows are loaded, reduced and transformed
// once; the pair's spectrum is parked lane-ordered in the workgroup's slice of p.zscratch (L2 / MALL resident, every
// thread re-reads only what it wrote) and every reference takes product, second transform and argmax from there.
// F32: float32-storage group (muse_group_create_f32, opt-in): the rows are float32 in HBM, widened exactly as they are
// consumed; the arithmetic is the float64 arithmetic of the float64 groups.
// ZREG (MULTI, n <= 8192): the pair's spectrum stays in REGISTERS over the references (256 VGPRs: half the resident waves)
// instead of being parked in the workgroup's slice of global scratch (n = 16384: 1024 threads per pair cap a lane at 128).
// WIN (n <= 2048; float64 rows with MULTI): masked argmax (muse_batch_score_in_window, muse_batch_score_many_in_window; r16_device.h,
// mask_window) -- the values outside the lag window p.win_lpos / p.win_lneg (MULTI: one window for every reference) are replaced by
// +0.0 right in front of the argmax
// SGN (xcorr_small_body.h, the body of this kernel and of xcorr_fused_small_signed below, included into each: the text of one kernel
// compiled under two names, so that this one keeps its symbols and its code): 0 here; +-1 = the signed mask of the WIN build
// (muse_batch_score_signed_in_lag_range)
template <int LOGN, bool PADDED, bool MULTI, bool F32 = false, bool WIN = false>
__global__ __launch_bounds__((LOGN >= 11 ? (1 << LOGN) / 16 : 256), ((MULTI && LOGN <= 13) ? 2 : 4)) void xcorr_fused_small(const FusedParams p)
{
    constexpr int SGN = 0;
    constexpr bool BAND = false;
#include "xcorr_small_body.h"
}
// the WIN build with the signed mask (FusedParams::win_sign), one reference: NEG false / true = the largest positive / the most
// negative value inside the window
template <int LOGN, bool PADDED, bool F32, bool NEG>
__global__ __launch_bounds__((LOGN >= 11 ? (1 << LOGN) / 16 : 256), 4) void xcorr_fused_small_signed(const FusedParams p)
{
    constexpr bool MULTI = false, WIN = true;
    constexpr int SGN = NEG ? -1 : 1;
    constexpr bool BAND = false;
#include "xcorr_small_body.h"
}
// the WIN build with the band mask (muse_batch_score_in_lag_band; FusedParams::win_band), one reference: the argmax over the one index
// interval p.win_a .. p.win_b, by magnitude (SGN = 0) or over the values of one sign (+-1)
template <int LOGN, bool PADDED, bool F32, int SGN>
__global__ __launch_bounds__((LOGN >= 11 ? (1 << LOGN) / 16 : 256), 4) void xcorr_fused_small_band(const FusedParams p)
{
    constexpr bool MULTI = false, WIN = true, BAND = true;
#include "xcorr_small_body.h"
}
// the MULTI + WIN build with the signed and / or the band mask (muse_batch_score_many_in_lag_band): R references in one pass, one
// sign and one window or band for all of them; float64 rows, as every MULTI + WIN build (SGN = 0 without BAND is xcorr_fused_small's)
template <int LOGN, bool PADDED, int SGN, bool BAND>
__global__ __launch_bounds__((LOGN >= 11 ? (1 << LOGN) / 16 : 256), 2) void xcorr_fused_small_many_band(const FusedParams p)
{
    static_assert(SGN != 0 || BAND, "by magnitude inside a window that holds lag 0: xcorr_fused_small<LOGN, PADDED, true, false, true>");
    constexpr bool MULTI = true, F32 = false, WIN = true;
#include "xcorr_small_body.h"
}

// The batched two-sided xCorr (xcorr.go:102-153) on the same transforms: pair i = (x_i, y_i), each zero-padded
// in front on its own (any Nx, Ny <= n).  With xr[j] = x[-j mod n] (the row read backwards: an address pattern) and
// z = xr + i y:  conj(X) = FFT(xr), Z = FFT(z) = Xr + i Y, Z^2 = (Xr^2 - Y^2) + 2 i Xr Y, so
//     cc = FFT(conj(X) Y) / n = Im FFT(Z^2) / (2 n)
// -- two forward transforms per pair as above, the spectrum product a square of what the thread already holds: no
// table, no mirrored element Z[-f] (round 3's first version fetched it through the Stockham engine's natural-order LDS image).
// Statistics first (xcorr.go:108-128: either sigma == 0 -> nil), both series centred and scaled to O(1) by exact powers of
// two (two_device.h).  Rows are requested where they are used: the kernel is bound by its arithmetic.
template <int LOGN, bool PADDED>
__global__ __launch_bounds__((LOGN >= 11 ? (1 << LOGN) / 16 : 256), 4) void xcorr_two_sided_small(const FusedParams p, const two::PairInv iv)
{
    using namespace occ4;
    using namespace fold;
    using namespace small;
    constexpr int n = 1 << LOGN;
    constexpr int S = n / 16;
    constexpr int TPB = LOGN >= 11 ? S : 256;
    constexpr int G = TPB / S;
    static_assert((LOGN >= 9 && LOGN <= 11) || LOGN == 13 || LOGN == 14, "n = 512, 1024, 2048, 8192, 16384");
    __shared__ double red[112];
    constexpr int NP_ = (LOGN + 3) / 4, R1_ = n >> (4 * (NP_ - 1));
    __shared__ double2 g2l[8 * R1_];
    __shared__ double2 xbuf[(TPB / 64) * 544];
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = S >= 64 ? __builtin_amdgcn_readfirstlane(t / S) : t / S;
    const int j = column_of_lane<LOGN>(t % S);
    double2 *const b = xbuf + g * (8 * S + S / 2);
    const int padx = PADDED ? n - p.Nx : 0, pady = PADDED ? n - p.N : 0;
    const bool normalize = p.normalize_y != 0;
    const double2 *__restrict__ twm = p.twm;
    const double2 *__restrict__ gs = p.gsmall;
    if (t < 8 * R1_)
        g2l[t] = tw_factor<R1_>(twm, t % R1_, t / R1_);
    __syncthreads();
    const long long total = p.npairs;
    const long long ngroups = (total + G - 1) / G;
    for (long long it = blockIdx.x; it < ngroups; it += gridDim.x) {
        const long long slot = it * G + g;
        const bool live = slot < total;
        const long long pair = live ? slot : total - 1; // idle sub-groups shadow the last pair
        const double *const rx = p.xrows + pair * p.xstride, *const ry = p.rows + pair * p.stride;
        double2 v[16];
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        {
            const double KA = normalize ? rx[0] : 0.0, KB = normalize ? ry[0] : 0.0;
            // position e = j + i S of the padded arrays holds y[e - pady] and x[(-e mod n) - padx]; four batches of four
#pragma unroll
            for (int h = 0; h < 4; h++) {
                double xa[4], yb[4];
                int jb = j;
                asm volatile("" : "+v"(jb)); // (a batch's offsets and masks are formed in the batch)
                jb &= S - 1;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int e = jb + (4 * h + k) * S;
                    const int ex = ((n - e) & (n - 1)) - padx, ey = e - pady;
                    if (S >= 64) { // the wave works on one pair: scalar bases + 32-bit lane offsets
                        xa[k] = __builtin_nontemporal_load(scalar_ptr(rx) + (unsigned)(PADDED && ex < 0 ? 0 : ex));
                        yb[k] = __builtin_nontemporal_load(scalar_ptr(ry) + (unsigned)(PADDED && ey < 0 ? 0 : ey));
                    } else {
                        xa[k] = __builtin_nontemporal_load(rx + (PADDED && ex < 0 ? 0 : ex));
                        yb[k] = __builtin_nontemporal_load(ry + (PADDED && ey < 0 ? 0 : ey));
                    }
                }
                fence();
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int e = jb + (4 * h + k) * S;
                    double da = xa[k] - KA, db = yb[k] - KB;
                    if (PADDED) {
                        da = ((n - e) & (n - 1)) - padx >= 0 ? da : 0.0;
                        db = e - pady >= 0 ? db : 0.0;
                    }
                    v[4 * h + k] = make_double2(da, db);
                    q[0] += da;
                    q[1] = fma(da, da, q[1]);
                    q[2] += db;
                    q[3] = fma(db, db, q[3]);
                }
            }
        }
        pair_sum4<S>(q[0], q[1], q[2], q[3], red, wave);
        const two::PairScale ps = two::pair_scale(q, iv, normalize);
        const bool dead = ps.nil || ps.nan;
        const double fac = ps.fac * (1.0 / (2.0 * n)); // (pair_scale's factor assumes a spectrum already divided by n; 1 / 2n is exact)
        {
            const double sA = dead ? 0.0 : ps.sA, sB = dead ? 0.0 : ps.sB, mA = dead ? 0.0 : ps.mA, mB = dead ? 0.0 : ps.mB;
            int jb = j;
            asm volatile("" : "+v"(jb)); // (the validity masks are recomputed, not kept across the statistics)
            jb &= S - 1;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int e = jb + i * S;
                const bool vx = !PADDED || ((n - e) & (n - 1)) - padx >= 0, vy = !PADDED || e - pady >= 0;
                v[i].x = vx ? fma(v[i].x, sA, -mA) : 0.0;
                v[i].y = vy ? fma(v[i].y, sB, -mB) : 0.0;
            }
        }
        forward<LOGN>(v, b, g2l, gs, j); // Z[j + r S] at v[BR16(r)]
        {
            double2 w[16];
#pragma unroll
            for (int r = 0; r < 16; r++) { // the square, renamed to natural order
                const double2 z = v[BR16(r)];
                w[r] = make_double2(fma(z.x, z.x, -(z.y * z.y)), (z.x + z.x) * z.y);
            }
#pragma unroll
            for (int r = 0; r < 16; r++)
                v[r] = w[r];
        }
        forward<LOGN>(v, b, g2l, gs, j); // 2 n cc[j + r S] at v[BR16(r)].y
        if (p.cc_out && live && !dead) {
            double *const cc = p.cc_out + pair * (long long)n;
#pragma unroll
            for (int r = 0; r < 16; r++)
                cc[j + r * S] = v[BR16(r)].y * fac;
        }
        // ---- maxAbsIndex (xcorr.go:39-50): ascending r = ascending index for this thread
        double sa = 0.0;
        int ra_ = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const double x = v[BR16(r)].y;
            const bool ga = fabs(x) > fabs(sa);
            sa = ga ? x : sa;
            ra_ = ga ? r : ra_;
        }
        const double ma = fabs(sa);
        const int ia = j + ra_ * S;
        const double cc0 = v[0].y; // (lane with j == 0: cc[0], reported when nothing is above 0)
        const double pa = pair_max<S>(ma, red, wave);
        const int ca = pair_min_i<S>((ma == pa && pa > 0.0) ? ia : 0x7fffffff, red + 96, wave);
        if (live) {
            const bool own = ca == 0x7fffffff ? j == 0 : (ia == ca && ma == pa);
            if (own) {
                const int idx = ca == 0x7fffffff ? 0 : ca;
                double mv = (ca == 0x7fffffff ? cc0 : sa) * fac;
                int lag = idx > n / 2 ? idx - n : idx;
                if (ps.nil) { mv = 0.0; lag = 0; }               // xcorr.go:110-127
                if (ps.nan) { mv = __builtin_nan(""); lag = 0; } // every cc is NaN: maxAbsIndex keeps index 0
                p.mv[pair] = mv;
                p.lag[pair] = lag;
                if (p.nil_out)
                    p.nil_out[pair] = ps.nil ? 1 : 0;
            }
        }
        if (S > 64)
            lds_barrier(); // (red is reused by the next pair's statistics)
    }
}

template <int LOGN>
static hipError_t launch_two_small_n(const FusedParams &p, int num_cus, hipStream_t stream)
{
    constexpr int TPB = LOGN >= 11 ? (1 << LOGN) / 16 : 256;
    constexpr int G = TPB / ((1 << LOGN) / 16);
    const long long ngroups = (p.npairs + G - 1) / G;
    const long long grid = std::min<long long>(ngroups, (long long)num_cus * (1024 / TPB) * 8);
    const two::PairInv iv = two::pair_inv(p.Nx, p.N, 1 << LOGN);
    if (p.Nx < (1 << LOGN) || p.N < (1 << LOGN))
        hipLaunchKernelGGL((xcorr_two_sided_small<LOGN, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p, iv);
    else
        hipLaunchKernelGGL((xcorr_two_sided_small<LOGN, false>), dim3((unsigned)grid), dim3(TPB), 0, stream, p, iv);
    return hipGetLastError();
}
// two-sided xCorr, n = 512, 1024, 2048, 8192, 16384 (launch_two_sided's argument checks apply)
hipError_t launch_two_sided_small(const FusedParams &p, int num_cus, hipStream_t stream)
{
    if (!p.xrows || !p.rows || !p.twm || !p.gsmall || !p.mv || !p.lag)
        return hipErrorInvalidValue;
    switch (p.logn) {
    case 9: return launch_two_small_n<9>(p, num_cus, stream);
    case 10: return launch_two_small_n<10>(p, num_cus, stream);
    case 11: return launch_two_small_n<11>(p, num_cus, stream);
    case 13: return launch_two_small_n<13>(p, num_cus, stream);
    case 14: return launch_two_small_n<14>(p, num_cus, stream);
    default: return hipErrorInvalidValue;
    }
}

template <int LOGN>
static hipError_t launch_small_n(const FusedParams &p, int num_cus, hipStream_t stream)
{
    constexpr int TPB = LOGN >= 11 ? (1 << LOGN) / 16 : 256;
    constexpr int G = TPB / ((1 << LOGN) / 16);
    const long long ngroups = (p.npairs + G - 1) / G;
    if (p.R > 1 && p.win && LOGN > 11)
        return hipErrorInvalidValue; // (the masked argmax is built for n = 512, 1024, 2048)
    if (p.win_sign && (!p.win || LOGN > 11 || (p.win_sign != 1 && p.win_sign != -1)))
        return hipErrorInvalidValue; // (the signed mask: a window, a sign of +-1; R > 1: xcorr_fused_small_many_band)
    if (p.win_band && (!p.win || LOGN > 11 || !band_bounds_ok(p, 1 << LOGN)))
        return hipErrorInvalidValue; // (the band mask: a window, one index interval on one side of lag 0; R > 1: xcorr_fused_small_many_band)
    if (p.R > 1) { // one pass for R references: exactly the resident workgroups (n = 16384: each with its slice of the spectrum scratch)
        constexpr bool ZREG = LOGN <= 13;
        if (!p.xcp_many || !p.mv_many || !p.lag_many || (!ZREG && !p.zscratch))
            return hipErrorInvalidValue;
        const long long grid = std::min<long long>(ngroups, (long long)num_cus * (ZREG ? std::max(1, 512 / TPB) : 1024 / TPB));
        if (!ZREG && (size_t)grid * TPB * 16 > (size_t)p.zslots * 4096)
            return hipErrorInvalidValue;
        if constexpr (LOGN <= 11) {
            if (p.win) { // the masked argmax, one window for every reference (muse_batch_score_many_in_window)
                if (p.pair_list || p.win_lpos < 0 || p.win_lneg < 0 || p.win_lpos > (1 << LOGN) / 2 || p.win_lneg > (1 << LOGN) / 2 - 1)
                    return hipErrorInvalidValue;
                if (p.win_sign || p.win_band) { // one sign and one band for every reference (muse_batch_score_many_in_lag_band)
                    with_bools([&](auto padded, auto band) {
                        with_sign(p.win_sign, [&](auto sgn) {
                            if constexpr (decltype(sgn)::value != 0 || decltype(band)::value)
                                hipLaunchKernelGGL((xcorr_fused_small_many_band<LOGN, decltype(padded)::value, decltype(sgn)::value, decltype(band)::value>),
                                                   dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                        });
                    }, p.N < (1 << LOGN), p.win_band != 0);
                    return hipGetLastError();
                }
                if (p.N < (1 << LOGN))
                    hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, true, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                else
                    hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, true, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                return hipGetLastError();
            }
        }
        if (p.N < (1 << LOGN))
            hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
        else
            hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
        return hipGetLastError();
    }
    const long long grid = std::min<long long>(ngroups, (long long)num_cus * (1024 / TPB) * 8);
    if (p.win) { // the masked argmax (muse_batch_score_in_window): n = 512, 1024, 2048
        if constexpr (LOGN <= 11) {
            if (p.pair_list || p.win_lpos < 0 || p.win_lneg < 0 || p.win_lpos > (1 << LOGN) / 2 || p.win_lneg > (1 << LOGN) / 2 - 1)
                return hipErrorInvalidValue;
            if (p.win_band) { // (muse_batch_score_in_lag_band)
                with_bools([&](auto padded, auto f32) {
                    with_sign(p.win_sign, [&](auto sgn) {
                        hipLaunchKernelGGL((xcorr_fused_small_band<LOGN, decltype(padded)::value, decltype(f32)::value, decltype(sgn)::value>),
                                           dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                    });
                }, p.N < (1 << LOGN), p.rows32 != nullptr);
                return hipGetLastError();
            }
            if (p.win_sign) { // (muse_batch_score_signed_in_lag_range)
                with_bools([&](auto padded, auto f32, auto neg) {
                    hipLaunchKernelGGL((xcorr_fused_small_signed<LOGN, decltype(padded)::value, decltype(f32)::value, decltype(neg)::value>),
                                       dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                }, p.N < (1 << LOGN), p.rows32 != nullptr, p.win_sign < 0);
                return hipGetLastError();
            }
            if (p.rows32) {
                if (p.N < (1 << LOGN))
                    hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, false, true, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
                else
                    hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, false, true, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
            } else if (p.N < (1 << LOGN))
                hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, false, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
            else
                hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, false, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (p.rows32) {
        if (p.N < (1 << LOGN))
            hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
        else
            hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, false, true>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
    } else if (p.N < (1 << LOGN))
        hipLaunchKernelGGL((xcorr_fused_small<LOGN, true, false>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
    else
        hipLaunchKernelGGL((xcorr_fused_small<LOGN, false, false>), dim3((unsigned)grid), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

// n = 512, 1024, 2048, 8192, 16384 (float64 rows); any N in (n/2, n]
// p.rows must carry n - N < n / 2 readable elements in front of row 0 (zero-padded rows are read unclamped and masked;
// capi_group.hip allocates every group with GROUP_GUARD >= SMALL_MAX_N / 2 such elements)
hipError_t launch_fused_small(const FusedParams &p_in, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    static_assert((1 << 14) <= SMALL_MAX_N, "the largest length built below");
    if ((!p.rows && !p.rows32) || !p.twm || (!p.xc && p.R <= 1) || !p.gsmall || (p.rows32 && p.R > 1))
        return hipErrorInvalidValue;
    switch (p.logn) {
    case 9: return launch_small_n<9>(p, num_cus, stream);
    case 10: return launch_small_n<10>(p, num_cus, stream);
    case 11: return launch_small_n<11>(p, num_cus, stream);
    case 13: return launch_small_n<13>(p, num_cus, stream);
    case 14: return launch_small_n<14>(p, num_cus, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace muse
