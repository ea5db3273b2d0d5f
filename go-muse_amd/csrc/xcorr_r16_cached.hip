// xcorr_r16_cached.hip -- the n = 4096 fp64 pass over a resident group's SPECTRUM CACHE (float64 rows, 2048 < N <= 4096).
//
// Of the two halves of xcorr_fused_n4096_fold (xcorr_r16_fold.hip) only the second depends on the reference: the first --
// shift by the first sample, sum of squares, Z = FFT(dA + i dB) -- depends on the group's rows alone, and a group is uploaded
// once and scored many times.  Z of a pair is 4096 double2 = 64 KB: exactly the bytes of the two rows it came from.  So a pass
// that reads Z instead of the rows moves the same HBM bytes and does about half the arithmetic, two of the four LDS
// transposes and five of the nine barriers.
//
//   zc[pair][i][t]   (double2) the value thread t holds in register v[i] right behind pass 3 of the first transform and its
//                    DC handling: register i of a workgroup is 4 KB contiguous, every access a full-width 16-byte one
//   zstat[pair][16]  (double)  [0, 8) the eight per-wave partial sums of d^2 (2 * wave + series), kept as partials and summed by
//                    finalize in the plain kernel's order; [8], [9] sum d of the two series (the DC bin)
//
// xcorr_cache_fill_n4096: the plain kernel plus the stores (results unchanged) over pairs [pair0, pair0 + npairs); the first
//                         `zpairs` of them are cached (0: none -- the plain arithmetic on a tail of the group).
// xcorr_cached_n4096:     per pair sixteen 16-byte loads of Z, requested one pair ahead where the plain kernel requests rows,
//                         the statistics through the scalar cache, then the plain kernel's second half, function by function:
//                         the same operations on the same doubles, so mv and lag come out bit for bit as from the rows.
// Pairs with NaN / Inf statistics or sigmas too far apart are listed exactly as by the plain kernel and redone FROM THE ROWS
// by the rescaling kernel behind the pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "foldk_device.h"

namespace muse {

namespace foldk {

#if defined(__HIP_DEVICE_COMPILE__)
typedef d2v __attribute__((address_space(1))) *zc_out_ptr;
typedef double __attribute__((address_space(1))) *zstat_out_ptr;
typedef const double __attribute__((address_space(4))) *zstat_in_ptr;
#endif

// the previous pair's results from its complete record: lane 0 of waves 0 / 1 writes one series each
__device__ __forceinline__ void finalize_prev(const double *prec, const int wave, const int lane, const double invN,
                                              const double invNm1, const FusedParams &p)
{
    if (lane == 0 && wave < 2 && prec[34] >= 0.0 && (wave == 0 || prec[35] != 0.0)) {
        const long long row = (long long)prec[34] + wave;
        if (finalize(prec, wave, invN, invNm1, p.mv + row, p.lag + row)) {
            const int slot = atomicAdd(p.ovf_count, 1);
            p.ovf_list[slot] = row >> 1;
        }
    }
}

} // namespace foldk

// ---------------------------------------------------------------------------------------------------------------- writer
template <bool PADDED>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_cache_fill_n4096(const FusedParams p, const SpectrumCacheArgs c)
{
    using namespace occ4;
    using namespace fold;
    using namespace foldk;
    __shared__ double2 xbuf[OCC_XBUF];
    __shared__ double2 g2s[128];
    __shared__ double red[2 * REC];
    __shared__ int next_s[2];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    double2 *const xw = xbuf + XW * wave;
    const int pad = PADDED ? 4096 - p.N : 0;
    const double invN = PADDED ? p.invN : 1.0 / 4096.0, invNm1 = PADDED ? p.invNm1 : 1.0 / 4095.0;

    if (t < 128)
        g2s[t] = p.g2[t];
    if (t < 2)
        red[REC * (t) + 34] = -1.0; // no previous pair yet (either parity)
    __syncthreads();
    const auto tl = [&]() __attribute__((always_inline)) { // (see xcorr_fused_n4096_fold)
        int x = t;
        if (PADDED)
            asm volatile("" : "+v"(x));
        return x;
    };

    int parity = 0;
    const long long first = c.pair0, total = c.pair0 + p.npairs;
    RawPair raw;
    constexpr bool WIDE = !PADDED;
    const auto request_rows = [&](long long pr) __attribute__((always_inline)) {
        if (WIDE)
            issue_row_loads_wide(raw, p, pr, t);
        else
            issue_row_loads<PADDED, false>(raw, p, pr, t, pad);
    };
    request_rows(first + blockIdx.x < total ? first + (long long)blockIdx.x : first);

    long long nextpair = 0;
    for (long long pair = first + blockIdx.x; pair < total; pair = nextpair) {
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const rec = red + REC * parity;
        const double *const prec = red + REC * (parity ^ 1);
        if (t == 0) // the pair after this one (relative to pair0): claimed now, read behind this pair's barriers
            next_s[parity] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
        double2 v[16];
        {
            const double KA = raw.ka, KB = raw.kb;
            double qa = 0.0, qb = 0.0;
            if (WIDE)
                widen_rows(raw);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const double da = raw.a[i] - KA, db = raw.b[i] - KB;
                v[i] = make_double2(da, db);
                qa = fma(da, da, qa);
                qb = fma(db, db, qb);
            }
            qa = wave_sum_dpp(qa);
            qb = wave_sum_dpp(qb);
            if (lane == 0) {
                rec[24 + 2 * wave] = qa;
                rec[24 + 2 * wave + 1] = qb;
            }
            if (t == 0) {
                rec[34] = (double)rA;
                rec[35] = hasB ? 1.0 : 0.0;
            }
        }
        // ================= Z = FFT(dA + i dB) =================
        dft16_nr(v);
        exchange_cross<0, 1, true>(v, xbuf, wave, t, WIDE ? wide_column(t) : -1);
        finalize_prev(prec, wave, lane, invN, invNm1, p);
        gdft16_nr(v, G2Fetch{g2s, t >> 4});
        exchange_local<1>(v, xw, tl());
        gdft16_nr_l2(v, G3Derived(p.g3a, t));
        double s1a, s1b;
        {
            s1a = readlane_f64(v[0].x, 0);
            s1b = readlane_f64(v[0].y, 0);
            if (!PADDED) {
                v[0].x = (t == 0) ? 0.0 : v[0].x;
                v[0].y = (t == 0) ? 0.0 : v[0].y;
            }
        }
        // ---- the cache: what the reader starts from (the sums of squares of this pair's record are visible behind the
        // barriers of the transpose above and stay until the pair after the next one begins, many barriers away)
        if (pair - first < c.zpairs) {
#if defined(__HIP_DEVICE_COMPILE__)
            const zc_out_ptr zo = (zc_out_ptr)(unsigned long long)(c.zc + (pair - first) * 4096) + t;
#pragma unroll
            for (int i = 0; i < 16; i++)
                __builtin_nontemporal_store(d2v{v[i].x, v[i].y}, zo + 256 * i);
            if (t < 10) {
                const zstat_out_ptr so = (zstat_out_ptr)(unsigned long long)(c.zstat + (pair - first) * ZC_STAT);
                so[t] = t < 8 ? rec[24 + t] : (t == 8 ? s1a : s1b);
            }
#endif
        }
        // ================= ccA + i ccB = FFT(Z conj(X)/n) (unscaled by 1/sigma) =================
        xc_stage1(v, [&](int j) __attribute__((always_inline)) {
            return ldg2(scalar_ptr_at(p.xcp, 256 * ((j + 1) & ~1)), t - 256 * (j & 1));
        });
        dft16_rn_s234(v);
        exchange_local<0>(v, xw, tl());
        if (PADDED && wave == 0 && lane == 0) {
            rec[32] = s1a;
            rec[33] = s1b;
        }
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        exchange_cross<1, 1>(v, xbuf, wave, t);
        nextpair = first + __builtin_amdgcn_readfirstlane(next_s[parity]);
        long long nxt = nextpair;
        nxt = nxt < total ? nxt : first; // last iteration: a dummy request
        gdft16_nr_l2(v, G3Derived(p.g3b, t));
        if (PADDED) { // cc(d - m 1_valid) = cc(d) - m c1, m = sum d / N
            const auto c1l = [&](int k) __attribute__((always_inline)) {
                return scalar_ptr_at(p.c1, 256 * ((k + 1) & ~1))[t - 256 * (k & 1)];
            };
            const double mA = rec[32] * invN, mB = rec[33] * invN;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                double cq[8];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    cq[k] = c1l(8 * h + k);
                fence();
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int r = BR16(8 * h + k);
                    v[r] = make_double2(fma(-mA, cq[k], v[r].x), fma(-mB, cq[k], v[r].y));
                }
            }
        }
        wave_argmax_store(v, wave, lane, rec + 6 * wave);
        fence();
        request_rows(nxt);
        fence();
        if (wave == 0 && lane == 0) {
            rec[32] = s1a;
            rec[33] = s1b;
        }
        parity ^= 1;
    }
    lds_barrier();
    {
        const double *const prec = red + REC * (parity ^ 1);
        if (t < 2 && prec[34] >= 0.0 && (t == 0 || prec[35] != 0.0)) {
            const long long row = (long long)prec[34] + t;
            if (finalize(prec, t, invN, invNm1, p.mv + row, p.lag + row)) {
                const int slot = atomicAdd(p.ovf_count, 1);
                p.ovf_list[slot] = row >> 1;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- reader
template <bool PADDED>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_cached_n4096(const FusedParams p, const SpectrumCacheArgs c)
{
    using namespace occ4;
    using namespace fold;
    using namespace foldk;
    __shared__ double2 xbuf[OCC_XBUF];
    __shared__ double2 g2s[128];
    __shared__ double red[2 * REC];
    __shared__ int next_s[2];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    double2 *const xw = xbuf + XW * wave;
    const double invN = PADDED ? p.invN : 1.0 / 4096.0, invNm1 = PADDED ? p.invNm1 : 1.0 / 4095.0;

    if (t < 128)
        g2s[t] = p.g2[t];
    if (t < 2)
        red[REC * (t) + 34] = -1.0; // no previous pair yet (either parity)
    __syncthreads();
    const auto tl = [&]() __attribute__((always_inline)) {
        int x = t;
        if (PADDED)
            asm volatile("" : "+v"(x));
        return x;
    };

    int parity = 0;
    const long long first = c.pair0, total = c.pair0 + p.npairs;
    d2v zn[16]; // the next pair's spectrum, in flight
    // one scalar base per two registers (the odd one at immediate offset -4096 B) + the shared lane offset 16 t; read once: non-temporal
    const auto request_z = [&](long long pr) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 16; i++)
            zn[i] = __builtin_nontemporal_load((gptr<d2v>)scalar_ptr_at(c.zc, (pr - first) * 4096 + 256 * ((i + 1) & ~1)) + (t - 256 * (i & 1)));
    };
    request_z(first + blockIdx.x < total ? first + (long long)blockIdx.x : first);

    long long nextpair = 0;
    for (long long pair = first + blockIdx.x; pair < total; pair = nextpair) {
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const rec = red + REC * parity;
        const double *const prec = red + REC * (parity ^ 1);
        if (t == 0)
            next_s[parity] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
        // the pair's statistics (a wave-uniform address: the scalar cache), used behind the workgroup transpose below
        double st[10];
#if defined(__HIP_DEVICE_COMPILE__)
        {
            const zstat_in_ptr sp = (zstat_in_ptr)(unsigned long long)(c.zstat + (pair - first) * ZC_STAT);
#pragma unroll
            for (int k = 0; k < 10; k++)
                st[k] = sp[k];
        }
#endif
        double2 v[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            v[i] = make_double2(zn[i].x, zn[i].y);
        // ================= ccA + i ccB = FFT(Z conj(X)/n) (unscaled by 1/sigma) =================
        xc_stage1(v, [&](int j) __attribute__((always_inline)) {
            return ldg2(scalar_ptr_at(p.xcp, 256 * ((j + 1) & ~1)), t - 256 * (j & 1));
        });
        dft16_rn_s234(v);
        exchange_local<0>(v, xw, tl());
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        // the tail barrier frees the waves' private quarters for the next pair's wave-local transpose (the plain kernel has
        // the first transform's workgroup transpose, which begins with a barrier, in between)
        exchange_cross<1, 1, true>(v, xbuf, wave, t);
        // behind the barriers: the previous pair's record is complete and visible, and nobody reads this parity's record any more
        // (its last reader was the finalize of the pair before the previous one, in front of these barriers)
        finalize_prev(prec, wave, lane, invN, invNm1, p);
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < 10; k++)
                rec[24 + k] = st[k];
            rec[34] = (double)rA;
            rec[35] = hasB ? 1.0 : 0.0;
        }
        nextpair = first + __builtin_amdgcn_readfirstlane(next_s[parity]);
        long long nxt = nextpair;
        nxt = nxt < total ? nxt : first; // last iteration: a dummy request
        gdft16_nr_l2(v, G3Derived(p.g3b, t));
        if (PADDED) { // cc(d - m 1_valid) = cc(d) - m c1, m = sum d / N
            const auto c1l = [&](int k) __attribute__((always_inline)) {
                return scalar_ptr_at(p.c1, 256 * ((k + 1) & ~1))[t - 256 * (k & 1)];
            };
            const double mA = st[8] * invN, mB = st[9] * invN;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                double cq[8];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    cq[k] = c1l(8 * h + k);
                fence();
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int r = BR16(8 * h + k);
                    v[r] = make_double2(fma(-mA, cq[k], v[r].x), fma(-mB, cq[k], v[r].y));
                }
            }
        }
        wave_argmax_store(v, wave, lane, rec + 6 * wave);
        // (requesting half of the next spectrum in front of the argmax fits the registers and changes nothing: 7.08 ms either
        // way at 1 M x 4096; all of it there, or any of it in front of pass 3, spills)
        fence();
        request_z(nxt);
        fence();
        parity ^= 1;
    }
    lds_barrier();
    {
        const double *const prec = red + REC * (parity ^ 1);
        if (t < 2 && prec[34] >= 0.0 && (t == 0 || prec[35] != 0.0)) {
            const long long row = (long long)prec[34] + t;
            if (finalize(prec, t, invN, invNm1, p.mv + row, p.lag + row)) {
                const int slot = atomicAdd(p.ovf_count, 1);
                p.ovf_list[slot] = row >> 1;
            }
        }
    }
}

static bool cache_launch_ok(const FusedParams &p, const SpectrumCacheArgs &c)
{
    return p.rows && !p.rows32 && p.n == 4096 && p.N > 2048 && p.N <= 4096 && p.npairs > 0 && c.pair0 >= 0 &&
           2 * (c.pair0 + p.npairs) <= p.M + 1 && p.work_counter && p.ovf_count && p.ovf_list && p.g2 && p.g3a && p.g3b && p.xcp &&
           (p.N == 4096 || p.c1);
}

// pairs [c.pair0, c.pair0 + p.npairs) of the group from the ROWS, the first c.zpairs of them into the cache; p.ovf_count is
// added to (not reset), p.work_counter must be zero
hipError_t launch_cache_fill(const FusedParams &p_in, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    if (!cache_launch_ok(p, c) || c.zpairs < 0 || c.zpairs > p.npairs || (c.zpairs > 0 && (!c.zc || !c.zstat)) ||
        2 * (c.pair0 + c.zpairs) > p.M) // (only pairs of two rows are cached)
        return hipErrorInvalidValue;
    const dim3 g((unsigned)std::min<long long>(p.npairs, (long long)num_cus * 4)), b(OCC_THREADS);
    if (p.N < 4096)
        hipLaunchKernelGGL((xcorr_cache_fill_n4096<true>), g, b, 0, stream, p, c);
    else
        hipLaunchKernelGGL((xcorr_cache_fill_n4096<false>), g, b, 0, stream, p, c);
    return hipGetLastError();
}

// pairs [c.pair0, c.pair0 + p.npairs) from the cache (all of them cached: c.zpairs >= p.npairs)
hipError_t launch_cached(const FusedParams &p_in, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    if (!cache_launch_ok(p, c) || !c.zc || !c.zstat || c.zpairs < p.npairs || 2 * (c.pair0 + p.npairs) > p.M)
        return hipErrorInvalidValue;
    const dim3 g((unsigned)std::min<long long>(p.npairs, (long long)num_cus * 4)), b(OCC_THREADS);
    if (p.N < 4096)
        hipLaunchKernelGGL((xcorr_cached_n4096<true>), g, b, 0, stream, p, c);
    else
        hipLaunchKernelGGL((xcorr_cached_n4096<false>), g, b, 0, stream, p, c);
    return hipGetLastError();
}

} // namespace muse
