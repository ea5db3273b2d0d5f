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
//   zstat[pair][16]  (double)  [0, 8) the eight per-wave partial sums of d^2 (2 * wave + series), kept as partials and summed in
//                    the plain kernel's order; [8], [9] sum d of the two series (the DC bin); [10], [11] 1 / sigma of the two
//                    series and [12] one word of bits -- the pair's VERDICT (foldk_device.h), which depends on the rows alone:
//                    the writer's finalize stores what it computed, the readers' finalize is the combine alone
//
// xcorr_cache_fill_n4096: the plain kernel plus the stores (results unchanged) over pairs [pair0, pair0 + npairs); the first
//                         `zpairs` of them are cached (0: none -- the plain arithmetic on a tail of the group).
// xcorr_cached_n4096:     per pair sixteen 16-byte loads of Z and the verdict through the scalar cache, both requested a whole
//                         pair ahead, then the plain kernel's second half, function by function: the same operations on the same
//                         doubles, so mv and lag come out bit for bit as from the rows.  Two workgroups per CU: the reference's
//                         table stays in registers for the whole launch; pairs are claimed two per atomic add.
// xcorr_cached_n4096_occ4: the reader at four workgroups per CU that one replaced (table from L2 in every pair, Z requested at
//                         the end of the pair before, one add per pair), behind a test hook to compare against.
// Pairs with NaN / Inf statistics or sigmas too far apart are listed exactly as by the plain kernel and redone FROM THE ROWS
// by the rescaling kernel behind the pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "n4096_pair_device.h"

namespace muse {

// ---------------------------------------------------------------------------------------------------------------- writer
// The cache: what the reader starts from, stored right behind the first transform (the sums of squares of this pair's record are
// visible behind the barriers of the transpose in front and stay until the pair after the next one begins, many barriers away)
struct CacheTap {
    const SpectrumCacheArgs c;
    const long long first;
    __device__ __forceinline__ void operator()(const double2 (&v)[16], const double *rec, const double s1a, const double s1b,
                                               const long long rel, const int t) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        if (rel < c.zpairs) {
            const foldk::zc_out_ptr zo = (foldk::zc_out_ptr)(unsigned long long)(c.zc + rel * 4096) + t;
#pragma unroll
            for (int i = 0; i < 16; i++)
                __builtin_nontemporal_store(occ4::d2v{v[i].x, v[i].y}, zo + 256 * i);
            if (t < 10) {
                const foldk::zstat_out_ptr so = (foldk::zstat_out_ptr)(unsigned long long)(c.zstat + rel * ZC_STAT);
                so[t] = t < 8 ? rec[24 + t] : (t == 8 ? s1a : s1b);
            }
        }
#endif
    }
    // finalize runs a pair behind the tap (and once behind the loop), in one lane per series: the pair comes from the record's row.
    // Series 0 of a full pair knows the whole word, and only full pairs are cached.
    __device__ __forceinline__ void verdict(const long long pair, const int series, const double y, const unsigned bits) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        const long long rel = pair - first;
        if (rel < c.zpairs) {
            const foldk::zstat_out_ptr so = (foldk::zstat_out_ptr)(unsigned long long)(c.zstat + rel * ZC_STAT);
            so[ZC_VERDICT + series] = y;
            if (series == 0)
                so[ZC_VERDICT + 2] = __hiloint2double(0, (int)bits);
        }
#endif
    }
};

template <bool PADDED>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_cache_fill_n4096(const FusedParams p, const SpectrumCacheArgs c)
{
    foldk::pair_loop_from_rows<false, PADDED, false, false, false>(p, CacheTap{c, c.pair0});
}

// ---------------------------------------------------------------------------------------------------------------- reader
// pass 3's factors from the two kept table entries, each one computed where it is asked for (G3Derived's formulas on the same
// doubles): eight factors kept across the pair loop would be 32 registers the reader does not have
struct G3Lazy {
    double2 w8, w16;
    __device__ __forceinline__ double2 operator()(int s) const
    {
        constexpr double H = 0.70710678118654752440;
        switch (s) {
        case 0: return foldk::G3Derived::sq(foldk::G3Derived::sq(w8));
        case 1: return foldk::G3Derived::sq(w8);
        case 2: return w8;
        case 3: return make_double2(H * (w8.x + w8.y), H * (w8.y - w8.x));
        case 4: return w16;
        case 5: return foldk::G3Derived::mulc(w16, fold::C16_1, fold::S16_1);
        case 6: return make_double2(H * (w16.x + w16.y), H * (w16.y - w16.x));
        default: return foldk::G3Derived::mulc(w16, fold::S16_1, fold::C16_1);
        }
    }
};

// Pairs are handed out in chunks of ZC_CLAIM consecutive pairs per add on the work counter.  One add per pair is 500 000 adds
// on ONE word per launch over 1 M rows, 71 per microsecond at 7 ms -- a single word takes about 88 (MI355X_MICROARCH.md,
// "dequeue") -- and the hand-out, not the stream or the arithmetic, paced the reader: with 2 pairs per add it takes 0.83 - 0.85
// of the time (profiles/spectrum_cache_reader_bench.txt; 3, 4, 8 and 16 pairs per add: 0.86).
constexpr int ZC_CLAIM = 2;

// Two workgroups per CU, 256 registers: what does not change from pair to pair stays in registers (the sixteen factors of the
// reference's table and the two entries pass 3's factors derive from), and the next pair's spectrum is requested right behind
// the multiply at the top of a pair, a whole pair before it is used: no load of the loop is waited for in the pair that
// requests it.  The full 16 x 272 buffer takes the workgroup transpose in one round: three barriers per pair.
template <bool PADDED>
__global__ __launch_bounds__(OCC_THREADS, 2) void xcorr_cached_n4096(const FusedParams p, const SpectrumCacheArgs c)
{
    using namespace occ4;
    using namespace fold;
    using namespace foldk;
    __shared__ double2 xbuf[OCC_XBUF_FULL];
    __shared__ double2 g2s[128];
    __shared__ alignas(16) double red[2 * REC];
    __shared__ int next_s[2];
    const PairThread th = pair_prologue<PADDED>(p, g2s, red + 34, REC);
    const int t = th.t, lane = th.lane, wave = th.wave;
    const double invN = th.invN;
    reader_prologue(red, t);
    double2 *const xw = xbuf + 1088 * wave;
    const long long first = c.pair0, total = c.pair0 + p.npairs;
    // N < 4096 has the -m c1 correction's registers on top and would spill with the request at the top of the pair: it requests
    // behind pass 3 and the correction's loads, in front of the argmax
    constexpr bool AHEAD = !PADDED;
    constexpr int ch = ZC_CLAIM;

    if (t == 0) // the workgroup's second chunk (the loop claims two chunks ahead); slot 1: the first chunk writes slot 0
        next_s[1] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
    d2v zn[16]; // the next pair's spectrum, in flight
    request_z(zn, c, first + (long long)ch * blockIdx.x, t); // (the grid has at most ceil(npairs / ch) workgroups)
    PairVerdict qn = load_pair_verdict<PADDED, false>(c.zstat, (long long)ch * blockIdx.x); // the next pair's verdict, in flight
    // launch-invariant: the reference's factors of this thread (xc for k3 = j) and pass 3's table entries of planes 2 and 4
    double2 xf[16];
#pragma unroll
    for (int j = 0; j < 16; j++)
        xf[j] = XcFetch{p.xcp, t}(j);
    G3Lazy g3{G3Fetch{p.g3b, t}(2), G3Fetch{p.g3b, t}(4)};
    __syncthreads();

    int parity = 0, cpar = 0;
    long long pair = first + (long long)ch * blockIdx.x;
    long long cbeg = pair, cend = pair + ch < total ? pair + ch : total; // the chunk of pairs in hand
    long long nchunk = first + (long long)ch * __builtin_amdgcn_readfirstlane(next_s[1]), after = 0;
    while (pair < total) {
        const bool claiming = pair == cbeg;
        const long long nextpair = pair + 1 < cend ? pair + 1 : nchunk;
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const rec = red + REC * parity;
        const double *const prec = red + REC * (parity ^ 1);
        const PairVerdict q = qn; // requested a pair ago, published behind the workgroup transpose below
        // ================= ccA + i ccB = FFT(Z conj(X)/n) (unscaled by 1/sigma) =================
        double2 v[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            v[i] = make_double2(zn[i].x, zn[i].y);
        xc_stage1_pre(v, xf);
        // the spectrum's registers are free again: the next pair's request goes out here, a whole pair before its use (in front of
        // the multiply the compiler would have to copy the sixteen registers out of the way first).
        // A chunk's first pair claims the chunk after the next one here too (relative to pair0 / ZC_CLAIM): published in front of
        // this pair's barriers, read behind them.  The counter's address goes through a vector register: with a uniform address the
        // compiler rewrites the add into a wave reduction that waits for the returned value on the spot, a round trip to L2; and
        // it stands behind the multiply, whose last wait for the spectrum would otherwise cover the add as well.
        int claim = 0;
#pragma unroll
        for (int i = 0; i < 16; i += 4) // (the products are complete HERE: the compiler would sink them below the branch of the add)
            asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i + 1].x), "+v"(v[i + 1].y), "+v"(v[i + 2].x), "+v"(v[i + 2].y), "+v"(v[i + 3].x), "+v"(v[i + 3].y));
#if defined(__HIP_DEVICE_COMPILE__)
        if (claiming && t == 0) {
            unsigned long long wc = (unsigned long long)p.work_counter;
            asm volatile("" : "+v"(wc));
            claim = __hip_atomic_fetch_add((int __attribute__((address_space(1))) *)wc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#endif
        const long long nxt = nextpair < total ? nextpair : first; // past the end: a dummy request
        if (AHEAD) {
            fence();
            request_z(zn, c, nxt, t);
            fence();
        }
        // (the compiler would otherwise derive all eight of pass 3's factors once, in front of the loop: 32 registers, spills)
        asm volatile("" : "+v"(g3.w8.x), "+v"(g3.w8.y), "+v"(g3.w16.x), "+v"(g3.w16.y));
        dft16_rn_s234(v);
        exchange_local_full<0>(v, xw, t);
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        if (claiming && t == 0)
            next_s[cpar] = (int)gridDim.x + claim;
        exchange_cross_full<1, 1>(v, xbuf, t);
        lds_barrier(); // the reads are done: the next pair's wave-local transpose writes without a barrier of its own
        // behind the barriers: the previous pair's record is complete and visible, and nobody reads this parity's record any more
        // (its last reader was the finalize of the pair before the previous one, in front of these barriers)
        finalize_pair_cached(prec, wave, lane == 0, p);
        publish_pair_verdict(rec, q, t, rA, hasB);
        if (claiming) {
            after = first + (long long)ch * __builtin_amdgcn_readfirstlane(next_s[cpar]);
            cpar ^= 1;
        }
        qn = load_pair_verdict<PADDED, true>(c.zstat, nxt - first); // behind the pair's last read of LDS
        gdft16_nr_l2(v, g3);
        if (PADDED) // all sixteen c1 values in front of the request: loads return in order, one behind it would wait for the spectrum
            correct_padded<16>(v, p.c1, t, q.s1a * invN, q.s1b * invN, [&]() __attribute__((always_inline)) {
                request_z(zn, c, nxt, t);
                fence();
            });
        wave_argmax_store(v, wave, lane, rec + 6 * wave);
        parity ^= 1;
        if (pair + 1 < cend) {
            pair++;
        } else {
            pair = cbeg = nchunk;
            cend = pair + ch < total ? pair + ch : total;
            nchunk = after;
        }
    }
    lds_barrier();
    finalize_pair_cached(red + REC * (parity ^ 1), t, true, p);
}

// ---------------------------------------------------------------------------------------------------------------- the reader at four workgroups per CU (test hook: muse_test_spectrum_cache_reader)
template <bool PADDED>
__global__ __launch_bounds__(OCC_THREADS, 4) void xcorr_cached_n4096_occ4(const FusedParams p, const SpectrumCacheArgs c)
{
    using namespace occ4;
    using namespace fold;
    using namespace foldk;
    __shared__ double2 xbuf[OCC_XBUF];
    __shared__ double2 g2s[128];
    __shared__ alignas(16) double red[2 * REC];
    __shared__ int next_s[2];
    const PairThread th = pair_prologue<PADDED>(p, g2s, red + 34, REC);
    const int t = th.t, lane = th.lane, wave = th.wave;
    const double invN = th.invN;
    reader_prologue(red, t);
    double2 *const xw = xbuf + XW * wave;
    __syncthreads();

    int parity = 0;
    const long long first = c.pair0, total = c.pair0 + p.npairs;
    d2v zn[16]; // the next pair's spectrum, in flight
    request_z(zn, c, first + blockIdx.x < total ? first + (long long)blockIdx.x : first, t);
    PairVerdict qn = load_pair_verdict<PADDED, false>(c.zstat, first + blockIdx.x < total ? (long long)blockIdx.x : 0); // the next pair's verdict, in flight

    long long nextpair = 0;
    for (long long pair = first + blockIdx.x; pair < total; pair = nextpair) {
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const rec = red + REC * parity;
        const double *const prec = red + REC * (parity ^ 1);
        if (t == 0)
            next_s[parity] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
        const PairVerdict q = qn; // requested a pair ago, published behind the workgroup transpose below
        double2 v[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            v[i] = make_double2(zn[i].x, zn[i].y);
        // ================= ccA + i ccB = FFT(Z conj(X)/n) (unscaled by 1/sigma) =================
        xc_stage1(v, XcFetch{p.xcp, t});
        dft16_rn_s234(v);
        exchange_local<0>(v, xw, tl<PADDED>(t));
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        // the tail barrier frees the waves' private quarters for the next pair's wave-local transpose (the plain kernel has
        // the first transform's workgroup transpose, which begins with a barrier, in between)
        exchange_cross<1, 1, true>(v, xbuf, wave, t);
        // behind the barriers: as in xcorr_cached_n4096
        finalize_pair_cached(prec, wave, lane == 0, p);
        publish_pair_verdict(rec, q, t, rA, hasB);
        nextpair = first + __builtin_amdgcn_readfirstlane(next_s[parity]);
        long long nxt = nextpair;
        nxt = nxt < total ? nxt : first; // last iteration: a dummy request
        qn = load_pair_verdict<PADDED, true>(c.zstat, nxt - first); // behind the pair's last read of LDS
        gdft16_nr_l2(v, G3Derived(p.g3b, t));
        if (PADDED)
            correct_padded<8>(v, p.c1, t, q.s1a * invN, q.s1b * invN);
        wave_argmax_store(v, wave, lane, rec + 6 * wave);
        // (requesting half of the next spectrum in front of the argmax fits the registers and changes nothing: 7.08 ms either
        // way at 1 M x 4096; all of it there, or any of it in front of pass 3, spills)
        fence();
        request_z(zn, c, nxt, t);
        fence();
        parity ^= 1;
    }
    lds_barrier();
    finalize_pair_cached(red + REC * (parity ^ 1), t, true, p);
}

static bool cache_launch_ok(const FusedParams &p, const SpectrumCacheArgs &c)
{
    return p.rows && !p.rows32 && p.n == 4096 && p.N > 2048 && p.N <= 4096 && p.npairs > 0 && c.pair0 >= 0 &&
           2 * (c.pair0 + p.npairs) <= p.M + 1 && p.work_counter && p.ovf_count && p.ovf_list && p.g2 && p.g3a && p.g3b && p.xcp &&
           (p.N == 4096 || p.c1);
}

// pairs [c.pair0, c.pair0 + p.npairs) of the group from the ROWS, the first c.zpairs of them into the cache (0: none -- the plain
// arithmetic on a tail of the group); p.ovf_count is added to (not reset), p.work_counter must be zero
hipError_t launch_cache_fill(const FusedParams &p_in, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream)
{
    const FusedParams p = with_reciprocals(p_in);
    if (!cache_launch_ok(p, c) || c.zpairs < 0 || c.zpairs > p.npairs || (c.zpairs > 0 && (!c.zc || !c.zstat)) ||
        2 * (c.pair0 + c.zpairs) > p.M) // (only pairs of two rows are cached)
        return hipErrorInvalidValue;
    const dim3 g((unsigned)std::min<long long>(p.npairs, (long long)num_cus * 4)), b(OCC_THREADS);
    with_bools([&](auto padded) { hipLaunchKernelGGL((xcorr_cache_fill_n4096<decltype(padded)::value>), g, b, 0, stream, p, c); }, p.N < 4096);
    return hipGetLastError();
}

// pairs [c.pair0, c.pair0 + p.npairs) from the cache (all of them cached: c.zpairs >= p.npairs); occ4: the reader at four
// workgroups per CU (test hook)
hipError_t launch_cached(const FusedParams &p_in, const SpectrumCacheArgs &c, int num_cus, hipStream_t stream, bool occ4)
{
    const FusedParams p = with_reciprocals(p_in);
    if (!cache_launch_ok(p, c) || !c.zc || !c.zstat || c.zpairs < p.npairs || 2 * (c.pair0 + p.npairs) > p.M ||
        p.M > 0x7fffffffLL) // (the readers' record carries the row as an int)
        return hipErrorInvalidValue;
    const dim3 g((unsigned)(occ4 ? std::min<long long>(p.npairs, (long long)num_cus * 4)
                                 : std::min<long long>((p.npairs + ZC_CLAIM - 1) / ZC_CLAIM, (long long)num_cus * 2))), b(OCC_THREADS);
    with_bools([&](auto four, auto padded) {
        if (decltype(four)::value)
            hipLaunchKernelGGL((xcorr_cached_n4096_occ4<decltype(padded)::value>), g, b, 0, stream, p, c);
        else
            hipLaunchKernelGGL((xcorr_cached_n4096<decltype(padded)::value>), g, b, 0, stream, p, c);
    }, occ4, p.N < 4096);
    return hipGetLastError();
}

} // namespace muse

#undef MUSE_CONSUME_ROWS // (n4096_pair_device.h: used through pair_loop_from_rows only)
