// n4096_pair_device.h -- the steps of one pair's pass through the n = 4096 kernel family, each defined once:
// xcorr_fused_n4096_fold and fold_multi_body (xcorr_r16_fold.hip), xcorr_cache_fill_n4096, xcorr_cached_n4096 and
// xcorr_cached_n4096_occ4 (xcorr_r16_cached.hip).  The plain kernel and the cache's writer are ONE pair loop
// (pair_loop_from_rows); the two readers and the many-references kernel keep their own loop skeletons -- their schedules
// differ on purpose -- and call the steps.  The transforms, transposes, record and argmax helpers are foldk_device.h's.
#pragma once
#include "foldk_device.h"

namespace muse {

namespace foldk {

#if defined(__HIP_DEVICE_COMPILE__)
typedef d2v __attribute__((address_space(1))) *zc_out_ptr;
typedef double __attribute__((address_space(1))) *zstat_out_ptr;
typedef const double __attribute__((address_space(4))) *zstat_in_ptr;
#endif

// what a thread knows about itself, and the launch's 1 / N and 1 / (N - 1)
// (PADDED: the launcher's quotients, kernel arguments in scalar registers -- formed in the kernel they came out of the vector
// divider and were parked in scratch across the whole pair loop)
struct PairThread {
    int t, lane, wave;
    double invN, invNm1;
};
// Head of every kernel of the family: pass 2's factors into LDS and "no previous pair yet" into the slot the finalize of a
// previous pair looks at, for either parity (prev_row = &record[0][slot], rec_stride doubles apart).  The workgroup barrier
// that makes both visible stays with the caller: some kernels have requests to issue in front of it.
template <bool PADDED>
__device__ __forceinline__ PairThread pair_prologue(const FusedParams &p, double2 *g2s, double *prev_row, const int rec_stride)
{
    PairThread th;
    th.t = threadIdx.x;
    th.lane = th.t & 63;
    th.wave = __builtin_amdgcn_readfirstlane(th.t >> 6); // wave-uniform by construction
    th.invN = PADDED ? p.invN : 1.0 / 4096.0;
    th.invNm1 = PADDED ? p.invNm1 : 1.0 / 4095.0;
    if (th.t < 128)
        g2s[th.t] = p.g2[th.t];
    if (th.t < 2)
        prev_row[rec_stride * th.t] = -1.0; // no previous pair yet (either parity)
    return th;
}

// The thread id where an LDS address or a window bound is formed from it.  PIN: opaque to the compiler, so that what is derived
// from it is formed where it is used -- hoisted out of the pair loop, the wave-local transposes' LDS addresses of the PADDED
// builds were parked in scratch and reloaded behind an s_waitcnt vmcnt(0) in the middle of every pair, and the many-references
// kernel, which has no register to spare, kept the window's two bounds relative to it across the whole pair loop.
template <bool PIN>
__device__ __forceinline__ int tl(const int t)
{
    int x = t;
    if (PIN)
        asm volatile("" : "+v"(x));
    return x;
}

// entry t of plane j of a lane-ordered table ([planes][256] behind tab + off): one scalar base per two planes (16-byte entries:
// the odd plane at immediate offset -4096 B) + the shared lane offset
template <typename T>
__device__ __forceinline__ gptr<T> lane_entry(const T *tab, const long long off, const int j, const int t)
{
    return scalar_ptr_at(tab, off + 256 * ((j + 1) & ~1)) + (t - 256 * (j & 1));
}
// the reference's spectrum factors of a thread: xc for k3 = j from the lane-ordered table (FusedParams::xcp, ::xcp_many[r])
struct XcFetch {
    const double2 *xcp;
    int t;
    __device__ __forceinline__ double2 operator()(int j) const { return ldg2(lane_entry(xcp, 0, j, t), 0); }
};

// the pair's rows into `raw` (the caller clamps `pr`): the loader of the build
// N == n float64 rows (neither PADDED nor F32): 16-byte requests on relabelled columns (r16_device.h, issue_row_loads_wide): -1.6 % (profiles/r03_fold_variants.txt)
template <bool PADDED, bool F32, bool SLIDE = false>
__device__ __forceinline__ void request_rows(RawPair &raw, const FusedParams &p, const long long pr, const int t, const int pad)
{
    constexpr bool WIDE = !PADDED && !F32;
    if (SLIDE && WIDE)
        issue_row_loads_wide_slide(raw, p, pr, t);
    else if (SLIDE && F32)
        issue_row_loads_slide<PADDED>(raw, p.rows32, p, pr, t, pad);
    else if (SLIDE)
        issue_row_loads_slide<PADDED>(raw, p.rows, p, pr, t, pad);
    else if (WIDE)
        issue_row_loads_wide(raw, p, pr, t);
    else
        issue_row_loads<PADDED, F32>(raw, p, pr, t, pad);
}

// Consume the prefetched rows: d = x - K (K = the row's first sample) bounds the cancellation in sum d^2 - (sum d)^2 / N and
// keeps a large level out of the transform's rounding; sum d is read off the DC bin (take_dc).  The per-wave partial sums of
// d^2 go to part[2 wave + series], the pair's first row and whether it has a second one to part[10], part[11].
// (PADDED: a pad position was loaded from the clamped index 0, i.e. it holds the row's first sample K itself, so
// d = K - K = 0 without any masking)
// A macro, the one step that is: as a function (raw and v by reference) the same statements leave the pair loop's carried
// registers in another order, and from there on the allocator differs -- three float32 builds of the plain kernel parked a
// double in scratch and the padded float32 many-references builds came out 1 % slower (profiles/n4096_family_refactor.txt, section 6).
#define MUSE_CONSUME_ROWS(WIDE, raw, v, part, t, lane, wave, rA, hasB)      \
    {                                                                       \
        const double KA = (raw).ka, KB = (raw).kb;                          \
        double qa = 0.0, qb = 0.0;                                          \
        if (WIDE)                                                           \
            widen_rows(raw);                                                \
        _Pragma("unroll") for (int i = 0; i < 16; i++) {                    \
            const double da = (raw).a[i] - KA, db = (raw).b[i] - KB;        \
            (v)[i] = make_double2(da, db);                                  \
            qa = fma(da, da, qa);                                           \
            qb = fma(db, db, qb);                                           \
        }                                                                   \
        qa = wave_sum_dpp(qa);                                              \
        qb = wave_sum_dpp(qb);                                              \
        if ((lane) == 0) {                                                  \
            (part)[2 * (wave)] = qa;                                        \
            (part)[2 * (wave) + 1] = qb;                                    \
        }                                                                   \
        if ((t) == 0) {                                                     \
            (part)[10] = (double)(rA);                                      \
            (part)[11] = (hasB) ? 1.0 : 0.0;                                \
        }                                                                   \
    }

// Behind pass 3 of the first transform: bin 0 (lane 0 of wave 0) = (sum dA, sum dB), taken into SGPRs; the centred series' DC
// bin is exactly 0 (PADDED keeps it: the mean is taken out of the results instead, correct_padded).  Branch-free on purpose.
template <bool PADDED>
__device__ __forceinline__ void take_dc(double2 (&v)[16], const int t, double &s1a, double &s1b)
{
    s1a = readlane_f64(v[0].x, 0);
    s1b = readlane_f64(v[0].y, 0);
    if (!PADDED) {
        v[0].x = (t == 0) ? 0.0 : v[0].x;
        v[0].y = (t == 0) ? 0.0 : v[0].y;
    }
}

// A pair's results from its complete record: among the threads with `writer` set, those with series 0 / 1 write one series
// each.  In a pair loop the previous pair's (lane 0 of waves 0 / 1, behind the first barriers of the current pair); behind the
// loop and an lds_barrier the last pair's (threads 0 / 1).
// tap.verdict(pair, series, y, bits) takes the series' verdict (foldk_device.h) where the kernel keeps it.
template <typename Tap>
__device__ __forceinline__ void finalize_pair(const double *prec, const int series, const bool writer, const double invN,
                                              const double invNm1, const FusedParams &p, const Tap &tap)
{
    if (writer && series < 2 && prec[34] >= 0.0 && (series == 0 || prec[35] != 0.0)) {
        const long long row = (long long)prec[34] + series;
        if (finalize(prec, series, invN, invNm1, p.mv + row, p.lag + row,
                     [&](const double y, const unsigned bits) __attribute__((always_inline)) { tap.verdict(row >> 1, series, y, bits); })) {
            const int slot = atomicAdd(p.ovf_count, 1);
            p.ovf_list[slot] = row >> 1;
        }
    }
}

// PADDED: cc(d - m 1_valid) = cc(d) - m c1 with m = sum d / N (mA, mB), on the sixteen values a lane ends with (cc index
// t + 256 k at v[BR16(k)]).  c1's values are requested B at a time; between() runs behind a batch's loads and in front of its
// FMAs.
struct Nothing {
    __device__ __forceinline__ void operator()() const {}
};
template <int B, typename Between = Nothing>
__device__ __forceinline__ void correct_padded(double2 (&v)[16], const double *c1, const int t, const double mA, const double mB,
                                               Between between = Between())
{
#pragma unroll
    for (int h = 0; h < 16 / B; h++) {
        double cq[B];
#pragma unroll
        for (int k = 0; k < B; k++)
            cq[k] = *lane_entry(c1, 0, B * h + k, t);
        fence();
        between();
#pragma unroll
        for (int k = 0; k < B; k++) {
            const int r = BR16(B * h + k);
            v[r] = make_double2(fma(-mA, cq[k], v[r].x), fma(-mB, cq[k], v[r].y));
        }
    }
}

// ---- the spectrum cache (xcorr_r16_cached.hip; layout: xcorr_kernels.h, SpectrumCacheArgs)
// the spectrum of pair `pr` of the group into zn: lane-ordered addresses; read once: non-temporal
__device__ __forceinline__ void request_z(d2v (&zn)[16], const SpectrumCacheArgs &c, const long long pr, const int t)
{
#pragma unroll
    for (int i = 0; i < 16; i++)
        zn[i] = __builtin_nontemporal_load((gptr<d2v>)lane_entry(c.zc, (pr - c.pair0) * 4096, i, t));
}
// The verdict of the segment's pair `rel` as the writer stored it (ZC_VERDICT; a wave-uniform address: the scalar cache), and
// with SUMS the two sums of d that N < 4096 takes the means from.  A reader requests it a pair ahead, behind the pair in hand's
// publish: it travels in scalar registers beside the pair in hand, and no wait of a pair is for a request of that pair.
struct PairVerdict {
    double yA, yB, s1a, s1b;
    unsigned bits;
};
// Scalar loads return out of order, so every wait for LDS behind the request is one for the request as well: IN_LOOP, the
// request stands behind the pair's last read of LDS (the waves' exchanges are complete behind their barrier, which the compiler
// cannot see: the explicit wait, for thread 0's two stores at the most, tells it), and the next wait is the first exchange of
// the next pair.
template <bool SUMS, bool IN_LOOP>
__device__ __forceinline__ PairVerdict load_pair_verdict(const double *zstat, const long long rel_)
{
    PairVerdict q = {};
#if defined(__HIP_DEVICE_COMPILE__)
    long long rel = rel_;
    if (IN_LOOP) {
        fence();
        __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0)
        asm volatile("" : "+s"(rel));       // (the address is formed, and the request issued, behind the wait)
    }
    const zstat_in_ptr sp = (zstat_in_ptr)(unsigned long long)(zstat + rel * ZC_STAT);
    if (SUMS) {
        q.s1a = sp[8];
        q.s1b = sp[9];
    }
    q.yA = sp[ZC_VERDICT];
    q.yB = sp[ZC_VERDICT + 1];
    q.bits = ((const unsigned __attribute__((address_space(4))) *)sp)[2 * (ZC_VERDICT + 2)]; // (one word: a register of the request that nobody reads is one the compiler reuses, behind a wait for the request)
    if (IN_LOOP)
        fence();
#endif
    return q;
}
// The readers' record of a pair: the four wave records at [0, 24) as everywhere, yA and yB at [24], [25], and in the four
// words of [26], [27] the verdict's bits, the pair's first row (-1: no pair yet) and whether it has a second one.
struct ReaderHead {
    unsigned bits;
    int row, hasB, unused;
};
__device__ __forceinline__ void reader_prologue(double *red, const int t)
{
    if (t < 2)
        *(ReaderHead *)(red + REC * t + 26) = ReaderHead{0u, -1, 0, 0};
}
// thread 0 publishes the pair in hand (two 16-byte stores) ...
__device__ __forceinline__ void publish_pair_verdict(double *rec, const PairVerdict &q, const int t, const long long rA, const bool hasB)
{
    if (t == 0) {
        *(double2 *)(rec + 24) = make_double2(q.yA, q.yB);
        *(ReaderHead *)(rec + 26) = ReaderHead{q.bits, (int)rA, hasB ? 1 : 0, 0};
    }
}
// ... and a pair behind, among the threads with `writer` set, those with series 0 / 1 combine one series each from the complete
// record, as finalize_pair does in the kernels that read rows: everything is read in one batch, then three compare-selects and
// one multiply; the redo list gets what the plain kernel's verdict would give it (verdict_redo).
__device__ __forceinline__ void finalize_pair_cached(const double *prec, const int series, const bool writer, const FusedParams &p)
{
    if (writer && series < 2) {
        const WaveRecords w = load_wave_records(prec, series);
        const double y = prec[24 + series];
        const ReaderHead h = *(const ReaderHead *)(prec + 26);
        fence(); // (one round trip to LDS: none of the reads behind the branch)
        if (h.row >= 0 && (series == 0 || h.hasB != 0)) {
            const long long row = (long long)h.row + series;
            combine(w, y, (h.bits & verdict_zero(series)) != 0u, (h.bits & verdict_nan(series)) != 0u, p.mv + row, p.lag + row);
            if (h.bits & verdict_redo(series)) {
                const int slot = atomicAdd(p.ovf_count, 1);
                p.ovf_list[slot] = row >> 1;
            }
        }
    }
}

// What pair_loop_from_rows does besides scoring: NoTap nothing, over the pairs [0, npairs) -- `first` a compile-time zero, so
// that nothing is added to the plain kernel's address arithmetic; CacheTap (xcorr_r16_cached.hip) the cache's stores.
struct NoTap {
    static constexpr long long first = 0;
    __device__ __forceinline__ void operator()(const double2 (&)[16], const double *, double, double, long long, int) const {}
    __device__ __forceinline__ void verdict(long long, int, double, unsigned) const {}
};

// The pair loop of the kernels that score from the ROWS, four workgroups per CU: pairs [tap.first, tap.first + p.npairs), handed
// out by the atomic counter (relative to tap.first); tap(v, rec, s1a, s1b, pair - tap.first, t) runs right behind the first
// transform.  The flags are xcorr_fused_n4096_fold's (xcorr_r16_fold.hip).
// SGN != 0 (WIN builds, named with Tap spelled out): the signed mask of r16_device.h (xcorr_fused_n4096_fold_signed).
// BAND (WIN builds, any SGN): the mask is the one index interval p.win_a .. p.win_b (xcorr_fused_n4096_fold_band).
template <bool TIMING, bool PADDED, bool F32, bool WIN, bool SLIDE, typename Tap, int SGN = 0, bool BAND = false>
__device__ __forceinline__ void pair_loop_from_rows(const FusedParams &p, const Tap tap)
{
    __shared__ double2 xbuf[OCC_XBUF];
    __shared__ double2 g2s[128];
    __shared__ double red[2 * REC];
    __shared__ int next_s[2];
    const PairThread th = pair_prologue<PADDED>(p, g2s, red + 34, REC);
    const int t = th.t, lane = th.lane, wave = th.wave;
    const double invN = th.invN, invNm1 = th.invNm1;
    double2 *const xw = xbuf + XW * wave;
    const int pad = PADDED ? 4096 - p.N : 0;
    __syncthreads();
    PhaseClock<TIMING> clk;
    clk.start();

    int parity = 0;
    const long long first = tap.first, total = first + p.npairs;
    RawPair raw;
    constexpr bool WIDE = !PADDED && !F32;
    request_rows<PADDED, F32, SLIDE>(raw, p, first + blockIdx.x < total ? first + (long long)blockIdx.x : first, t, pad);

    long long nextpair = 0;
    for (long long pair = first + blockIdx.x; pair < total; pair = nextpair) {
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        double *const rec = red + REC * parity;
        const double *const prec = red + REC * (parity ^ 1);
        if (t == 0) // the pair after this one (relative to `first`): claimed now, read behind this pair's barriers
            next_s[parity] = (int)gridDim.x + atomicAdd(p.work_counter, 1);
        if (SLIDE) { // rules 2 and 3: every load of this pair has returned in every wave, then the new rows go back in place
            fence();
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            fence();
            if (WIDE)
                store_slid_rows_wide(raw, p, pair, t);
            else if (F32)
                store_slid_rows<PADDED>(raw, const_cast<float *>(p.rows32), p, pair, t, pad);
            else
                store_slid_rows<PADDED>(raw, const_cast<double *>(p.rows), p, pair, t, pad);
        }
        double2 v[16];
        if (TIMING)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        clk.template stamp<0>();
        MUSE_CONSUME_ROWS(WIDE, raw, v, rec + 24, t, lane, wave, rA, hasB)
        clk.template stamp<1>();
        // ================= Z = FFT(dA + i dB) =================
        // pass 1: plain DFT over a (thread (b, c) = (hi, lo)) -> k1 at v[BR16(k1)]
        dft16_nr(v);
        clk.template stamp<2>();
        // -> thread (k1 = hi, c = lo), input b at v[b]; the tail barrier frees the wave's private quarter for the
        // wave-local transpose below while the waves are still in step
        exchange_cross<0, 1, true>(v, xbuf, wave, t, WIDE ? wide_column(t) : -1);
        // the previous pair's record is complete and visible
        finalize_pair(prec, wave, lane == 0, invN, invNm1, p, tap);
        clk.template stamp<3>();
        // pass 2: generalised DFT over b, delta = k1 / 16 (carries W_256^(b k1))
        gdft16_nr(v, G2Fetch{g2s, t >> 4});
        clk.template stamp<4>();
        exchange_local<1>(v, xw, tl<PADDED>(t)); // -> thread (k1 = hi, k2 = lo), input c at v[c]
        clk.template stamp<5>();
        // pass 3: generalised DFT over c, delta = (k1 + 16 k2) / 256 (carries W_4096^(c k1) W_256^(c k2));
        // Z[hi + 16 lo + 256 k3] at v[BR16(k3)]
        gdft16_nr_l2(v, G3Derived(p.g3a, t));
        double s1a, s1b; // kept in SGPRs until the record is written
        take_dc<PADDED>(v, t, s1a, s1b);
        tap(v, rec, s1a, s1b, pair - first, t);
        clk.template stamp<6>();
        // ================= ccA + i ccB = FFT(Z conj(X)/n) (unscaled by 1/sigma) =================
        // element f = 256 a' + 16 b' + c' with a' = k3 (register BR16(a')), b' = lo, c' = hi
        // pass 1: plain DFT over a' with the spectrum factors folded into its first stage -> m1 at v[m1]
        xc_stage1(v, XcFetch{p.xcp, t});
        dft16_rn_s234(v);
        clk.template stamp<7>();
        exchange_local<0>(v, xw, tl<PADDED>(t)); // (c' = hi, b' = lo) -> (c' = hi, m1 = lo), input b' at v[b']: same wave
        if (PADDED && wave == 0 && lane == 0) { // every lane needs the means before its argmax: visible behind
            rec[32] = s1a;                      // the four barriers of the transpose below
            rec[33] = s1b;
        }
        clk.template stamp<8>();
        // pass 2: generalised DFT over b', delta = m1 / 16, m1 = lo
        gdft16_nr(v, G2Fetch{g2s, t & 15});
        clk.template stamp<9>();
        exchange_cross<1, 1>(v, xbuf, wave, t); // -> thread (m1 = lo, m2 = hi), input c' at v[c']
        clk.template stamp<10>();
        // pass 3: generalised DFT over c', delta = (m1 + 16 m2) / 256 = t / 256: cc index t + 256 m3 at v[BR16(m3)]
        nextpair = first + __builtin_amdgcn_readfirstlane(next_s[parity]);
        long long nxt = nextpair; // last iteration: pair `first` (L2-resident dummy)
        nxt = nxt < total ? nxt : first;
        gdft16_nr_l2(v, G3Derived(p.g3b, t));
        if (PADDED)
            correct_padded<8>(v, p.c1, t, rec[32] * invN, rec[33] * invN);
        if (WIN) // cc index t + 256 m3 at v[BR16(m3)]
            mask_window<true, 256, SGN, BAND>(v, tl<PADDED>(t), BAND ? p.win_b : p.win_lpos, BAND ? p.win_a : 4096 - p.win_lneg);
        clk.template stamp<11>();
        // float32 rows take 34 registers instead of 66: room to request them BEFORE the argmax, which then runs under
        // the HBM latency (float64 rows: behind it, there is no register left to land them in)
        if (F32) {
            fence();
            request_rows<PADDED, F32, SLIDE>(raw, p, nxt, t, pad);
            fence();
        }
        wave_argmax_store(v, wave, lane, rec + 6 * wave);
        clk.template stamp<13>();
        fence();
        if (!F32)
            request_rows<PADDED, F32, SLIDE>(raw, p, nxt, t, pad);
        fence();
        if (wave == 0 && lane == 0) {
            rec[32] = s1a;
            rec[33] = s1b;
        }
        parity ^= 1;
        clk.template stamp<12>();
    }
    lds_barrier();
    finalize_pair(red + REC * (parity ^ 1), t, true, invN, invNm1, p, tap);
    if (TIMING && p.dbg && lane == 0) {
#pragma unroll
        for (int i = 0; i < NPHASE; i++)
            p.dbg[((long long)blockIdx.x * 4 + wave) * NPHASE + i] = clk.acc[i];
    }
}

} // namespace foldk

} // namespace muse
