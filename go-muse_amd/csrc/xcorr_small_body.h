// xcorr_small_body.h -- the body of xcorr_fused_small, xcorr_fused_small_signed and xcorr_fused_small_band (xcorr_small.hip), included
// inside each kernel's braces: no include guard, nothing but statements.  The including kernel provides p (const FusedParams) and the
// compile-time constants LOGN, PADDED, MULTI, F32, WIN (the flags xcorr_small.hip describes), SGN (0: the argmax by magnitude; +-1 with
// WIN: the signed mask, r16_device.h) and BAND (with WIN: the mask is the one index interval p.win_a .. p.win_b).  Kept as text so that
// the kernels are one source under three names and xcorr_fused_small compiles to the code it had as a kernel with the body written out.
    using namespace occ4;
    using namespace fold;
    using namespace small;
    constexpr int n = 1 << LOGN;
    constexpr int S = n / 16;   // threads per pair: 32, 64, 128
    constexpr int TPB = LOGN >= 11 ? S : 256;
    constexpr int G = TPB / S;  // pairs per workgroup iteration: 8, 4, 1, 1, 1
    static_assert((LOGN >= 9 && LOGN <= 11) || LOGN == 13 || LOGN == 14, "n = 512, 1024, 2048, 8192, 16384");
    static_assert(!WIN || LOGN <= 11, "the masked argmax is built for n = 512, 1024, 2048");
    __shared__ double red[112]; // multi-wave pair reductions (n >= 2048): sums [4][16], maxima [2][16], indices [2][16] ints
    // pass 2's eight factors per phase m2 / R1: 8 x R1 distinct values for the whole workgroup.  Gathered per lane from the
    // W_65536 table they were the kernel's longest stall (scattered L2 lines in front of the first butterfly of a pass:
    // tools/ablate/small_exp.sh, + 15-20 % with them out of the way); from LDS they are one broadcast read each.
    constexpr int NP_ = (LOGN + 3) / 4, R1_ = n >> (4 * (NP_ - 1));
    __shared__ double2 g2l[8 * R1_];
    __shared__ double2 xbuf[(TPB / 64) * 544]; // 8.7 KB per wave: half-round buffers of the pairs (8 S 17/16 double2 per pair)
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // (S >= 64: a wave works on one pair -- the pair slot is wave-uniform and everything derived from it stays scalar)
    const int g = S >= 64 ? __builtin_amdgcn_readfirstlane(t / S) : t / S;
    const int j = column_of_lane<LOGN>(t % S);
    double2 *const b = xbuf + g * (8 * S + S / 2);
    const int N = PADDED ? p.N : n, pad = PADDED ? n - N : 0;
    const double invN = PADDED ? p.invN : 1.0 / (double)n, invNm1 = PADDED ? p.invNm1 : 1.0 / (double)(n - 1); // (the launcher's quotients: scalar registers)
    const double2 *__restrict__ twm = p.twm;
    const double2 *__restrict__ gs = p.gsmall;
    if (t < 8 * R1_)
        g2l[t] = tw_factor<R1_>(twm, t % R1_, t / R1_);
    __syncthreads();
    // optional indirection (filter-and-refine Run): process pair_list[0 .. *pair_count) instead of every pair
    // (WIN: never listed -- the count read through a vector load kept the group count, a wave-uniform value, in vector registers,
    // which the n = 512 builds park in scratch)
    const long long *const plist = WIN ? nullptr : p.pair_list;
    const long long total = plist ? (long long)*p.pair_count : p.npairs;
    const long long ngroups = (total + G - 1) / G;

    // The rows of the NEXT iteration are requested behind the per-lane argmax of the current one (the transform registers
    // are free then) and consumed at the top of the loop: element j + i S of the padded series is sample j + i S - pad; a pad
    // position reads up to `pad` samples IN FRONT of the row (the end of the previous row, or the guard the group
    // allocation keeps in front of row 0: capi_group.hip, GROUP_GUARD) and is masked -- no clamp, so every load is one
    // base plus a compile-time offset.
    double xa[16], xb[16], KA, KB;
    const auto request = [&](long long it2) __attribute__((always_inline)) {
        if (it2 >= ngroups)
            it2 = ngroups - 1; // (nothing left: an L2-hot dummy)
        const long long slot = it2 * G + g;
        const long long sl = slot < total ? slot : total - 1;
        const long long pair = plist ? plist[sl] : sl;
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        int jr = j;
        asm volatile("" : "+v"(jr)); // (offsets derived per request, not hoisted)
        jr &= S - 1;                 // (the range the compiler no longer sees: keeps global offsets 32-bit, saddr + voffset loads)
        if (F32) { // the same requests on float32 rows (half the bytes per request)
            const float *ra = p.rows32 + rA * p.stride, *rb = p.rows32 + (hasB ? rA + 1 : rA) * p.stride;
            const auto all_pad = [&](int i) __attribute__((always_inline)) { return PADDED && i < 8 && (i + 1) * S <= pad; };
            if (S >= 64) {
                KA = (double)scalar_ptr(ra)[0];
                KB = (double)scalar_ptr(rb)[0];
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const long long off = all_pad(i) ? 0ll : (long long)i * S - pad;
                    xa[i] = (double)__builtin_nontemporal_load(scalar_ptr_at(ra, off) + (unsigned)jr);
                    xb[i] = (double)__builtin_nontemporal_load(scalar_ptr_at(rb, off) + (unsigned)jr);
                }
            } else {
                KA = (double)ra[0];
                KB = (double)rb[0];
                const float *la = ra - pad + jr, *lb = rb - pad + jr;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    xa[i] = (double)__builtin_nontemporal_load(all_pad(i) ? ra + jr : la + i * S);
                    xb[i] = (double)__builtin_nontemporal_load(all_pad(i) ? rb + jr : lb + i * S);
                }
            }
            return;
        }
        const double *ra = p.rows + rA * p.stride, *rb = p.rows + (hasB ? rA + 1 : rA) * p.stride;
        // PADDED: the elements i S .. (i + 1) S - 1 of the padded series are all pad when (i + 1) S <= pad (a wave-uniform
        // test; pad < n / 2, so only i < 8 can be).  Such a request would fetch the end of the previous row from HBM only to be
        // masked (N = 5000 -> n = 8192: six of the sixteen requests, N = 480 -> 512: one): it is pointed at the row's own
        // first S samples instead -- the same unconditional load instruction (a branch around it parks the row registers in
        // scratch), an L2 hit instead of HBM bytes.
        const auto all_pad = [&](int i) __attribute__((always_inline)) { return PADDED && i < 8 && (i + 1) * S <= pad; };
        if (S >= 64 && !PADDED) { // the wave works on one pair: scalar bases + the shared VGPR offset 8 j; ONE base per row serves
                                  // every request whose immediate offset (-4096 ... 4095 bytes) reaches it
            KA = scalar_ptr(ra)[0];
            KB = scalar_ptr(rb)[0];
            constexpr int PER = S <= 64 ? 8 : S <= 128 ? 4 : S <= 512 ? 2 : 1;
#pragma unroll
            for (int gq = 0; gq < 16 / PER; gq++) {
                constexpr int HALF = PER / 2;
                const int c = (gq * PER + HALF) * S;
                const gptr<double> ba = scalar_ptr_at(ra, c), bb = scalar_ptr_at(rb, c);
#pragma unroll
                for (int k = 0; k < PER; k++) {
                    const int i = gq * PER + k;
                    xa[i] = __builtin_nontemporal_load(ba + (i * S - c) + (unsigned)jr);
                    xb[i] = __builtin_nontemporal_load(bb + (i * S - c) + (unsigned)jr);
                }
            }
        } else if (S >= 64) {
            KA = scalar_ptr(ra)[0];
            KB = scalar_ptr(rb)[0];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const long long off = all_pad(i) ? 0ll : (long long)i * S - pad;
                xa[i] = __builtin_nontemporal_load(scalar_ptr_at(ra, off) + (unsigned)jr);
                xb[i] = __builtin_nontemporal_load(scalar_ptr_at(rb, off) + (unsigned)jr);
            }
        } else { // two pairs per wave: one 64-bit base per lane and row, immediate offsets 256 i bytes
            KA = ra[0];
            KB = rb[0];
            const double *la = ra - pad + jr, *lb = rb - pad + jr;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                xa[i] = __builtin_nontemporal_load(all_pad(i) ? ra + jr : la + i * S);
                xb[i] = __builtin_nontemporal_load(all_pad(i) ? rb + jr : lb + i * S);
            }
        }
    };
    // n <= 1024 (a wave holds one or two whole pairs, no workgroup barrier anywhere): the rows are requested where they are
    // consumed -- the sixteen waves of a CU hide the latency, and the 64 registers a prefetch would hold across the argmax
    // and the write-out are worth more (n = 512: 0.543 -> 0.453 ms per 400 000 series, 37.9 -> 45.4 % of the roofline;
    // n = 1024: +2 %; from n = 2048 the prefetch wins, at n = 16384 by 7 %).
    constexpr bool PREFETCH = MULTI || LOGN >= 11;
    if (PREFETCH && blockIdx.x < ngroups)
        request(blockIdx.x);
    for (long long it = blockIdx.x; it < ngroups; it += gridDim.x) {
        if (!PREFETCH)
            request(it);
        const long long slot = it * G + g;
        const bool live = slot < total;
        const long long sl = live ? slot : total - 1; // idle sub-groups shadow the last pair
        const long long pair = plist ? plist[sl] : sl;
        const long long rA = 2 * pair;
        const bool hasB = rA + 1 < p.M;
        // ---- d = x - K with K the first sample, shifted statistics
        double2 v[16];
        int js = j;
        asm volatile("" : "+v"(js)); // (per-sample validity derived per iteration, not hoisted: 16 masks)
        js &= S - 1;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const bool valid = !PADDED || i >= 8 || js + i * S - pad >= 0; // (pad < n / 2: the upper half is always data)
            const double da = valid ? xa[i] - KA : 0.0, db = valid ? xb[i] - KB : 0.0;
            v[i] = make_double2(da, db);
            q0 += da;
            q1 = fma(da, da, q1);
            q2 += db;
            q3 = fma(db, db, q3);
        }
        pair_sum4<S>(q0, q1, q2, q3, red, wave);
        const Stat stA{q0, q1}, stB{q2, q3};
        bool zeroA, nanA, zeroB, nanB;
        const double varA0 = variance(stA, invN, invNm1, zeroA, nanA);
        const double varB0 = variance(stB, invN, invNm1, zeroB, nanB);
        const bool deadA = zeroA || nanA, deadB = zeroB || nanB || !hasB;
        // both series go into the shared transform at O(1): exact power-of-two scales close to 1/sigma
        // (fft_device.h, pow2_inv_sigma), folded into the mean removal; the variances scale along exactly
        const double sA = deadA ? 1.0 : pow2_inv_sigma(varA0), sB = deadB ? 1.0 : pow2_inv_sigma(varB0);
        // (a pair that fills its wave(s): the scaled variances wait for the result write-out in SGPRs, not in four registers the
        // allocator parks in scratch across the transforms)
        const double varA = S >= 64 ? uniform(varA0 * sA * sA) : varA0 * sA * sA, varB = S >= 64 ? uniform(varB0 * sB * sB) : varB0 * sB * sB;
        const double mA = q0 * invN * sA, mB = q2 * invN * sB;
        asm volatile("" : "+v"(js));
        js &= S - 1;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const bool valid = !PADDED || i >= 8 || js + i * S - pad >= 0; // (pad < n / 2: the upper half is always data)
            v[i].x = valid ? fma(v[i].x, sA, -mA) : 0.0;
            v[i].y = valid ? fma(v[i].y, sB, -mB) : 0.0;
        }
        if (deadA || deadB) { // uniform over the pair, rare: a sigma == 0 / NaN series (or the missing partner of an odd
                              // last row) must contribute exact zeros to the shared complex transform
#pragma unroll
            for (int i = 0; i < 16; i++) {
                v[i].x = deadA ? 0.0 : v[i].x;
                v[i].y = deadB ? 0.0 : v[i].y;
            }
        }
        // ---- Z = FFT(yA + i yB);  V = Z conj(X)/n;  ccA + i ccB = FFT(V)
        forward<LOGN>(v, b, g2l, gs, j);
        // the workgroup's slice of the spectrum scratch: element i of thread gt at [i][gt] (scalar base + 32-bit lane offset)
        const long long ZT = (long long)gridDim.x * TPB;
        const auto zslot = [&](int i) __attribute__((always_inline)) {
            int gt = t;
            asm volatile("" : "+v"(gt)); // (derived per use, not hoisted)
            gt &= TPB - 1;
            return (d2v __attribute__((address_space(1))) *)scalar_ptr_at(p.zscratch, i * ZT + (long long)blockIdx.x * TPB) + (unsigned)gt;
        };
        constexpr bool ZREG = MULTI && LOGN <= 13;
        double2 Z[16];
        if (MULTI) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (ZREG)
                    Z[i] = v[i];
                else
                    *zslot(i) = d2v{v[i].x, v[i].y};
            }
        }
        const int R = MULTI ? p.R : 1;
#pragma clang loop unroll(disable)
        for (int ref = 0; ref < R; ref++) {
        const double2 *__restrict__ xcr = MULTI ? uniform_ptr(p.xcp_many[ref]) : p.xc;
        if (MULTI) {
            fence();
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (ZREG) {
                    v[i] = Z[i];
                } else {
                    const d2v z = *zslot(i);
                    v[i] = make_double2(z.x, z.y);
                }
            }
        }
        { // V = Z conj(X)/n in place, the factors in four batches of four (two in flight: 32 registers), then the
          // registers renamed to natural order (X[j + r S] sits at v[BR16(r)])
            int jx = j;
            asm volatile("" : "+v"(jx)); // (the table offsets are derived here, not hoisted out of the pair loop)
            jx &= S - 1;
            // one scalar base per PERX table rows (16 S bytes apart; immediate offsets -4096 ... 4095 bytes), formed once
            constexpr int PERX = S <= 32 ? 16 : S <= 64 ? 8 : S <= 128 ? 4 : S <= 256 ? 2 : 1;
            gptr<double2> xbase[16 / PERX];
#pragma unroll
            for (int gq = 0; gq < 16 / PERX; gq++)
                xbase[gq] = scalar_ptr_at(xcr, (gq * PERX + PERX / 2) * S);
            const auto xcl = [&](int r) __attribute__((always_inline)) {
                return ldg2u(xbase[r / PERX] + (r * S - ((r / PERX) * PERX + PERX / 2) * S), (unsigned)jx);
            };
            double2 xq[2][4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                xq[0][k] = xcl(k);
#pragma unroll
            for (int bt = 0; bt < 4; bt++) {
                fence();
                if (bt < 3) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        xq[(bt + 1) & 1][k] = xcl(4 * (bt + 1) + k);
                }
                fence();
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int r = 4 * bt + k;
                    v[BR16(r)] = cmul(v[BR16(r)], xq[bt & 1][k]);
                }
            }
            double2 w[16];
#pragma unroll
            for (int r = 0; r < 16; r++)
                w[r] = v[BR16(r)];
#pragma unroll
            for (int r = 0; r < 16; r++)
                v[r] = w[r];
        }
        forward<LOGN>(v, b, g2l, gs, j); // cc[j + r S] at v[BR16(r)]
        if (WIN) {
            int jw = j;
            asm volatile("" : "+v"(jw)); // (derived here, not hoisted)
            jw &= S - 1;
            mask_window<true, S, SGN, BAND>(v, jw, BAND ? p.win_b : p.win_lpos, BAND ? p.win_a : n - p.win_lneg);
        }
        // ---- maxAbsIndex (xcorr.go:39-50) per series: ascending r = ascending index for this thread
        double sa = 0.0, sb = 0.0; // signed value of the lane's first maximum of |cc|, and its register index
        int ra_ = 0, rb_ = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const double xa = v[BR16(r)].x, xb = v[BR16(r)].y;
            const bool ga = fabs(xa) > fabs(sa), gb = fabs(xb) > fabs(sb);
            sa = ga ? xa : sa;
            ra_ = ga ? r : ra_;
            sb = gb ? xb : sb;
            rb_ = gb ? r : rb_;
        }
        const double ma = fabs(sa), mb = fabs(sb);
        const int ia = j + ra_ * S, ib = j + rb_ * S;
        const double cc0a = v[0].x, cc0b = v[0].y; // (lane 0: cc[0], reported when nothing is above 0)
        fence();
        if (!MULTI && PREFETCH)
            request(it + gridDim.x); // the next iteration's rows: in flight during the reductions and the result write-out
        fence();
        double pa = ma, pb = mb;
        pair_max2<S>(pa, pb, red, wave);
        int ca = (ma == pa && pa > 0.0) ? ia : 0x7fffffff, cb = (mb == pb && pb > 0.0) ? ib : 0x7fffffff;
        pair_min_i2<S>(ca, cb, red, wave);
        // the lane that owns the winning index writes the result (nothing above 0: lane 0 reports cc[0] at index 0)
        if (live) {
            const bool ownA = ca == 0x7fffffff ? j == 0 : (ia == ca && ma == pa);
            if (ownA) {
                double y = __builtin_amdgcn_rsq(varA);
                y = y * fma(-0.5 * varA * y, y, 1.5);
                y = y * fma(-0.5 * varA * y, y, 1.5);
                double mv = (ca == 0x7fffffff ? cc0a : sa) * y;
                const int idx = ca == 0x7fffffff ? 0 : ca;
                int lag = idx > n / 2 ? idx - n : idx;
                if (zeroA) { mv = 0.0; lag = 0; }               // xcorr.go:166-167
                if (nanA) { mv = __builtin_nan(""); lag = 0; }
                (MULTI ? p.mv_many[ref] : p.mv)[rA] = mv;
                (MULTI ? p.lag_many[ref] : p.lag)[rA] = lag;
            }
            const bool ownB = cb == 0x7fffffff ? j == 0 : (ib == cb && mb == pb);
            if (ownB && hasB) {
                double y = __builtin_amdgcn_rsq(varB);
                y = y * fma(-0.5 * varB * y, y, 1.5);
                y = y * fma(-0.5 * varB * y, y, 1.5);
                double mv = (cb == 0x7fffffff ? cc0b : sb) * y;
                const int idx = cb == 0x7fffffff ? 0 : cb;
                int lag = idx > n / 2 ? idx - n : idx;
                if (zeroB) { mv = 0.0; lag = 0; }
                if (nanB) { mv = __builtin_nan(""); lag = 0; }
                (MULTI ? p.mv_many[ref] : p.mv)[rA + 1] = mv;
                (MULTI ? p.lag_many[ref] : p.lag)[rA + 1] = lag;
            }
        }
        } // (references)
        if (MULTI) { // (requested inside the loop the 64 row registers would be live across all references)
            fence();
            request(it + gridDim.x);
        }
    }
