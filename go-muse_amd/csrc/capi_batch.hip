// capi_batch.hip -- NewBatch (muse_batch.go:23-52): reference spectrum and tables; the all-scores pass and its kernel selection
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"
#include "xcorr_huge.h"

using namespace muse;


// ------------------------------------------------------------------- batch
int ilog2(int64_t n)
{
    int l = 0;
    while (((int64_t)1 << l) < n)
        l++;
    return l;
}

// device reference spectrum for (ref, N) at FFT length n: fills X, xc
int build_spectrum(muse_ctx *ctx, const double *ref_host, int N, int n, int normalize, double x_scale,
                          double xc_scale, double2 *X, double2 *xc, float2 *xcf, double *xs, int *zero_std)
{
    double *dref = nullptr;
    int *dstat = nullptr;
    double2 *dscr = nullptr; // n > 8192: global work buffer for the radix-2 passes
    HIP_TRY(dmalloc(ctx, &dref, (size_t)N * sizeof(double)));
    hipError_t e = dmalloc(ctx, &dstat, sizeof(int));
    if (e == hipSuccess && n > GENERIC_LDS_MAX_N)
        e = dmalloc(ctx, &dscr, (size_t)n * sizeof(double2));
    if (e == hipSuccess)
        e = hipMemcpyAsync(dref, ref_host, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = launch_ref_spectrum(dref, N, n, ilog2(n), normalize, x_scale, xc_scale, ctx->twm, X, xc, xcf, xs, dscr,
                                dstat, ctx->stream);
    int st = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(&st, dstat, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    dfree(ctx, dref);
    dfree(ctx, dstat);
    dfree(ctx, dscr);
    HIP_TRY(e);
    *zero_std = st;
    return MUSE_OK;
}

hipError_t ensure_gscratch(muse_ctx *ctx, int64_t n, int slices_per_cu)
{
    if (n < GENERIC_LDS_MAX_N) // generic kernel above 8192: one slice per workgroup; Stockham from 8192: up to two
        return hipSuccess;
    std::lock_guard<std::mutex> lock(ctx->stage_mu); // launches that use the buffer hold the same lock (muse_batch_score)
    return ctx->gscratch.ensure(ctx, (int64_t)ctx->num_cus * slices_per_cu * n, ctx->stream);
}

// the base table of the long-series sweeps' twiddles, [4096] W_n^(m2) (n = 16384, 32768, 65536): built on first use per length
// (rare, so always under the lock -- no unlocked read of the pointer another thread may be storing)
hipError_t ensure_twl(muse_ctx *ctx, int64_t n)
{
    const int li = ilog2(n) - 14;
    if (li < 0 || li > 2)
        return hipErrorInvalidValue;
    std::lock_guard<std::mutex> lock(ctx->stage_mu);
    if (ctx->twl[li])
        return hipSuccess;
    std::vector<double2> tl(4096);
    for (int m2 = 0; m2 < 4096; m2++)
        fill_twiddle(tl, (size_t)m2, (long long)m2, n);
    double2 *d = nullptr;
    hipError_t e = hipMalloc(&d, tl.size() * sizeof(double2));
    if (e == hipSuccess)
        e = hipMemcpy(d, tl.data(), tl.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        ctx->twl[li] = d;
    else
        (void)hipFree(d);
    return e;
}

void adopt_spectrum(muse_batch *b)
{
    b->X = b->sp->X;
    b->xc = b->sp->xc;
    b->xcp = b->sp->xcp;
    b->xcw = b->sp->xcw;
    b->xcf = b->sp->xcf;
    b->xs = b->sp->xs;
    b->c1 = b->sp->c1;
}

extern "C" int muse_batch_create(muse_ctx *ctx, muse_group *g, const double *ref, int32_t N, muse_batch **out)
{
    if (!out)
        return fail(MUSE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (N < 1) // muse.go:24-26
        return fail(MUSE_ERR_EMPTY, "Reference series length must be greater than zero");
    if (!g || !ref || g->ctx != ctx)
        return fail(MUSE_ERR_INVALID, "bad batch arguments");
    if (g->N != N) // muse_batch.go:24-28
        return fail(MUSE_ERR_LENGTH, "comparison group series does not have the same length as the reference (%d vs %d)",
                    g->N, N);
    if (N < 2)
        return fail(MUSE_ERR_INVALID, "series length 1 has no sample standard deviation");
    const int64_t n = muse_next_pow2((double)N); // muse_batch.go:35
    if (n > HUGE_MAX_N)
        return fail(MUSE_ERR_UNSUPPORTED, "FFT length %lld > %d is not built", (long long)n, HUGE_MAX_N);
    const bool huge = n > GENERIC_MAX_N; // series longer than 65 536 samples: xcorr_huge.hip
    muse_batch *b = new (std::nothrow) muse_batch();
    if (!b)
        return fail(MUSE_ERR_NOMEM, "host allocation failed");
    b->ctx = ctx;
    b->g = g;
    g->refs.fetch_add(1);
    ctx->refs.fetch_add(1);
    b->N = N;
    b->n = (int32_t)n;
    b->logn = ilog2(n);
    hipError_t e = dmalloc(ctx, &b->ovf_count, 2 * sizeof(int)); // [0] overflow-pair count, [1] dynamic work counter
    if (e == hipSuccess && !huge)
        e = ensure_gscratch(ctx, n);
    muse_spectrum *sp = new (std::nothrow) muse_spectrum();
    if (!sp)
        e = hipErrorOutOfMemory;
    b->sp = sp;
    if (e == hipSuccess)
        e = dmalloc(ctx, &sp->X, (size_t)(n / 2 + 1) * sizeof(double2));
    if (huge) {
        // the spectrum in natural order (muse_batch_spectrum) and as the lane-ordered multiplier rows of huge_rows: the only
        // two tables these lengths use (no fp32 screening copy, no time-domain copy, no indicator correlation)
        if (e == hipSuccess)
            e = dmalloc(ctx, &sp->xcp, (size_t)n * sizeof(double2));
        if (e != hipSuccess) {
            muse_batch_free(b);
            return fail(MUSE_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
        }
        adopt_spectrum(b);
        int zero = 0;
        rc = huge_reference(ctx, ref, N, (int)n, sp->X, sp->xcp, &zero);
        if (rc) {
            muse_batch_free(b);
            return rc;
        }
        if (zero) { // muse_batch.go:39-41
            muse_batch_free(b);
            return fail(MUSE_ERR_ZERO_STD, "Invalid input query, Standard deviation of zero");
        }
        *out = b;
        return MUSE_OK;
    }
    if (e == hipSuccess)
        e = dmalloc(ctx, &sp->xc, (size_t)n * sizeof(double2));
    if (e == hipSuccess)
        e = dmalloc(ctx, &sp->xcf, (size_t)n * sizeof(float2));
    if (e == hipSuccess)
        e = dmalloc(ctx, &sp->xs, (size_t)n * sizeof(double));
    const bool long_n = n == 16384 || n == 32768 || n == 65536; // xcorr_long.hip: spectrum rows in lane order, sweep twiddles
    if (e == hipSuccess && (n == 4096 || long_n))
        e = dmalloc(ctx, &sp->xcp, (size_t)n * sizeof(double2));
    if (e == hipSuccess && n == 8192) // xcorr_fused_real8k: the spectrum at its threads' bins, lane-ordered
        e = dmalloc(ctx, &sp->xcp, (size_t)4096 * sizeof(double2));
    if (e == hipSuccess && n == 32768) // xcorr_real.hip, the 16 x 1024 split: xc at the threads' lower eight bins and their mirror bins
        e = dmalloc(ctx, &sp->xcw, (size_t)16385 * sizeof(double2)); // ([16384]: the reference's bin n / 4)
    if (e == hipSuccess && (n == 4096 || long_n) && N < n)
        e = dmalloc(ctx, &sp->c1, (size_t)n * sizeof(double));
    if (e != hipSuccess) {
        muse_batch_free(b);
        return fail(MUSE_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    adopt_spectrum(b);
    int zero = 0;
    // x = zNormalize(ref) / (N-1), zeroPad, FFT   (muse_batch.go:38-47)
    rc = build_spectrum(ctx, ref, N, (int)n, 1, 1.0 / (double)(N - 1), 1.0 / (double)n, b->X, b->xc, b->xcf, b->xs,
                        &zero);
    if (rc) {
        muse_batch_free(b);
        return rc;
    }
    if (n == 4096) {
        e = launch_lane_order(b->xc, b->xcp, ctx->stream);
        if (e == hipSuccess && b->c1)
            e = launch_indicator_corr(b->xs, 4096, 4096 - N, b->c1, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            muse_batch_free(b);
            return fail(MUSE_ERR_HIP, "lane-order table: %s", hipGetErrorString(e));
        }
    }
    if (n == 8192) {
        e = launch_real8k_tables(b->xc, b->xcp, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            muse_batch_free(b);
            return fail(MUSE_ERR_HIP, "n = 8192 lane-order table: %s", hipGetErrorString(e));
        }
    }
    if (long_n) {
        const int R1 = (int)(n / 4096);
        e = ensure_twl(ctx, n);
        if (e == hipSuccess)
            e = launch_lane_order_rows(b->xc, b->xcp, R1, ctx->stream);
        if (e == hipSuccess && b->xcw)
            e = launch_real_split_tables(b->xc, b->xcw, ctx->stream);
        if (e == hipSuccess && b->c1)
            e = launch_indicator_corr(b->xs, (int)n, (int)(n - N), b->c1, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            muse_batch_free(b);
            return fail(MUSE_ERR_HIP, "long-series tables: %s", hipGetErrorString(e));
        }
    }
    if (zero) { // muse_batch.go:39-41
        muse_batch_free(b);
        return fail(MUSE_ERR_ZERO_STD, "Invalid input query, Standard deviation of zero");
    }
    *out = b;
    return MUSE_OK;
}

extern "C" int muse_batch_create_like(muse_batch *src, muse_group *g, muse_batch **out)
{
    if (!out)
        return fail(MUSE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!src || !g || g->ctx != src->ctx)
        return fail(MUSE_ERR_INVALID, "bad batch arguments");
    if (g->N != src->N) // muse_batch.go:24-28 / muse.go:68-70
        return fail(MUSE_ERR_LENGTH, "comparison group series does not have the same length as the reference (%d vs %d)",
                    g->N, src->N);
    muse_ctx *ctx = src->ctx;
    int rc = use_device(ctx);
    if (rc)
        return rc;
    muse_batch *b = new (std::nothrow) muse_batch();
    if (!b)
        return fail(MUSE_ERR_NOMEM, "host allocation failed");
    b->ctx = ctx;
    b->g = g;
    g->refs.fetch_add(1);
    ctx->refs.fetch_add(1);
    b->N = src->N;
    b->n = src->n;
    b->logn = src->logn;
    b->sp = src->sp;
    b->sp->refs.fetch_add(1);
    adopt_spectrum(b);
    hipError_t e = dmalloc(ctx, &b->ovf_count, 2 * sizeof(int));
    if (e != hipSuccess) {
        muse_batch_free(b);
        return fail(MUSE_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    *out = b;
    return MUSE_OK;
}

extern "C" int muse_batch_fft_len(muse_batch *b, int32_t *n)
{
    if (!b || !n)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    *n = b->n;
    return MUSE_OK;
}

extern "C" int muse_batch_spectrum(muse_batch *b, double *out)
{
    if (!b || !out)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    int rc = use_device(b->ctx);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(out, b->X, (size_t)(b->n / 2 + 1) * sizeof(double2), hipMemcpyDeviceToHost));
    return MUSE_OK;
}

int ensure_scores(muse_batch *b)
{
    const int64_t M = b->g->M;
    HIP_TRY(b->mv.ensure(b->ctx, M, b->stream()));
    HIP_TRY(b->lag.ensure(b->ctx, M, b->stream()));
    return MUSE_OK;
}

// the launch parameters every fused kernel shares for batch b (group flushed, M > 0, scores allocated)
FusedParams base_params(muse_batch *b)
{
    muse_ctx *ctx = b->ctx;
    const int64_t M = b->g->M;
    FusedParams p{};
    p.rows = b->g->f32 ? nullptr : b->g->rows;
    p.rows32 = b->g->f32 ? b->g->rows32 : nullptr;
    p.M = M;
    p.stride = b->g->stride;
    p.npairs = (M + 1) / 2;
    p.N = b->N;
    p.n = b->n;
    p.logn = b->logn;
    p.normalize_y = 1;
    p.xc = b->xc;
    p.tw1 = ctx->tw1;
    p.tw2 = ctx->tw2;
    p.twm = ctx->twm;
    p.gscratch = ctx->gscratch.p;
    p.gscratch_slices = b->n > 0 ? (long long)(ctx->gscratch.cap / b->n) : 0;
    p.mv = b->mv.p;
    p.lag = b->lag.p;
    p.cc_out = nullptr;
    p.nil_out = nullptr;
    p.g2 = ctx->g2;
    p.g3a = ctx->g3a;
    p.g3b = ctx->g3b;
    p.gsmall = (b->logn >= 9 && b->logn <= 11) ? ctx->gsmall[b->logn - 9] : (b->logn == 13 || b->logn == 14) ? ctx->gsmall[b->logn - 10] : nullptr;
    p.xcp = b->xcp;
    p.xcw = b->xcw;
    p.gsmall_b = ctx->gsmall[1];
    p.wsplit = ctx->wsplit;
    p.c1 = b->c1;
    p.twl = (b->logn >= 14 && b->logn <= 16) ? ctx->twl[b->logn - 14] : nullptr;
    p.tw1f = ctx->tw1f;
    p.twmf = ctx->twmf;
    p.tw2f = ctx->tw2f;
    p.xcf = b->xcf;
    p.xs = b->xs;
    p.screen_delta = ctx->screen_delta;
#ifdef MUSE_REAL64_STAMPS
    // diagnostic build (tools/ablate/ab_real64_stamps.sh): phase stamps of xcorr_fused_real64k, dumped when the context goes
    if (!ctx->dbg_stamps && hipMalloc(&ctx->dbg_stamps, (size_t)ctx->num_cus * 4 * 16 * 16 * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(ctx->dbg_stamps, 0, (size_t)ctx->num_cus * 4 * 16 * 16 * sizeof(unsigned long long));
    p.dbg = ctx->dbg_stamps;
#endif
    return p;
}

// The kernel the all-scores pass of batch b takes (ctx->variant 0 = automatic selection; the others are test hooks,
// muse_hip_test.h): decided HERE, for muse_batch_score's launch and for the name muse_batch_kernel_name reports.
struct KernelChoice {
    int variant = KERNEL_GENERIC;
    const double2 *gsmall = nullptr; // the pass table the kernel wants instead of base_params' (nullptr: keep)
    const char *error = nullptr;
};
static KernelChoice choose_kernel(muse_batch *b, long long npairs)
{
    muse_ctx *ctx = b->ctx;
    const int64_t M = b->g->M;
    const bool has_twl = b->logn >= 14 && b->logn <= 16 && ctx->twl[b->logn - 14];
    KernelChoice kc;
    if (b->n == 4096) {
        switch (ctx->variant) {
        case 0: case 10: kc.variant = KERNEL_R16_FOLD; break; // fastest measured (profiles/)
        case 7: kc.variant = KERNEL_R16_OCC3; break;          // rescales both series before the shared transform
        default: kc.variant = KERNEL_GENERIC; break;
        }
        if (b->g->f32 && kc.variant == KERNEL_GENERIC) {
            kc.error = "the generic kernel does not read float32-storage groups";
            return kc;
        }
        if (kc.variant == KERNEL_R16_FOLD && b->N != 4096 && !b->c1) // (N < n needs the batch's correction table)
            kc.variant = KERNEL_R16_OCC3;
        // a group of mixed-unit series (sigmas far apart inside most pairs) makes the default kernel hand most
        // pairs to kernel 7 anyway: once a pass over these rows has shown that, go there directly
        if (kc.variant == KERNEL_R16_FOLD && ctx->variant == 0 && b->handoff_host && b->handoff_M == M &&
            b->handoff_rewrites == b->g->rewrites && (long long)*(volatile int *)b->handoff_host * 8 > npairs)
            kc.variant = KERNEL_R16_OCC3;
    } else if (b->g->f32 && !(((b->n >= 512 && b->n <= 2048) || b->n == 8192 || b->n == 16384) && (ctx->variant == 0 || ctx->variant == 12))) {
        kc.error = "float32-storage groups run on the default kernels only (FFT lengths 512 ... 16384)";
    } else if (b->n == 8192 && (ctx->variant == 0 || ctx->variant == 14) && !b->g->f32 && b->xcp) {
        kc.variant = KERNEL_REAL; // one real series per 256-thread workgroup on the n = 4096 kernel's transforms (xcorr_real.hip)
    } else if (b->n == 16384 && (ctx->variant == 0 || ctx->variant == 14) && !b->g->f32 && ctx->gsmall[3]) {
        kc.variant = KERNEL_REAL; // one real series per 512-thread workgroup on the 8192-point complex transform, two workgroups per CU
        kc.gsmall = ctx->gsmall[3];
    } else if (b->n == 32768 && (ctx->variant == 0 || ctx->variant == 15) && !b->g->f32 && ctx->gsmall[4] && b->xcw && ctx->wsplit) {
        // one real series per 1024-thread workgroup with each 16384-point transform as 16 x 1024 (wave-local 1024-point transforms around one
        // workgroup transpose): + 1 ... 4 % over test hook 14's three-transpose form on every box measured (profiles/r05_real_transform.txt)
        kc.variant = KERNEL_REAL_SPLIT;
        kc.gsmall = ctx->gsmall[4];
    } else if ((b->n == 32768 || (b->n == 65536 && (b->N == b->n || b->c1))) && (ctx->variant == 0 || ctx->variant == 14) && !b->g->f32 && ctx->gsmall[4]) {
        // one real series per 1024-thread workgroup on the 16384-point complex transform (xcorr_real.hip): n = 32768 never leaves the CU,
        // n = 65536 in two passes with 1 MB parked per series (3 x the algorithmic bytes; the four-step kernel: 5 x)
        kc.variant = KERNEL_REAL;
        kc.gsmall = ctx->gsmall[4];
    } else if (b->xcp && has_twl && (b->N == b->n || b->c1) && ((b->n >= 32768 && ctx->variant == 0) || (b->n >= 16384 && ctx->variant == 13))) {
        kc.variant = KERNEL_LONG; // four-step, 4096-point rows on the n = 4096 kernel's transforms (xcorr_long.hip)
    } else if (((b->n >= 512 && b->n <= 2048) || b->n == 8192 || b->n == 16384) && (ctx->variant == 0 || ctx->variant == 12)) {
        kc.variant = KERNEL_SMALL; // half-round transposes at 16 waves per CU (xcorr_small.hip)
    } else if (((b->n >= 512 && b->n <= 2048) || b->n >= 8192) && (ctx->variant == 0 || ctx->variant == 11)) {
        kc.variant = KERNEL_STOCKHAM; // radix-16 Stockham through LDS / global scratch (xcorr_stockham.hip)
    }
    return kc;
}

// ------------------------------------------------------------------- spectrum cache
int spectrum_cache_policy(int64_t rows, int32_t N, bool f32, int mode, int64_t min_rows, int64_t free_bytes, int64_t budget,
                          int64_t *rows_cached, int64_t *bytes)
{
    *rows_cached = 0;
    *bytes = 0;
    // float64 rows at FFT length 4096 (2048 < N <= 4096), automatic mode, a group large enough to be worth its footprint
    if (mode != 1 || f32 || N <= 2048 || N > 4096 || rows < std::max<int64_t>(min_rows, 2))
        return ZC_POLICY_NONE;
    const int64_t pairs = rows / 2; // a trailing single row is never cached
    *rows_cached = 2 * pairs;
    *bytes = pairs * ZC_PAIR_BYTES;
    const int64_t limit = budget >= 0 ? budget : free_bytes / 2; // at most half of what is free
    return *bytes <= limit ? ZC_POLICY_BUILD : ZC_POLICY_DECLINED;
}

void group_drop_spectrum_cache(muse_group *g)
{
    for (auto &sg : g->zc_segs)
        dfree(g->ctx, sg.mem);
    g->zc_segs.clear();
    g->zc_state = muse_group::ZC_NONE;
    g->zc_rows = g->zc_bytes = 0;
    g->zc_passes = 0;
    g->zc_declined_M = -1;
}

// does this batch's all-scores pass go through the group's spectrum cache at all (the default n = 4096 kernel under automatic
// selection on the context's stream, a float64 group that keeps its rows)?  Mode, size and memory: spectrum_cache_policy.
static bool spectrum_cache_candidate(const muse_batch *b, int variant)
{
    return variant == KERNEL_R16_FOLD && b->ctx->variant == 0 && b->n == 4096 && !b->g->f32 && !b->g->transient &&
           !b->own_stream;
}

// What this pass launches (ready_mu held): `readers` segments from the cache, then the pairs from tail_pair0 on from the rows, the
// first tail_zpairs of them into tail_seg.  use == false: the plain kernel over everything.
struct ZcPlan {
    bool use = false;
    std::vector<muse_group::ZcSegment> readers;
    int64_t tail_pair0 = 0, tail_zpairs = 0;
    muse_group::ZcSegment tail_seg;
};
static int plan_spectrum_cache(muse_batch *b, ZcPlan &plan)
{
    muse_ctx *ctx = b->ctx;
    muse_group *g = b->g;
    const int64_t M = g->M;
    if (g->zc_rewrites != g->rewrites) { // rows below M were rewritten: what was cached describes other rows
        if (!g->zc_segs.empty())
            HIP_TRY(hipStreamSynchronize(ctx->stream)); // (a pass enqueued earlier may still be reading the blocks)
        group_drop_spectrum_cache(g);
        g->zc_rewrites = g->rewrites;
    }
    const int mode = ctx->zc_mode.load();
    const int64_t min_rows = ctx->zc_min_rows.load(), budget = ctx->zc_budget.load();
    int64_t want_rows = 0, want_bytes = 0;
    if (spectrum_cache_policy(M, b->N, g->f32, mode, min_rows, 0, 0, &want_rows, &want_bytes) == ZC_POLICY_NONE)
        return MUSE_OK; // (mode 0 leaves an existing cache alone and unused: muse_group_drop_spectrum_cache gives the HBM back)
    // a block for the pairs [pair0, pair0 + pairs), if half of the free HBM (or the test hook's budget) holds it
    const auto grow = [&](int64_t pair0, int64_t pairs, muse_group::ZcSegment &sg) -> bool {
        size_t free_b = 0, total_b = 0;
        if (budget < 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        const int64_t bytes = pairs * ZC_PAIR_BYTES;
        if (bytes > (budget >= 0 ? budget - g->zc_bytes : (int64_t)(free_b / 2)))
            return false;
        void *mem = nullptr;
        if (pool_alloc(ctx, false, &mem, (size_t)bytes, false) != hipSuccess) { // (never at the price of the allocation cache)
            (void)hipGetLastError();
            return false;
        }
        sg.mem = mem;
        sg.pair0 = pair0;
        sg.pairs = pairs;
        g->zc_segs.push_back(sg);
        g->zc_bytes += bytes;
        return true;
    };
    if (g->zc_state != muse_group::ZC_VALID) {
        if (g->zc_state == muse_group::ZC_DECLINED && g->zc_declined_M == M)
            return MUSE_OK;
        if (++g->zc_passes < 2) // the first pass over these rows: a group scored once pays nothing
            return MUSE_OK;
        if (!grow(0, want_rows / 2, plan.tail_seg)) {
            g->zc_state = muse_group::ZC_DECLINED;
            g->zc_declined_M = M;
            return MUSE_OK;
        }
        g->zc_state = muse_group::ZC_VALID;
        g->zc_rows = want_rows;
        plan.use = true;
        plan.tail_pair0 = 0;
        plan.tail_zpairs = want_rows / 2;
        return MUSE_OK;
    }
    plan.use = true;
    plan.readers = g->zc_segs;
    plan.tail_pair0 = g->zc_rows / 2;
    const int64_t more = M / 2 - g->zc_rows / 2; // pairs of two rows appended behind the cache
    if (more > 0 && (int)g->zc_segs.size() < ZC_MAX_SEGMENTS && g->zc_declined_M != M) {
        if (grow(plan.tail_pair0, more, plan.tail_seg)) {
            plan.tail_zpairs = more;
            g->zc_rows = 2 * (M / 2);
        } else {
            g->zc_declined_M = M; // (the cached rows stay; the tail is asked for again once M changes)
        }
    }
    return MUSE_OK;
}

extern "C" int muse_ctx_set_spectrum_cache(muse_ctx *ctx, int32_t mode)
{
    if (!ctx || (mode != 0 && mode != 1))
        return fail(MUSE_ERR_INVALID, "spectrum cache mode is 0 (off) or 1 (automatic)");
    ctx->zc_mode.store(mode);
    return MUSE_OK;
}

extern "C" int muse_group_spectrum_cache(muse_group *g, int64_t *rows_cached, int64_t *bytes)
{
    if (!g)
        return fail(MUSE_ERR_INVALID, "NULL group");
    std::lock_guard<std::mutex> lock(g->ready_mu);
    if (rows_cached)
        *rows_cached = (g->zc_state == muse_group::ZC_VALID && g->zc_rewrites == g->rewrites) ? g->zc_rows : 0;
    if (bytes)
        *bytes = g->zc_bytes;
    return MUSE_OK;
}

extern "C" int muse_group_drop_spectrum_cache(muse_group *g)
{
    if (!g)
        return fail(MUSE_ERR_INVALID, "NULL group");
    std::lock_guard<std::mutex> lock(g->ready_mu);
    if (g->zc_segs.empty() && g->zc_state == muse_group::ZC_NONE)
        return MUSE_OK;
    int rc = use_device(g->ctx);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(g->ctx->stream)); // a pass enqueued earlier may still be reading the blocks
    group_drop_spectrum_cache(g);
    return MUSE_OK;
}

extern "C" int muse_test_spectrum_cache_limits(muse_ctx *ctx, int64_t min_rows, int64_t budget_bytes)
{
    if (!ctx)
        return fail(MUSE_ERR_INVALID, "NULL context");
    ctx->zc_min_rows.store(min_rows < 0 ? ZC_MIN_ROWS : min_rows);
    ctx->zc_budget.store(budget_bytes < 0 ? -1 : budget_bytes);
    return MUSE_OK;
}

extern "C" int muse_test_spectrum_cache_reader(muse_ctx *ctx, int32_t reader)
{
    if (!ctx)
        return fail(MUSE_ERR_INVALID, "NULL context");
    if (reader != 0 && reader != 1)
        return fail(MUSE_ERR_INVALID, "spectrum cache reader %d (0 = two workgroups per CU, 1 = four)", (int)reader);
    ctx->zc_reader.store(reader);
    return MUSE_OK;
}

extern "C" int muse_test_spectrum_cache_policy(int64_t rows, int32_t N, int32_t f32, int32_t mode, int64_t min_rows,
                                               int64_t free_bytes, int64_t budget_bytes, int32_t *decision,
                                               int64_t *rows_cached, int64_t *bytes)
{
    if (!decision || !rows_cached || !bytes)
        return fail(MUSE_ERR_INVALID, "NULL output");
    *decision = spectrum_cache_policy(rows, N, f32 != 0, mode, min_rows < 0 ? ZC_MIN_ROWS : min_rows, free_bytes,
                                      budget_bytes < 0 ? -1 : budget_bytes, rows_cached, bytes);
    return MUSE_OK;
}

// test hook: the pairs the last n = 4096 all-scores pass of this batch listed for the rescaling kernel, in list order
extern "C" int muse_test_batch_redo_pairs(muse_batch *b, int64_t *pairs, int64_t cap, int64_t *count)
{
    if (!b || !count || cap < 0 || (cap > 0 && !pairs))
        return fail(MUSE_ERR_INVALID, "bad redo-list arguments");
    *count = 0;
    int rc = use_device(b->ctx);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(b->stream()));
    if (!b->ovf_count || !b->ovf_list.p)
        return MUSE_OK;
    int listed = 0;
    HIP_TRY(hipMemcpy(&listed, b->ovf_count, sizeof(int), hipMemcpyDeviceToHost));
    *count = listed;
    const int64_t k = std::min<int64_t>(std::min<int64_t>(listed, cap), b->ovf_list.cap);
    if (k > 0)
        HIP_TRY(hipMemcpy(pairs, b->ovf_list.p, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost));
    return MUSE_OK;
}

extern "C" int muse_batch_score(muse_batch *b)
{
    return batch_score(b, ScorePass{});
}

// the masked argmax is built into the default kernels of n = 512 ... 4096 and the rescaling kernel behind the n = 4096 one
static int check_mask(const muse_batch *b, int variant, const LagRange &mask)
{
    if (!(variant == KERNEL_R16_FOLD || variant == KERNEL_R16_OCC3 || (variant == KERNEL_SMALL && b->logn <= 11)) || 2 * mask.hi > b->n)
        return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass runs on the default kernels of FFT lengths 512 ... 4096");
    if (2 * mask.lneg > b->n - 2)
        return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass takes at most n / 2 - 1 lags below zero");
    return MUSE_OK;
}

// (the refusals below in the order batch_score meets them)
int batch_score_check(muse_batch *b, const LagRange *mask, int *variant)
{
    *variant = -1;
    if (b->n > GENERIC_MAX_N)
        return b->g->f32 ? fail(MUSE_ERR_UNSUPPORTED, "float32-storage groups run on the default kernels only (FFT lengths 512 ... 16384)") : MUSE_OK;
    const KernelChoice kc = choose_kernel(b, (b->g->M + 1) / 2);
    if (kc.error)
        return fail(MUSE_ERR_UNSUPPORTED, "%s", kc.error);
    if (mask && check_mask(b, kc.variant, *mask))
        return MUSE_ERR_UNSUPPORTED;
    *variant = kc.variant;
    return MUSE_OK;
}

int batch_score(muse_batch *b, const ScorePass &pass)
{
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    muse_ctx *ctx = b->ctx;
    int rc = use_device(ctx);
    if (rc)
        return rc;
    rc = group_ready(b->g, b->stream()); // rows still in the staging buffer are uploaded (copy stream) ahead of the kernel
    if (rc)
        return rc;
    const int64_t M = b->g->M;
    if (M == 0)
        return MUSE_OK;
    const hipStream_t st = b->stream();
    rc = ensure_scores(b);
    if (rc)
        return rc;
    b->origin = ScoreOrigin{};
    if (pass.window ? pass.direct() : b->windowed()) { // the best match inside the window, directly (xcorr_window.hip): no transform, never screened
        b->scores_exact = true;
        return score_direct(b, pass.window ? *pass.window : lag_window_range(b->n, b->lag_window), true, pass.window ? pass.sign : 0);
    }
    if (b->n > GENERIC_MAX_N) { // series longer than 65 536 samples: a sequence of chip-wide kernels per batch of pairs (xcorr_huge.hip)
        if (b->g->f32)
            return fail(MUSE_ERR_UNSUPPORTED, "float32-storage groups run on the default kernels only (FFT lengths 512 ... 16384)");
        b->scores_exact = true;
        return huge_score(b);
    }
    // long series work in the context's scratch buffer: its pointer must not be swapped (a concurrent
    // muse_batch_create growing it) between reading it and enqueueing the launch
    std::unique_lock<std::mutex> scratch_lock(ctx->stage_mu, std::defer_lock);
    if (b->n >= GENERIC_LDS_MAX_N)
        scratch_lock.lock();
    FusedParams p = base_params(b);
    b->scores_exact = true;
    // kernel selection: ctx->variant 0 = auto; the others are test hooks (muse_hip_test.h).  One helper decides, for the launch
    // here and for the name muse_batch_kernel_name reports (bench.py keys its counters by it)
    const KernelChoice kc = choose_kernel(b, p.npairs);
    if (kc.error)
        return fail(MUSE_ERR_UNSUPPORTED, "%s", kc.error);
    const int variant = kc.variant;
    if (kc.gsmall)
        p.gsmall = kc.gsmall;
    const LagRange *mask = pass.mask();
    if (mask) { // the two bounds as the caller clipped them
        rc = check_mask(b, variant, *mask);
        if (rc)
            return rc;
        b->origin = ScoreOrigin::in_window(MUSE_IN_WINDOW_MASKED, *mask, variant);
        set_window(p, *mask); // (a band: the band builds of the same kernels, the rescaling kernel behind the n = 4096 one included)
        p.win_sign = pass.sign; // (+-1: the signed builds of the same kernels, the rescaling kernel behind the n = 4096 one included)
        b->origin.sign = pass.sign;
    }
    const bool allow_spectrum_cache = pass.allow_spectrum_cache;
    const SlideFuse *slide = pass.slide;
    if (slide) { // (the rows are rewritten by the launch: only the kernel that was built for it may see the tails)
        if (variant != KERNEL_R16_FOLD || allow_spectrum_cache)
            return fail(MUSE_ERR_INVALID, "the fused slide runs in the default n = 4096 kernel, off the rows");
        p.slide_tails = slide->tails;
        p.slide_k = slide->k;
    }
    if (variant == KERNEL_GENERIC && b->n <= GENERIC_LDS_MAX_N)
        p.gscratch = nullptr; // the generic kernel takes a non-NULL scratch pointer as "work in global memory"
    LaunchTimer timer(ctx, false, st); // (brackets the fused launch alone: not the counter reset in front of it, not the redo launch behind it)
    LaunchTimer redo_timer(ctx, true, st); // the launch that redoes the listed pairs: its own sum (muse_ctx_redo_time)
    if (variant == KERNEL_R16_FOLD) {
        // pairs with a NaN/Inf series or with sigmas too far apart for one shared transform are listed by the kernel
        // (once per such series: 2 entries per pair) and redone by the rescaling kernel right behind it (no host round
        // trip: the count stays on the device and bounds the second launch's loop)
        HIP_TRY(b->ovf_list.ensure(ctx, 2 * p.npairs, st));
        p.ovf_count = b->ovf_count;
        p.work_counter = b->ovf_count + 1;
        p.ovf_list = b->ovf_list.p;
        HIP_TRY(hipMemsetAsync(b->ovf_count, 0, 2 * sizeof(int), st));
        // the group's spectrum cache: decided and enqueued under the group's lock, so that of two batches scored from
        // two host threads one builds and the other one's reader sits behind that writer on the stream
        ZcPlan plan;
        std::unique_lock<std::mutex> zc_lock(b->g->ready_mu, std::defer_lock);
        if (allow_spectrum_cache && !mask && spectrum_cache_candidate(b, variant)) { // (a masked pass always reads the rows)
            zc_lock.lock();
            rc = plan_spectrum_cache(b, plan);
            if (rc)
                return rc;
            if (!plan.use)
                zc_lock.unlock();
        }
        HIP_TRY(timer.begin());
        if (plan.use) { // (one bracket around the pass's launches: in steady state the reader alone)
            bool launched = false;
            const auto next_launch = [&]() { // every launch hands its pairs out from a counter of zero
                const hipError_t e = launched ? hipMemsetAsync(b->ovf_count + 1, 0, sizeof(int), st) : hipSuccess;
                launched = true;
                return e;
            };
            const bool occ4_reader = ctx->zc_reader.load() == 1;
            for (const auto &sg : plan.readers) {
                FusedParams r = p;
                r.npairs = sg.pairs;
                HIP_TRY(next_launch());
                HIP_TRY(launch_cached(r, SpectrumCacheArgs{sg.zc(), sg.zstat(), sg.pair0, sg.pairs}, ctx->num_cus, st, occ4_reader));
            }
            if (plan.tail_pair0 < p.npairs) {
                FusedParams w = p;
                w.npairs = p.npairs - plan.tail_pair0;
                HIP_TRY(next_launch());
                HIP_TRY(launch_cache_fill(w, SpectrumCacheArgs{plan.tail_zpairs ? plan.tail_seg.zc() : nullptr,
                                                               plan.tail_zpairs ? plan.tail_seg.zstat() : nullptr,
                                                               plan.tail_pair0, plan.tail_zpairs}, ctx->num_cus, st));
            }
            zc_lock.unlock();
        } else {
            HIP_TRY(launch_fused(p, variant, ctx->num_cus, st));
        }
        HIP_TRY(timer.end());
        FusedParams q = p;
        q.slide_tails = nullptr; // (the rescaling kernel reads the rows as the launch in front of it left them)
        q.slide_k = 0;
        q.pair_list = b->ovf_list.p;
        q.pair_count = b->ovf_count;
        // a dense list (the same threshold as the hand-off rule above) makes the redo kernel redo EVERY pair: the results of a
        // mixed-unit group then come from kernel 7 in this pass exactly as in the later ones that go there directly
        q.dense_total = ctx->variant == 0 ? p.npairs : 0;
        // grid size only (the loop bound is *pair_count): one resident set, so a group with MANY listed pairs
        // (mixed-unit metrics: sigmas far apart) is redone at full width; an empty list costs a few microseconds
        q.npairs = std::min<long long>(p.npairs, (long long)ctx->num_cus * 3);
        HIP_TRY(redo_timer.begin());
        HIP_TRY(launch_fused(q, KERNEL_R16_OCC3, ctx->num_cus, st));
        HIP_TRY(redo_timer.end());
        // (small groups: a pinned allocation costs more than it can save; the same rows again: the count is known, no second copy --
        // measured: the 4-byte copy was not visible in a Run over 10 000 x 4096 either way)
        if (p.npairs >= 1024 && !(b->handoff_host && b->handoff_M == M && b->handoff_rewrites == b->g->rewrites)) {
            if (!b->handoff_host)
                HIP_TRY(hmalloc(ctx, &b->handoff_host, sizeof(int)));
            *b->handoff_host = 0;
            b->handoff_M = M;
            b->handoff_rewrites = b->g->rewrites;
            HIP_TRY(hipMemcpyAsync(b->handoff_host, b->ovf_count, sizeof(int), hipMemcpyDeviceToHost, st));
        }
    } else if (variant == KERNEL_LONG) {
        // as above: NaN / Inf and sigma-spread pairs are listed (one entry per pair) and redone by the four-step kernel that
        // isolates and rescales the series first
        HIP_TRY(b->ovf_list.ensure(ctx, 2 * p.npairs, st));
        p.ovf_count = b->ovf_count;
        p.ovf_list = b->ovf_list.p;
        HIP_TRY(hipMemsetAsync(b->ovf_count, 0, 2 * sizeof(int), st));
        HIP_TRY(timer.begin());
        HIP_TRY(launch_fused(p, variant, ctx->num_cus, st));
        HIP_TRY(timer.end());
        FusedParams q = p;
        q.pair_list = b->ovf_list.p;
        q.pair_count = b->ovf_count;
        q.npairs = std::min<long long>(p.npairs, (long long)ctx->num_cus * STOCKHAM_GLOBAL_WGS_PER_CU);
        HIP_TRY(redo_timer.begin());
        HIP_TRY(launch_fused(q, KERNEL_STOCKHAM, ctx->num_cus, st));
        HIP_TRY(redo_timer.end());
    } else {
        HIP_TRY(timer.begin());
        HIP_TRY(launch_fused(p, variant, ctx->num_cus, st));
        HIP_TRY(timer.end());
    }
    return MUSE_OK;
}

extern "C" int muse_batch_scores(muse_batch *b, int32_t *lag, double *mv)
{
    int rc = muse_batch_score(b);
    if (rc)
        return rc;
    const int64_t M = b->g->M;
    if (M == 0)
        return MUSE_OK;
    if (!lag || !mv)
        return fail(MUSE_ERR_INVALID, "NULL output");
    HIP_TRY(hipMemcpyAsync(lag, b->lag.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, b->stream()));
    HIP_TRY(hipMemcpyAsync(mv, b->mv.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, b->stream()));
    HIP_TRY(hipStreamSynchronize(b->stream()));
    return MUSE_OK;
}

// the kernel automatic selection takes for this batch's all-scores pass (bench.py names it in its roofline object)
// the kernel the all-scores pass takes for this batch (bench.py names it in its roofline object), from the same choice the launch
// makes -- test hooks, missing tables and the learned hand-off included
extern "C" int muse_batch_kernel_name(muse_batch *b, char *name, int32_t cap)
{
    if (!b || !name || cap < 1)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    // (the names rocprofv3 prints for the instantiations: profiles/r*_counters.json is keyed by them)
    char k[96] = "xcorr_fused_generic";
    const char *padded = b->N < b->n ? "true" : "false", *f32 = b->g->f32 ? "true" : "false";
    const ScoreOrigin &o = b->origin; // (the in-window and packed kinds: an argument of a call, not a setting the next pass takes)
    if (o.slide == MUSE_SLIDE_IN_WINDOW_FUSED) { // (muse_batch_slide_score_in_window's one kernel: plain or masked argmax)
        snprintf(k, sizeof(k), "xcorr_fused_n4096_fold<false, %s, %s, %s, true>", padded, f32, o.kind == ScoreOrigin::MASKED ? "true" : "false");
    } else if (o.kind == ScoreOrigin::MASKED && o.variant == ScoreOrigin::MANY && (o.sign != 0 || o.window.band())) {
        // (muse_batch_score_many_in_lag_band's one masked pass: n = 4096, and n = 512 ... 2048 on float64 rows)
        if (b->n == 4096)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_fold_multi_band<%s, %s, %d, %s>", padded, f32, o.sign, o.window.band() ? "true" : "false");
        else
            snprintf(k, sizeof(k), "xcorr_fused_small_many_band<%d, %s, %d, %s>", b->logn, padded, o.sign, o.window.band() ? "true" : "false");
    } else if (o.kind == ScoreOrigin::MASKED && o.window.band()) { // (muse_batch_score_in_lag_band: the band builds, any sign)
        if (b->n == 4096)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_%s_band<%s, %s, %d>", o.variant == KERNEL_R16_OCC3 ? "occ4" : "fold", padded, f32, o.sign);
        else
            snprintf(k, sizeof(k), "xcorr_fused_small_band<%d, %s, %s, %d>", b->logn, padded, f32, o.sign);
    } else if (o.kind == ScoreOrigin::MFMA && o.window.band()) {
        snprintf(k, sizeof(k), "xcorr_window_band_mfma<%d, %s, %d>", o.mfma_tiles(), window_wide(b->g->rows, b->g->stride) ? "true" : "false", o.sign);
    } else if (o.kind == ScoreOrigin::MASKED && o.sign != 0) { // (muse_batch_score_signed_in_lag_range: the signed builds)
        const char *neg = o.sign < 0 ? "true" : "false";
        if (b->n == 4096)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_%s_signed<%s, %s, %s>", o.variant == KERNEL_R16_OCC3 ? "occ4" : "fold", padded, f32, neg);
        else
            snprintf(k, sizeof(k), "xcorr_fused_small_signed<%d, %s, %s, %s>", b->logn, padded, f32, neg);
    } else if (o.kind == ScoreOrigin::MFMA && o.sign != 0) {
        snprintf(k, sizeof(k), "xcorr_window_signed_mfma<%d, %s, %d>", o.mfma_tiles(), window_wide(b->g->rows, b->g->stride) ? "true" : "false", o.sign);
    } else if (o.kind == ScoreOrigin::MASKED) {
        if (o.variant == ScoreOrigin::MANY && b->n == 4096) // (muse_batch_score_many_in_window's one pass)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_fold_multi<%s, %s, true>", padded, f32);
        else if (o.variant == ScoreOrigin::MANY)
            snprintf(k, sizeof(k), "xcorr_fused_small<%d, %s, true, false, true>", b->logn, padded);
        else if (b->n == 4096 && o.variant == KERNEL_R16_OCC3) // (the learned hand-off, or no correction table)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_occ4<%s, 3, false, %s, true>", padded, f32);
        else if (b->n == 4096)
            snprintf(k, sizeof(k), "xcorr_fused_n4096_fold<false, %s, %s, true>", padded, f32);
        else
            snprintf(k, sizeof(k), "xcorr_fused_small<%d, %s, false, %s, true>", b->logn, padded, f32);
    } else if (o.kind == ScoreOrigin::MFMA) { // (the direct product with the call's window, whatever the batch's own setting)
        snprintf(k, sizeof(k), "xcorr_window_mfma<%d, %s>", o.mfma_tiles(),
                 window_wide(b->g->rows, b->g->stride) ? "true" : "false");
    } else if (o.kind == ScoreOrigin::PACKED_EACH) { // (muse_batch_score_many_in_lag_bands' mixed packed launches)
        snprintf(k, sizeof(k), "xcorr_window_many_each_mfma<%d, %s>", o.tiles, window_wide(b->g->rows, b->g->stride) ? "true" : "false");
    } else if (o.kind == ScoreOrigin::PACKED && (o.sign != 0 || o.window.band())) { // (muse_batch_score_many_in_lag_band's packed launches)
        snprintf(k, sizeof(k), "xcorr_window_many_signed_mfma<%d, %s, %d, %s>", o.tiles, window_wide(b->g->rows, b->g->stride) ? "true" : "false",
                 o.sign, o.window.band() ? "true" : "false");
    } else if (o.kind == ScoreOrigin::PACKED) {
        snprintf(k, sizeof(k), "xcorr_window_many_mfma<%d, %s>", o.tiles, window_wide(b->g->rows, b->g->stride) ? "true" : "false");
    } else if (b->windowed()) {
        snprintf(k, sizeof(k), "xcorr_window_mfma<%d, %s>", (lag_window_range(b->n, b->lag_window).rows() + 15) / 16,
                 window_wide(b->g->rows, b->g->stride) ? "true" : "false");
    } else if (b->n > GENERIC_MAX_N) { // (the pass is a sequence of kernels: the one that moves the most bytes)
        snprintf(k, sizeof(k), "huge_rows<false>");
    } else {
        const KernelChoice kc = choose_kernel(b, (b->g->M + 1) / 2);
        switch (kc.error ? -1 : kc.variant) {
        case KERNEL_R16_FOLD: {
            // the reader once the group's spectrum cache is valid for the rows as they are (what the next pass launches first)
            bool cached = false;
            if (spectrum_cache_candidate(b, kc.variant)) {
                std::lock_guard<std::mutex> lock(b->g->ready_mu);
                int64_t rc_ = 0, by_ = 0;
                cached = b->g->zc_state == muse_group::ZC_VALID && b->g->zc_rewrites == b->g->rewrites && b->g->zc_rows > 0 &&
                         spectrum_cache_policy(b->g->M, b->N, false, b->ctx->zc_mode.load(), b->ctx->zc_min_rows.load(), 0, 0, &rc_, &by_) != ZC_POLICY_NONE;
            }
            if (cached)
                snprintf(k, sizeof(k), "xcorr_cached_n4096%s<%s>", b->ctx->zc_reader.load() == 1 ? "_occ4" : "", padded);
            else
                snprintf(k, sizeof(k), "xcorr_fused_n4096_fold<false, %s, %s>", padded, f32);
            break;
        }
        case KERNEL_R16_OCC3: snprintf(k, sizeof(k), "xcorr_fused_n4096_occ4"); break;
        case KERNEL_SMALL: snprintf(k, sizeof(k), "xcorr_fused_small<%d, %s, false, %s>", b->logn, padded, f32); break;
        case KERNEL_LONG: snprintf(k, sizeof(k), "xcorr_fused_long<%d, %s, false>", b->logn, padded); break;
        case KERNEL_STOCKHAM: snprintf(k, sizeof(k), b->n >= 8192 ? "xcorr_fused_stk_4step" : "xcorr_fused_stockham"); break;
        case KERNEL_REAL_SPLIT: snprintf(k, sizeof(k), "xcorr_fused_real32k_split<%s>", padded); break;
        case KERNEL_REAL: snprintf(k, sizeof(k), "xcorr_fused_real%dk<%s>", b->n / 1024, padded); break;
        default: break;
        }
    }
    snprintf(name, (size_t)cap, "%s", k);
    return MUSE_OK;
}

extern "C" int muse_batch_free(muse_batch *b)
{
    if (!b)
        return MUSE_OK;
    muse_ctx *const c = b->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(b->stream());
    if (b->sp && b->sp->refs.fetch_sub(1) == 1) {
        dfree(c, b->sp->X);
        dfree(c, b->sp->xc);
        dfree(c, b->sp->xcp);
        dfree(c, b->sp->xcw);
        dfree(c, b->sp->xcf);
        dfree(c, b->sp->xs);
        dfree(c, b->sp->c1);
        delete b->sp;
    }
    if (b->small_out) { // kept by the context for its next batch (coherent pinned memory is slow to allocate)
        std::lock_guard<std::mutex> lock(c->small_mu);
        c->small_free.emplace_back(b->small_out, b->small_cap);
    }
    dfree(c, b->ovf_count);
    hfree(c, b->handoff_host);
    hfree(c, b->refine_host);
    hfree(c, b->err_host);
    dfree(c, b->err_dev);
    b->ovf_list.release(c);
    b->mv.release(c);
    b->lag.release(c);
    b->gid_dev.release(c);
    b->gkey.release(c);
    b->gfirst.release(c);
    b->gwin.release(c);
    b->rec.release(c);
    b->selkey.release(c);
    b->cand.release(c);
    b->cnt.release(c);
    b->cand_host.release(c);
    b->cnt_host.release(c);
    b->rec_host.release(c);
    b->key_host.release(c);
    b->scr_flags.release(c);
    b->scr_var.release(c);
    b->include.release(c);
    b->scr_keys.release(c);
    b->scr_gmay.release(c);
    b->scr_gkplus.release(c);
    b->scr_gcert.release(c);
    b->est_save.release(c);
    b->win_e.release(c);
    b->win_pw.release(c);
    b->prof_e.release(c);
    b->prof_pw.release(c);
    b->prof_out.release(c);
    b->prof_idx_host.release(c);
    b->prof_idx.release(c);
    if (b->prof_copied)
        (void)hipEventDestroy(b->prof_copied);
    muse_group *g = b->g;
    muse_ctx *ctx = b->ctx;
    delete b;
    group_release(g);
    ctx_release(ctx);
    return MUSE_OK;
}
