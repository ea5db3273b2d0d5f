// capi_many.hip -- many references against one resident Group in one pass
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;


// -------------------------------------------------------- many references
// The device pointer table of a many-reference pass (score_many_pass, screen_many): the caller's columns of R pointers
// each in `tab`, which becomes the host image the asynchronous copy reads (kept by the context until the next pass has waited
// for the stream).  With `zscratch`, the one-pass kernels' scratch slices too (allocated on first use).
int upload_many_tab(muse_ctx *ctx, std::vector<void *> &tab, bool zscratch)
{
    if (zscratch) // one 64 KB slice per resident workgroup
        HIP_TRY(ctx->zscratch.ensure(ctx, (int64_t)ctx->num_cus * 4 * 4096, ctx->stream));
    HIP_TRY(ctx->many_tab.ensure(ctx, (int64_t)tab.size(), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // the previous pass may still be reading the host image
    ctx->many_host.swap(tab);
    HIP_TRY(hipMemcpyAsync(ctx->many_tab.p, ctx->many_host.data(), ctx->many_host.size() * sizeof(void *),
                           hipMemcpyHostToDevice, ctx->stream));
    return MUSE_OK;
}

extern "C" int muse_batch_read_scores(muse_batch *b, int32_t *lag, double *mv)
{
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    int rc = use_device(b->ctx);
    if (rc)
        return rc;
    const int64_t M = b->g->M;
    if (M == 0)
        return MUSE_OK;
    if (!lag || !mv)
        return fail(MUSE_ERR_INVALID, "NULL output");
    if (M > b->mv.cap || M > b->lag.cap)
        return fail(MUSE_ERR_INVALID, "the batch has not been scored since the group grew");
    if (!b->scores_exact) { // the last Run screened in fp32 and re-evaluated only the rows it needed
        rc = muse_batch_score(b);
        if (rc)
            return rc;
    }
    HIP_TRY(hipMemcpyAsync(lag, b->lag.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, b->ctx->stream));
    HIP_TRY(hipMemcpyAsync(mv, b->mv.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    return MUSE_OK;
}

int check_batch_list(muse_batch *const *bs, int32_t R)
{
    if (!bs || R < 1)
        return fail(MUSE_ERR_INVALID, "bad batch list");
    for (int r = 0; r < R; r++) {
        if (!bs[r])
            return fail(MUSE_ERR_INVALID, "NULL batch in list");
        if (bs[r]->ctx != bs[0]->ctx || bs[r]->g != bs[0]->g)
            return fail(MUSE_ERR_INVALID, "batches of one pass must share the context and the comparison group");
        for (int q = 0; q < r; q++)
            if (bs[q] == bs[r])
                return fail(MUSE_ERR_INVALID, "the same batch appears twice in the list");
    }
    return MUSE_OK;
}

ManyKind many_kind(muse_batch *const *bs, int32_t R)
{
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    // the one-pass kernel is built for N == n == 4096 (and is only taken under automatic kernel
    // selection); everything else scores the batches one after the other
    const bool small_n = (b0->n >= 512 && b0->n <= 2048) || b0->n == 8192 || b0->n == 16384; // xcorr_small.hip's lengths
    // (float32-storage groups: the n = 4096 one-pass kernel reads them; the other lengths' one-pass builds do not)
    // long series (xcorr_long.hip, MULTI): 3 + 3 R slice crossings per pair against 4 R -- from three references on
    // n = 32768 (round 6): ONE real series per workgroup, first-transformed once, every reference from the parked spectrum
    // (xcorr_fused_real32k_multi: 1 x the row bytes where the four-step kernel below moves 5 x); from three references on (two: as
    // fast as two passes -- profiles/r06_many_refs.txt)
    bool real_n = b0->n == 32768 && R >= 3 && !b0->g->f32 && ctx->variant == 0 && ctx->gsmall[4] && ctx->wsplit;
    for (int r = 0; r < R && real_n; r++)
        real_n = bs[r]->N == b0->N && bs[r]->xcw != nullptr;
    const bool long_n = !real_n && (b0->n == 32768 || b0->n == 65536) && R >= 3 && !b0->g->f32 && ctx->variant == 0 && b0->logn >= 14 && ctx->twl[b0->logn - 14];
    bool one_pass = R > 1 &&
                    ((b0->n == 4096 && (ctx->variant == 0 || ctx->variant == 10)) ||
                     (small_n && !b0->g->f32 && (ctx->variant == 0 || ctx->variant == 12)) || long_n || real_n);
    for (int r = 0; r < R && one_pass; r++)
        one_pass = bs[r]->N == b0->N && (small_n || real_n || b0->N == b0->n || bs[r]->c1 != nullptr) && (!long_n || bs[r]->xcp != nullptr);
    if (!one_pass)
        return MANY_NONE;
    return small_n ? MANY_SMALL : real_n ? MANY_REAL : long_n ? MANY_LONG : MANY_MULTI;
}

int score_many_pass(muse_batch *const *bs, int32_t R, ManyKind kind, const LagRange *mask, int sign)
{
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    const bool small_n = kind == MANY_SMALL, real_n = kind == MANY_REAL, long_n = kind == MANY_LONG;
    // the unmasked pass is what each batch's own setting takes too: it says so from the start.  The masked pass is an argument of
    // its call: it names itself once its launches are enqueued (below)
    for (int r = 0; r < R && !mask; r++)
        bs[r]->origin = ScoreOrigin{};
    int rc = use_device(ctx);
    if (rc)
        return rc;
    rc = group_ready(b0->g);
    if (rc)
        return rc;
    const int64_t M = b0->g->M;
    if (M == 0)
        return MUSE_OK;
    for (int r = 0; r < R; r++) {
        rc = ensure_scores(bs[r]);
        if (rc)
            return rc;
    }
    // the two kinds that work in the context's scratch buffer size it differently:
    if (long_n) // two n-element slices per resident workgroup
        HIP_TRY(ensure_gscratch(ctx, b0->n, 2 * LONG_WGS_PER_CU));
    if (real_n) // (half an n-element slice per workgroup: the batches' own creation sized the buffer for far more)
        HIP_TRY(ensure_gscratch(ctx, b0->n));
    std::vector<void *> tab((size_t)R * 4);
    for (int r = 0; r < R; r++) {
        tab[(size_t)r] = small_n ? bs[r]->xc : real_n ? bs[r]->xcw : bs[r]->xcp;
        tab[(size_t)R + r] = bs[r]->mv.p;
        tab[(size_t)2 * R + r] = bs[r]->lag.p;
        tab[(size_t)3 * R + r] = bs[r]->c1;
    }
    // scratch slices at n = 16384 only: every other length keeps the spectra in registers (the masked lengths are among them)
    rc = upload_many_tab(ctx, tab, b0->n == 16384);
    if (rc)
        return rc;
    void **const t = ctx->many_tab.p;
    FusedParams p = base_params(b0);
    p.R = R;
    p.xcp_many = (const double2 *const *)t;
    p.mv_many = (double *const *)(t + R);
    p.lag_many = (int *const *)(t + 2 * R);
    p.c1_many = (const double *const *)(t + 3 * R);
    p.zscratch = ctx->zscratch.p; // (read at n = 16384 only)
    p.zslots = (int)(ctx->zscratch.cap / 4096);
    if (mask) { // (the two bounds as the caller clipped them; a band: its one interval; the sign of muse_batch_score_many_in_lag_band)
        set_window(p, *mask);
        p.win_sign = sign;
    }
    HIP_TRY(b0->ovf_list.ensure(ctx, 2 * p.npairs, b0->stream()));
    p.ovf_count = b0->ovf_count;
    p.work_counter = b0->ovf_count + 1;
    p.ovf_list = b0->ovf_list.p;
    // (the long-series kernel works in the context's scratch buffer: its pointer must not be swapped between reading it and the launch)
    std::unique_lock<std::mutex> scratch_lock(ctx->stage_mu, std::defer_lock);
    if (long_n || real_n) {
        scratch_lock.lock();
        p.gscratch = ctx->gscratch.p;
        p.gscratch_slices = (long long)(ctx->gscratch.cap / b0->n);
    }
    LaunchTimer timer(ctx);
    HIP_TRY(hipMemsetAsync(b0->ovf_count, 0, 2 * sizeof(int), ctx->stream));
    HIP_TRY(timer.begin());
    if (small_n) { // (this kernel isolates dead series itself: nothing is handed on)
        HIP_TRY(launch_fused_small(p, ctx->num_cus, ctx->stream));
    } else if (real_n) { // (one series per transform: nothing to isolate, no redo list)
        p.gsmall = ctx->gsmall[4];
        HIP_TRY(launch_fused_real_split(p, ctx->num_cus, ctx->stream));
    } else if (long_n)
        HIP_TRY(launch_fused_long(p, ctx->num_cus, ctx->stream));
    else
        HIP_TRY(launch_fused_multi(p, ctx->num_cus, ctx->stream));
    HIP_TRY(timer.end());
    // pairs holding a NaN/Inf series or sigmas too far apart (listed once, by reference 0): redone per reference by the
    // kernel that isolates and rescales the series before the shared transform
    const bool redo = !small_n && !real_n;
    LaunchTimer redo_timer(ctx, true); // (one bracket around the R redo launches)
    if (redo)
        HIP_TRY(redo_timer.begin());
    for (int r = 0; r < R && redo; r++) {
        FusedParams q = base_params(bs[r]);
        q.pair_list = b0->ovf_list.p;
        q.pair_count = b0->ovf_count;
        if (mask) { // the redone pairs keep their window (the WIN build of the redo kernel), its sign and its band
            set_window(q, *mask);
            q.win_sign = sign;
        }
        if (long_n) { // (the four-step kernel that isolates and rescales first, as behind a single long-series pass)
            q.npairs = std::min<long long>(q.npairs, (long long)ctx->num_cus * STOCKHAM_GLOBAL_WGS_PER_CU);
            HIP_TRY(launch_fused(q, KERNEL_STOCKHAM, ctx->num_cus, ctx->stream));
        } else {
            q.npairs = std::min<long long>(q.npairs, (long long)ctx->num_cus * 3);
            HIP_TRY(launch_fused(q, KERNEL_R16_OCC3, ctx->num_cus, ctx->stream));
        }
    }
    HIP_TRY(redo_timer.end());
    for (int r = 0; r < R; r++) {
        muse_batch *b = bs[r];
        b->scores_exact = true; // mv / lag of every batch now hold fp64 results for every row
        if (mask) { // as muse_batch_score_in_window leaves a batch; the unmasked pass, as muse_batch_score, leaves what the last Run did alone
            b->last_path = MUSE_RUN_PATH_FP64;
            b->last_screened = false;
            b->origin = ScoreOrigin::in_window(MUSE_IN_WINDOW_MASKED, *mask, ScoreOrigin::MANY);
            b->origin.sign = sign;
        }
    }
    return MUSE_OK;
}

extern "C" int muse_batch_score_many(muse_batch *const *bs, int32_t R)
{
    int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    for (int r = 0; r < R; r++)
        if (bs[r]->windowed())
            return fail(MUSE_ERR_UNSUPPORTED, "a batch with a lag window cannot take part in a many-references pass");
    return score_many_every_lag(bs, R, ScorePass{false}); // (a many-references pass never builds or reads the spectrum cache)
}

int score_many_every_lag(muse_batch *const *bs, int32_t R, const ScorePass &each)
{
    const ManyKind kind = many_kind(bs, R);
    if (kind != MANY_NONE)
        return score_many_pass(bs, R, kind, nullptr);
    for (int r = 0; r < R; r++) {
        const int rc = batch_score(bs[r], each);
        if (rc)
            return rc;
    }
    return MUSE_OK;
}

int run_many_select(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n,
                    double threshold, int32_t sign_filter, int32_t abs_scores, bool prescreened, int64_t *out_series,
                    int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs)
{
    const size_t cap = (size_t)std::max(top_n, 0);
    for (int r = 0; r < R; r++) {
        const int rc = run_scored(bs[r], group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores,
                                  out_series ? out_series + cap * r : nullptr, out_lag ? out_lag + cap * r : nullptr,
                                  out_score ? out_score + cap * r : nullptr, out_count ? out_count + r : nullptr,
                                  out_mean_abs ? out_mean_abs + r : nullptr, prescreened);
        if (rc)
            return rc;
    }
    return MUSE_OK;
}

extern "C" int muse_batch_run_many(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                   int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                   int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                   int32_t *out_count, double *out_mean_abs)
{
    for (int r = 0; bs && r < R; r++) // (before the list is validated: a windowed batch in a bad list is reported as windowed)
        if (bs[r] && bs[r]->windowed())
            return fail(MUSE_ERR_UNSUPPORTED, "a batch with a lag window cannot take part in a many-references pass");
    bool prescreened = false;
    int rc = screen_many(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, prescreened);
    if (rc)
        return rc;
    if (!prescreened) {
        rc = muse_batch_score_many(bs, R);
        if (rc)
            return rc;
    }
    return run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, prescreened, out_series, out_lag,
                           out_score, out_count, out_mean_abs);
}
