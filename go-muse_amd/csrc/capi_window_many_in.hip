// capi_window_many_in.hip -- many references inside a lag window of any width in one pass (muse_batch_score_many_in_window /
// _run_many_in_window): the dispatch between muse_batch_score_many, muse_batch_score_many_windowed and the many-references
// transform kernels with a masked argmax (the WIN builds of xcorr_fused_n4096_fold_multi and of the MULTI xcorr_fused_small)
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// The dispatch, a pure host function: which pass scores R references against series of N samples (float32 storage or not) inside
// +-max_lag.  The first two rows and the last are in_window_plan's (capi_window.hip); the masked lengths split in two:
//   n = 4096 (either storage), n in {512, 1024, 2048} on float64, R >= 2 : ONE masked many-references pass
//   the other masked cases (R == 1, float32 storage at n <= 2048)         : R single masked passes (muse_batch_score_in_window each)
// (what only the handles know -- a forced kernel variant, a missing correction table -- sends a MASKED list to MASKED_EACH at run time)
static int many_in_window_plan(int32_t N, bool f32, int32_t max_lag, int32_t R)
{
    const int64_t n = muse_next_pow2((double)N);
    const int64_t L = std::min<int64_t>(max_lag, n / 2);
    if (2 * L == n)
        return MUSE_IN_WINDOW_PLAIN;
    if (!f32 && L <= MUSE_LAG_WINDOW_MAX && n <= GENERIC_MAX_N)
        return MUSE_IN_WINDOW_MFMA;
    if (!(n == 512 || n == 1024 || n == 2048 || n == 4096))
        return MUSE_IN_WINDOW_UNSUPPORTED;
    return R >= 2 && (n == 4096 || !f32) ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_MASKED_EACH;
}

extern "C" int muse_test_many_in_window_plan(int32_t N, int32_t f32, int32_t max_lag, int32_t R, int32_t *path)
{
    if (!path || N < 2 || max_lag < 0 || R < 1)
        return fail(MUSE_ERR_INVALID, "bad many-in-window plan arguments (N >= 2, max_lag >= 0, R >= 1)");
    *path = many_in_window_plan(N, f32 != 0, max_lag, R);
    return MUSE_OK;
}

// the list checks of muse_batch_score_many, then the window's: nothing is changed before the last of them has passed
static int check_many_in_window(muse_batch *const *bs, int32_t R, int32_t max_lag)
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
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed many-references pass needs a lag window >= 0");
    for (int r = 0; r < R; r++)
        if (bs[r]->windowed() && bs[r]->lag_window != max_lag)
            return fail(MUSE_ERR_INVALID, "batch %d has a lag window of %d of its own: it must be off or equal to the pass's (%d)", r,
                        bs[r]->lag_window, max_lag);
    return MUSE_OK;
}

// the one masked pass over the rows: muse_batch_score_many's launch sequence with the window in the kernels' arguments
// (device selected by the caller's checks; n in {512, 1024, 2048, 4096}, the one-pass conditions hold)
static int score_many_masked(muse_batch *const *bs, int32_t R, int L)
{
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
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
    const bool small_n = b0->n < 4096;
    std::vector<void *> tab((size_t)R * 4);
    for (int r = 0; r < R; r++) {
        tab[(size_t)r] = small_n ? bs[r]->xc : bs[r]->xcp;
        tab[(size_t)R + r] = bs[r]->mv.p;
        tab[(size_t)2 * R + r] = bs[r]->lag.p;
        tab[(size_t)3 * R + r] = bs[r]->c1;
    }
    rc = upload_many_tab(ctx, tab, false); // (these lengths keep the spectra in registers: no scratch)
    if (rc)
        return rc;
    void **const t = ctx->many_tab.p;
    FusedParams p = base_params(b0);
    p.R = R;
    p.xcp_many = (const double2 *const *)t;
    p.mv_many = (double *const *)(t + R);
    p.lag_many = (int *const *)(t + 2 * R);
    p.c1_many = (const double *const *)(t + 3 * R);
    p.win = 1;
    p.win_lpos = L;
    p.win_lneg = 2 * L == b0->n ? L - 1 : L; // index n / 2 is lag +n/2 (xcorr.go:192-194), as in window_params
    HIP_TRY(b0->ovf_list.ensure(ctx, 2 * p.npairs, b0->stream()));
    p.ovf_count = b0->ovf_count;
    p.work_counter = b0->ovf_count + 1;
    p.ovf_list = b0->ovf_list.p;
    LaunchTimer timer(ctx);
    HIP_TRY(hipMemsetAsync(b0->ovf_count, 0, 2 * sizeof(int), ctx->stream));
    HIP_TRY(timer.begin());
    if (small_n) // (this kernel isolates dead series itself: nothing is handed on)
        HIP_TRY(launch_fused_small(p, ctx->num_cus, ctx->stream));
    else
        HIP_TRY(launch_fused_multi(p, ctx->num_cus, ctx->stream));
    HIP_TRY(timer.end());
    // n = 4096: pairs holding a NaN/Inf series or sigmas too far apart (listed once, by reference 0) are redone per reference by
    // the WIN build of the kernel that isolates and rescales before the shared transform: they keep their window
    LaunchTimer redo_timer(ctx, true); // (one bracket around the R redo launches)
    if (!small_n)
        HIP_TRY(redo_timer.begin());
    for (int r = 0; r < R && !small_n; r++) {
        FusedParams q = base_params(bs[r]);
        q.pair_list = b0->ovf_list.p;
        q.pair_count = b0->ovf_count;
        q.win = 1;
        q.win_lpos = p.win_lpos;
        q.win_lneg = p.win_lneg;
        q.npairs = std::min<long long>(q.npairs, (long long)ctx->num_cus * 3);
        HIP_TRY(launch_fused(q, KERNEL_R16_OCC3, ctx->num_cus, ctx->stream));
    }
    HIP_TRY(redo_timer.end());
    for (int r = 0; r < R; r++) {
        muse_batch *b = bs[r];
        b->many_tiles = 0;
        b->scores_exact = true; // mv / lag of every batch hold fp64 results for every row
        b->last_path = MUSE_RUN_PATH_FP64;
        b->last_screened = false;
        b->in_window_path = MUSE_IN_WINDOW_MASKED;
        b->in_window_L = L;
        b->in_window_variant = IN_WINDOW_VARIANT_MANY;
    }
    return MUSE_OK;
}

extern "C" int muse_batch_score_many_in_window(muse_batch *const *bs, int32_t R, int32_t max_lag)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = check_many_in_window(bs, R, max_lag);
    if (rc)
        return rc;
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    const bool f32 = b0->g->f32;
    int path = many_in_window_plan(b0->N, f32, max_lag, R); // (batches of one group share N, and with it the FFT length)
    if (path == MUSE_IN_WINDOW_UNSUPPORTED)
        return fail(MUSE_ERR_UNSUPPORTED, "a lag window of %d over series of %d samples%s is not built: wider than MUSE_LAG_WINDOW_MAX (%d) and for "
                    "float32 storage the window is a masked argmax of the transform kernels of FFT lengths 512 ... 4096",
                    max_lag, b0->N, f32 ? " in float32 storage" : "", MUSE_LAG_WINDOW_MAX);
    if (path == MUSE_IN_WINDOW_MFMA) // (its own checks come before anything it changes)
        return muse_batch_score_many_windowed(bs, R, max_lag);
    if (path == MUSE_IN_WINDOW_PLAIN) { // the window is every lag: the unwindowed pass; a batch's own (equal) setting is put back, whatever the outcome
        std::vector<int32_t> own((size_t)R);
        for (int r = 0; r < R; r++) {
            own[(size_t)r] = bs[r]->lag_window;
            bs[r]->lag_window = -1;
        }
        rc = muse_batch_score_many(bs, R);
        for (int r = 0; r < R; r++)
            bs[r]->lag_window = own[(size_t)r];
        return rc;
    }
    // the masked lengths.  A kernel forced by a test hook that has no masked build is refused, never run unmasked
    const int v = ctx->variant;
    if (!(b0->n == 4096 ? (v == 0 || v == 10 || v == 7) : (v == 0 || v == 12)))
        return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass runs on the default kernels of FFT lengths 512 ... 4096");
    if (path == MUSE_IN_WINDOW_MASKED) { // muse_batch_score_many's own one-pass conditions
        bool one_pass = b0->n == 4096 ? (v == 0 || v == 10) : (v == 0 || v == 12);
        for (int r = 0; r < R && one_pass; r++)
            one_pass = bs[r]->N == b0->N && (b0->n < 4096 || b0->N == b0->n || bs[r]->c1 != nullptr);
        if (!one_pass)
            path = MUSE_IN_WINDOW_MASKED_EACH;
    }
    if (path == MUSE_IN_WINDOW_MASKED_EACH) {
        for (int r = 0; r < R; r++) {
            rc = muse_batch_score_in_window(bs[r], max_lag);
            if (rc)
                return rc;
        }
        return MUSE_OK;
    }
    return score_many_masked(bs, R, std::min(max_lag, b0->n / 2));
}

extern "C" int muse_batch_run_many_in_window(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                             int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                             int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                             int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_window)
    if (sign_filter < -1 || sign_filter > 1)
        return fail(MUSE_ERR_INVALID, "sign_filter must be -1, 0 or 1");
    if (group_id && G < 0)
        return fail(MUSE_ERR_INVALID, "negative group count");
    int rc = muse_batch_score_many_in_window(bs, R, max_lag);
    if (rc)
        return rc;
    const size_t cap = (size_t)std::max(top_n, 0);
    for (int r = 0; r < R; r++) {
        muse_batch *b = bs[r];
        const int32_t path = b->in_window_path, L = b->in_window_L, variant = b->in_window_variant, tiles = b->many_tiles;
        std::vector<muse_record> sel;
        rc = run_select(b, group_id, G, 0, max_lag, top_n, threshold, sign_filter, abs_scores, sel, true, false);
        if (rc)
            return rc;
        b->in_window_path = path; // (the selection scores nothing: the scores are still this pass's)
        b->in_window_L = L;
        b->in_window_variant = variant;
        b->many_tiles = tiles;
        emit(sel, out_series ? out_series + cap * r : nullptr, out_lag ? out_lag + cap * r : nullptr,
             out_score ? out_score + cap * r : nullptr, out_count ? out_count + r : nullptr,
             out_mean_abs ? out_mean_abs + r : nullptr);
    }
    return MUSE_OK;
}
