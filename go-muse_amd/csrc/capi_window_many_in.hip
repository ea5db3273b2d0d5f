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

extern "C" int muse_batch_score_many_in_window(muse_batch *const *bs, int32_t R, int32_t max_lag)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed many-references pass needs a lag window >= 0");
    for (int r = 0; r < R; r++) {
        rc = check_own_window(bs[r], max_lag, r);
        if (rc)
            return rc;
    }
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
    // ONE pass where muse_batch_score_many would take one at these lengths (the masked builds: n = 4096, and the small lengths up to 2048)
    const ManyKind kind = path == MUSE_IN_WINDOW_MASKED ? many_kind(bs, R) : MANY_NONE;
    if (kind == MANY_MULTI || (kind == MANY_SMALL && b0->n <= 2048))
        return score_many_pass(bs, R, kind, std::min(max_lag, b0->n / 2));
    for (int r = 0; r < R; r++) {
        rc = muse_batch_score_in_window(bs[r], max_lag);
        if (rc)
            return rc;
    }
    return MUSE_OK;
}

extern "C" int muse_batch_run_many_in_window(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                             int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                             int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                             int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_window)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_many_in_window(bs, R, max_lag);
    if (rc)
        return rc;
    return run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag,
                           out_score, out_count, out_mean_abs);
}
