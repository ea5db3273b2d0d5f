// capi_window_many_in.hip -- many references inside a lag window of any width, or a lag range lag_lo .. lag_hi, in one pass
// (muse_batch_score_many_in_window / _run_many_in_window, muse_batch_score_many_in_lag_range / _run_many_in_lag_range): one dispatch
// with two argument shapes, between muse_batch_score_many, the direct product with the references' table rows packed
// (score_many_direct, capi_window_many.hip) and the many-references transform kernels with a masked argmax (score_many_pass,
// capi_many.hip: the WIN builds of xcorr_fused_n4096_fold_multi and of the MULTI xcorr_fused_small)
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// The dispatch, a pure host function: which pass scores R references against series of N samples (float32 storage or not) inside w.
// It is window_plan's (capi_window.hip) with the masked lengths split in two:
//   n = 4096 (either storage), n in {512, 1024, 2048} on float64, R >= 2 : ONE masked many-references pass
//   the other masked cases (R == 1, float32 storage at n <= 2048)         : R single masked passes (score_in_window each)
// (what only the handles know -- a forced kernel variant, a missing correction table -- sends a MASKED list to MASKED_EACH at run time)
static int many_plan(int32_t N, bool f32, const LagRange &w, int32_t R)
{
    const int path = window_plan(N, f32, w, false);
    if (path != MUSE_IN_WINDOW_MASKED)
        return path;
    return R >= 2 && (muse_next_pow2((double)N) == 4096 || !f32) ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_MASKED_EACH;
}

extern "C" int muse_test_many_in_window_plan(int32_t N, int32_t f32, int32_t max_lag, int32_t R, int32_t *path)
{
    if (!path || N < 2 || max_lag < 0 || R < 1)
        return fail(MUSE_ERR_INVALID, "bad many-in-window plan arguments (N >= 2, max_lag >= 0, R >= 1)");
    *path = many_plan(N, f32 != 0, lag_window_range(muse_next_pow2((double)N), max_lag), R);
    return MUSE_OK;
}

extern "C" int muse_test_many_lag_range_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t R, int32_t *path)
{
    if (!path || N < 2 || lag_lo > 0 || lag_hi < 0 || R < 1)
        return fail(MUSE_ERR_INVALID, "bad many-lag-range plan arguments (N >= 2, lag_lo <= 0 <= lag_hi, R >= 1)");
    *path = many_plan(N, f32 != 0, clip_lag_range(muse_next_pow2((double)N), lag_lo, lag_hi), R);
    return MUSE_OK;
}

// the single dispatch batch after batch (the clipping is per length): every refusal first, nothing enqueued before the last check
static int score_each(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi)
{
    int rc = MUSE_OK;
    ScorePass pass;
    for (int r = 0; r < R && !rc; r++)
        rc = plan_in_window(bs[r], clip_lag_range(bs[r]->n, lag_lo, lag_hi), &pass);
    for (int r = 0; r < R && !rc; r++)
        rc = score_in_window(bs[r], clip_lag_range(bs[r]->n, lag_lo, lag_hi));
    return rc;
}

// a checked list inside lag_lo .. lag_hi (lag_lo <= 0 <= lag_hi; the window +-L is -L .. L)
static int score_many_in(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = MUSE_OK;
    for (int r = 0; r < R && !rc; r++)
        rc = check_own_window(bs[r], lag_lo, lag_hi, r);
    if (rc)
        return rc;
    if (!one_length(bs, R)) // reference by reference, each by its own single dispatch
        return score_each(bs, R, lag_lo, lag_hi);
    muse_batch *b0 = bs[0];
    const LagRange w = clip_lag_range(b0->n, lag_lo, lag_hi);
    const int path = many_plan(b0->N, b0->g->f32, w, R);
    bool built = path != MUSE_IN_WINDOW_UNSUPPORTED;
    for (int r = 0; r < R && path == MUSE_IN_WINDOW_MFMA; r++)
        built = built && bs[r]->xs;
    if (!built)
        return fail(MUSE_ERR_UNSUPPORTED, "the lags %d .. %d over series of %d samples%s are not built: more than %d table rows and float32 "
                    "storage take the masked argmax of the transform kernels of FFT lengths 512 ... 4096",
                    -w.lneg, w.hi, b0->N, b0->g->f32 ? " in float32 storage" : "", 2 * MUSE_LAG_WINDOW_MAX + 1);
    if (path == MUSE_IN_WINDOW_MFMA) // (a reference alone in its launch is named as the single call names it: a window +-L by the batch's own setting)
        return score_many_direct(bs, R, w, (int64_t)lag_lo == -(int64_t)lag_hi ? ScoreOrigin{} : ScoreOrigin::in_window(path, w));
    if (path == MUSE_IN_WINDOW_PLAIN) // every lag: the unwindowed pass, a batch's own (equal) setting out of its way
        return score_many_every_lag(bs, R, ScorePass{false, &w, path});
    // the masked lengths.  A kernel forced by a test hook that has no masked build is refused, never run unmasked
    const int v = b0->ctx->variant;
    if (!(b0->n == 4096 ? (v == 0 || v == 10 || v == 7) : (v == 0 || v == 12)))
        return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass runs on the default kernels of FFT lengths 512 ... 4096");
    // ONE pass where muse_batch_score_many would take one at these lengths (the masked builds: n = 4096, and the small lengths up to 2048)
    const ManyKind kind = path == MUSE_IN_WINDOW_MASKED ? many_kind(bs, R) : MANY_NONE;
    if (kind == MANY_MULTI || (kind == MANY_SMALL && b0->n <= 2048))
        return score_many_pass(bs, R, kind, &w);
    return score_each(bs, R, lag_lo, lag_hi);
}

extern "C" int muse_batch_score_many_in_window(muse_batch *const *bs, int32_t R, int32_t max_lag)
{
    const int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed many-references pass needs a lag window >= 0");
    return score_many_in(bs, R, -max_lag, max_lag);
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
    return rc ? rc : run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag, out_score, out_count, out_mean_abs);
}

extern "C" int muse_batch_score_many_in_lag_range(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi)
{
    const int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    if (lag_lo > 0 || lag_hi < 0)
        return fail(MUSE_ERR_INVALID, "the lag range %d .. %d does not hold lag 0 (lag_lo <= 0 <= lag_hi)", lag_lo, lag_hi);
    return score_many_in(bs, R, lag_lo, lag_hi);
}

extern "C" int muse_batch_run_many_in_lag_range(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                                int32_t lag_lo, int32_t lag_hi, int32_t top_n, double threshold, int32_t sign_filter,
                                                int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                                int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_lag_range)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_many_in_lag_range(bs, R, lag_lo, lag_hi);
    return rc ? rc : run_many_select(bs, R, group_id, G, range_max_lag(lag_lo, lag_hi), top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag, out_score, out_count, out_mean_abs);
}
