// capi_window_many_band.hip -- many references inside a lag band or under a sign, in one pass (muse_batch_score_many_in_lag_band /
// _run_many_in_lag_band): the many-references row of the lag-window family for what muse_batch_score_in_lag_band answers for one
// reference -- lags lag_lo .. lag_hi that need not hold lag 0, the argmax by magnitude or over the values of one sign.  sign == 0
// with lag 0 inside IS muse_batch_score_many_in_lag_range (capi_window_many_in.hip): the call delegates.  Otherwise the packed direct
// product with the signed / band scan (score_many_direct with a sign; xcorr_window_many_signed_mfma), the one masked many-references
// pass (score_many_pass with a sign; xcorr_fused_n4096_fold_multi_band, xcorr_fused_small_many_band), or the single call reference
// by reference.
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// The dispatch, a pure host function: which pass scores R references against series of N samples inside the clipped band w under
// `sign` (not both sign == 0 and lag 0 inside: that is many_plan's, capi_window_many_in.hip).  It is signed_window_plan's
// (capi_window.hip) with the masked lengths split in two:
//   n = 4096 (either storage), n in {512, 1024, 2048} on float64, R >= 2 : ONE masked many-references pass
//   the other masked cases (R == 1, float32 storage at n <= 2048)         : R single masked passes
// (many_plan's split, capi_window_many_in.hip; what only the handles know -- a forced kernel variant, a missing correction table, the
// force-transform hook -- is applied at run time)
static int many_band_plan(int32_t N, bool f32, const LagRange &w, int sign, int32_t R, bool force_transform)
{
    const int path = signed_window_plan(N, f32, w, sign, force_transform);
    if (path != MUSE_IN_WINDOW_MASKED)
        return path;
    return R >= 2 && (muse_next_pow2((double)N) == 4096 || !f32) ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_MASKED_EACH;
}

extern "C" int muse_test_many_lag_band_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t R, int32_t *path)
{
    if (!path || N < 2 || R < 1)
        return fail(MUSE_ERR_INVALID, "bad many-lag-band plan arguments (N >= 2, R >= 1, a path to fill)");
    const int rc = check_band_args(lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    if (sign == MUSE_SIGN_ANY && lag_lo <= 0 && lag_hi >= 0)
        return muse_test_many_lag_range_plan(N, f32, lag_lo, lag_hi, R, path);
    const int64_t n = muse_next_pow2((double)N);
    LagRange w;
    if (!clip_band_or_range(n, lag_lo, lag_hi, &w))
        return fail_empty_band(lag_lo, lag_hi, n);
    *path = many_band_plan(N, f32 != 0, w, sign, R, false);
    return MUSE_OK;
}

// the single dispatch batch after batch, each inside its own clipped band: every refusal first, nothing enqueued before the last check
static int score_each_band(muse_batch *const *bs, int32_t R, const std::vector<LagRange> &ws, int sign)
{
    int rc = MUSE_OK;
    ScorePass pass;
    for (int r = 0; r < R && !rc; r++)
        rc = plan_in_window(bs[r], ws[(size_t)r], &pass, sign);
    for (int r = 0; r < R && !rc; r++)
        rc = score_in_window(bs[r], ws[(size_t)r], sign);
    return rc;
}

extern "C" int muse_batch_score_many_in_lag_band(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi, int32_t sign)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = check_batch_list(bs, R);
    if (!rc)
        rc = check_band_args(lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    if (sign == MUSE_SIGN_ANY && lag_lo <= 0 && lag_hi >= 0) // by magnitude with lag 0 inside: the range call, bit for bit on every path
        return muse_batch_score_many_in_lag_range(bs, R, lag_lo, lag_hi);
    std::vector<LagRange> ws((size_t)R);
    for (int r = 0; r < R; r++)
        if (!clip_band_or_range(bs[r]->n, lag_lo, lag_hi, &ws[(size_t)r]))
            return fail_empty_band(lag_lo, lag_hi, bs[r]->n);
    for (int r = 0; r < R && !rc; r++)
        rc = check_own_window(bs[r], lag_lo, lag_hi, r);
    if (rc)
        return rc;
    if (!one_length(bs, R)) // reference by reference, each by its own single dispatch
        return score_each_band(bs, R, ws, sign);
    muse_batch *b0 = bs[0];
    const LagRange w = ws[0];
    const int path = many_band_plan(b0->N, b0->g->f32, w, sign, R, b0->ctx->in_window_force.load());
    if (path == MUSE_IN_WINDOW_MFMA) {
        bool built = true;
        for (int r = 0; r < R; r++)
            built = built && bs[r]->xs;
        if (built) {
            ScoreOrigin alone = ScoreOrigin::in_window(path, w); // (a reference alone in its launch is named as the single call names it)
            alone.sign = sign;
            return score_many_direct(bs, R, w, alone, sign);
        }
    }
    if (path == MUSE_IN_WINDOW_MASKED) {
        // A kernel forced by a test hook that has no masked build is refused, never run unmasked
        const int v = b0->ctx->variant;
        if (!(b0->n == 4096 ? (v == 0 || v == 10 || v == 7) : (v == 0 || v == 12)))
            return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass runs on the default kernels of FFT lengths 512 ... 4096");
        // ONE pass where muse_batch_score_many would take one at these lengths; a list it would score one after the other (a missing
        // correction table, MANY_NONE): the single calls
        const ManyKind kind = many_kind(bs, R);
        if (kind == MANY_MULTI || (kind == MANY_SMALL && b0->n <= 2048))
            return score_many_pass(bs, R, kind, &w, sign);
    }
    // MASKED_EACH, and what the single call refuses (not built: its MUSE_ERR_UNSUPPORTED, nothing changed)
    return score_each_band(bs, R, ws, sign);
}

extern "C" int muse_batch_run_many_in_lag_band(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                               int32_t lag_lo, int32_t lag_hi, int32_t top_n, double threshold, int32_t sign_filter,
                                               int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                               int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_lag_band: they refuse a sign_filter outside -1 .. 1)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_many_in_lag_band(bs, R, lag_lo, lag_hi, sign_filter);
    const int32_t max_lag = (int32_t)std::min<int64_t>(std::max<int64_t>(std::llabs((long long)lag_lo), std::llabs((long long)lag_hi)), INT32_MAX);
    return rc ? rc : run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag,
                                     out_score, out_count, out_mean_abs);
}
