// capi_window_many_range.hip -- many references inside a lag range lag_lo .. lag_hi in one pass (muse_batch_score_many_in_lag_range /
// _run_many_in_lag_range): the dispatch between muse_batch_score_many, the direct product with the references' table rows packed
// (score_many_direct, capi_window_many.hip) and the many-references transform kernels with a masked argmax whose two bounds are set
// independently (score_many_pass, capi_many.hip)
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// The dispatch, a pure host function: which pass scores R references against series of N samples (float32 storage or not) inside
// lag_lo .. lag_hi; W = the lags of the clipped range.  The first two rows and the last are lag_range_plan's (capi_window.hip), the
// masked lengths split as many_in_window_plan splits them (capi_window_many_in.hip); for lag_lo == -lag_hi it is that table row for row.
//   the range is every lag                               : muse_batch_score_many
//   float64, W <= 2 MUSE_LAG_WINDOW_MAX + 1, n <= 65536    : the direct product, packed where window_many_plan packs
//   n = 4096 (either storage), n in {512, 1024, 2048} on float64, R >= 2 : ONE masked many-references pass
//   the other masked cases (R == 1, float32 storage at n <= 2048)         : R single masked passes (muse_batch_score_in_lag_range each)
// (what only the handles know -- a forced kernel variant, a missing correction table -- sends a MASKED list to MASKED_EACH at run time)
static int many_lag_range_plan(int32_t N, bool f32, int32_t lag_lo, int32_t lag_hi, int32_t R)
{
    const int64_t n = muse_next_pow2((double)N);
    const LagRange r = clip_lag_range(n, lag_lo, lag_hi);
    if (2 * (int64_t)r.hi == n && r.lneg == n / 2 - 1)
        return MUSE_IN_WINDOW_PLAIN;
    if (!f32 && r.W() <= 2 * MUSE_LAG_WINDOW_MAX + 1 && n <= GENERIC_MAX_N)
        return MUSE_IN_WINDOW_MFMA;
    if (!(n == 512 || n == 1024 || n == 2048 || n == 4096))
        return MUSE_IN_WINDOW_UNSUPPORTED;
    return R >= 2 && (n == 4096 || !f32) ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_MASKED_EACH;
}

extern "C" int muse_test_many_lag_range_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t R, int32_t *path)
{
    if (!path || N < 2 || lag_lo > 0 || lag_hi < 0 || R < 1)
        return fail(MUSE_ERR_INVALID, "bad many-lag-range plan arguments (N >= 2, lag_lo <= 0 <= lag_hi, R >= 1)");
    *path = many_lag_range_plan(N, f32 != 0, lag_lo, lag_hi, R);
    return MUSE_OK;
}

static int fail_not_built(const muse_batch *b, int32_t lag_lo, int32_t lag_hi)
{
    return fail(MUSE_ERR_UNSUPPORTED, "the lag range %d .. %d over series of %d samples%s is not built: more than %d lags and float32 "
                "storage take the masked argmax of the transform kernels of FFT lengths 512 ... 4096",
                lag_lo, lag_hi, b->N, b->g->f32 ? " in float32 storage" : "", 2 * MUSE_LAG_WINDOW_MAX + 1);
}

// muse_batch_score_in_lag_range batch after batch, for batches that call would not refuse (checked by the caller)
static int score_each(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi)
{
    for (int r = 0; r < R; r++) {
        const int rc = muse_batch_score_in_lag_range(bs[r], lag_lo, lag_hi);
        if (rc)
            return rc;
    }
    return MUSE_OK;
}

// what muse_batch_score_in_lag_range(b, lag_lo, lag_hi) would refuse for a batch without a window of its own, nothing enqueued
static int check_single(muse_batch *b, int32_t lag_lo, int32_t lag_hi)
{
    const int path = lag_range_plan(b->N, b->g->f32, lag_lo, lag_hi, b->ctx->in_window_force.load());
    if (path == MUSE_IN_WINDOW_UNSUPPORTED || (path == MUSE_IN_WINDOW_MFMA && !b->xs))
        return fail_not_built(b, lag_lo, lag_hi);
    if (path == MUSE_IN_WINDOW_MFMA)
        return MUSE_OK;
    int variant = -1;
    return batch_score_check(b, path == MUSE_IN_WINDOW_MASKED ? clip_lag_range(b->n, lag_lo, lag_hi).hi : -1, &variant);
}

extern "C" int muse_batch_score_many_in_lag_range(muse_batch *const *bs, int32_t R, int32_t lag_lo, int32_t lag_hi)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    if (lag_lo > 0 || lag_hi < 0)
        return fail(MUSE_ERR_INVALID, "the lag range %d .. %d does not hold lag 0 (lag_lo <= 0 <= lag_hi)", lag_lo, lag_hi);
    if ((int64_t)lag_lo == -(int64_t)lag_hi) // by definition: the symmetric window's pass, bit for bit on every path
        return muse_batch_score_many_in_window(bs, R, lag_hi);
    for (int r = 0; r < R; r++)
        if (bs[r]->windowed())
            return fail(MUSE_ERR_INVALID, "batch %d has a lag window of %d of its own: it must be off, or equal to a range -L .. L", r,
                        bs[r]->lag_window);
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    bool same = true;
    for (int r = 1; r < R; r++)
        same = same && bs[r]->N == b0->N && bs[r]->n == b0->n;
    if (!same) { // the clipping is per length: reference by reference, each by its own single dispatch
        for (int r = 0; r < R; r++) {
            rc = check_single(bs[r], lag_lo, lag_hi);
            if (rc)
                return rc;
        }
        return score_each(bs, R, lag_lo, lag_hi);
    }
    const int path = many_lag_range_plan(b0->N, b0->g->f32, lag_lo, lag_hi, R);
    if (path == MUSE_IN_WINDOW_UNSUPPORTED)
        return fail_not_built(b0, lag_lo, lag_hi);
    const LagRange range = clip_lag_range(b0->n, lag_lo, lag_hi);
    if (path == MUSE_IN_WINDOW_MFMA) {
        for (int r = 0; r < R; r++)
            if (!bs[r]->xs)
                return fail_not_built(bs[r], lag_lo, lag_hi);
        return score_many_direct(bs, R, 0, &range);
    }
    if (path == MUSE_IN_WINDOW_PLAIN) // the range is every lag: the unwindowed pass (no batch has a window of its own here)
        return muse_batch_score_many(bs, R);
    // the masked lengths.  A kernel forced by a test hook that has no masked build is refused, never run unmasked
    const int v = ctx->variant;
    if (!(b0->n == 4096 ? (v == 0 || v == 10 || v == 7) : (v == 0 || v == 12)))
        return fail(MUSE_ERR_UNSUPPORTED, "the masked transform pass runs on the default kernels of FFT lengths 512 ... 4096");
    // ONE pass where muse_batch_score_many would take one at these lengths, as muse_batch_score_many_in_window decides it
    const ManyKind kind = path == MUSE_IN_WINDOW_MASKED ? many_kind(bs, R) : MANY_NONE;
    if (kind == MANY_MULTI || (kind == MANY_SMALL && b0->n <= 2048))
        return score_many_pass(bs, R, kind, range.hi, range.lneg);
    for (int r = 0; r < R; r++) {
        rc = check_single(bs[r], lag_lo, lag_hi);
        if (rc)
            return rc;
    }
    return score_each(bs, R, lag_lo, lag_hi);
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
    if (rc)
        return rc;
    // Results.MaxLag = max(-lag_lo, lag_hi): every lag of the range passes the lag filter
    const int32_t max_lag = (int32_t)std::min<int64_t>(std::max<int64_t>(-(int64_t)lag_lo, lag_hi), INT32_MAX);
    return run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag,
                           out_score, out_count, out_mean_abs);
}
