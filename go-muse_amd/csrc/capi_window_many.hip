// capi_window_many.hip -- many references inside a lag window in one pass (muse_batch_score_many_windowed / _run_many_windowed)
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// test hooks: the planner alone (xcorr_window_many.hip), no device; W = the rows of a reference's table
static void plan_rows(int32_t R, int32_t W, int32_t *launches, int32_t *launch_of, int32_t *tiles_of, int32_t *max_refs, int32_t *img_of,
                      int32_t *kc_of)
{
    std::vector<int> of((size_t)R), tiles((size_t)R);
    const int n = window_many_plan(R, W, of.data(), tiles.data());
    *launches = n;
    if (max_refs)
        *max_refs = window_many_max_refs(W);
    std::vector<int> refs((size_t)n, 0);
    for (int r = 0; r < R; r++) {
        refs[(size_t)of[(size_t)r]]++;
        if (launch_of)
            launch_of[r] = of[(size_t)r];
    }
    for (int l = 0; l < n; l++) {
        const int kc = refs[(size_t)l] > 1 ? window_many_kc(W, refs[(size_t)l]) : WIN_KC; // (one reference: xcorr_window_mfma's chunk)
        if (tiles_of)
            tiles_of[l] = tiles[(size_t)l];
        if (kc_of)
            kc_of[l] = kc;
        if (img_of)
            img_of[l] = refs[(size_t)l] > 1 ? window_many_img(W, kc) : WIN_KC + WIN_E_TAIL;
    }
}

extern "C" int muse_test_window_many_plan(int32_t R, int32_t L, int32_t *launches, int32_t *launch_of, int32_t *tiles_of,
                                          int32_t *max_refs, int32_t *img_of, int32_t *kc_of)
{
    if (R < 1 || L < 0 || L > MUSE_LAG_WINDOW_MAX || !launches)
        return fail(MUSE_ERR_INVALID, "window plan: R >= 1, 0 <= L <= %d", MUSE_LAG_WINDOW_MAX);
    plan_rows(R, 2 * L + 1, launches, launch_of, tiles_of, max_refs, img_of, kc_of);
    return MUSE_OK;
}

extern "C" int muse_test_window_many_plan_rows(int32_t R, int32_t W, int32_t *launches, int32_t *launch_of, int32_t *tiles_of,
                                               int32_t *max_refs, int32_t *img_of, int32_t *kc_of)
{
    if (R < 1 || W < 1 || W > 2 * MUSE_LAG_WINDOW_MAX + 1 || !launches)
        return fail(MUSE_ERR_INVALID, "window plan: R >= 1, 1 <= W <= %d", 2 * MUSE_LAG_WINDOW_MAX + 1);
    plan_rows(R, W, launches, launch_of, tiles_of, max_refs, img_of, kc_of);
    return MUSE_OK;
}

extern "C" int muse_batch_score_many_windowed(muse_batch *const *bs, int32_t R, int32_t max_lag)
{
    // the list checks, then the window's: nothing is changed before the last of them has passed
    int rc = check_batch_list(bs, R);
    if (rc)
        return rc;
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed many-references pass needs a lag window >= 0");
    for (int r = 0; r < R; r++) { // (the batches share the group and the window: behind r = 0 only the length check can still refuse)
        rc = check_window_request(bs[r], max_lag, bs[r]->g->f32);
        if (!rc)
            rc = check_own_window(bs[r], -max_lag, max_lag, r);
        if (rc)
            return rc;
    }
    // (a reference alone in its launch: the single-reference kernel, named as before the pass by the batch's own setting)
    if (one_length(bs, R))
        return score_many_direct(bs, R, lag_window_range(bs[0]->n, max_lag), ScoreOrigin{});
    for (int r = 0; r < R && !rc; r++) // the clipping is per length: reference by reference
        rc = score_many_direct(bs + r, 1, lag_window_range(bs[r]->n, max_lag), ScoreOrigin{});
    return rc;
}

// The direct product inside w for a checked list of one length, in as few launches as the planner gives.  Each batch's tables are its
// own, cached as score_direct caches them (window_tables): the packed and the single pass serve each other's tables.  sign != 0 or a
// band w: the signed / band scan (launch_window_many_signed; a reference alone: launch_window_signed / launch_window_band)
int score_many_direct(muse_batch *const *bs, int32_t R, LagRange w, const ScoreOrigin &alone, int sign)
{
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    if (!one_length(bs, R))
        return fail(MUSE_ERR_INVALID, "a packed lag window needs batches of one length");
    int rc = use_device(ctx);
    if (rc)
        return rc;
    rc = group_ready(b0->g);
    if (rc)
        return rc;
    const int64_t M = b0->g->M;
    if (M == 0)
        return MUSE_OK;
    const hipStream_t st = ctx->stream;
    for (int r = 0; r < R; r++) {
        rc = ensure_scores(bs[r]);
        if (!rc)
            rc = window_tables(bs[r], w, bs[r]->win_e, bs[r]->win_pw, &bs[r]->win_key, st);
        if (rc)
            return rc;
    }
    std::vector<int> launch_of((size_t)R), tiles_of((size_t)R);
    window_many_plan(R, w.rows(), launch_of.data(), tiles_of.data());
    bool packed = false;
    for (int r = 0; r + 1 < R; r++)
        packed = packed || launch_of[(size_t)r] == launch_of[(size_t)r + 1];
    void **tab_dev = nullptr;
    if (packed) { // columns of R pointers: e, pw, mv, lag (a launch takes its slice of each)
        std::vector<void *> tab((size_t)R * 4);
        for (int r = 0; r < R; r++) {
            tab[(size_t)r] = bs[r]->win_e.p;
            tab[(size_t)R + r] = bs[r]->win_pw.p;
            tab[(size_t)2 * R + r] = bs[r]->mv.p;
            tab[(size_t)3 * R + r] = bs[r]->lag.p;
        }
        rc = upload_many_tab(ctx, tab, false);
        if (rc)
            return rc;
        tab_dev = ctx->many_tab.p;
    }
    LaunchTimer timer(ctx, false, st); // one bracket around all launches of the pass
    HIP_TRY(timer.begin());
    for (int r0 = 0; r0 < R;) {
        int r1 = r0 + 1;
        while (r1 < R && launch_of[(size_t)r1] == launch_of[(size_t)r0])
            r1++;
        if (r1 - r0 == 1) { // a reference that fills its launch alone: the single-reference kernel
            rc = score_direct(bs[r0], w, false, sign);
            if (rc)
                return rc;
        } else {
            WindowManyParams p{};
            static_cast<WindowShape &>(p) = window_params(bs[r0], w, nullptr, nullptr);
            p.R = r1 - r0;
            p.e = (const double *const *)(tab_dev + r0);
            p.pw = (const double *const *)(tab_dev + R + r0);
            p.mv = (double *const *)(tab_dev + 2 * R + r0);
            p.lag = (int *const *)(tab_dev + 3 * R + r0);
            HIP_TRY(launch_window_many_signed(p, sign, st)); // (no sign, lag 0 inside: launch_window_many)
        }
        for (int r = r0; r < r1; r++) {
            bs[r]->scores_exact = true;
            bs[r]->last_path = MUSE_RUN_PATH_FP64;
            bs[r]->last_screened = false;
            bs[r]->origin = r1 - r0 > 1 ? ScoreOrigin::packed(tiles_of[(size_t)launch_of[(size_t)r0]]) : alone;
            if (r1 - r0 > 1 && (sign != 0 || w.band())) { // (what names the packed signed / band kernel)
                bs[r]->origin.window = w;
                bs[r]->origin.sign = sign;
            }
        }
        r0 = r1;
    }
    HIP_TRY(timer.end());
    return MUSE_OK;
}

extern "C" int muse_batch_run_many_windowed(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                            int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                            int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                            int32_t *out_count, double *out_mean_abs)
{
    const int rc = muse_batch_score_many_windowed(bs, R, max_lag); // (no pre-check of the selection's arguments: run_select's own comes behind the pass)
    if (rc)
        return rc;
    return run_many_select(bs, R, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, false, out_series, out_lag,
                           out_score, out_count, out_mean_abs);
}
