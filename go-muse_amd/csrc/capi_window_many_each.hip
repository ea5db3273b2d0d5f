// capi_window_many_each.hip -- many references, EACH inside its own lag range or band and under its own sign, in one pass
// (muse_batch_score_many_in_lag_bands / _run_many_in_lag_bands): what muse_batch_score_in_lag_band(batches[r], lag_lo[r], lag_hi[r],
// sign[r]) answers for every r, from one read of the rows where the references are on the direct product.  A list that shares one
// (lag_lo, lag_hi, sign) IS muse_batch_score_many_in_lag_band (capi_window_many_band.hip): the call delegates.  Otherwise the
// references the single dispatch sends to the direct product are cut into launches by window_each_plan (xcorr_window_many_each.hip):
// a launch whose members differ is xcorr_window_many_each_mfma, one whose members share range and sign the uniform packed kernel
// (launch_window_many_signed), a reference alone in its launch the single-reference kernel (score_direct); every other reference
// takes its own single pass (score_in_window) behind them.
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

#include <cstring>

using namespace muse;

static int sign_of(const int32_t *sign, int r) { return sign ? sign[r] : MUSE_SIGN_ANY; }

// the argument checks that need no batch: every reference's band and sign (r: the index a refusal names through the checks' own text)
static int check_bands_args(int32_t R, const int32_t *lag_lo, const int32_t *lag_hi, const int32_t *sign)
{
    if (!lag_lo || !lag_hi)
        return fail(MUSE_ERR_INVALID, "NULL lag_lo / lag_hi: one band per reference");
    for (int r = 0; r < R; r++) {
        const int rc = check_band_args(lag_lo[r], lag_hi[r], sign_of(sign, r));
        if (rc)
            return rc;
    }
    return MUSE_OK;
}

static bool uniform_bands(int32_t R, const int32_t *lag_lo, const int32_t *lag_hi, const int32_t *sign)
{
    for (int r = 1; r < R; r++)
        if (lag_lo[r] != lag_lo[0] || lag_hi[r] != lag_hi[0] || sign_of(sign, r) != sign_of(sign, 0))
            return false;
    return true;
}

// a clipped range or band as the planner and the kernel take it
static int rows_of(int path, bool built, const LagRange &w) { return path == MUSE_IN_WINDOW_MFMA && built ? w.rows() : 0; }

// The planner alone, no device: per reference the path of the single dispatch (signed_window_plan; the masked lengths as they are:
// every reference off the direct product takes its own single pass) and, for those on the direct product, window_each_plan's launches
extern "C" int muse_test_many_lag_bands_plan(int32_t N, int32_t f32, int32_t R, const int32_t *lag_lo, const int32_t *lag_hi,
                                             const int32_t *sign, int32_t *path, int32_t *launch_of, int32_t *launches,
                                             int32_t *tiles_of, int32_t *kc_of, int32_t *img0)
{
    if (N < 2 || R < 1 || !path || !launch_of || !launches || !tiles_of || !kc_of || !img0)
        return fail(MUSE_ERR_INVALID, "bad many-lag-bands plan arguments (N >= 2, R >= 1, outputs to fill)");
    int rc = check_bands_args(R, lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    const int64_t n = muse_next_pow2((double)N);
    std::vector<int> W((size_t)R), paths((size_t)R);
    for (int r = 0; r < R; r++) {
        LagRange w;
        if (!clip_band_or_range(n, lag_lo[r], lag_hi[r], &w))
            return fail_empty_band(lag_lo[r], lag_hi[r], n);
        paths[(size_t)r] = signed_window_plan(N, f32 != 0, w, sign_of(sign, r), false);
        W[(size_t)r] = rows_of(paths[(size_t)r], true, w);
    }
    std::vector<int> of((size_t)R), tiles((size_t)R), kc((size_t)R), at((size_t)R);
    const int k = window_each_plan(R, W.data(), of.data(), tiles.data(), kc.data(), at.data());
    *launches = k;
    for (int r = 0; r < R; r++) {
        path[r] = paths[(size_t)r];
        launch_of[r] = of[(size_t)r];
        img0[r] = at[(size_t)r];
    }
    for (int l = 0; l < k; l++) {
        tiles_of[l] = tiles[(size_t)l];
        kc_of[l] = kc[(size_t)l];
    }
    return MUSE_OK;
}

// as every in-window entry point leaves a batch its pass has scored
static void scored(muse_batch *b, const ScoreOrigin &origin)
{
    b->scores_exact = true;
    b->last_path = MUSE_RUN_PATH_FP64;
    b->last_screened = false;
    b->origin = origin;
}

// The direct product for the members `direct` (indices into bs, list order) of a checked list of one length, each inside its own
// ws[r] under its own sign, in the launches window_each_plan gives.  Each batch's tables are its own, cached as score_direct caches
// them (window_tables): the packed and the single passes serve each other's tables
static int score_each_direct(muse_batch *const *bs, const std::vector<int> &direct, const std::vector<LagRange> &ws, const int32_t *sign)
{
    muse_batch *b0 = bs[0];
    muse_ctx *ctx = b0->ctx;
    int rc = use_device(ctx);
    if (rc)
        return rc;
    rc = group_ready(b0->g);
    if (rc)
        return rc;
    if (b0->g->M == 0)
        return MUSE_OK;
    const hipStream_t st = ctx->stream;
    const int D = (int)direct.size();
    std::vector<int> W((size_t)D);
    for (int k = 0; k < D; k++) {
        muse_batch *b = bs[direct[(size_t)k]];
        rc = ensure_scores(b);
        if (!rc)
            rc = window_tables(b, ws[(size_t)direct[(size_t)k]], b->win_e, b->win_pw, &b->win_key, st);
        if (rc)
            return rc;
        W[(size_t)k] = ws[(size_t)direct[(size_t)k]].rows();
    }
    std::vector<int> launch_of((size_t)D), tiles_of((size_t)D), kc_of((size_t)D), img0((size_t)D);
    const int launches = window_each_plan(D, W.data(), launch_of.data(), tiles_of.data(), kc_of.data(), img0.data());
    std::vector<std::vector<int>> members((size_t)launches); // (positions in `direct`)
    for (int k = 0; k < D; k++)
        members[(size_t)launch_of[(size_t)k]].push_back(k);
    // per packed launch of m members: columns of m pointers -- e, pw, mv, lag -- and behind them its m descriptors
    constexpr size_t DESC_SLOTS = sizeof(WindowEachRef) / sizeof(void *);
    static_assert(sizeof(WindowEachRef) % sizeof(void *) == 0 && alignof(WindowEachRef) <= alignof(void *), "descriptors ride in the pointer table");
    std::vector<size_t> base((size_t)launches, 0);
    std::vector<std::vector<WindowEachRef>> descs((size_t)launches);
    std::vector<void *> tab;
    for (int l = 0; l < launches; l++) {
        const std::vector<int> &mem = members[(size_t)l];
        const size_t m = mem.size();
        if (m < 2)
            continue;
        base[(size_t)l] = tab.size();
        tab.resize(tab.size() + m * (4 + DESC_SLOTS), nullptr);
        int row0 = 0;
        for (size_t j = 0; j < m; j++) {
            const int r = direct[(size_t)mem[j]];
            const LagRange &w = ws[(size_t)r];
            tab[base[(size_t)l] + j] = bs[r]->win_e.p;
            tab[base[(size_t)l] + m + j] = bs[r]->win_pw.p;
            tab[base[(size_t)l] + 2 * m + j] = bs[r]->mv.p;
            tab[base[(size_t)l] + 3 * m + j] = bs[r]->lag.p;
            descs[(size_t)l].push_back(WindowEachRef{w.hi, w.lneg, w.origin, w.rows(), sign_of(sign, r), w.band() ? 1 : 0, row0, img0[(size_t)mem[j]]});
            row0 += w.rows();
        }
        std::memcpy(&tab[base[(size_t)l] + 4 * m], descs[(size_t)l].data(), m * sizeof(WindowEachRef));
    }
    void **tab_dev = nullptr;
    if (!tab.empty()) {
        rc = upload_many_tab(ctx, tab, false);
        if (rc)
            return rc;
        tab_dev = ctx->many_tab.p;
    }
    LaunchTimer timer(ctx, false, st); // one bracket around all launches of the pass
    HIP_TRY(timer.begin());
    for (int l = 0; l < launches; l++) {
        const std::vector<int> &mem = members[(size_t)l];
        const int m = (int)mem.size();
        const int r0 = direct[(size_t)mem[0]];
        const LagRange &w0 = ws[(size_t)r0];
        const int s0 = sign_of(sign, r0);
        if (m == 1) { // a reference that fills its launch alone: the single-reference kernel, named as the single call names it
            rc = score_direct(bs[r0], w0, false, s0);
            if (rc)
                return rc;
            ScoreOrigin alone = ScoreOrigin::in_window(MUSE_IN_WINDOW_MFMA, w0);
            alone.sign = s0;
            scored(bs[r0], alone);
            continue;
        }
        bool uniform = true;
        for (int j = 1; j < m; j++) {
            const int r = direct[(size_t)mem[(size_t)j]];
            const LagRange &w = ws[(size_t)r];
            uniform = uniform && w.hi == w0.hi && w.lneg == w0.lneg && w.origin == w0.origin && sign_of(sign, r) == s0;
        }
        void **t0 = tab_dev + base[(size_t)l];
        ScoreOrigin origin;
        if (uniform) { // one shape for the launch: the uniform packed kernels, the bits and the name of the uniform call
            WindowManyParams p{};
            static_cast<WindowShape &>(p) = window_params(bs[r0], w0, nullptr, nullptr);
            p.R = m;
            p.e = (const double *const *)t0;
            p.pw = (const double *const *)(t0 + m);
            p.mv = (double *const *)(t0 + 2 * m);
            p.lag = (int *const *)(t0 + 3 * m);
            HIP_TRY(launch_window_many_signed(p, s0, st)); // (no sign, lag 0 inside: launch_window_many)
            origin = ScoreOrigin::packed(tiles_of[(size_t)l]);
            if (s0 != 0 || w0.band()) { // (what names the packed signed / band kernel)
                origin.window = w0;
                origin.sign = s0;
            }
        } else {
            WindowEachParams p{};
            p.rows = b0->g->rows;
            p.M = b0->g->M;
            p.stride = b0->g->stride;
            p.N = b0->N;
            p.invN = 1.0 / (double)b0->N;
            p.invNm1 = 1.0 / (double)(b0->N - 1);
            p.R = m;
            p.e = (const double *const *)t0;
            p.pw = (const double *const *)(t0 + m);
            p.mv = (double *const *)(t0 + 2 * m);
            p.lag = (int *const *)(t0 + 3 * m);
            p.ref = (const WindowEachRef *)(t0 + 4 * m);
            HIP_TRY(launch_window_many_each(p, descs[(size_t)l].data(), st));
            origin = ScoreOrigin::packed_each(tiles_of[(size_t)l]);
        }
        for (int j = 0; j < m; j++)
            scored(bs[direct[(size_t)mem[(size_t)j]]], origin);
    }
    HIP_TRY(timer.end());
    return MUSE_OK;
}

extern "C" int muse_batch_score_many_in_lag_bands(muse_batch *const *bs, int32_t R, const int32_t *lag_lo, const int32_t *lag_hi,
                                                  const int32_t *sign)
{
    // everything is checked before anything is enqueued: on a refusal every batch is unchanged
    int rc = check_batch_list(bs, R);
    if (!rc)
        rc = check_bands_args(R, lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    if (uniform_bands(R, lag_lo, lag_hi, sign)) // one question for the whole list: the uniform call, bit for bit and kernel for kernel
        return muse_batch_score_many_in_lag_band(bs, R, lag_lo[0], lag_hi[0], sign_of(sign, 0));
    std::vector<LagRange> ws((size_t)R);
    for (int r = 0; r < R; r++)
        if (!clip_band_or_range(bs[r]->n, lag_lo[r], lag_hi[r], &ws[(size_t)r]))
            return fail_empty_band(lag_lo[r], lag_hi[r], bs[r]->n);
    for (int r = 0; r < R && !rc; r++)
        rc = check_own_window(bs[r], lag_lo[r], lag_hi[r], r);
    if (rc)
        return rc;
    // the references on the direct product (lists of mixed length: none, reference by reference); the single dispatch's own refusal
    // for every other one
    const bool pack = one_length(bs, R);
    std::vector<int> direct, each;
    for (int r = 0; r < R; r++) {
        muse_batch *b = bs[r];
        const int path = signed_window_plan(b->N, b->g->f32, ws[(size_t)r], sign_of(sign, r), b->ctx->in_window_force.load());
        if (pack && rows_of(path, b->xs != nullptr, ws[(size_t)r]) > 0) {
            direct.push_back(r);
            continue;
        }
        ScorePass pass;
        rc = plan_in_window(b, ws[(size_t)r], &pass, sign_of(sign, r));
        if (rc)
            return rc;
        each.push_back(r);
    }
    if (!direct.empty())
        rc = score_each_direct(bs, direct, ws, sign);
    for (size_t k = 0; k < each.size() && !rc; k++)
        rc = score_in_window(bs[each[k]], ws[(size_t)each[k]], sign_of(sign, each[k]));
    return rc;
}

extern "C" int muse_batch_run_many_in_lag_bands(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G,
                                                const int32_t *lag_lo, const int32_t *lag_hi, const int32_t *top_n,
                                                const double *threshold, const int32_t *sign_filter, int32_t abs_scores,
                                                int32_t out_stride, int64_t *out_series, int32_t *out_lag, double *out_score,
                                                int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, per reference, as in muse_batch_run_in_lag_band: they refuse a sign_filter
    // outside -1 .. 1; then the rows of the outputs)
    if (R < 1 || !top_n || !threshold)
        return fail(MUSE_ERR_INVALID, "bad batch list, or NULL top_n / threshold: one of each per reference");
    int rc = MUSE_OK;
    for (int r = 0; r < R && !rc; r++) {
        rc = check_select_args(group_id, G, sign_of(sign_filter, r));
        if (!rc && top_n[r] > out_stride)
            rc = fail(MUSE_ERR_INVALID, "out_stride %d is smaller than top_n[%d] = %d", out_stride, r, top_n[r]);
    }
    if (!rc)
        rc = muse_batch_score_many_in_lag_bands(bs, R, lag_lo, lag_hi, sign_filter);
    const size_t stride = (size_t)std::max(out_stride, 0);
    for (int r = 0; r < R && !rc; r++) {
        const int32_t max_lag = (int32_t)std::min<int64_t>(std::max<int64_t>(std::llabs((long long)lag_lo[r]), std::llabs((long long)lag_hi[r])), INT32_MAX);
        rc = run_scored(bs[r], group_id, G, max_lag, top_n[r], threshold[r], sign_of(sign_filter, r), abs_scores,
                        out_series ? out_series + stride * r : nullptr, out_lag ? out_lag + stride * r : nullptr,
                        out_score ? out_score + stride * r : nullptr, out_count ? out_count + r : nullptr,
                        out_mean_abs ? out_mean_abs + r : nullptr);
    }
    return rc;
}
