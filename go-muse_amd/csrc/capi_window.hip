// capi_window.hip -- the lag window of a batch (muse_batch_set_lag_window): the setting, its tables, the windowed all-scores pass,
// that pass fused with the slide of the group's rows (muse_batch_slide_score_windowed / _slide_run_windowed), and the window of any
// width as an argument (muse_batch_score_in_window / _run_in_window: the direct product or the masked transform kernels), one-sided
// and asymmetric too (muse_batch_score_in_lag_range / _run_in_lag_range), and lag bands that need not hold lag 0
// (muse_batch_score_in_lag_band / _run_in_lag_band)
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

int check_window_request(const muse_batch *b, int32_t max_lag, bool f32)
{
    if (max_lag > MUSE_LAG_WINDOW_MAX)
        return fail(MUSE_ERR_UNSUPPORTED, "lag window %d > MUSE_LAG_WINDOW_MAX (%d): beyond it the direct product costs more than the transform",
                    max_lag, MUSE_LAG_WINDOW_MAX);
    if (f32)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag-window pass reads float64 groups only");
    if (b->n > GENERIC_MAX_N || !b->xs)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag-window pass is built for series of up to %d samples", GENERIC_MAX_N);
    return MUSE_OK;
}

int check_own_window(const muse_batch *b, int32_t lag_lo, int32_t lag_hi, int r)
{
    if (!b->windowed() || ((int64_t)lag_lo == -(int64_t)lag_hi && b->lag_window == lag_hi))
        return MUSE_OK;
    char who[32] = "the batch";
    if (r >= 0)
        snprintf(who, sizeof(who), "batch %d", r);
    return fail(MUSE_ERR_INVALID, "%s has a lag window of %d of its own: it must be off or equal to the call's (lags %d .. %d)", who,
                b->lag_window, lag_lo, lag_hi);
}

extern "C" int muse_batch_set_lag_window(muse_batch *b, int32_t max_lag)
{
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    if (max_lag < 0) { // off: the transform kernels, as if the window had never been set
        b->lag_window = -1;
        return MUSE_OK;
    }
    const int rc = check_window_request(b, max_lag, b->g->f32);
    if (rc)
        return rc;
    b->lag_window = max_lag;
    return MUSE_OK;
}

extern "C" int muse_batch_lag_window(muse_batch *b, int32_t *max_lag)
{
    if (!b || !max_lag)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    *max_lag = b->windowed() ? b->lag_window : -1;
    return MUSE_OK;
}

int window_tables(muse_batch *b, const LagRange &w, PoolBuf<double> &e, PoolBuf<double> &pw, int32_t *key, hipStream_t st)
{
    // (a band's origin is -lo, anywhere in -32768 .. 32767: its keys have a bit of their own, 29, as the panel tables' have bit 30)
    const int32_t k = w.band() ? (1 << 29) | ((w.origin + 32768) * 256 + w.rows()) : w.origin * 256 + w.rows();
    if (*key == k)
        return MUSE_OK;
    *key = -1;
    const long long e_len = window_e_len(b->N);
    HIP_TRY(e.ensure(b->ctx, e_len, st));
    HIP_TRY(pw.ensure(b->ctx, 2 * MUSE_LAG_WINDOW_MAX + 1, st));
    if (w.band())
        HIP_TRY(launch_window_tables_band(b->xs, b->N, b->n, w.lo(), w.rows(), e.p, e_len, pw.p, st));
    else
        HIP_TRY(launch_window_tables(b->xs, b->N, b->n, w.origin, w.rows(), e.p, e_len, pw.p, st));
    *key = k;
    return MUSE_OK;
}

WindowParams window_params(const muse_batch *b, const LagRange &w, const double *e, const double *pw)
{
    WindowParams p{};
    p.rows = b->g->rows;
    p.M = b->g->M;
    p.stride = b->g->stride;
    p.N = b->N;
    p.L = w.hi;
    p.Lneg = w.lneg;
    p.invN = 1.0 / (double)b->N;
    p.invNm1 = 1.0 / (double)(b->N - 1);
    p.origin = w.origin;
    p.e = e;
    p.pw = pw;
    p.mv = b->mv.p;
    p.lag = b->lag.p;
    return p;
}

// the one direct-product pass: a batch's own window (muse_batch_score) and a call's (the MFMA path of every in-window entry point)
int score_direct(muse_batch *b, const LagRange &w, bool bracket, int sign)
{
    const hipStream_t st = b->stream();
    const int rc = window_tables(b, w, b->win_e, b->win_pw, &b->win_key, st);
    if (rc)
        return rc;
    LaunchTimer timer(b->ctx, false, st);
    if (bracket)
        HIP_TRY(timer.begin());
    if (w.band())
        HIP_TRY(launch_window_band(window_params(b, w, b->win_e.p, b->win_pw.p), sign, st));
    else
        HIP_TRY(launch_window_signed(window_params(b, w, b->win_e.p, b->win_pw.p), sign, st)); // (sign 0: launch_window)
    HIP_TRY(timer.end());
    return MUSE_OK;
}

// the slide arguments of the calls that move the whole group of a batch and score it (muse_group_slide's refusals)
static int check_slide_args(const muse_batch *b, const double *tails, int32_t k, int64_t tail_stride)
{
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    const muse_group *g = b->g;
    if (k < 0 || k > g->N)
        return fail(MUSE_ERR_INVALID, "slide by %d samples: outside 0 .. N = %d", k, g->N);
    if (tail_stride < k)
        return fail(MUSE_ERR_INVALID, "tail_stride %lld is smaller than k = %d", (long long)tail_stride, k);
    if (!tails && g->M > 0 && k > 0)
        return fail(MUSE_ERR_INVALID, "tails is NULL");
    if (g->win_rows)
        return fail(MUSE_ERR_INVALID, "the group has an open staging window");
    return MUSE_OK;
}

// ---- the slide and the windowed pass in one kernel (xcorr_window_slide.hip)
extern "C" int muse_batch_slide_score_windowed(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride, int32_t max_lag)
{
    // everything is checked before anything is enqueued: on an error the batch and the group are unchanged
    int rc = check_slide_args(b, tails, k, tail_stride);
    if (rc)
        return rc;
    muse_group *g = b->g;
    const int64_t M = g->M;
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed pass needs a lag window >= 0");
    rc = check_window_request(b, max_lag, g->f32);
    if (!rc)
        rc = check_own_window(b, -max_lag, max_lag);
    if (rc)
        return rc;
    if (M == 0) // nothing to move, nothing to score
        return MUSE_OK;
    muse_ctx *ctx = b->ctx;
    rc = use_device(ctx);
    if (rc)
        return rc;
    const hipStream_t st = b->stream();
    rc = group_ready(g, st); // rows packed but not sent yet go first
    if (rc)
        return rc;
    rc = ensure_scores(b);
    if (rc)
        return rc;
    b->origin = ScoreOrigin{};
    b->scores_exact = true;
    const LagRange w = lag_window_range(b->n, max_lag);
    if (k == 0) // nothing moves and nothing is invalidated: the windowed pass alone
        return score_direct(b, w);
    rc = window_tables(b, w, b->win_e, b->win_pw, &b->win_key, st);
    if (rc)
        return rc;
    rc = slide_upload_tails(g, M, tails, k, tail_stride);
    if (rc)
        return rc;
    // as muse_group_slide: the kernel rewrites rows that work enqueued earlier on any stream of the device may still be reading
    // (the tails and the tables have landed with it), and the call returns once the kernel has finished
    HIP_TRY(hipDeviceSynchronize());
    slide_invalidate(g, 0);
    LaunchTimer timer(ctx, false, st);
    HIP_TRY(timer.begin());
    HIP_TRY(launch_window_slide(window_params(b, w, b->win_e.p, b->win_pw.p), (const double *)g->slide_dev.p, k, st));
    HIP_TRY(timer.end());
    HIP_TRY(hipStreamSynchronize(st));
    return MUSE_OK;
}

extern "C" int muse_batch_slide_run_windowed(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                                             const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                                             int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                                             double *out_score, int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first: a refusal leaves the rows where they were)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_slide_score_windowed(b, tails, k, tail_stride, max_lag);
    return rc ? rc : run_scored(b, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// ---- the window as an argument: any width (muse_batch_score_in_window), one-sided and asymmetric too (muse_batch_score_in_lag_range)
// The dispatch of all of them, a pure host function: which pass scores series of N samples (float32 storage or not) inside w.
//   w is every lag                                        : the plain pass of batch_score, any length, any storage
//   float64, at most 2 MUSE_LAG_WINDOW_MAX + 1 table rows, n <= 65536 : the direct product (score_direct), its table starting at w.origin
//                                                           (unless `force_transform` and the length has masked kernels)
//   n in {512, 1024, 2048, 4096}, wider or float32        : the transform kernels with a masked argmax (the WIN builds), the two bounds
//                                                           set independently
//   anything else                                         : not built
int window_plan(int32_t N, bool f32, const LagRange &w, bool force_transform)
{
    const int64_t n = muse_next_pow2((double)N);
    if (w.every_lag(n))
        return MUSE_IN_WINDOW_PLAIN;
    const bool masked_len = n == 512 || n == 1024 || n == 2048 || n == 4096;
    if (!f32 && w.rows() <= 2 * MUSE_LAG_WINDOW_MAX + 1 && n <= GENERIC_MAX_N && !(force_transform && masked_len))
        return MUSE_IN_WINDOW_MFMA;
    return masked_len ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_UNSUPPORTED;
}

// The dispatch of the signed best match (muse_batch_score_signed_in_lag_range), a pure host function; sign == 0: window_plan.
//   window_plan says MFMA                                  : the direct product with the signed scan (xcorr_window_signed_mfma)
//   window_plan says MASKED                                : the transform kernels' WIN builds with the signed mask, both storages
//   window_plan says PLAIN, n in {512, 1024, 2048, 4096}   : the same masked kernels with both bounds at their widest (off the rows)
//   anything else                                          : not built
int signed_window_plan(int32_t N, bool f32, const LagRange &w, int sign, bool force_transform)
{
    const int path = window_plan(N, f32, w, force_transform);
    if (sign == 0 || path != MUSE_IN_WINDOW_PLAIN)
        return path;
    const int64_t n = muse_next_pow2((double)N);
    return n == 512 || n == 1024 || n == 2048 || n == 4096 ? MUSE_IN_WINDOW_MASKED : MUSE_IN_WINDOW_UNSUPPORTED;
}

extern "C" int muse_test_signed_lag_range_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t *path)
{
    if (!path || N < 2 || lag_lo > 0 || lag_hi < 0 || sign < -1 || sign > 1)
        return fail(MUSE_ERR_INVALID, "bad signed lag-range plan arguments (N >= 2, lag_lo <= 0 <= lag_hi, sign -1 .. 1)");
    *path = signed_window_plan(N, f32 != 0, clip_lag_range(muse_next_pow2((double)N), lag_lo, lag_hi), sign, false);
    return MUSE_OK;
}

extern "C" int muse_test_in_window_plan(int32_t N, int32_t f32, int32_t max_lag, int32_t *path)
{
    if (!path || N < 2 || max_lag < 0)
        return fail(MUSE_ERR_INVALID, "bad in-window plan arguments (N >= 2, max_lag >= 0)");
    *path = window_plan(N, f32 != 0, lag_window_range(muse_next_pow2((double)N), max_lag), false);
    return MUSE_OK;
}

extern "C" int muse_test_lag_range_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t *path)
{
    if (!path || N < 2 || lag_lo > 0 || lag_hi < 0)
        return fail(MUSE_ERR_INVALID, "bad lag-range plan arguments (N >= 2, lag_lo <= 0 <= lag_hi)");
    *path = window_plan(N, f32 != 0, clip_lag_range(muse_next_pow2((double)N), lag_lo, lag_hi), false);
    return MUSE_OK;
}

extern "C" int muse_test_in_window_force_transform(muse_ctx *ctx, int32_t on)
{
    if (!ctx)
        return fail(MUSE_ERR_INVALID, "NULL context");
    ctx->in_window_force.store(on != 0);
    return MUSE_OK;
}

extern "C" int muse_test_last_in_window_path(muse_batch *b, int32_t *path)
{
    if (!b || !path)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    *path = b->origin.in_window_path();
    return MUSE_OK;
}

static int fail_not_built(const muse_batch *b, const LagRange &w)
{
    return fail(MUSE_ERR_UNSUPPORTED, "the lags %d .. %d over series of %d samples%s are not built: more than %d table rows and float32 "
                "storage take the masked argmax of the transform kernels of FFT lengths 512 ... 4096",
                w.lo(), w.hi, b->N, b->g->f32 ? " in float32 storage" : "", 2 * MUSE_LAG_WINDOW_MAX + 1);
}

int plan_in_window(muse_batch *b, const LagRange &w, ScorePass *pass, int sign)
{
    const int path = signed_window_plan(b->N, b->g->f32, w, sign, b->ctx->in_window_force.load());
    if (path == MUSE_IN_WINDOW_UNSUPPORTED || (path == MUSE_IN_WINDOW_MFMA && !b->xs))
        return sign && w.every_lag(b->n) ? fail(MUSE_ERR_UNSUPPORTED, "the signed best match at every lag over series of %d samples is not built: "
                                                "it takes the masked argmax of the transform kernels of FFT lengths 512 ... 4096", b->N)
                                         : fail_not_built(b, w);
    *pass = ScorePass{path == MUSE_IN_WINDOW_PLAIN, &w, path}; // (a masked pass always reads the rows)
    pass->sign = sign;
    if (path == MUSE_IN_WINDOW_MFMA)
        return MUSE_OK;
    int variant = -1; // (what batch_score would refuse -- a forced kernel without a masked build -- before it touches the batch)
    return batch_score_check(b, pass->mask(), &variant);
}

// as every in-window entry point leaves a batch it has scored
static void scored_in_window(muse_batch *b, int path, const LagRange &w, int sign = 0)
{
    b->scores_exact = true;
    b->last_path = MUSE_RUN_PATH_FP64;
    b->last_screened = false;
    if (path != MUSE_IN_WINDOW_MASKED) // (batch_score records the masked origin: it knows the kernel it launches first)
        b->origin = ScoreOrigin::in_window(path, w);
    b->origin.sign = sign;
}

int score_in_window(muse_batch *b, const LagRange &w, int sign)
{
    ScorePass pass;
    int rc = plan_in_window(b, w, &pass, sign);
    if (!rc)
        rc = batch_score(b, pass);
    if (!rc && b->g->M > 0)
        scored_in_window(b, pass.path, w, sign);
    return rc;
}

extern "C" int muse_batch_score_in_window(muse_batch *b, int32_t max_lag)
{
    // everything is checked before anything is enqueued: on a refusal the batch is unchanged
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed pass needs a lag window >= 0");
    const int rc = check_own_window(b, -max_lag, max_lag);
    return rc ? rc : score_in_window(b, lag_window_range(b->n, max_lag));
}

extern "C" int muse_batch_run_in_window(muse_batch *b, const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n,
                                        double threshold, int32_t sign_filter, int32_t abs_scores, int64_t *out_series,
                                        int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_slide_run_windowed)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_in_window(b, max_lag);
    return rc ? rc : run_scored(b, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

extern "C" int muse_batch_score_in_lag_range(muse_batch *b, int32_t lag_lo, int32_t lag_hi)
{
    // everything is checked before anything is enqueued: on a refusal the batch is unchanged
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    if (lag_lo > 0 || lag_hi < 0)
        return fail(MUSE_ERR_INVALID, "the lag range %d .. %d does not hold lag 0 (lag_lo <= 0 <= lag_hi)", lag_lo, lag_hi);
    const int rc = check_own_window(b, lag_lo, lag_hi);
    return rc ? rc : score_in_window(b, clip_lag_range(b->n, lag_lo, lag_hi));
}

extern "C" int muse_batch_run_in_lag_range(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                                           int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                                           int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count,
                                           double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_window)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_in_lag_range(b, lag_lo, lag_hi);
    return rc ? rc : run_scored(b, group_id, G, range_max_lag(lag_lo, lag_hi), top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// ---- the signed best match inside a lag range: the argmax restricted to the values of one sign, not its answer filtered
extern "C" int muse_batch_score_signed_in_lag_range(muse_batch *b, int32_t lag_lo, int32_t lag_hi, int32_t sign)
{
    // everything is checked before anything is enqueued: on a refusal the batch is unchanged
    if (sign == MUSE_SIGN_ANY)
        return muse_batch_score_in_lag_range(b, lag_lo, lag_hi);
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    if (sign != MUSE_SIGN_POS && sign != MUSE_SIGN_NEG)
        return fail(MUSE_ERR_INVALID, "sign %d: one of MUSE_SIGN_ANY (0), MUSE_SIGN_POS (1), MUSE_SIGN_NEG (-1)", sign);
    if (lag_lo > 0 || lag_hi < 0)
        return fail(MUSE_ERR_INVALID, "the lag range %d .. %d does not hold lag 0 (lag_lo <= 0 <= lag_hi)", lag_lo, lag_hi);
    const int rc = check_own_window(b, lag_lo, lag_hi);
    return rc ? rc : score_in_window(b, clip_lag_range(b->n, lag_lo, lag_hi), sign);
}

extern "C" int muse_batch_run_signed_in_lag_range(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                                                  int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                                                  int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count,
                                                  double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_in_lag_range: they refuse a sign_filter outside -1 .. 1)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_signed_in_lag_range(b, lag_lo, lag_hi, sign_filter);
    return rc ? rc : run_scored(b, group_id, G, range_max_lag(lag_lo, lag_hi), top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// ---- lag bands: the best match inside lags lag_lo .. lag_hi that need not hold lag 0 (muse_batch_score_in_lag_band).  A band that
// holds lag 0 IS the signed range call; one that does not is a LagRange with lag 0 outside (capi_internal.h: band()), which
// window_plan / signed_window_plan dispatch by its rows as they are -- never every lag -- and score_direct / batch_score send to the
// band builds of the kernels (xcorr_window_band_mfma; the BAND builds of the masked transform kernels)
int check_band_args(int32_t lag_lo, int32_t lag_hi, int32_t sign)
{
    if (sign != MUSE_SIGN_ANY && sign != MUSE_SIGN_POS && sign != MUSE_SIGN_NEG)
        return fail(MUSE_ERR_INVALID, "sign %d: one of MUSE_SIGN_ANY (0), MUSE_SIGN_POS (1), MUSE_SIGN_NEG (-1)", sign);
    if (lag_lo > lag_hi)
        return fail(MUSE_ERR_INVALID, "the lag band %d .. %d is empty (lag_lo <= lag_hi)", lag_lo, lag_hi);
    return MUSE_OK;
}

int fail_empty_band(int32_t lag_lo, int32_t lag_hi, int64_t n)
{
    return fail(MUSE_ERR_INVALID, "nothing of the lag band %d .. %d is left inside the lags %lld .. %lld of FFT length %lld", lag_lo, lag_hi,
                -(long long)(n / 2 - 1), (long long)(n / 2), (long long)n);
}

extern "C" int muse_test_lag_band_plan(int32_t N, int32_t f32, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t *path)
{
    if (!path || N < 2)
        return fail(MUSE_ERR_INVALID, "bad lag-band plan arguments (N >= 2, a path to fill)");
    const int rc = check_band_args(lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    if (lag_lo <= 0 && lag_hi >= 0)
        return muse_test_signed_lag_range_plan(N, f32, lag_lo, lag_hi, sign, path);
    const int64_t n = muse_next_pow2((double)N);
    LagRange w;
    if (!clip_lag_band(n, lag_lo, lag_hi, &w))
        return fail_empty_band(lag_lo, lag_hi, n);
    *path = signed_window_plan(N, f32 != 0, w, sign, false);
    return MUSE_OK;
}

extern "C" int muse_batch_score_in_lag_band(muse_batch *b, int32_t lag_lo, int32_t lag_hi, int32_t sign)
{
    // everything is checked before anything is enqueued: on a refusal the batch is unchanged
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    int rc = check_band_args(lag_lo, lag_hi, sign);
    if (rc)
        return rc;
    if (lag_lo <= 0 && lag_hi >= 0) // (clipping moves neither bound across lag 0)
        return muse_batch_score_signed_in_lag_range(b, lag_lo, lag_hi, sign);
    LagRange w;
    if (!clip_lag_band(b->n, lag_lo, lag_hi, &w))
        return fail_empty_band(lag_lo, lag_hi, b->n);
    rc = check_own_window(b, lag_lo, lag_hi); // (no band is a symmetric window: any window of the batch's own refuses it)
    return rc ? rc : score_in_window(b, w, sign);
}

extern "C" int muse_batch_run_in_lag_band(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                                          int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores, int64_t *out_series,
                                          int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first, as in muse_batch_run_signed_in_lag_range: they refuse a sign_filter outside -1 .. 1)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_score_in_lag_band(b, lag_lo, lag_hi, sign_filter);
    const int32_t max_lag = (int32_t)std::min<int64_t>(std::max<int64_t>(std::llabs((long long)lag_lo), std::llabs((long long)lag_hi)), INT32_MAX);
    return rc ? rc : run_scored(b, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// ---- the slide and the pass of any window in one call (muse_batch_slide_score_in_window)
// The dispatch, a pure host function: how series at FFT length n are slid and scored inside a window that window_plan sends to `pass`.
//   window_plan says UNSUPPORTED                       : not built
//   window_plan says MFMA                              : muse_batch_slide_score_windowed (xcorr_window_slide.hip)
//   PLAIN or MASKED at FFT length 4096                 : the SLIDE builds of xcorr_fused_n4096_fold (one read and one write of the rows)
//   anything else                                      : launch_row_slide and then the pass
// Measured (tools/slide_in_window_bench.py, profiles/slide_in_window_bench.txt): the fused kernel against the two kernels
// it replaces, per listed shape; no slide distance is routed away from it.
static int slide_in_window_plan(int pass, int64_t n)
{
    if (pass == MUSE_IN_WINDOW_UNSUPPORTED)
        return MUSE_SLIDE_IN_WINDOW_UNSUPPORTED;
    if (pass == MUSE_IN_WINDOW_MFMA)
        return MUSE_SLIDE_IN_WINDOW_MFMA;
    return n == 4096 ? MUSE_SLIDE_IN_WINDOW_FUSED : MUSE_SLIDE_IN_WINDOW_TWO_STEP;
}

extern "C" int muse_test_slide_in_window_plan(int32_t N, int32_t f32, int32_t max_lag, int32_t k, int32_t *path)
{
    if (!path || N < 2 || max_lag < 0 || k < 0 || k > N)
        return fail(MUSE_ERR_INVALID, "bad slide-in-window plan arguments (N >= 2, max_lag >= 0, 0 <= k <= N)");
    const int64_t n = muse_next_pow2((double)N);
    *path = slide_in_window_plan(window_plan(N, f32 != 0, lag_window_range(n, max_lag), false), n);
    return MUSE_OK;
}

extern "C" int muse_test_slide_in_window_force(muse_ctx *ctx, int32_t mode)
{
    if (!ctx || mode < 0 || mode > 1)
        return fail(MUSE_ERR_INVALID, "the slide-in-window hook takes a context and mode 0 (the table) or 1 (two steps)");
    ctx->slide_in_window_force.store(mode);
    return MUSE_OK;
}

extern "C" int muse_test_last_slide_path(muse_batch *b, int32_t *path)
{
    if (!b || !path)
        return fail(MUSE_ERR_INVALID, "NULL argument");
    *path = b->origin.slide;
    return MUSE_OK;
}

extern "C" int muse_batch_slide_score_in_window(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride, int32_t max_lag)
{
    // everything is checked before anything is enqueued: on a refusal the rows, the batch and the group are unchanged
    int rc = check_slide_args(b, tails, k, tail_stride);
    if (rc)
        return rc;
    muse_group *g = b->g;
    muse_ctx *ctx = b->ctx;
    const int64_t M = g->M;
    if (max_lag < 0)
        return fail(MUSE_ERR_INVALID, "a windowed pass needs a lag window >= 0");
    rc = check_own_window(b, -max_lag, max_lag);
    if (rc)
        return rc;
    const LagRange w = lag_window_range(b->n, max_lag);
    ScorePass pass{false, &w, window_plan(b->N, g->f32, w, ctx->in_window_force.load())}; // (the rows move: the spectrum cache stays out)
    int path = slide_in_window_plan(pass.path, b->n);
    if (path == MUSE_SLIDE_IN_WINDOW_UNSUPPORTED || (path == MUSE_SLIDE_IN_WINDOW_MFMA && !b->xs))
        return fail_not_built(b, w);
    if (M == 0) // nothing to move, nothing to score
        return MUSE_OK;
    if (k == 0) // nothing moves and nothing is invalidated: the pass alone
        return muse_batch_score_in_window(b, max_lag);
    if (path == MUSE_SLIDE_IN_WINDOW_MFMA) { // the direct product has a slide kernel of its own; the origin is muse_batch_score_in_window's
        rc = muse_batch_slide_score_windowed(b, tails, k, tail_stride, max_lag);
        if (rc)
            return rc;
        scored_in_window(b, pass.path, w);
        b->origin.slide = path;
        return MUSE_OK;
    }
    // the pass as muse_batch_score_in_window launches it, the plain one or the masked one: the call's, whatever the batch's own setting
    int variant = -1;
    rc = batch_score_check(b, pass.mask(), &variant);
    if (rc)
        return rc;
    // FUSED is the default n = 4096 kernel's build: a forced variant, a missing correction table or a hand-off learned from the rows
    // as they are sends the call the long way round (and so do rows the kernel cannot move in its 16-byte units: never a group's)
    if (path == MUSE_SLIDE_IN_WINDOW_FUSED &&
        (ctx->slide_in_window_force.load() == 1 || variant != KERNEL_R16_FOLD || g->stride != g->N ||
         (b->N == 4096 && !g->f32 && !window_wide(g->rows, g->stride))))
        path = MUSE_SLIDE_IN_WINDOW_TWO_STEP;
    rc = use_device(ctx);
    if (rc)
        return rc;
    const hipStream_t st = b->stream();
    rc = group_ready(g, st); // rows packed but not sent yet go first
    if (rc)
        return rc;
    rc = ensure_scores(b);
    if (rc)
        return rc;
    rc = slide_upload_tails(g, M, tails, k, tail_stride);
    if (rc)
        return rc;
    // as muse_group_slide: the kernels rewrite rows that work enqueued earlier on any stream of the device may still be reading (the
    // tails have landed with it), and the call returns once they have finished
    HIP_TRY(hipDeviceSynchronize());
    slide_invalidate(g, 0);
    const SlideFuse fuse{g->slide_dev.p, k};
    if (path == MUSE_SLIDE_IN_WINDOW_FUSED) {
        pass.slide = &fuse;
    } else {
        LaunchTimer timer(ctx, false, st);
        hipError_t e = timer.begin();
        if (e == hipSuccess)
            e = launch_row_slide(g->base(), g->f32, M, g->N, k, g->slide_dev.p, ctx->num_cus, st);
        if (e == hipSuccess)
            e = timer.end();
        if (e != hipSuccess)
            return fail(MUSE_ERR_HIP, "the row slide failed: %s", hipGetErrorString(e));
    }
    rc = batch_score(b, pass);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    scored_in_window(b, pass.path, w);
    b->origin.slide = path;
    return MUSE_OK;
}

extern "C" int muse_batch_slide_run_in_window(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                                              const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                                              int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                                              double *out_score, int32_t *out_count, double *out_mean_abs)
{
    // (the selection's own argument checks come first: a refusal leaves the rows where they were)
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc)
        rc = muse_batch_slide_score_in_window(b, tails, k, tail_stride, max_lag);
    return rc ? rc : run_scored(b, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// the reference's Run on the slid rows: the global argmax of every series, then the filter on Results.MaxLag
extern "C" int muse_batch_slide_run(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                                    const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                                    int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                                    double *out_score, int32_t *out_count, double *out_mean_abs)
{
    int rc = check_select_args(group_id, G, sign_filter);
    if (!rc && b && b->windowed())
        rc = fail(MUSE_ERR_INVALID, "the batch has a lag window of %d of its own: muse_batch_slide_run scores every lag", b->lag_window);
    if (!rc)
        rc = muse_batch_slide_score_in_window(b, tails, k, tail_stride, b ? b->n / 2 : 0);
    return rc ? rc : run_scored(b, group_id, G, max_lag, top_n, threshold, sign_filter, abs_scores, out_series, out_lag, out_score, out_count, out_mean_abs);
}

// test hook: the planner alone (xcorr_window_slide.hip), no device
extern "C" int muse_test_slide_score_plan(int32_t N, int32_t k, int32_t wide, int32_t *load_bytes, int32_t *store_bytes)
{
    if (!load_bytes || !store_bytes || N < 2 || k < 0 || k > N || (wide != 0 && N % 2 != 0))
        return fail(MUSE_ERR_INVALID, "bad slide-score plan arguments (N >= 2, 0 <= k <= N, wide rows have an even N)");
    int lb = 0, sb = 0;
    slide_score_plan(N, k, wide != 0, &lb, &sb);
    *load_bytes = lb;
    *store_bytes = sb;
    return MUSE_OK;
}
