// capi_window.hip -- the lag window of a batch (muse_batch_set_lag_window): the setting, its tables and the windowed all-scores pass
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

extern "C" int muse_batch_set_lag_window(muse_batch *b, int32_t max_lag)
{
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    if (max_lag < 0) { // off: the transform kernels, as if the window had never been set
        b->lag_window = -1;
        return MUSE_OK;
    }
    if (max_lag > MUSE_LAG_WINDOW_MAX)
        return fail(MUSE_ERR_UNSUPPORTED, "lag window %d > MUSE_LAG_WINDOW_MAX (%d): beyond it the direct product costs more than the transform",
                    max_lag, MUSE_LAG_WINDOW_MAX);
    if (b->g->f32)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag-window pass reads float64 groups only");
    if (b->n > GENERIC_MAX_N || !b->xs)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag-window pass is built for series of up to %d samples", GENERIC_MAX_N);
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

// muse_batch_score of a batch with a window (device selected, rows uploaded, M > 0, mv / lag allocated)
int score_windowed(muse_batch *b)
{
    muse_ctx *ctx = b->ctx;
    const hipStream_t st = b->stream();
    const int L = std::min(b->lag_window, b->n / 2);
    if (b->win_L != L) { // the shifted-reference image and its window sums, once per window
        b->win_L = -1;
        const long long e_len = window_e_len(b->N);
        HIP_TRY(b->win_e.ensure(ctx, e_len, st));
        HIP_TRY(b->win_pw.ensure(ctx, 2 * MUSE_LAG_WINDOW_MAX + 1, st));
        HIP_TRY(launch_window_tables(b->xs, b->N, b->n, L, b->win_e.p, e_len, b->win_pw.p, st));
        b->win_L = L;
    }
    WindowParams p{};
    p.rows = b->g->rows;
    p.M = b->g->M;
    p.stride = b->g->stride;
    p.N = b->N;
    p.L = L;
    p.Lneg = 2 * L == b->n ? L - 1 : L; // index n / 2 is lag +n/2 (xcorr.go:192-194): it is scanned once
    p.e = b->win_e.p;
    p.pw = b->win_pw.p;
    p.invN = 1.0 / (double)b->N;
    p.invNm1 = 1.0 / (double)(b->N - 1);
    p.mv = b->mv.p;
    p.lag = b->lag.p;
    LaunchTimer timer(ctx, false, st);
    HIP_TRY(timer.begin());
    HIP_TRY(launch_window(p, st));
    HIP_TRY(timer.end());
    return MUSE_OK;
}
