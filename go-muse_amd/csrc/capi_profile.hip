// capi_profile.hip -- lag profiles (muse_batch_lag_profile / _lag_profile_device): the cc of the lags lag_lo .. lag_hi of a resident
// group's series against a batch's reference, written out by the direct product (xcorr_window_profile.hip) -- the argument checks,
// the planner's launches with their tables, the device form and the host form with its chunked staging.
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
#include "capi_internal.h"

using namespace muse;

// The argument checks of both entry points and of muse_test_lag_profile_plan, a pure host function: series of N samples (f32: float32
// storage; has_ref: the batch holds its time-domain reference) in a group of M rows, K listed series (series == nullptr: the whole
// group), the lags and the output's row stride.  Nothing is touched.
static int check_profile_args(int32_t N, bool f32, bool has_ref, int64_t M, const int64_t *series, int64_t K, int32_t lag_lo,
                              int32_t lag_hi, int64_t out_stride)
{
    if (N < 2)
        return fail(MUSE_ERR_INVALID, "a lag profile needs series of at least 2 samples");
    if (lag_lo > lag_hi)
        return fail(MUSE_ERR_INVALID, "the lags %d .. %d are empty (lag_lo <= lag_hi)", lag_lo, lag_hi);
    const int64_t n = muse_next_pow2((double)N);
    if (n > GENERIC_MAX_N)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag profile is built for series of up to %d samples", GENERIC_MAX_N);
    if (lag_lo < -(n / 2 - 1) || lag_hi > n / 2)
        return fail(MUSE_ERR_INVALID, "the lags %d .. %d leave the lags %lld .. %lld of FFT length %lld (a profile is not clipped: its columns are its lags)",
                    lag_lo, lag_hi, -(long long)(n / 2 - 1), (long long)(n / 2), (long long)n);
    if (f32)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag profile reads float64 groups only");
    if (!has_ref)
        return fail(MUSE_ERR_UNSUPPORTED, "the lag profile needs the batch's time-domain reference");
    const int64_t W = (int64_t)lag_hi - lag_lo + 1;
    if (out_stride < W)
        return fail(MUSE_ERR_INVALID, "out_stride %lld is smaller than the %lld lags of a row", (long long)out_stride, (long long)W);
    if (K < 0 || (!series && K != 0 && K != M))
        return fail(MUSE_ERR_INVALID, "K = %lld: without a list it is 0 or the group's %lld series", (long long)K, (long long)M);
    for (int64_t i = 0; series && i < K; i++)
        if (series[i] < 0 || series[i] >= M)
            return fail(MUSE_ERR_INVALID, "series %lld of the list is %lld: outside the group's series [0, %lld)", (long long)i,
                        (long long)series[i], (long long)M);
    return MUSE_OK;
}

extern "C" int muse_test_lag_profile_plan(int32_t N, int32_t lag_lo, int32_t lag_hi, int32_t *launches, int32_t *lo_of, int32_t *rows_of,
                                          int32_t cap)
{
    if (!launches || cap < 0 || (cap > 0 && (!lo_of || !rows_of)))
        return fail(MUSE_ERR_INVALID, "bad lag-profile plan arguments (a count to fill, cap >= 0 entries in both arrays)");
    const int rc = check_profile_args(N, false, true, 0, nullptr, 0, lag_lo, lag_hi, (int64_t)lag_hi - lag_lo + 1);
    if (rc)
        return rc;
    *launches = window_profile_plan(lag_lo, lag_hi, lo_of, rows_of, cap);
    return MUSE_OK;
}

// the list entries [first, first + count) into b->prof_idx through the pinned image, on st (the image is rewritten only behind the
// copy that last read it)
static int upload_series(muse_batch *b, const int64_t *series, int64_t count, hipStream_t st)
{
    muse_ctx *ctx = b->ctx;
    if (!b->prof_copied)
        HIP_TRY(hipEventCreateWithFlags(&b->prof_copied, hipEventDisableTiming));
    else
        HIP_TRY(hipEventSynchronize(b->prof_copied));
    HIP_TRY(b->prof_idx_host.ensure(ctx, count, st));
    HIP_TRY(b->prof_idx.ensure(ctx, count, st));
    for (int64_t i = 0; i < count; i++)
        b->prof_idx_host.p[i] = (long long)series[i];
    HIP_TRY(hipMemcpyAsync(b->prof_idx.p, b->prof_idx_host.p, (size_t)count * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(b->prof_copied, st));
    return MUSE_OK;
}

// the planner's launches for `count` output rows into out (device memory, row stride out_stride): rows [row0, row0 + count) of the
// group, or the `count` entries of b->prof_idx (listed).  Each launch builds its tables into b->prof_e / prof_pw on the stream in
// front of itself, so the launches of a call, and of one call after another, share the one pair of buffers in stream order.
static int profile_launches(muse_batch *b, int64_t row0, int64_t count, bool listed, int32_t lag_lo, int32_t lag_hi, double *out,
                            int64_t out_stride, hipStream_t st)
{
    const muse_group *g = b->g;
    const long long e_len = window_e_len(b->N);
    HIP_TRY(b->prof_e.ensure(b->ctx, e_len, st));
    HIP_TRY(b->prof_pw.ensure(b->ctx, 2 * MUSE_LAG_WINDOW_MAX + 1, st));
    const int launches = window_profile_plan(lag_lo, lag_hi, nullptr, nullptr, 0);
    for (int j = 0; j < launches; j++) {
        const int lo = lag_lo + j * (2 * MUSE_LAG_WINDOW_MAX + 1);
        const int W = (int)std::min<int64_t>(2 * MUSE_LAG_WINDOW_MAX + 1, (int64_t)lag_hi - lo + 1);
        HIP_TRY(launch_window_tables_at(b->xs, b->N, b->n, -lo, W, b->prof_e.p, e_len, b->prof_pw.p, st));
        WindowProfileParams p{};
        p.rows = listed ? g->rows : g->rows + row0 * g->stride;
        p.M = count;
        p.stride = g->stride;
        p.N = b->N;
        p.W = W;
        p.invN = 1.0 / (double)b->N;
        p.invNm1 = 1.0 / (double)(b->N - 1);
        p.e = b->prof_e.p;
        p.pw = b->prof_pw.p;
        p.series = listed ? b->prof_idx.p : nullptr;
        p.out = out + (lo - lag_lo);
        p.out_stride = out_stride;
        LaunchTimer timer(b->ctx, false, st);
        HIP_TRY(timer.begin());
        HIP_TRY(launch_window_profile(p, st));
        HIP_TRY(timer.end());
    }
    return MUSE_OK;
}

// what both forms do before they enqueue: the checks, then the device and the rows.  *rows = the output rows (0: nothing to do)
static int profile_begin(muse_batch *b, const int64_t *series, int64_t K, int32_t lag_lo, int32_t lag_hi, const double *out,
                         int64_t out_stride, int64_t *rows)
{
    // everything is checked before anything is enqueued: on a refusal the batch and the output are unchanged
    if (!b)
        return fail(MUSE_ERR_INVALID, "NULL batch");
    const muse_group *g = b->g;
    int rc = check_profile_args(b->N, g->f32, b->xs != nullptr, g->M, series, K, lag_lo, lag_hi, out_stride);
    if (rc)
        return rc;
    *rows = series ? K : g->M;
    if (*rows == 0)
        return MUSE_OK;
    if (!out)
        return fail(MUSE_ERR_INVALID, "NULL output");
    rc = use_device(b->ctx);
    if (rc)
        return rc;
    return group_ready(b->g, b->stream()); // rows packed but not sent yet go first
}

extern "C" int muse_batch_lag_profile_device(muse_batch *b, const int64_t *series, int64_t K, int32_t lag_lo, int32_t lag_hi,
                                             double *dev_out, int64_t out_stride)
{
    int64_t rows = 0;
    int rc = profile_begin(b, series, K, lag_lo, lag_hi, dev_out, out_stride, &rows);
    if (rc || rows == 0)
        return rc;
    const hipStream_t st = b->stream();
    if (series) {
        rc = upload_series(b, series, rows, st);
        if (rc)
            return rc;
    }
    return profile_launches(b, 0, rows, series != nullptr, lag_lo, lag_hi, dev_out, out_stride, st);
}

extern "C" int muse_batch_lag_profile(muse_batch *b, const int64_t *series, int64_t K, int32_t lag_lo, int32_t lag_hi, double *out,
                                      int64_t out_stride)
{
    int64_t rows = 0;
    int rc = profile_begin(b, series, K, lag_lo, lag_hi, out, out_stride, &rows);
    if (rc || rows == 0)
        return rc;
    const hipStream_t st = b->stream();
    // chunks of whole workgroups (16 rows) of W doubles each inside MUSE_LAG_PROFILE_STAGE_BYTES: the widest profile, every lag of
    // 65536 samples, is 512 KiB a row
    const int64_t W = (int64_t)lag_hi - lag_lo + 1;
    const int64_t fit = MUSE_LAG_PROFILE_STAGE_BYTES / (int64_t)sizeof(double) / W / 16 * 16;
    const int64_t chunk = std::min<int64_t>(rows, std::max<int64_t>(fit, 16));
    HIP_TRY(b->prof_out.ensure(b->ctx, chunk * W, st));
    for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
        const int64_t count = std::min<int64_t>(chunk, rows - r0);
        if (series) {
            rc = upload_series(b, series + r0, count, st);
            if (rc)
                return rc;
        }
        rc = profile_launches(b, r0, count, series != nullptr, lag_lo, lag_hi, b->prof_out.p, W, st);
        if (rc)
            return rc;
        HIP_TRY(hipMemcpy2DAsync(out + r0 * out_stride, (size_t)out_stride * sizeof(double), b->prof_out.p, (size_t)W * sizeof(double),
                                 (size_t)W * sizeof(double), (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st)); // the data is there, and the staging rows are free for the next chunk
    }
    return MUSE_OK;
}
