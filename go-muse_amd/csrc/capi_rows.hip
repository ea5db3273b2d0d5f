// capi_rows.hip -- Muse.Run (muse.go:46-92) as ONE call: the rows of one small label group from host memory against a
// template batch's reference, the group's winner back.
// Part of the implementation of the C ABI declared in include/muse_hip.h (capi_internal.h: the handles and the helpers the
// parts share).  Host-side orchestration only; there is no CPU compute fallback anywhere: without a gfx950 device every
// compute entry point returns MUSE_ERR_NO_DEVICE.
//
// Why it exists: muse_group_upload + muse_batch_create_like + muse_batch_run + two frees cost a dozen hipMalloc / hipFree
// (each a device-wide synchronisation) and three stream synchronisations per Muse.Run -- 110 us for 5 x 480 samples, all of it
// host side.  Here a context keeps a small pool of SLOTS (pinned staging, device rows behind the usual guard, score buffers,
// a pinned result record, an event); a call takes a slot, copies the rows into the staging buffer, and enqueues exactly
//     one host -> HBM copy, the fused kernel automatic selection takes for the length, one single-workgroup kernel that
//     reduces the group (reduce_kernels.hip, single_group_kernel) and writes the winner straight into pinned host memory,
//     one event
// on the SLOT's stream, waits for the event and returns the slot.  Steady state: no allocation, no hipFree, no device-wide
// synchronisation.  Many goroutines may drive one Muse (muse_test.go:203-214): every call in flight owns its slot, and
// since every slot owns a stream the callers' kernels -- a few dozen workgroups each -- run beside each other instead of
// queueing on one stream (round 5: sixteen callers gained 1.85 x over one; profiles/r06_cold_path.txt for now).  FFT lengths
// whose kernels work in the context's shared scratch buffer (n >= 8192) stay on the context's stream.
//
// The WINDOWED forms (muse_batch_run_rows_windowed / _run_row_ptrs_windowed / _run_group_rows_windowed) are the same calls with the
// per-row (lag, mv) of the lag window (muse_batch_set_lag_window) in place of the transform kernel's: the window is an argument of
// the call, no batch's own setting is touched.  The slot keeps its own window tables (the e image and pw of launch_window_tables),
// keyed by (the template spectrum's serial number, window_tables' key) and rebuilt on the slot's stream when the key differs -- any number of host
// threads share one template, so nothing is cached on it.  The window kernels need none of the context's shared scratch: every FFT
// length runs on the slot's stream.  Few rows of long series take the split-K kernels (xcorr_window_split.hip) when
// window_rows_plan says so; otherwise launch_window, the kernel of muse_batch_set_lag_window, untouched.
//
// The LAG-RANGE forms (muse_batch_run_rows_in_lag_range / _run_row_ptrs_in_lag_range / _run_group_rows_in_lag_range) are the windowed
// calls with the lags lag_lo .. lag_hi of muse_batch_score_in_lag_range in place of +-max_lag (WindowCall carries a LagRange; the
// _windowed forms are its symmetric constructor).  rows_lag_range_plan, a pure host function, picks the pass: every lag -- the
// unwindowed call; up to 127 lags -- the kernels above over a table that starts at lag_lo; up to 2048 lags -- the panel kernels
// (xcorr_window_panels.hip), which split the lags over workgroups too; the slot's table cache keys the wide tables apart.
#include "capi_internal.h"

using namespace muse;

namespace {
constexpr size_t ROWS_GUARD = 8192;            // = capi_group.hip's GROUP_GUARD: padded series read in front of row 0
constexpr size_t ROWS_SLOT_MIN_ELEMS = 1u << 16;   // 512 KB: 5 ... 50 series of 480 ... 1000 samples without ever growing
constexpr size_t ROWS_SLOT_MAX_ELEMS = 1u << 24;   // 128 MB: larger groups take the general path (the copies dominate there)
constexpr size_t ROWS_ZERO_COPY_BYTES = 256u << 10; // up to here the kernel reads the pinned staging buffer itself
constexpr size_t ROWS_SLOT_KEEP_ELEMS = 1u << 20;   // 8 MB: a slot that grew beyond hands its buffers back when it is returned
constexpr int ROWS_SLOTS_KEPT = 16;            // slots kept per context when idle (more callers in flight: created and freed)
} // namespace

struct RowsSlot {
    muse_group g;            // rows = the slot's device buffer; N / stride / M set per call
    muse_batch b;            // spectrum tables rebound per call (the template's)
    double *dev = nullptr;   // allocation base (guard in front of g.rows)
    double *host = nullptr;  // pinned staging (ROWS_GUARD zeroed elements in front of it)
    double *host_dev = nullptr; // the same memory as the device addresses it
    size_t cap_elems = 0;
    SingleGroupOut *out = nullptr; // pinned: the winner record, written by the device
    hipEvent_t done = nullptr;
    hipStream_t stream = nullptr;  // the slot's own stream
    // the windowed forms: the tables of launch_window_tables for (win_serial, win_key) (0: none; window_tables' key), and the slabs of the split-K kernels
    PoolBuf<double> win_e, win_pw, win_slabs;
    uint64_t win_serial = 0;
    int32_t win_key = -1;
};

// what a windowed call adds to a Muse.Run: its lags, and (the test hooks) where the per-row results go before the slot is returned.
// The _windowed forms are the symmetric constructor (lags -max_lag .. max_lag, at most MUSE_LAG_WINDOW_MAX either way, always the window
// kernels); the _in_lag_range forms take the dispatch table of muse_batch_run_rows_in_lag_range (rows_lag_range_plan).
struct WindowCall {
    int32_t lo, hi;
    bool ranged;   // an _in_lag_range form
    int32_t *lag_out;
    double *mv_out;
    // filled in by check_window_call: the lags clipped at the template's FFT length, and the pass
    LagRange w{0, 0, 0};
    bool plain = false; // every lag: the unwindowed namesake's pass
    bool wide = false;  // more than 2 MUSE_LAG_WINDOW_MAX + 1 table rows: the panel kernels
    static WindowCall window(int32_t max_lag, int32_t *lag_out = nullptr, double *mv_out = nullptr)
    {
        return WindowCall{max_lag < 0 ? max_lag : -max_lag, max_lag, false, lag_out, mv_out};
    }
    static WindowCall range(int32_t lo, int32_t hi, int32_t *lag_out = nullptr, double *mv_out = nullptr)
    {
        return WindowCall{lo, hi, true, lag_out, mv_out};
    }
    bool direct() const { return !plain; } // the window kernels score it: every FFT length on the slot's stream
};

static void slot_destroy(RowsSlot *s)
{
    if (!s)
        return;
    muse_ctx *ctx = s->b.ctx;
    if (s->stream)
        (void)hipStreamSynchronize(s->stream);
    dfree(ctx, s->dev);
    if (s->host)
        hfree(ctx, s->host - ROWS_GUARD);
    if (s->out)
        (void)hipHostFree(s->out);
    if (s->done)
        (void)hipEventDestroy(s->done);
    s->g.hstats.release(ctx);
    s->b.mv.release(ctx);
    s->b.lag.release(ctx);
    s->win_e.release(ctx);
    s->win_pw.release(ctx);
    s->win_slabs.release(ctx);
    s->b.ovf_list.release(ctx);
    dfree(ctx, s->b.ovf_count);
    hfree(ctx, s->b.handoff_host);
    if (s->stream)
        (void)hipStreamDestroy(s->stream);
    delete s;
}

// called by ctx_release with the context's streams idle
void rows_slots_free(muse_ctx *ctx)
{
    for (void *p : ctx->rows_slots)
        slot_destroy((RowsSlot *)p);
    ctx->rows_slots.clear();
}

static int slot_reserve(RowsSlot *s, size_t elems)
{
    if (elems <= s->cap_elems)
        return MUSE_OK;
    size_t cap = ROWS_SLOT_MIN_ELEMS;
    while (cap < elems)
        cap *= 2;
    muse_ctx *ctx = s->b.ctx;
    dfree(ctx, s->dev);
    if (s->host)
        hfree(ctx, s->host - ROWS_GUARD);
    s->dev = nullptr;
    s->host = nullptr;
    s->cap_elems = 0;
    s->g.rows = nullptr;
    HIP_TRY(dmalloc(ctx, &s->dev, (cap + ROWS_GUARD) * sizeof(double)));
    HIP_TRY(hipMemsetAsync(s->dev, 0, ROWS_GUARD * sizeof(double), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (growth is rare; the call may go on to use the context's stream instead of the slot's)
    // (the staging buffer carries the same zeroed guard: the smallest groups are read by the kernel straight out of it)
    double *hbase = nullptr;
    HIP_TRY(hmalloc(ctx, &hbase, (cap + ROWS_GUARD) * sizeof(double)));
    memset(hbase, 0, ROWS_GUARD * sizeof(double));
    s->host = hbase + ROWS_GUARD;
    s->host_dev = nullptr;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hbase, 0) == hipSuccess && dp)
        s->host_dev = (double *)dp + ROWS_GUARD;
    s->g.rows = s->dev + ROWS_GUARD;
    s->cap_elems = cap;
    return MUSE_OK;
}

static int slot_acquire(muse_ctx *ctx, size_t elems, RowsSlot **out)
{
    RowsSlot *s = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->rows_mu);
        if (!ctx->rows_slots.empty()) {
            s = (RowsSlot *)ctx->rows_slots.back();
            ctx->rows_slots.pop_back();
        }
    }
    if (!s) {
        s = new (std::nothrow) RowsSlot();
        if (!s)
            return fail(MUSE_ERR_NOMEM, "host allocation failed");
        s->g.ctx = ctx;
        s->b.ctx = ctx;
        s->b.g = &s->g;
        // (coherent whatever HIP_HOST_COHERENT says: the caller polls the record's state word while the kernel that writes it is still running)
        hipError_t e = hipHostMalloc((void **)&s->out, sizeof(SingleGroupOut), hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
        if (e == hipSuccess)
            e = dmalloc(ctx, &s->b.ovf_count, 2 * sizeof(int));
        if (e != hipSuccess) {
            slot_destroy(s);
            return fail(MUSE_ERR_HIP, "slot set-up failed: %s", hipGetErrorString(e));
        }
    }
    int rc = slot_reserve(s, elems);
    if (rc) {
        slot_destroy(s);
        return rc;
    }
    *out = s;
    return MUSE_OK;
}

static void slot_return(muse_ctx *ctx, RowsSlot *s)
{
    if (s->cap_elems > ROWS_SLOT_KEEP_ELEMS) { // one burst of large groups must not pin 16 x 128 MB for the life of the context
        dfree(ctx, s->dev);
        hfree(ctx, s->host - ROWS_GUARD);
        s->dev = nullptr;
        s->host = s->host_dev = nullptr;
        s->g.rows = nullptr;
        s->cap_elems = 0;
    }
    {
        std::lock_guard<std::mutex> lock(ctx->rows_mu);
        if ((int)ctx->rows_slots.size() < ROWS_SLOTS_KEPT) {
            ctx->rows_slots.push_back(s);
            return;
        }
    }
    slot_destroy(s); // (the slot's work has completed: its event was waited for)
}

// a slot shaped for M rows of the template's length against the template's reference (rows: s->g.rows, set by the caller)
// (windowed: the window kernels need none of the context's shared scratch -- every length on the slot's stream)
static int slot_take(muse_batch *tmpl, int64_t M, size_t elems, RowsSlot **out, bool windowed = false)
{
    muse_ctx *ctx = tmpl->ctx;
    const int32_t N = tmpl->N;
    RowsSlot *s = nullptr;
    int rc = slot_acquire(ctx, elems, &s);
    if (rc)
        return rc;
    // the slot's group and batch take this call's shape and the template's reference
    s->g.N = N;
    s->g.stride = N;
    s->g.M = M;
    s->g.cap = M;
    s->g.hstats_rows = 0; // (other rows than the slot's last call: no kept statistics)
    s->g.transient = true; // (nor a spectrum cache)
    s->b.N = tmpl->N;
    s->b.n = tmpl->n;
    s->b.logn = tmpl->logn;
    s->b.sp = tmpl->sp;
    adopt_spectrum(&s->b);
    s->b.handoff_M = -1; // (no kernel-selection memory across unrelated groups)
    // kernels that work in the context's shared scratch buffer are serialised on the context's stream
    s->b.own_stream = tmpl->n >= GENERIC_LDS_MAX_N && !windowed ? nullptr : s->stream;
    const int64_t cap = std::max<int64_t>(M, 4096); // (grown in steps that small groups never reach twice)
    hipError_t ea = s->b.mv.ensure(ctx, cap, s->stream);
    if (ea == hipSuccess)
        ea = s->b.lag.ensure(ctx, cap, s->stream);
    if (ea != hipSuccess) {
        slot_destroy(s);
        return fail(MUSE_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(ea));
    }
    *out = s;
    return MUSE_OK;
}

// The dispatch of the _in_lag_range forms, a pure host function of (M, N, CUs, the clipped range): MUSE_ROWS_LAG_RANGE_*
//   w is every lag                              : PLAIN, the unwindowed namesake's pass
//   at most 2 MUSE_LAG_WINDOW_MAX + 1 table rows, n <= 65536 : the existing kernels -- WINDOW (launch_window), or SPLIT
//                                                 (launch_window_split) when window_rows_plan says S > 1
//   up to WIN_PANEL_MAX_ROWS rows, n <= 65536   : PANELS (xcorr_window_panels.hip), S by window_panels_plan
//   anything else                               : not built
static int rows_lag_range_plan(int64_t M, int32_t N, int num_cus, const LagRange &w, int *panels, int *S)
{
    const int64_t n = muse_next_pow2((double)N);
    *panels = 0;
    *S = 0;
    if (w.every_lag(n))
        return MUSE_ROWS_LAG_RANGE_PLAIN;
    if (n > GENERIC_MAX_N || w.rows() > WIN_PANEL_MAX_ROWS)
        return MUSE_ROWS_LAG_RANGE_UNSUPPORTED;
    if (w.rows() <= 2 * MUSE_LAG_WINDOW_MAX + 1) {
        *panels = 1;
        *S = window_rows_plan(M, N, num_cus, nullptr);
        return *S > 1 ? MUSE_ROWS_LAG_RANGE_SPLIT : MUSE_ROWS_LAG_RANGE_WINDOW;
    }
    *S = window_panels_plan(M, N, num_cus, w.rows(), panels);
    return MUSE_ROWS_LAG_RANGE_PANELS;
}

// the panel pass over b's rows inside w (device selected, rows in place, M > 0, mv / lag allocated): the wide tables in e / pw, cached
// under *key -- (origin, rows) of up to 2048 each above bit 30, where no key of window_tables (origin 256 + rows, both <= 127) lies --
// then launch_window_panels into `slabs`, all on b's stream
static int score_panels(muse_batch *b, const LagRange &w, PoolBuf<double> &e, PoolBuf<double> &pw, PoolBuf<double> &slabs, int32_t *key)
{
    muse_ctx *ctx = b->ctx;
    const hipStream_t st = b->stream();
    const int W = w.rows();
    const int32_t k = 0x40000000 + w.origin * 4096 + W;
    if (*key != k) {
        *key = -1;
        const long long e_len = window_panels_e_len(b->N, W);
        HIP_TRY(e.ensure(ctx, e_len, st));
        HIP_TRY(pw.ensure(ctx, W, st));
        HIP_TRY(launch_window_tables_wide(b->xs, b->N, b->n, w.origin, W, e.p, e_len, pw.p, st));
        *key = k;
    }
    const WindowParams p = window_params(b, w, e.p, pw.p);
    const int chunks = (b->N + WIN_KC - 1) / WIN_KC;
    const int forced = ctx->win_rows_slices.load(std::memory_order_relaxed);
    int panels = 0;
    int S = window_panels_plan(p.M, p.N, ctx->num_cus, W, &panels);
    if (forced >= 1)
        S = std::min(forced, chunks);
    HIP_TRY(slabs.ensure(ctx, (p.M + 15) / 16 * panels * S * window_panels_slab_doubles(), st));
    LaunchTimer timer(ctx, false, st);
    HIP_TRY(timer.begin());
    HIP_TRY(launch_window_panels(p, S, slabs.p, st));
    HIP_TRY(timer.end());
    return MUSE_OK;
}

// the windowed per-row pass of a slot (rows in place or their copy enqueued, mv / lag allocated): the slot's tables for
// (spectrum, origin, rows), then launch_window or -- few rows of long series -- the split-K kernels, or -- more than 127 table rows --
// the panel kernels, all on the slot's stream
static int slot_score_windowed(muse_ctx *ctx, RowsSlot *s, const WindowCall &wc)
{
    muse_batch *b = &s->b;
    const hipStream_t st = b->stream();
    const LagRange w = wc.w;
    if (s->win_serial != b->sp->serial) // (another reference: whatever window the tables were built for)
        s->win_key = -1;
    if (wc.wide) {
        const int prc = score_panels(b, w, s->win_e, s->win_pw, s->win_slabs, &s->win_key);
        if (!prc)
            s->win_serial = b->sp->serial;
        return prc;
    }
    const int rc = window_tables(b, w, s->win_e, s->win_pw, &s->win_key, st);
    if (rc)
        return rc;
    s->win_serial = b->sp->serial;
    const WindowParams p = window_params(b, w, s->win_e.p, s->win_pw.p);
    const int chunks = (b->N + WIN_KC - 1) / WIN_KC;
    const int forced = ctx->win_rows_slices.load(std::memory_order_relaxed);
    const int S = forced >= 1 ? std::min(forced, chunks) : window_rows_plan(p.M, p.N, ctx->num_cus, nullptr);
    if (S > 1)
        HIP_TRY(s->win_slabs.ensure(ctx, (p.M + 15) / 16 * S * window_split_slab_doubles(p), st));
    LaunchTimer timer(ctx, false, st);
    HIP_TRY(timer.begin());
    if (S > 1)
        HIP_TRY(launch_window_split(p, S, s->win_slabs.p, st));
    else
        HIP_TRY(launch_window(p, st));
    HIP_TRY(timer.end());
    return MUSE_OK;
}

// the slot's rows in place (or their copy enqueued: e its status): the fused kernel, the reduction into the pinned record, the
// wait for it; the slot goes back to the context
static int slot_finish(muse_ctx *ctx, RowsSlot *s, int64_t M, int32_t abs_scores, hipError_t e, muse_record *out_winner,
                       uint8_t *out_state, const WindowCall *wc = nullptr)
{
    const hipStream_t st = s->b.stream();
    int rc = MUSE_OK;
    if (e == hipSuccess) {
        // the fused kernel automatic selection takes for this length (and its redo launch, if any), or the window kernels
        rc = wc && wc->direct() ? slot_score_windowed(ctx, s, *wc) : muse_batch_score(&s->b);
        if (!rc)
            e = launch_single_group(s->b.mv.p, s->b.lag.p, M, abs_scores ? 1 : 0, 0, s->out, st);
    }
    if (e != hipSuccess || rc) {
        (void)hipStreamSynchronize(st); // nothing of this call may still be using the slot
        slot_return(ctx, s);
        return rc ? rc : fail(MUSE_ERR_HIP, "muse_batch_run_rows: %s", hipGetErrorString(e));
    }
    // The reduction kernel's last act is the record (rec, a system-scope fence, then state) in coherent pinned memory: the
    // caller polls the state word instead of recording and waiting for an event -- one command-processor packet and one
    // runtime wait fewer per Muse.Run.  A kernel that never delivers (a device fault) is found by the stream synchronisation
    // the poll falls back to.
    {
        volatile unsigned long long *flag = (volatile unsigned long long *)&s->out->state;
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (unsigned spin = 1; *flag == ~0ull; spin++) {
            __builtin_ia32_pause();
            if ((spin & 1023u) == 0) {
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > 200000000ll) // 0.2 s: hand over to the runtime
                    break;
            }
        }
        if (*flag == ~0ull) {
            e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                slot_destroy(s);
                return fail(MUSE_ERR_HIP, "muse_batch_run_rows: %s", hipGetErrorString(e));
            }
        }
    }
    const unsigned long long stt = *(volatile unsigned long long *)&s->out->state;
    *out_winner = s->out->rec;
    // TEST HOOK ONLY (muse_test_run_rows_windowed_scores; the product's calls leave lag_out / mv_out NULL and skip this): the slot's
    // per-row pairs, copied back here because the slot is about to be returned (the record arrived: the scores are behind it on the
    // same stream)
    if (wc && wc->lag_out && wc->mv_out) {
        e = hipMemcpyAsync(wc->lag_out, s->b.lag.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(wc->mv_out, s->b.mv.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            slot_destroy(s);
            return fail(MUSE_ERR_HIP, "muse_test_run_rows_windowed_scores: %s", hipGetErrorString(e));
        }
    }
    slot_return(ctx, s);
    if (stt > 2ull)
        return fail(MUSE_ERR_HIP, "muse_batch_run_rows: the result record did not arrive");
    *out_state = (uint8_t)stt;
    return MUSE_OK;
}

// the refusals of the windowed forms (nothing is changed before the last of them has passed), and the call's pass
static int check_window_call(const muse_batch *tmpl, WindowCall *wc)
{
    if (!wc->ranged) {
        const int32_t max_lag = wc->hi;
        if (max_lag < 0)
            return fail(MUSE_ERR_INVALID, "a windowed Muse.Run needs a lag window >= 0");
        if (tmpl->windowed() && tmpl->lag_window != max_lag)
            return fail(MUSE_ERR_INVALID, "the template has a lag window of %d of its own: it must be off or equal to the call's (%d)",
                        tmpl->lag_window, max_lag);
        wc->w = lag_window_range(tmpl->n, max_lag);
        return check_window_request(tmpl, max_lag, false); // (the rows are the call's own float64: the template's group is not read)
    }
    if (wc->lo > 0 || wc->hi < 0)
        return fail(MUSE_ERR_INVALID, "the lag range %d .. %d does not hold lag 0 (lag_lo <= 0 <= lag_hi)", wc->lo, wc->hi);
    const int rc = check_own_window(tmpl, wc->lo, wc->hi);
    if (rc)
        return rc;
    wc->w = clip_lag_range(tmpl->n, wc->lo, wc->hi);
    int panels = 0, S = 0;
    const int path = rows_lag_range_plan(1, tmpl->N, 1, wc->w, &panels, &S); // (which pass: M and the CUs choose S only)
    wc->plain = path == MUSE_ROWS_LAG_RANGE_PLAIN;
    wc->wide = path == MUSE_ROWS_LAG_RANGE_PANELS;
    if (path == MUSE_ROWS_LAG_RANGE_UNSUPPORTED || (!wc->plain && !tmpl->xs))
        return fail(MUSE_ERR_UNSUPPORTED, "a Muse.Run inside the lags %d .. %d over series of %d samples is not built: up to %d lags of "
                    "series of up to %d samples, or every lag", -wc->w.lneg, wc->w.hi, tmpl->N, WIN_PANEL_MAX_ROWS, GENERIC_MAX_N);
    return MUSE_OK;
}

// the pass of a general path's private batch inside the call's lags: the direct product of batch_score up to 127 table rows, the
// panel pass beyond (its slabs: the caller's, released behind the Run)
struct GeneralPass {
    const WindowCall *wc;
    PoolBuf<double> *slabs;
};
static int general_score(muse_batch *b, const void *arg)
{
    const GeneralPass *gp = (const GeneralPass *)arg;
    const WindowCall *wc = gp->wc;
    if (!wc->wide) {
        ScorePass pass;
        pass.window = &wc->w;
        pass.path = MUSE_IN_WINDOW_MFMA;
        return batch_score(b, pass);
    }
    // as batch_score prepares a pass
    int rc = use_device(b->ctx);
    if (!rc)
        rc = group_ready(b->g, b->stream());
    if (rc || b->g->M == 0)
        return rc;
    rc = ensure_scores(b);
    if (rc)
        return rc;
    b->origin = ScoreOrigin{};
    b->scores_exact = true;
    return score_panels(b, wc->w, b->win_e, b->win_pw, *gp->slabs, &b->win_key);
}

// the private batch of a general path: like tmpl over g, with the call's window (if any); Run with G = 1; the test hook's scores
static int run_general_batch(muse_batch *tmpl, muse_group *g, int64_t M, int32_t abs_scores, muse_record *out_winner,
                             uint8_t *out_state, const WindowCall *wc)
{
    muse_batch *b = nullptr;
    int rc = muse_batch_create_like(tmpl, g, &b);
    PoolBuf<double> slabs;
    if (!rc) {
        std::vector<int32_t> gid((size_t)M, 0);
        const GeneralPass gp{wc, &slabs};
        const bool direct = wc && wc->direct();
        rc = run_groups(b, gid.data(), 1, 0, abs_scores, out_winner, out_state, direct ? general_score : nullptr, &gp);
    }
    if (!rc && wc && wc->lag_out && wc->mv_out)
        rc = muse_batch_read_scores(b, wc->lag_out, wc->mv_out);
    if (slabs.p) {
        (void)hipStreamSynchronize(b->stream()); // nothing of this call may still be using the slabs
        slabs.release(tmpl->ctx);
    }
    muse_batch_free(b);
    return rc;
}

// the general path for groups too large for a slot: what the host mirrors did per Muse.Run before this entry point existed
static int run_rows_general(muse_batch *tmpl, const double *rows, const double *const *row_ptrs, int64_t M, int64_t row_stride,
                            int32_t abs_scores, muse_record *out_winner, uint8_t *out_state, const WindowCall *wc)
{
    muse_group *g = nullptr;
    int rc;
    if (rows) {
        rc = muse_group_upload(tmpl->ctx, rows, M, tmpl->N, row_stride, &g);
    } else {
        rc = muse_group_create(tmpl->ctx, M, tmpl->N, &g);
        for (int64_t r = 0; r < M && !rc; r++)
            rc = muse_group_append(g, row_ptrs[r], 1, tmpl->N);
    }
    if (rc) {
        muse_group_free(g);
        return rc;
    }
    rc = run_general_batch(tmpl, g, M, abs_scores, out_winner, out_state, wc);
    muse_group_free(g);
    return rc;
}

// rows: M x N with stride row_stride, or (rows == NULL) row_ptrs[r] -> the N samples of row r
// wc: the windowed forms (NULL: the transform kernels)
static int run_rows(muse_batch *tmpl, const double *rows, const double *const *row_ptrs, int64_t M, int64_t row_stride,
                    int32_t abs_scores, muse_record *out_winner, uint8_t *out_state, WindowCall *wc = nullptr)
{
    if (!tmpl || !out_winner || !out_state || M < 0 || (M > 0 && !rows && !row_ptrs))
        return fail(MUSE_ERR_INVALID, "bad arguments");
    *out_winner = muse_record{-1, 0.0, 0, 0};
    *out_state = 0;
    if (wc) {
        const int wrc = check_window_call(tmpl, wc);
        if (wrc)
            return wrc;
    } else if (tmpl->windowed()) {
        return fail(MUSE_ERR_UNSUPPORTED, "a batch with a lag window cannot be the template of a Muse.Run");
    }
    if (M == 0) // muse.go:47-50: nothing to compare
        return MUSE_OK;
    const int32_t N = tmpl->N;
    if (rows && row_stride < N) // muse.go:68-70
        return fail(MUSE_ERR_LENGTH, "Encountered a comparison graph with differing length than the reference (%lld vs %d)",
                    (long long)row_stride, N);
    if (!rows)
        for (int64_t r = 0; r < M; r++)
            if (!row_ptrs[r])
                return fail(MUSE_ERR_INVALID, "row %lld is NULL", (long long)r);
    muse_ctx *ctx = tmpl->ctx;
    int rc = use_device(ctx);
    if (rc)
        return rc;
    const size_t elems = (size_t)M * (size_t)N;
    if (elems > ROWS_SLOT_MAX_ELEMS)
        return run_rows_general(tmpl, rows, row_ptrs, M, row_stride, abs_scores, out_winner, out_state, wc);
    RowsSlot *s = nullptr;
    rc = slot_take(tmpl, M, elems, &s, wc && wc->direct());
    if (rc)
        return rc;
    const hipStream_t st = s->b.stream();
    if (rows && row_stride == N) {
        memcpy(s->host, rows, elems * sizeof(double));
    } else {
        for (int64_t r = 0; r < M; r++)
            memcpy(s->host + (size_t)r * (size_t)N, rows ? rows + (size_t)r * (size_t)row_stride : row_ptrs[r], (size_t)N * sizeof(double));
    }
    s->out->state = ~0ull;
    // The smallest groups are not copied at all: the fused kernel reads its rows once, so it reads them straight from the
    // pinned staging buffer over PCIe (a copy command in front of the kernel costs more than its 19 KB take to cross)
    hipError_t e = hipSuccess;
    if (s->host_dev && elems * sizeof(double) <= ROWS_ZERO_COPY_BYTES && !ctx->rows_always_copy.load(std::memory_order_relaxed)) {
        s->g.rows = s->host_dev;
    } else {
        s->g.rows = s->dev + ROWS_GUARD;
        e = hipMemcpyAsync(s->g.rows, s->host, elems * sizeof(double), hipMemcpyHostToDevice, st);
    }
    return slot_finish(ctx, s, M, abs_scores, e, out_winner, out_state, wc);
}

extern "C" int muse_batch_run_rows(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride, int32_t abs_scores,
                                   muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    return run_rows(tmpl, rows, nullptr, M, row_stride, abs_scores, out_winner, out_state);
}

// the same with one pointer per row (each to the template's N samples): the series of a Muse.Run are separate slices
// (muse.go:46, compGraphs []*Series) -- they are gathered straight into the slot's pinned buffer, not packed by the caller first
extern "C" int muse_batch_run_row_ptrs(muse_batch *tmpl, const double *const *rows, int64_t M, int32_t abs_scores,
                                       muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    return run_rows(tmpl, nullptr, rows, M, 0, abs_scores, out_winner, out_state);
}

// ---- Muse.Run over rows that are already resident in a group: no host copy and no PCIe transfer of samples
// the general path for groups too large for a slot: the rows gathered into a group of their own, then the existing Run
static int run_group_rows_general(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M, int32_t abs_scores,
                                  muse_record *out_winner, uint8_t *out_state, const WindowCall *wc)
{
    muse_group *g = nullptr;
    int rc = muse_group_create(tmpl->ctx, M, tmpl->N, &g);
    if (!rc)
        rc = group_gather(g, src, rows, M); // (a float32 src is widened into the float64 group)
    if (!rc)
        rc = run_general_batch(tmpl, g, M, abs_scores, out_winner, out_state, wc);
    muse_group_free(g);
    return rc;
}

static int run_group_rows(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M, int32_t abs_scores,
                          muse_record *out_winner, uint8_t *out_state, WindowCall *wc)
{
    if (!tmpl || !src || !out_winner || !out_state || M < 0 || (M > 0 && !rows))
        return fail(MUSE_ERR_INVALID, "bad arguments");
    *out_winner = muse_record{-1, 0.0, 0, 0};
    *out_state = 0;
    if (wc) {
        const int wrc = check_window_call(tmpl, wc);
        if (wrc)
            return wrc;
    } else if (tmpl->windowed()) {
        return fail(MUSE_ERR_UNSUPPORTED, "a batch with a lag window cannot be the template of a Muse.Run");
    }
    if (src->ctx != tmpl->ctx)
        return fail(MUSE_ERR_INVALID, "the group and the template belong to different contexts");
    if (src->win_rows)
        return fail(MUSE_ERR_INVALID, "the group has an open staging window");
    const int32_t N = tmpl->N;
    if (src->N != N) // muse.go:68-70
        return fail(MUSE_ERR_LENGTH, "Encountered a comparison graph with differing length than the reference (%d vs %d)", src->N, N);
    int rc = check_row_list(src, rows, M);
    if (rc || M == 0) // muse.go:47-50: nothing to compare
        return rc;
    muse_ctx *ctx = tmpl->ctx;
    rc = use_device(ctx);
    if (rc)
        return rc;
    const size_t elems = (size_t)M * (size_t)N;
    if (elems > ROWS_SLOT_MAX_ELEMS)
        return run_group_rows_general(tmpl, src, rows, M, abs_scores, out_winner, out_state, wc);
    // one ascending run of a float64 group is scored where it lies (a padded length reads up to n - N samples in front of the
    // first row and masks them: the row in front of it, or the group's guard in front of row 0)
    bool contiguous = !src->f32;
    for (int64_t i = 1; i < M && contiguous; i++)
        contiguous = rows[i] == rows[0] + i;
    // the index list rides at the end of the slot's device buffer (behind the M x N gathered rows)
    RowsSlot *s = nullptr;
    rc = slot_take(tmpl, M, contiguous ? elems : elems + (size_t)M, &s, wc && wc->direct());
    if (rc)
        return rc;
    const hipStream_t st = s->b.stream();
    s->out->state = ~0ull;
    hipError_t e = hipSuccess;
    // src's packed rows enqueued and this call's stream behind every write into src
    rc = group_ready_shared(src, st);
    if (!rc) {
        if (contiguous) {
            s->g.rows = src->rows + rows[0] * src->stride;
        } else {
            s->g.rows = s->dev + ROWS_GUARD;
            memcpy(s->host, rows, (size_t)M * sizeof(long long));
            // (a short list is read by the gather straight from the pinned buffer, as the smallest groups' rows are by run_rows)
            const long long *idx = (const long long *)s->host_dev;
            if (!idx || elems * sizeof(double) > ROWS_ZERO_COPY_BYTES || ctx->rows_always_copy.load(std::memory_order_relaxed)) {
                idx = (const long long *)(s->g.rows + elems);
                e = hipMemcpyAsync((void *)idx, s->host, (size_t)M * sizeof(long long), hipMemcpyHostToDevice, st);
            }
            if (e == hipSuccess)
                e = launch_row_gather(src->base(), src->f32, s->g.rows, false, idx, M, N, ctx->num_cus,
                                      ctx->gather_nt.load(std::memory_order_relaxed), st);
        }
    }
    if (rc) {
        (void)hipStreamSynchronize(st);
        slot_return(ctx, s);
        return rc;
    }
    return slot_finish(ctx, s, M, abs_scores, e, out_winner, out_state, wc);
}

extern "C" int muse_batch_run_group_rows(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M, int32_t abs_scores,
                                         muse_record *out_winner, uint8_t *out_state)
{
    return run_group_rows(tmpl, src, rows, M, abs_scores, out_winner, out_state, nullptr);
}

// ---- the windowed forms: the per-row (lag, mv) is the lag window's (muse_batch_set_lag_window), everything behind it unchanged
extern "C" int muse_batch_run_rows_windowed(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride, int32_t max_lag,
                                            int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    WindowCall wc = WindowCall::window(max_lag);
    return run_rows(tmpl, rows, nullptr, M, row_stride, abs_scores, out_winner, out_state, &wc);
}

extern "C" int muse_batch_run_row_ptrs_windowed(muse_batch *tmpl, const double *const *rows, int64_t M, int32_t max_lag,
                                                int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    WindowCall wc = WindowCall::window(max_lag);
    return run_rows(tmpl, nullptr, rows, M, 0, abs_scores, out_winner, out_state, &wc);
}

extern "C" int muse_batch_run_group_rows_windowed(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M, int32_t max_lag,
                                                  int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    WindowCall wc = WindowCall::window(max_lag);
    return run_group_rows(tmpl, src, rows, M, abs_scores, out_winner, out_state, &wc);
}

// ---- the same inside the lags lag_lo .. lag_hi (lag_lo <= 0 <= lag_hi): the per-row (lag, mv) is muse_batch_score_in_lag_range's,
// for up to MUSE_RUN_ROWS_LAG_RANGE_MAX lags (rows_lag_range_plan), everything behind it unchanged
extern "C" int muse_batch_run_rows_in_lag_range(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride, int32_t lag_lo,
                                                int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    WindowCall wc = WindowCall::range(lag_lo, lag_hi);
    return run_rows(tmpl, rows, nullptr, M, row_stride, abs_scores, out_winner, out_state, &wc);
}

extern "C" int muse_batch_run_row_ptrs_in_lag_range(muse_batch *tmpl, const double *const *rows, int64_t M, int32_t lag_lo,
                                                    int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    if (M > 0 && !rows)
        return fail(MUSE_ERR_INVALID, "bad arguments");
    WindowCall wc = WindowCall::range(lag_lo, lag_hi);
    return run_rows(tmpl, nullptr, rows, M, 0, abs_scores, out_winner, out_state, &wc);
}

extern "C" int muse_batch_run_group_rows_in_lag_range(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M, int32_t lag_lo,
                                                      int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state)
{
    WindowCall wc = WindowCall::range(lag_lo, lag_hi);
    return run_group_rows(tmpl, src, rows, M, abs_scores, out_winner, out_state, &wc);
}

// ---- test hooks of the windowed forms (include/muse_hip_test.h)
extern "C" int muse_test_rows_lag_range_plan(int64_t M, int32_t N, int32_t num_cus, int32_t lag_lo, int32_t lag_hi, int32_t *path,
                                             int32_t *panels, int32_t *S)
{
    if (M < 1 || N < 2 || num_cus < 1 || lag_lo > 0 || lag_hi < 0 || !path)
        return fail(MUSE_ERR_INVALID, "rows lag-range plan: M >= 1, N >= 2, num_cus >= 1, lag_lo <= 0 <= lag_hi");
    int pn = 0, s = 0;
    *path = rows_lag_range_plan(M, N, num_cus, clip_lag_range(muse_next_pow2((double)N), lag_lo, lag_hi), &pn, &s);
    if (panels)
        *panels = pn;
    if (S)
        *S = s;
    return MUSE_OK;
}

extern "C" int muse_test_run_rows_in_lag_range_scores(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride,
                                                      int32_t lag_lo, int32_t lag_hi, int32_t *lag_out, double *mv_out)
{
    if (M > 0 && (!rows || !lag_out || !mv_out))
        return fail(MUSE_ERR_INVALID, "bad arguments");
    muse_record win;
    uint8_t state = 0;
    WindowCall wc = WindowCall::range(lag_lo, lag_hi, lag_out, mv_out);
    return run_rows(tmpl, rows, nullptr, M, row_stride, 0, &win, &state, &wc);
}

extern "C" int muse_test_window_rows_plan(int64_t M, int32_t N, int32_t num_cus, int32_t *S, int32_t *chunks_per_slice)
{
    if (M < 1 || N < 2 || num_cus < 1 || !S)
        return fail(MUSE_ERR_INVALID, "window rows plan: M >= 1, N >= 2, num_cus >= 1");
    int cps = 0;
    *S = window_rows_plan(M, N, num_cus, &cps);
    if (chunks_per_slice)
        *chunks_per_slice = cps;
    return MUSE_OK;
}

extern "C" int muse_test_window_rows_slices(muse_ctx *ctx, int32_t S)
{
    if (!ctx || S < 0)
        return fail(MUSE_ERR_INVALID, "window rows slices: a context and S >= 0");
    ctx->win_rows_slices.store(S);
    return MUSE_OK;
}

extern "C" int muse_test_run_rows_windowed_scores(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride,
                                                  int32_t max_lag, int32_t *lag_out, double *mv_out)
{
    if (M > 0 && (!rows || !lag_out || !mv_out))
        return fail(MUSE_ERR_INVALID, "bad arguments");
    muse_record win;
    uint8_t state = 0;
    WindowCall wc = WindowCall::window(max_lag, lag_out, mv_out);
    return run_rows(tmpl, rows, nullptr, M, row_stride, 0, &win, &state, &wc);
}

extern "C" int muse_test_rows_always_copy(muse_ctx *ctx, int32_t always_copy)
{
    if (!ctx)
        return fail(MUSE_ERR_INVALID, "NULL context");
    ctx->rows_always_copy.store(always_copy != 0);
    return MUSE_OK;
}
