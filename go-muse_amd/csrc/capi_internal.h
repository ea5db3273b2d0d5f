// capi_internal.h -- what the parts of the C-ABI implementation (capi_*.hip) share: the handle structures behind
// include/muse_hip.h's opaque types, error reporting, the launch timer and the helpers that cross file boundaries.
// Internal to libmuse_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <map>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "muse_hip.h"
#include "muse_hip_test.h"
#include "xcorr_kernels.h"

using namespace muse;

extern thread_local std::string g_last_error; // muse_last_error(): per host thread (capi_context.hip)
int fail(int status, const char *fmt, ...);
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(MUSE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                        __FILE__, __LINE__);                                                       \
    } while (0)

// ----------------------------------------------------------------- handles
// Per-context cache of device and pinned-host allocations (capi_context.hip: dmalloc / dfree / hmalloc / hfree).  hipMalloc,
// hipFree (a device-wide synchronisation each) and hipHostMalloc (hundreds of microseconds) were most of a cold
// NewGroup -> Add -> NewBatch -> Run -> free cycle (profiles/r06_cold_path.txt); a freed block is kept by size class and handed to
// the next request of that class.  A block handed back must no longer be in use by the device: work buffers that grow keep
// that rule through PoolBuf below; a bare dfree / hfree is left only right behind a synchronisation of the streams that used
// the block (handle teardown, one-shot temporaries).
struct MemPool {
    std::mutex mu;
    std::unordered_map<void *, size_t> size_of;            // every block this pool allocated (in use or cached): its class size
    std::multimap<size_t, void *> idle;                     // cached blocks by class size
    size_t idle_bytes = 0;
    size_t idle_cap = 0;                                    // cached bytes kept at most
    size_t block_cap = 0;                                   // larger blocks are never cached
};
// (drain_on_failure: out of memory with blocks cached -> give them back and try once more)
hipError_t pool_alloc(muse_ctx *ctx, bool host, void **out, size_t bytes, bool drain_on_failure = true); // capi_context.hip
void pool_free(muse_ctx *ctx, bool host, void *p);
// A work buffer that grows on demand: `cap` elements of T from the context's device pool (Host: its pinned host pool).
template <class T, bool Host = false> struct PoolBuf {
    T *p = nullptr;
    int64_t cap = 0;
    // at least `count` elements (any rounding is the caller's); before a held block goes back to the pool, `busy` -- the stream
    // its users were enqueued on -- is waited for.  On failure p == nullptr and cap == 0.
    hipError_t ensure(muse_ctx *ctx, int64_t count, hipStream_t busy)
    {
        if (count <= cap)
            return hipSuccess;
        if (p) {
            const hipError_t e = hipStreamSynchronize(busy);
            if (e != hipSuccess)
                return e;
        }
        release(ctx);
        const hipError_t e = pool_alloc(ctx, Host, (void **)&p, (size_t)count * sizeof(T));
        if (e == hipSuccess)
            cap = count;
        return e;
    }
    // without a wait: teardown, behind a synchronisation of the streams that used the block
    void release(muse_ctx *ctx)
    {
        pool_free(ctx, Host, p);
        p = nullptr;
        cap = 0;
    }
};
template <class T> using HostBuf = PoolBuf<T, true>;
// FFT lengths 2^17 ... 2^20 (xcorr_huge.hip, capi_huge.hip): twiddle tables per length, the work buffer of one batch of pairs,
// per-pair multiplier tables (two-sided xCorr), chunk sums / flags / tile maxima; grown on demand under muse_ctx::huge_mu
struct HugeWork {
    double2 *thi[4] = {nullptr, nullptr, nullptr, nullptr}, *tlo[4] = {nullptr, nullptr, nullptr, nullptr};
    PoolBuf<double2> Y, T;
    PoolBuf<double> part, snorm, sfin, sfin_x, amax;
    // the all-scores pass runs its batches on TWO streams alternately (the tail of one batch's kernels under the head of the
    // next one's): a second work buffer and tile-maximum buffer, the second stream, and the events that fork / join it
    PoolBuf<double2> Y2;
    PoolBuf<double> amax2;
    hipStream_t stream2 = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};
constexpr int64_t ZC_MIN_ROWS = 65536; // smaller groups are never cached: a pass over them is under 0.6 ms (the small-Run regime)
constexpr int ZC_MAX_SEGMENTS = 64;    // appends extend the cache by one segment each; beyond this many the tail stays on the rows
constexpr int PROBE_WINDOWS = 4096; // clock probe (muse_test_clock_probe_*): windows its pinned buffer holds; the window count and the stop flag sit behind them
struct muse_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // every kernel of the context
    hipStream_t copy_stream = nullptr; // host -> HBM uploads of muse_group_append: run beside a score pass
    int num_cus = 0;
    int64_t hbm = 0;
    char name[64] = {0};
    double2 *tw1 = nullptr, *tw2 = nullptr, *twm = nullptr;
    double2 *g2 = nullptr, *g3a = nullptr, *g3b = nullptr; // folded-twiddle tables (xcorr_r16_fold.hip)
    double2 *twl[3] = {nullptr, nullptr, nullptr};          // xcorr_long.hip (n = 16384, 32768, 65536): [4096] W_n^(m2), built on first use
    double2 *gsmall[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // the same for xcorr_small.hip: n = 512, 1024, 2048: [8][n/16]; n = 8192: [8][32] + [8][512]; n = 16384: [8][64] + [8][1024]
    double2 *wsplit = nullptr; // xcorr_real.hip: [15][1024] W_16384^(j k1) (FusedParams::wsplit)
    float2 *tw1f = nullptr, *tw2f = nullptr, *twmf = nullptr; // fp32 copies for the screening kernels
    // many-reference pass (muse_batch_score_many): parked spectra + device pointer tables
    // pinned staging buffers (32 MB each) lent to groups that receive many small appends; allocated once
    // (hipHostMalloc of 32 MB costs milliseconds) and returned when the group is released
    // work buffers of the generic / Stockham kernels for n >= 8192: one allocation per context, grown on demand
    // (every kernel that uses it runs on the context's single stream)
    PoolBuf<double2> gscratch;
    std::vector<double *> stage_pool;
    std::mutex stage_mu;
    PoolBuf<double2> zscratch; // [slots][4096] (upload_many_tab)
    PoolBuf<void *> many_tab;  // columns of R pointers ({xcp, mv, lag, ...}: upload_many_tab)
    std::vector<void *> many_host; // host image of many_tab (outlives the asynchronous copy)
    double screen_delta = 1e-4;
    // filter-and-refine Run (run_select), OPT-IN (muse_ctx_set_screening): 1 = Runs over large groups screen in fp32 and
    // re-evaluate in fp64 only the rows that can reach the top-N; 0 (default) = every Run scores all rows in fp64, the
    // arithmetic of the reference (xcorr.go:160-197)
    int screening = 0;
    // smaller groups: the plain fp64 pass is as fast (tools/screen_crossover.py: the crossover is at ~25 000 rows of 4096
    // samples).  Default: M * n >= 32768 * 4096 samples; an explicit row count (muse_ctx_set_screening(ctx, rows)) overrides.
    int64_t screen_min_rows = 0;
    double screen_e_scale = 1.0;     // test hook (muse_test_set_screen_bound_scale): scales the error bound, to exercise the guard
    int variant = 0;
    int xcorr_repeat = 1; // measurement hook (muse_test_xcorr_repeat)
    unsigned long long *dbg_stamps = nullptr; // diagnostic builds only (-DMUSE_REAL64_STAMPS): [CUs][16 waves][16 phases] cycle sums
    // measurement hook (muse_test_clock_probe_*): a one-wave kernel on its own stream sampling the shader clock
    hipStream_t probe_stream = nullptr;
    unsigned long long *probe_buf = nullptr; // pinned host memory: [2 * PROBE_WINDOWS] ticks + the window count behind them
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events, redo_events;
    double total_ms = 0.0, redo_ms = 0.0;
    int64_t launches = 0, redo_launches = 0;
    char pci[32] = {0}; // PCI bus id of the device ("0000:05:00.0"): tells two contexts on one GPU from two GPUs
    // muse_batch_run_rows (capi_rows.hip): idle slots (RowsSlot *) -- pinned staging, device rows, score buffers, a pinned
    // result record and an event each -- so that a Muse.Run allocates nothing in steady state
    MemPool dev_pool, host_pool;   // dmalloc / hmalloc
    HugeWork huge;                 // series longer than 65 536 samples
    int huge_batch_mb = 0;         // measurement hook (muse_test_huge_batch_mb): 0 = HUGE_BATCH_BYTES; negative: |mb| on ONE stream
    std::mutex huge_mu;
    std::mutex small_mu;           // small_free: the pinned record buffers of small Runs between batches (capi_run.hip)
    std::vector<std::pair<unsigned char *, int>> small_free; // (buffer, its capacity in slots)
    unsigned long long small_token = 0; // the stamp of the context's last small Run
    std::mutex timing_mu;          // events / redo_events (LaunchTimer::end from concurrent muse_batch_run_rows callers)
    std::atomic<bool> rows_always_copy{false}; // test hook (muse_test_rows_always_copy): never let a kernel read the pinned staging buffer
    std::vector<void *> rows_slots;
    std::mutex rows_mu;
    // spectrum cache of resident float64 groups at FFT length 4096 (muse_ctx_set_spectrum_cache; capi_batch.hip):
    // 0 = off, 1 = automatic.  zc_min_rows / zc_budget: test hooks (muse_test_spectrum_cache_limits; budget < 0 = half of the free HBM)
    std::atomic<int> zc_mode{1};
    std::atomic<int64_t> zc_min_rows{ZC_MIN_ROWS};
    std::atomic<int64_t> zc_budget{-1};
    std::atomic<int> zc_reader{0}; // test hook (muse_test_spectrum_cache_reader): 1 = the reader at four workgroups per CU
    std::atomic<int> win_rows_slices{0}; // test hook (muse_test_window_rows_slices): 0 = window_rows_plan; S >= 1 forces the slice count of the windowed Muse.Run
    std::atomic<bool> in_window_force{false}; // test hook (muse_test_in_window_force_transform): float64 windows <= MUSE_LAG_WINDOW_MAX of muse_batch_score_in_window take the masked transform kernels
    std::atomic<int> slide_in_window_force{0}; // test hook (muse_test_slide_in_window_force): 1 = muse_batch_slide_score_in_window never takes the fused n = 4096 kernel (TWO_STEP)
    std::atomic<bool> gather_nt{false}; // measurement hook (muse_test_gather_nontemporal): the row gather's stores bypass the caches
    // Handles may be released in any order (Go finalizers, Python GC): the
    // context lives until it is destroyed AND its last group/batch is freed.
    std::atomic<int> refs{1};
};

struct muse_group {
    std::atomic<int> refs{1}; // the handle itself + one per batch built on it
    muse_ctx *ctx = nullptr;
    double *rows = nullptr; // float64 storage (the default: what the reference holds)
    float *rows32 = nullptr; // float32 storage (muse_group_create_f32, opt-in): exactly one of the two is used
    bool f32 = false;
    size_t elem() const { return f32 ? sizeof(float) : sizeof(double); }
    void *base() const { return f32 ? (void *)rows32 : (void *)rows; }
    int64_t cap = 0, M = 0, stride = 0; // M counts staged rows too
    // FFT lengths above 65 536 (capi_huge.hip): the rows never change, so neither do a series' zNormalize statistics -- first sample,
    // mean of the shifted samples, 1 / sigma, flag per row, computed by the first pass that needs them and kept for every later Run
    // and every other reference (rows appended later are added; a re-allocation starts over)
    PoolBuf<double> hstats; // [cap][4]
    int64_t hstats_rows = 0;
    uint64_t rewrites = 0;          // how often rows already in the group were rewritten (muse_group_fill_synthetic, muse_group_slide: rows are otherwise immutable)
    // allocations the group has outgrown: kept until the group goes (kernels enqueued before the growth may still read them),
    // so that growing never waits for the device (group_reserve)
    std::vector<void *> retired;
    int32_t N = 0;
    // Appends that are small (Group.Add calls muse_group_append once per Series) are packed into two pinned staging buffers
    // borrowed from the context's pool and uploaded asynchronously on the context's copy stream: a piece goes out whenever
    // STAGE_FLUSH_BYTES have gathered (so the copies run beside the caller's next Adds), the buffers alternate when one is
    // full; kernels are ordered behind the copies through `uploaded`.
    double *stage[2] = {nullptr, nullptr};
    hipEvent_t stage_done[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t staged = 0;     // rows packed into stage[cur] (already counted in M)
    int64_t flushed = 0;    // of those, the rows whose upload is enqueued
    int64_t stage_rows = 0; // capacity of one staging buffer, in rows
    int small_appends = 0;  // the first small append goes straight to the device (Muse.Run: one upload per group)
    // an open window (muse_group_stage): the caller is filling rows [0, win_rows) of stage[cur] itself -- from any number of
    // threads -- and commits them piece by piece (muse_group_commit); they become rows [M, M + win_rows) of the group
    int64_t win_rows = 0, win_committed = 0;
    std::mutex win_mu;
    // uploads run on the context's copy stream; `uploaded` is recorded behind the last one enqueued and the compute stream
    // waits for it (hipStreamWaitEvent) before a kernel reads the rows: an append of NEW rows overlaps a running score pass
    hipEvent_t uploaded = nullptr;
    bool upload_pending = false;
    // the flush of the packed rows, upload_pending and the wait for `uploaded` (group_ready, and every caller that reads the
    // rows on a stream of its own: muse_batch_run_group_rows from any number of host threads)
    std::mutex ready_mu;
    // muse_group_append_from: the index list of the last gather into this group (pinned image and device copy), reused by the
    // next one once `gather_done` has passed
    HostBuf<long long> gidx_host;
    PoolBuf<long long> gidx_dev;
    hipEvent_t gather_done = nullptr;
    // muse_group_slide: the tails of the last slide -- two pinned halves the host packs (and narrows) into alternately, each
    // reused once its copy (`slide_copied`) has left it, and the dense count x k device image the kernel reads; kept for the next slide
    HostBuf<unsigned char> slide_host;
    PoolBuf<unsigned char> slide_dev;
    hipEvent_t slide_copied[2] = {nullptr, nullptr};
    // Spectrum cache (n = 4096, float64 rows; xcorr_r16_cached.hip): per pair of rows what the default kernel's first
    // half computes from the rows alone, kept for every later pass of every batch over the group.  Rows [0, zc_rows) are covered
    // (zc_rows even: a trailing single row's pair changes when a row is appended), in segments in pair order -- an append adds a
    // segment, nothing is rebuilt or moved.  Valid for the rows as they were after `zc_rewrites` rewrites.  All of it under ready_mu;
    // every kernel that writes or reads it runs on the context's compute stream, in the order it was enqueued under that lock.
    struct ZcSegment {
        void *mem = nullptr; // one block: zc[pairs][4096] double2, then zstat[pairs][ZC_STAT] double
        int64_t pair0 = 0, pairs = 0;
        double2 *zc() const { return (double2 *)mem; }
        double *zstat() const { return (double *)((char *)mem + (size_t)pairs * 4096 * sizeof(double2)); }
    };
    enum { ZC_NONE = 0, ZC_DECLINED = 1, ZC_VALID = 2 };
    std::vector<ZcSegment> zc_segs;
    int zc_state = ZC_NONE;
    int64_t zc_rows = 0, zc_bytes = 0;
    uint64_t zc_rewrites = 0;
    int64_t zc_passes = 0;       // eligible passes over the rows as they are (a group scored once pays nothing: the second one builds)
    int64_t zc_declined_M = -1;  // ZC_DECLINED: the row count that did not fit (asked again once it changes)
    bool transient = false;      // the slot groups of muse_batch_run_rows: other rows on every call, never cached
};

// The reference spectrum and the tables derived from it: shared (reference-counted) by the batches
// created with muse_batch_create_like -- Muse.Run builds one small group per call against ONE reference.
inline std::atomic<uint64_t> g_spectrum_serial{0}; // one per library: muse_spectrum::serial
struct muse_spectrum {
    std::atomic<int> refs{1};
    // never 0 and never handed out twice: what a cache of tables derived from the spectrum is keyed by (a freed spectrum's address
    // may come back with the next one; its serial does not) -- the window tables of a muse_batch_run_rows_windowed slot (capi_rows.hip)
    const uint64_t serial = g_spectrum_serial.fetch_add(1, std::memory_order_relaxed) + 1;
    double2 *X = nullptr, *xc = nullptr, *xcp = nullptr;
    double2 *xcw = nullptr; // n == 32768: FusedParams::xcw
    float2 *xcf = nullptr;
    double *xs = nullptr;
    double *c1 = nullptr; // n == 4096, N < 4096: indicator correlation (xcorr_r16_fast.hip, PADDED)
    double xmax = -1.0;   // max |X[f]| (lazily, by the first screened Run): scales the fp32 error bound
};

// The lags a window +-L holds below zero at FFT length n: index n / 2 is lag +n/2 (xcorr.go:192-194), it is scanned once
inline int window_lneg(int L, int n) { return 2 * L == n ? L - 1 : L; }
// A window of lags as every pass takes it at FFT length n: lags -lneg .. hi (hi <= n / 2, lneg <= n / 2 - 1), and `origin`, the lags
// below zero at which the direct product's table starts (row v of it is lag v - origin).  A table is determined by (origin, rows).
// A BAND (muse_batch_score_in_lag_band) is the same three numbers with lag 0 outside: lags lo .. hi with 0 < lo (lneg = -lo < 0) or
// hi < 0, origin = lneg = -lo, so rows() is its W = hi - lo + 1 and it is never every lag; what differs per pass asks band()
struct LagRange {
    int hi, lneg, origin;
    int rows() const { return origin + hi + 1; }
    bool every_lag(int64_t n) const { return 2 * (int64_t)hi == n && lneg == n / 2 - 1; }
    bool band() const { return hi < 0 || lneg < 0; }
    int lo() const { return -lneg; }
};
// the window +-L (muse_batch_set_lag_window, muse_batch_score_in_window): the table starts L lags below zero, at L == n / 2 too
// (where lag -n/2 is lag +n/2 and row 0 is not scanned)
inline LagRange lag_window_range(int64_t n, int64_t L)
{
    const int hi = (int)std::min<int64_t>(L, n / 2);
    return LagRange{hi, window_lneg(hi, (int)n), hi};
}
// the range lag_lo .. lag_hi (lag_lo <= 0 <= lag_hi; muse_batch_score_in_lag_range): the table starts at its lowest lag.  A range
// -L .. L is the window +-L, so the two are one pass bit for bit
inline LagRange clip_lag_range(int64_t n, int32_t lag_lo, int32_t lag_hi)
{
    if ((int64_t)lag_lo == -(int64_t)lag_hi)
        return lag_window_range(n, lag_hi);
    const int lneg = (int)std::min<int64_t>(-(int64_t)lag_lo, n / 2 - 1);
    return LagRange{(int)std::min<int64_t>(lag_hi, n / 2), lneg, lneg};
}

// the band lag_lo .. lag_hi (lag_lo <= lag_hi, lag 0 outside) clipped to -(n / 2 - 1) .. n / 2; false: nothing of it is left
inline bool clip_lag_band(int64_t n, int32_t lag_lo, int32_t lag_hi, LagRange *w)
{
    const int64_t hi = std::min<int64_t>(lag_hi, n / 2), lo = std::max<int64_t>(lag_lo, -(n / 2 - 1));
    if (lo > hi)
        return false;
    *w = LagRange{(int)hi, (int)-lo, (int)-lo};
    return true;
}

// lag_lo .. lag_hi clipped at FFT length n: the band where lag 0 is outside (false: nothing of it is left), the range otherwise
inline bool clip_band_or_range(int64_t n, int32_t lag_lo, int32_t lag_hi, LagRange *w)
{
    if (lag_lo <= 0 && lag_hi >= 0) { // (clipping moves neither bound across lag 0)
        *w = clip_lag_range(n, lag_lo, lag_hi);
        return true;
    }
    return clip_lag_band(n, lag_lo, lag_hi, w);
}

// Which pass filled a batch's mv / lag.  The in-window kinds carry the MUSE_IN_WINDOW_* value (muse_hip_test.h) they report.
struct ScoreOrigin {
    enum Kind : int32_t {
        PACKED_EACH = -2, // a packed launch of muse_batch_score_many_in_lag_bands whose members differ in range, band or sign (`tiles` tiles)
        PACKED = -1, // a packed launch of muse_batch_score_many_windowed (capi_window_many.hip) of `tiles` accumulator tiles
        OWN = 0,     // the batch's own setting: choose_kernel, or its own lag window (what the next muse_batch_score takes too)
        PLAIN = MUSE_IN_WINDOW_PLAIN, MFMA = MUSE_IN_WINDOW_MFMA, MASKED = MUSE_IN_WINDOW_MASKED // a call's window (`window`)
    };
    static constexpr int32_t MANY = -1; // `variant` of muse_batch_score_many_in_window's one masked pass (no KERNEL_* is negative)
    Kind kind = OWN;
    LagRange window{0, 0, 0}; // PLAIN / MFMA / MASKED: the call's window, clipped
    int32_t variant = 0; // MASKED: the KERNEL_* the pass launched first, or MANY
    int32_t tiles = 0;   // PACKED
    int32_t slide = 0;   // the MUSE_SLIDE_IN_WINDOW_* path if the pass was muse_batch_slide_score_in_window's and moved the rows, 0 otherwise
    int32_t sign = 0;    // MFMA / MASKED: +-1 if the pass was muse_batch_score_signed_in_lag_range's signed best match, 0 otherwise
    static ScoreOrigin packed(int32_t tiles) { return ScoreOrigin{PACKED, LagRange{0, 0, 0}, 0, tiles}; }
    static ScoreOrigin packed_each(int32_t tiles) { return ScoreOrigin{PACKED_EACH, LagRange{0, 0, 0}, 0, tiles}; }
    static ScoreOrigin in_window(int32_t path, const LagRange &w, int32_t variant = 0) { return ScoreOrigin{(Kind)path, w, variant}; }
    int32_t in_window_path() const { return kind > OWN ? (int32_t)kind : 0; }
    int32_t mfma_tiles() const { return (window.rows() + 15) / 16; } // MFMA: the accumulator tiles of the direct product
};

struct muse_batch {
    muse_ctx *ctx = nullptr;
    muse_group *g = nullptr;
    // the stream this batch's kernels and copies are enqueued on: the context's, except for the slot batches of
    // muse_batch_run_rows (capi_rows.hip), which own one each so that concurrent callers' kernels overlap
    hipStream_t own_stream = nullptr;
    hipStream_t stream() const { return own_stream ? own_stream : ctx->stream; }
    int32_t N = 0, n = 0, logn = 0;
    muse_spectrum *sp = nullptr; // owner of the five tables below (the pointers are copies)
    double *c1 = nullptr;
    double2 *X = nullptr, *xc = nullptr;
    double2 *xcp = nullptr; // n == 4096: xc in the lane order of xcorr_r16_fast.hip
    double2 *xcw = nullptr; // n == 32768: FusedParams::xcw (xcorr_real.hip)
    float2 *xcf = nullptr; // fp32 conj(X)/n (screening kernel)
    double *xs = nullptr;  // padded time-domain reference (exact re-evaluation)
    int *ovf_count = nullptr;
    // automatic kernel selection learns from the previous pass over the same (immutable) rows: the number of
    // pairs the default N = 4096 kernel handed to the rescaling kernel lands here (pinned, asynchronous copy)
    int *handoff_host = nullptr;
    int64_t handoff_M = -1;         // the rows the count was taken over: M of them, after handoff_rewrites rewrites of the group
    uint64_t handoff_rewrites = 0;
    PoolBuf<long long> ovf_list;
    PoolBuf<double> mv;
    PoolBuf<int> lag;
    // small Runs (launch_small_groups): small_cap slots of coherent pinned memory, handed back to the context on free
    unsigned char *small_out = nullptr;
    int small_cap = 0;
    // selection workspace
    PoolBuf<int> gid_dev;
    std::vector<int32_t> gid_host;
    bool gid_valid = false;
    PoolBuf<unsigned long long> gkey; // the GroupWork of the label-group reduction (gw())
    PoolBuf<long long> gfirst, gwin;
    GroupWork gw() const { return GroupWork{gkey.p, gfirst.p, gwin.p}; }
    PoolBuf<muse_record> rec;
    PoolBuf<unsigned long long> selkey;
    PoolBuf<muse_record> cand;
    PoolBuf<int> cnt;
    // pinned host images of cand / cnt: the device top-N pre-selection comes back in two truly asynchronous
    // copies and one synchronisation
    HostBuf<muse_record> cand_host;
    HostBuf<int> cnt_host;
    // pinned host images of rec / selkey: a Run over up to EXACT_FEED_MAX_GROUPS groups feeds the heap one Score per group
    HostBuf<muse_record> rec_host;
    HostBuf<unsigned long long> key_host;
    // filter-and-refine Run
    PoolBuf<unsigned> scr_flags;        // [M] SCR_* bits of the screening pass
    PoolBuf<double> scr_var;            // [M] sample variances from the screening pass
    PoolBuf<unsigned char> include;     // [M] rows re-evaluated in fp64 (the only ones the selection may take)
    PoolBuf<unsigned long long> scr_keys;
    PoolBuf<unsigned long long> scr_gmay, scr_gkplus; // label groups: per-group bounds
    PoolBuf<int> scr_gcert;
    int *refine_host = nullptr;         // pinned: pairs re-evaluated by the last screened Run
    PoolBuf<double> est_save;           // estimates of the listed rows (2 per pair), for the guard of the bound
    unsigned long long *err_dev = nullptr, *err_host = nullptr; // largest | |estimate| - |fp64 score| | of the last screened Run
    double last_E = 0.0;                // the bound that Run assumed
    // a screened Run with these filters over this many rows re-evaluated too many of them: the same Run is not
    // screened again (other filters on the same batch still are); a tripped guard switches the batch off for good
    struct RunKey {
        int64_t M = -1, G = 0;
        int32_t max_lag = 0, top_n = 0, sign_filter = 0, abs_scores = 0, grouped = 0;
        double threshold = 0.0;
        bool operator==(const RunKey &o) const
        {
            return M == o.M && G == o.G && max_lag == o.max_lag && top_n == o.top_n && sign_filter == o.sign_filter &&
                   abs_scores == o.abs_scores && grouped == o.grouped && threshold == o.threshold;
        }
    };
    RunKey costly_key;                  // (M = -1: none)
    bool guard_off = false;
    int32_t last_path = 0;              // MUSE_RUN_PATH_* of the last Run
    bool scores_exact = true;           // mv / lag hold fp64 results for every row (false after a screened Run)
    bool last_screened = false;         // the last Run took the filter-and-refine path
    int64_t guard_trips = 0;            // Runs redone in fp64 because an estimate left its bound
    uint64_t guard_salt = 0;            // varies the guard's row sample from Run to Run
    // lag window (muse_batch_set_lag_window, capi_window.hip): < 0 = off; otherwise every scoring pass takes xcorr_window.hip
    // with L = min(lag_window, n / 2).  win_e / win_pw: the shifted-reference image and its window sums of the window or lag range
    // win_key names (window_tables: built by the first pass that needs them; -1: none yet)
    int32_t lag_window = -1;
    int32_t win_key = -1;
    PoolBuf<double> win_e, win_pw;
    bool windowed() const { return lag_window >= 0; }
    // lag profiles (muse_batch_lag_profile, capi_profile.hip): the tables of the launch in flight (a sibling of win_e / win_pw with
    // no key: win_key and what it names stay as the scoring calls left them), the host form's staging rows, and the series list --
    // a pinned image and its device copy, the image reused once `prof_copied` has passed
    PoolBuf<double> prof_e, prof_pw, prof_out;
    HostBuf<long long> prof_idx_host;
    PoolBuf<long long> prof_idx;
    hipEvent_t prof_copied = nullptr;
    // which pass filled mv / lag (muse_batch_kernel_name names it, muse_test_last_in_window_path reports it): every scoring pass
    // assigns a whole value, a selection and a refused call leave it alone
    ScoreOrigin origin;
};

int use_device(muse_ctx *ctx);

// HIP-event bracket of ONE kernel launch on the context's stream (muse_ctx_kernel_timing): begin() right in front of the
// launch, end() right behind it; a bracket that never reaches end() (an error return in between) destroys its events.
struct LaunchTimer {
    muse_ctx *ctx;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool redo; // the bracket of the launches that redo listed pairs behind a fused launch (muse_ctx_redo_time)
    hipStream_t stream; // the stream the bracketed launch goes to
    explicit LaunchTimer(muse_ctx *c, bool redo_ = false, hipStream_t s = nullptr) : ctx(c), redo(redo_), stream(s ? s : c->stream) {}
    LaunchTimer(const LaunchTimer &) = delete;
    LaunchTimer &operator=(const LaunchTimer &) = delete;
    hipError_t begin()
    {
        if (!ctx->timing)
            return hipSuccess;
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess)
            e = hipEventCreate(&e1);
        if (e == hipSuccess)
            e = hipEventRecord(e0, stream);
        return e;
    }
    hipError_t end()
    {
        if (!e0 || !e1)
            return hipSuccess;
        const hipError_t e = hipEventRecord(e1, stream);
        if (e == hipSuccess) {
            std::lock_guard<std::mutex> lock(ctx->timing_mu); // (muse_batch_run_rows: any number of callers on one context)
            (redo ? ctx->redo_events : ctx->events).emplace_back(e0, e1);
            e0 = e1 = nullptr;
        }
        return e;
    }
    ~LaunchTimer()
    {
        if (e0)
            (void)hipEventDestroy(e0);
        if (e1)
            (void)hipEventDestroy(e1);
    }
};

// ---- helpers shared by the parts
void pool_drain(muse_ctx *ctx);                                            // frees every cached block (context teardown, tests)
template <class T> inline hipError_t dmalloc(muse_ctx *ctx, T **out, size_t bytes) { return pool_alloc(ctx, false, (void **)out, bytes); }
template <class T> inline hipError_t hmalloc(muse_ctx *ctx, T **out, size_t bytes) { return pool_alloc(ctx, true, (void **)out, bytes); }
inline void dfree(muse_ctx *ctx, void *p) { pool_free(ctx, false, p); }
inline void hfree(muse_ctx *ctx, void *p) { pool_free(ctx, true, p); }
void fill_twiddle(std::vector<double2> &v, size_t i, long long num, long long den);
void ctx_release(muse_ctx *ctx);                       // capi_context.hip: drops one reference, frees the context with the last
int group_ready(muse_group *g, hipStream_t stream = nullptr); // capi_group.hip: staged rows uploaded, the compute stream behind the copies
int group_ready_shared(muse_group *g, hipStream_t stream); // capi_group.hip: the same for a caller's own stream, any number of callers
// capi_group.hip: rows src[rows[i]] become rows [M, M + count) of dst, gathered on the copy stream (arguments checked by the
// caller; a float32 src into a float64 dst is widened)
int group_gather(muse_group *dst, muse_group *src, const int64_t *rows, int64_t count);
// capi_group.hip: the index-list checks both resident-row entry points share (MUSE_ERR_INVALID outside [0, src->M))
int check_row_list(const muse_group *src, const int64_t *rows, int64_t count);
void group_release(muse_group *g);
// capi_group.hip, the host side of a slide (muse_group_slide, muse_batch_slide_score_windowed): `count` rows' tails (k >= 1 samples
// each, arguments checked by the caller) packed and enqueued on the copy stream into g->slide_dev; and the invalidation of what
// described the rows from `first` on (rewrites++, hstats_rows)
int slide_upload_tails(muse_group *g, int64_t count, const double *tails, int32_t k, int64_t tail_stride);
void slide_invalidate(muse_group *g, int64_t first);
void rows_slots_free(muse_ctx *ctx);                   // capi_rows.hip: the idle slots of muse_batch_run_rows (streams idle)
int ilog2(int64_t n);                                  // capi_batch.hip
// capi_huge.hip: FFT lengths above GENERIC_MAX_N up to HUGE_MAX_N (xcorr_huge.h)
void huge_free(muse_ctx *ctx);
int huge_reference(muse_ctx *ctx, const double *ref_host, int N, int n, double2 *X, double2 *table, int *zero_std);
int huge_score(muse_batch *b);
int huge_pairs(muse_ctx *ctx, const double *xrows, int64_t xstride, int Nx, int normalize_x, double x_scale, const double *yrows,
               int64_t ystride, int Ny, int normalize_y, int64_t M, int n, double cc_scale, double *mv, int *lag, int *nil, double *cc);
void adopt_spectrum(muse_batch *b);                    // the batch's table pointers from its muse_spectrum
int build_spectrum(muse_ctx *ctx, const double *ref_host, int N, int n, int normalize, double x_scale,
                          double xc_scale, double2 *X, double2 *xc, float2 *xcf, double *xs, int *zero_std);
hipError_t ensure_gscratch(muse_ctx *ctx, int64_t n, int slices_per_cu = muse::GSCRATCH_SLICES_PER_CU);
hipError_t ensure_twl(muse_ctx *ctx, int64_t n);
int ensure_scores(muse_batch *b);
// slide != nullptr: the slide of the group's rows fused into the pass (muse_batch_slide_score_in_window, FUSED): the n = 4096 kernel reads the
// rows moved forward by slide->k samples (slide->tails: the group's device image of the tails) and stores them in place on the way; the
// caller has made sure of the kernel (batch_score_check: KERNEL_R16_FOLD) and keeps the spectrum cache out (allow_spectrum_cache false)
struct SlideFuse {
    const void *tails;
    int32_t k;
};
// What batch_score runs.  window == nullptr: the batch's own setting (its lag window if it has one, every lag otherwise).  Otherwise
// the pass is a call's and the batch's own window is neither read nor touched: `window` scored as `path` says -- MUSE_IN_WINDOW_PLAIN
// (it is every lag), _MFMA (the direct product) or _MASKED (the same launch sequence with the argmax of the transform kernels restricted
// to it: n = 512 ... 4096, the spectrum cache neither read nor touched)
struct ScorePass {
    bool allow_spectrum_cache = true; // (the many-references fallback passes false)
    const LagRange *window = nullptr;
    int32_t path = MUSE_IN_WINDOW_PLAIN;
    const SlideFuse *slide = nullptr;
    int32_t sign = 0; // MFMA / MASKED: +-1 = the signed best match inside the window (muse_batch_score_signed_in_lag_range), 0 = the best by magnitude
    const LagRange *mask() const { return window && path == MUSE_IN_WINDOW_MASKED ? window : nullptr; }
    bool direct() const { return window && path == MUSE_IN_WINDOW_MFMA; }
};
int batch_score(muse_batch *b, const ScorePass &pass); // capi_batch.hip: muse_batch_score is batch_score(b, {})
// what a call's pass through the transform kernels (every lag, or the argmax masked to *mask) would refuse for the batch as it stands
// (kernel selection, storage, length), without enqueueing anything; *variant = the KERNEL_* the pass would launch first (-1: none of
// them: a series longer than 65 536 samples)
int batch_score_check(muse_batch *b, const LagRange *mask, int *variant);
// the spectrum cache's policy, a pure host function: what a pass over `rows` rows of length N does about a cache
// that does not exist yet -- nothing, build one of *bytes for *rows_cached rows, or decline for lack of memory
enum { ZC_POLICY_NONE = 0, ZC_POLICY_BUILD = 1, ZC_POLICY_DECLINED = 2 };
int spectrum_cache_policy(int64_t rows, int32_t N, bool f32, int mode, int64_t min_rows, int64_t free_bytes, int64_t budget,
                          int64_t *rows_cached, int64_t *bytes);
void group_drop_spectrum_cache(muse_group *g);             // capi_batch.hip: frees the segments (ready_mu held, compute stream idle)
// capi_window.hip, what every caller of the lag-window kernels shares.  check_window_request: the refusals of a window of max_lag >= 0
// over b's reference (f32: the rows are float32 storage); window_tables: the shifted-reference image and its window sums of b for
// the window w in e / pw, once per (origin, rows) (cached under *key: -1 = none, both at most 127; a band's key carries bit 29 and its origin offset by 32768, so no
// two tables share a key; the caller drops it when the
// reference changes); window_params: the kernels' arguments for b's group and scores with those tables
int check_window_request(const muse_batch *b, int32_t max_lag, bool f32);
int window_tables(muse_batch *b, const LagRange &w, PoolBuf<double> &e, PoolBuf<double> &pw, int32_t *key, hipStream_t st);
muse::WindowParams window_params(const muse_batch *b, const LagRange &w, const double *e, const double *pw);
// the direct product over b's rows inside w, from b's own tables (device selected, rows uploaded, M > 0, mv / lag allocated); bracket:
// the launch under a LaunchTimer of its own
// sign: +-1 = the signed scan (launch_window_signed), 0 = the scan by magnitude
int score_direct(muse_batch *b, const LagRange &w, bool bracket = true, int sign = 0);
// The dispatch of every in-window entry point, a pure host function (MUSE_IN_WINDOW_*): which pass scores series of N samples (float32
// storage or not) inside w, a window clipped at the FFT length of N
int window_plan(int32_t N, bool f32, const LagRange &w, bool force_transform);
// the same for the signed best match (muse_batch_score_signed_in_lag_range): sign == 0 is window_plan; otherwise its MFMA and MASKED
// stand, and every lag (its PLAIN) is the masked pass with both bounds at their widest where the length has masked kernels
int signed_window_plan(int32_t N, bool f32, const LagRange &w, int sign, bool force_transform);
// a call's window over one batch: plan_in_window fills *pass with what batch_score is to run, or refuses (nothing enqueued, the batch
// unchanged); score_in_window plans, runs and names the pass
int plan_in_window(muse_batch *b, const LagRange &w, ScorePass *pass, int sign = 0);
int score_in_window(muse_batch *b, const LagRange &w, int sign = 0);
// the masked argmax of the transform kernels (their WIN builds): cc indices 0 .. hi and n - lneg .. n - 1 in the kernel's arguments;
// a band: the one interval lo .. hi, or n + lo .. n + hi below zero (their BAND builds; p.n is set)
inline void set_window(muse::FusedParams &p, const LagRange &w)
{
    p.win = 1;
    if (w.band()) {
        p.win_band = 1;
        p.win_a = w.hi < 0 ? p.n + w.lo() : w.lo();
        p.win_b = w.hi < 0 ? p.n + w.hi : w.hi;
        return;
    }
    p.win_lpos = w.hi;
    p.win_lneg = w.lneg;
}
// capi_window.hip: a call's lags lag_lo .. lag_hi against the batch's own window, which must be off or equal, i.e. L with -L .. L the
// call's (r: the batch's index in a list, -1: a single batch)
int check_own_window(const muse_batch *b, int32_t lag_lo, int32_t lag_hi, int r = -1);
// capi_window.hip, the band calls' own argument checks (a sign of -1 .. 1, lag_lo <= lag_hi) and the refusal of a band of which
// nothing is left inside the lags of FFT length n: shared by muse_batch_score_in_lag_band and muse_batch_score_many_in_lag_band
int check_band_args(int32_t lag_lo, int32_t lag_hi, int32_t sign);
int fail_empty_band(int32_t lag_lo, int32_t lag_hi, int64_t n);
// Results.MaxLag of a Run inside lag_lo .. lag_hi: max(-lag_lo, lag_hi), every lag of the range passes the lag filter
inline int32_t range_max_lag(int32_t lag_lo, int32_t lag_hi)
{
    return (int32_t)std::min<int64_t>(std::max<int64_t>(-(int64_t)lag_lo, lag_hi), INT32_MAX);
}
muse::FusedParams base_params(muse_batch *b);
int ensure_select_ws(muse_batch *b, int64_t M, int64_t G, bool with_gid, int K, bool on_device);
// the selection of a Run happens on the device (each chunk's best top_n) only beyond EXACT_FEED_MAX_GROUPS groups: capi_run.hip, run_select
inline bool select_on_device(int32_t top_n, int64_t G) { return top_n <= TOPN_DEVICE_MAX && G > EXACT_FEED_MAX_GROUPS; }
muse_batch::RunKey run_key(const muse_batch *b, const int32_t *group_id, int64_t G, int32_t max_lag, int32_t top_n,
                                  double threshold, int32_t sign_filter, int32_t abs_scores);
int32_t screen_path(const muse_batch *b, const muse_batch::RunKey &key, bool already_scored);
int score_screened(muse_batch *b, int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                          int32_t abs_scores, const int *gid_dev = nullptr, int64_t G = 0);
int upload_group_ids(muse_batch *b, const int32_t *group_id, int64_t M);
bool screen_guard_tripped(muse_batch *b);
int run_select(muse_batch *b, const int32_t *group_id, int32_t G_in, int64_t series_offset, int32_t max_lag,
                      int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                      std::vector<muse_record> &out, bool already_scored = false, bool prescreened = false);
void emit(const std::vector<muse_record> &sel, int64_t *out_series, int32_t *out_lag, double *out_score,
                 int32_t *out_count, double *out_mean_abs);
// the Run of a scored batch: run_select, then emit
int run_scored(muse_batch *b, const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
               int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs,
               bool prescreened = false);
// muse_batch_run_groups with `score(b, score_arg)` filling mv / lag in place of muse_batch_score (nullptr: muse_batch_score)
int run_groups(muse_batch *b, const int32_t *group_id, int32_t G, int64_t series_offset, int32_t abs_scores,
               muse_record *out_records, uint8_t *out_state, int (*score)(muse_batch *, const void *), const void *score_arg);
// capi_run.hip: the selection's own argument checks (run_select applies them; a wrapper that moves or scores first applies them before)
int check_select_args(const int32_t *group_id, int32_t G, int32_t sign_filter);
// ---- capi_many.hip, what the many-references entry points share
int upload_many_tab(muse_ctx *ctx, std::vector<void *> &tab, bool zscratch);
// the list checks: a list, no NULL, one context and one group, no batch twice
int check_batch_list(muse_batch *const *bs, int32_t R);
// which one-pass kernel family serves the list, a pure host decision (NONE: the batches are scored one after the other)
enum ManyKind { MANY_NONE, MANY_SMALL, MANY_MULTI, MANY_LONG, MANY_REAL };
ManyKind many_kind(muse_batch *const *bs, int32_t R);
// ONE pass of the `kind` kernels over the rows for every batch of a checked list; mask != nullptr: the argmax masked to it (SMALL at
// n <= 2048 and MULTI only); sign (with a mask): +-1 = the signed mask; a band mask and a sign reach the redo launches too
// (muse_batch_score_many_in_lag_band)
int score_many_pass(muse_batch *const *bs, int32_t R, ManyKind kind, const LagRange *mask, int sign = 0);
// every lag for a checked list: that one pass where a kernel family serves the list, batch_score(., each) batch after batch otherwise
int score_many_every_lag(muse_batch *const *bs, int32_t R, const ScorePass &each);
// batches of one group share N, and with it (muse_batch_create) the FFT length; a list that does not is scored reference by reference
inline bool one_length(muse_batch *const *bs, int32_t R)
{
    bool same = true;
    for (int r = 1; r < R; r++)
        same = same && bs[r]->N == bs[0]->N && bs[r]->n == bs[0]->n;
    return same;
}
// capi_window_many.hip: the direct product inside w for a checked list of float64 batches of one length with time-domain references,
// packed launches where the planner packs; alone: what names a reference that fills its launch alone; sign / a band w: the signed /
// band scan (muse_batch_score_many_in_lag_band)
int score_many_direct(muse_batch *const *bs, int32_t R, LagRange w, const ScoreOrigin &alone, int sign = 0);
// the Run of every batch of a scored list: run_select, then emit into row r of the caller's arrays
int run_many_select(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n,
                    double threshold, int32_t sign_filter, int32_t abs_scores, bool prescreened, int64_t *out_series,
                    int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
int screen_many(muse_batch *const *bs, int32_t R, const int32_t *group_id, int32_t G_in, int32_t max_lag,
                       int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores, bool &done);
