/*
 * muse_hip.h -- C ABI of libmuse_hip.so: the MI355X (gfx950) engine behind
 * go-muse's z-normalized cross-correlation hot path.
 *
 * The reference (aouyang1/go-muse, pure Go) has no FFI layer; the natural
 * seam is its exported batch API.  Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference).  The Go-side
 * cgo binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns MUSE_OK (0) or a negative
 *     muse_status; text for the last error on the calling thread comes from
 *     muse_last_error().
 *   - no caller pointer is retained after a call returns (cgo rule): uploads
 *     copy.  Caller data is never mutated (the reference's zNormalize mutates
 *     Series values in place, xcorr.go:86,93; this engine does not).
 *   - one context = one GPU.  Several contexts may live in one process, on
 *     different devices or on the same one: the host mirrors shard a Group
 *     over a list of contexts inside ONE process (one host thread per
 *     context: muse.hpp Engine::List, muse_hip.go SetDevices, muse.py
 *     Batch(engines=...)); under torch.distributed / RCCL it is one process
 *     and one context per GPU (go-muse_amd/dist.py).  A handle may be used
 *     from any host thread.  Calls on DIFFERENT group / batch handles of one
 *     context may be in flight at the same time (muse_test.go:203-214 drives
 *     one Muse from many goroutines: every Muse.Run owns its group and batch);
 *     at most one call per handle, at most one muse_batch_score_many /
 *     _run_many per context, and kernel timing (muse_ctx_kernel_timing) only
 *     with a single caller.  All work of a context runs on its one stream.
 *   - there is NO CPU fallback: every compute entry point fails with
 *     MUSE_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef MUSE_HIP_H
#define MUSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUSE_HIP_ABI_VERSION 5

typedef enum muse_status {
    MUSE_OK = 0,
    MUSE_ERR_INVALID = -1,     /* bad argument / NULL handle                      */
    MUSE_ERR_LENGTH = -2,      /* length mismatch: muse_batch.go:24-28, muse.go:68-70, group.go:45-51 */
    MUSE_ERR_ZERO_STD = -3,    /* "Invalid input query": sigma(ref)==0, muse_batch.go:39-41 */
    MUSE_ERR_NO_DEVICE = -4,   /* no usable gfx950 device                         */
    MUSE_ERR_HIP = -5,         /* a HIP runtime call failed                       */
    MUSE_ERR_UNSUPPORTED = -6, /* FFT length outside the built kernels (n > 65536) */
    MUSE_ERR_NOMEM = -7,
    MUSE_ERR_EMPTY = -8        /* empty reference: muse.go:24-26                  */
} muse_status;

/* SignFilter values: results.go:20-26 */
#define MUSE_SIGN_ANY 0
#define MUSE_SIGN_POS 1
#define MUSE_SIGN_NEG (-1)

typedef struct muse_ctx muse_ctx;
typedef struct muse_group muse_group;
typedef struct muse_batch muse_batch;

/* One top-N candidate as exchanged between shards. 24 bytes. */
typedef struct muse_record {
    int64_t series; /* global series (row) index of the group's winner */
    double score;   /* clamped score: |mv| (Batch) or signed mv (Muse)  */
    int32_t lag;
    int32_t group;  /* group id (or series index when ungrouped, truncated) */
} muse_record;

int muse_abi_version(void);
const char *muse_last_error(void);
const char *muse_status_string(int status);

/* ------------------------------------------------------------ context */
/* Streams, twiddle tables, scratch.  device = HIP device ordinal.      */
int muse_ctx_create(int32_t device, muse_ctx **out);
/* Number of usable (gfx950) devices, ordinals 0 .. count-1: a host that shards a Group over the GPUs of a node
 *  creates one context per device and one host thread per context. */
int muse_device_count(int32_t *count);
int muse_ctx_destroy(muse_ctx *ctx);
int muse_ctx_synchronize(muse_ctx *ctx);
/* A context keeps the device and pinned-host blocks its groups and batches hand back (by size class, at most 1 GB of HBM
 * and 192 MB of pinned memory) and gives them to the next group / batch of the same shape: a steady
 * NewGroup -> Add -> NewBatch -> Run -> free cycle then makes no hipMalloc / hipFree / hipHostMalloc (each a device-wide
 * synchronisation or hundreds of microseconds).  muse_ctx_trim returns every cached block to the system. */
int muse_ctx_trim(muse_ctx *ctx);
/* name: >= 64 bytes.  Any out pointer may be NULL. */
int muse_ctx_device_info(muse_ctx *ctx, char *name, int32_t name_cap,
                         int32_t *compute_units, int64_t *hbm_bytes);
/* PCI bus id of the context's device ("0000:05:00.0"; cap >= 16): what tells N contexts on N GPUs from N contexts on one
 * (the sharded Runs of SURVEY 8e report it per shard; bench.py prints it per rank). */
int muse_ctx_device_pci_bus_id(muse_ctx *ctx, char *out, int32_t cap);
/* Filter-and-refine Run: OPT-IN (off by default: every Run scores every series with the float64 kernel, the
 * arithmetic of the reference, xcorr.go:160-197).  enable = 1: Runs over groups of >= 32768 * 4096 samples after
 * padding, where it starts to pay; enable = n > 1: Runs over >= n series; 0: off.  When enabled, a muse_batch_run /
 * muse_batch_run_shard / muse_batch_run_many (with or without label groups) over that many series of length
 * 257 .. 65536 screens every series with an fp32 transform (a bound E on its error is derived from the reference's
 * spectrum), re-evaluates in fp64 exactly those rows whose optimistic selection key reaches the top_n-th best
 * pessimistic key, and selects among the re-evaluated rows only: the records returned are the ones the all-fp64 Run
 * returns (a run-time guard re-does the Run in fp64 if an estimate is found outside the bound).
 * muse_batch_read_scores after such a Run re-scores every row in fp64 first.
 * Not every Run can take it: muse_batch_run_groups and muse_batch_run_rows always score in float64, and the host mirrors'
 * Batch.Run goes through muse_batch_run_groups whenever it has at most 65 536 label groups (it feeds Results one Score per
 * group, the reference's own order among exactly tied scores) -- so with the mirrors screening only ever applies to Runs
 * over more label groups than that (Run(nil) over a large Group). */
int muse_ctx_set_screening(muse_ctx *ctx, int32_t enable);
/* Spectrum cache of resident groups: mode 1 (the default) = automatic, 0 = off.  Of what the default
 * kernel for FFT length 4096 computes per pair of series, the first half -- shift, sum of squares, forward transform --
 * depends on the group's rows alone.  A float64-storage group of series of length 2049 .. 4096 with at least 65 536 rows
 * that is scored a SECOND time (by any batch, against any reference) keeps that half in HBM: 64 KB + 128 B per pair of rows,
 * i.e. the group's footprint doubles, taken only if it fits in half of the device memory that is free at that moment.
 * Every later all-scores pass over the group reads the kept spectra instead of the rows: the same bytes, about half the
 * arithmetic, bit-identical scores and lags.  Every pass still scores every series; nothing of a Run's result is cached.
 * Rows appended later are added to the cache by the next pass; muse_group_slide and muse_group_fill_synthetic over existing rows drop it.
 * Mode 0 neither builds nor reads a cache (one that exists stays until muse_group_drop_spectrum_cache or muse_group_free). */
int muse_ctx_set_spectrum_cache(muse_ctx *ctx, int32_t mode);
/* Which path the last muse_batch_run / muse_batch_run_shard on this batch took: *screened = 1 for filter-and-refine,
 * *refined_pairs = pairs of series it re-evaluated in fp64.  Any out pointer may be NULL. */
int muse_batch_last_run_info(muse_batch *b, int32_t *screened, int64_t *refined_pairs);
/* ... and why: MUSE_RUN_PATH_FP64 (screening off or the Run not eligible), _SCREENED, _FP64_COSTLY (an earlier
 * screened Run with exactly these filters over these rows re-evaluated more than a quarter of the pairs: the plain
 * fp64 pass is cheaper for it; other filters on the same batch are still screened), _FP64_GUARD (an estimate was once
 * found outside the bound: the batch stays on the fp64 path). */
#define MUSE_RUN_PATH_FP64 0
#define MUSE_RUN_PATH_SCREENED 1
#define MUSE_RUN_PATH_FP64_COSTLY 2
#define MUSE_RUN_PATH_FP64_GUARD 3
int muse_batch_last_run_path(muse_batch *b, int32_t *path);
/* HIP-event timing of the fused kernel on the stream it is launched on:
 * enable, run, then read (sum of launch durations in ms, launch count). */
int muse_ctx_kernel_timing(muse_ctx *ctx, int32_t enable);
int muse_ctx_kernel_time(muse_ctx *ctx, double *total_ms, int64_t *launches);
/* The same for what muse_ctx_kernel_time leaves out: the launches that REDO the pairs a fused launch listed (a NaN / Inf
 * series, sigmas too far apart for one shared transform) with the kernel that isolates and rescales first -- one bracket per
 * pass (many references: one around the R redo launches).  Microseconds for an empty list, a second pass for a group of
 * mixed-unit series. */
int muse_ctx_redo_time(muse_ctx *ctx, double *total_ms, int64_t *brackets);
/* Name of the kernel automatic selection takes for this batch's all-scores pass (name: >= 64 bytes). */
int muse_batch_kernel_name(muse_batch *b, char *name, int32_t name_cap);

/* -------------------------------------------------------------- group */
/* Device-resident row-major M x N float64 comparison matrix; replaces the
 * per-Series []float64 storage behind Group.Add (group.go:31-56: one length
 * per group).  Never mutated by any run. */
int muse_group_create(muse_ctx *ctx, int64_t capacity_rows, int32_t N,
                      muse_group **out);
/* OPT-IN float32-STORAGE group: the rows are kept as float32 in HBM -- half the bytes the float64 group
 * streams per Run -- and widened exactly to float64 as the kernels consume them; all arithmetic stays float64.
 * muse_group_append narrows the caller's float64 samples (round to nearest) on the way in, so scores are those of
 * the reference applied to the ROUNDED inputs, not to the caller's: they no longer match the float64 reference to
 * 1e-6 in general (relative input perturbation 6e-8 per sample), which is why this is never the default.
 * Built for series of length 257 .. 16384 (FFT lengths 512 ... 16384: the float32-row loaders live in the kernels
 * automatic selection takes for them); MUSE_ERR_UNSUPPORTED otherwise.  Such a group works with muse_batch_create /
 * _score(s) / _run / _run_shard / _run_groups / _score_many (one pass per reference); the opt-in filter-and-refine
 * Run and the two-sided xCorr do not apply to it.  muse_group_read returns the stored values widened to float64. */
int muse_group_create_f32(muse_ctx *ctx, int64_t capacity_rows, int32_t N,
                          muse_group **out);
/* Appends count rows read from host memory (row_stride in doubles, >= N).
 * This is what Group.Add calls once per Series (count = 1) or per slab. */
int muse_group_append(muse_group *g, const double *rows, int64_t count,
                      int64_t row_stride);
/* The same without a staging copy inside the library (Group.Add "stages series into a C-allocated pinned
 * buffer"): muse_group_stage opens a WINDOW of pinned host memory for up to `count` more rows -- *granted <= count of them,
 * row-major, N doubles per row, at *window -- which the caller fills itself, from as many threads (goroutines) as it likes:
 * the copy out of the Series' own slices (series.go:20) is the only one the host makes.  muse_group_commit(first, k) hands
 * rows [first, first + k) of the window to the copy stream as soon as they are filled (any thread, any order, every row of
 * the window exactly once); the upload of the first pieces runs beside the filling of the later ones, and with the last
 * commit the rows join the group as rows [M, M + granted).  Two windows alternate: the next muse_group_stage returns while
 * the previous window is still crossing PCIe.  One window at a time per group; no other call on the group between
 * _stage and its last _commit.  float64 groups only (MUSE_ERR_UNSUPPORTED for float32-storage groups). */
int muse_group_stage(muse_group *g, int64_t count, double **window, int64_t *granted);
int muse_group_commit(muse_group *g, int64_t first, int64_t count);
/* Group.Add of series that already live in another group on the same context (go-muse's Group.Add keeps the caller's
 * slice, group.go:53, and FilterByLabelValues hands back the same *Series, group.go:60-71, so building a sub-group copies
 * nothing): rows src[rows[i]] become rows [M, M + count) of dst, in list order, copied HBM -> HBM (no host copy, nothing
 * crosses PCIe but the index list).  Duplicates and any order are allowed.  MUSE_ERR_INVALID for a NULL handle, count < 0,
 * an index outside [0, src's M), groups on different contexts, src == dst, different storage types (float32 / float64) or an
 * open staging window on either group; MUSE_ERR_LENGTH when the lengths differ.  Everything is checked before anything is
 * enqueued: on an error dst is unchanged.  count == 0 does nothing.  Asynchronous like muse_group_append: the gather runs on
 * the context's copy stream behind both groups' earlier uploads and in front of dst's later ones, and every later kernel
 * that reads dst waits for it; src may be freed right after the call.  Rows are taken as immutable once added: the
 * gather copies what src holds when it runs. */
int muse_group_append_from(muse_group *dst, muse_group *src, const int64_t *rows, int64_t count);
/* The rows follow time: rows [first, first + count) of g move forward by k samples -- row r becomes
 *   old row r [k .. N)  followed by  tails[(r - first) * tail_stride + 0 .. k)
 * in place in HBM (row_slide.hip); only count x k samples cross PCIe.  Both storage types and every N a group allows; a
 * float32-storage group narrows the tails with (float)x, exactly as muse_group_append narrows rows.  k == N replaces the rows
 * outright.  MUSE_ERR_INVALID -- everything is checked before anything is enqueued, the group is unchanged -- for a NULL group,
 * first < 0, count < 0, first + count > M, k < 0, k > N, tail_stride < k, NULL tails with count > 0 and k > 0, or an open
 * staging window.  k == 0 or count == 0 returns MUSE_OK and changes nothing (no cache is dropped).
 * `tails` is not retained after the call (as with muse_group_append).
 * Ordering: rows packed by earlier small appends are sent first.  The slide REWRITES rows that earlier work may still be
 * reading, so the call waits until the context's device is idle -- every stream: score passes, gathers that read this group,
 * muse_batch_run_group_rows calls in flight -- before its kernel is enqueued, and returns after the kernel has finished (as
 * muse_group_fill_synthetic does).  Calling it while other host threads are inside calls that read the same group is the
 * caller's error, as it is for muse_group_free.  The guard in front of row 0, the rows outside the range and the memory behind
 * row M are never written.
 * What describes the old rows goes with them: the group's spectrum cache is dropped by the next pass (muse_group_spectrum_cache
 * reports 0 rows right after the slide) and built again by the second pass over the new rows -- a group that slides between
 * every two passes never builds one --, the kept statistics of long series are recomputed from row `first` on, and automatic
 * kernel selection forgets what it learned from the old rows.  Scores a batch computed before the slide are those of the old
 * rows until its next scoring pass. */
int muse_group_slide(muse_group *g, int64_t first, int64_t count, const double *tails, int32_t k, int64_t tail_stride);
/* create + append in one call */
int muse_group_upload(muse_ctx *ctx, const double *rows, int64_t M, int32_t N,
                      int64_t row_stride, muse_group **out);
/* Fills rows [first, first+count) ON DEVICE with the rect+noise workload of
 * SURVEY 8d (after example_test.go:15-20), keyed by (seed, global row index =
 * global_first + local row, sample index): bench/test utility; rows become
 * part of the group (size grows to first+count if needed). ref_out (N doubles,
 * host, may be NULL) receives the reference series of the workload.
 * By default 1 row in 1024 is an exact copy of the reference (score 1, lag 0) and 1 in 1024 a constant row
 * (sigma == 0 path), as SURVEY 8d prescribes; flags switch either off (a workload whose top-N is NOT a tie
 * among copies). */
#define MUSE_SYNTH_NO_COPIES 1u
#define MUSE_SYNTH_NO_CONSTANTS 2u
int muse_group_fill_synthetic(muse_group *g, int64_t first, int64_t count,
                              int64_t global_first, uint64_t seed,
                              uint32_t flags, double *ref_out);
int muse_group_shape(muse_group *g, int64_t *M, int32_t *N);
/* D2H copy of rows [first, first+count) (dense, N doubles per row): lets a
 * checker feed byte-identical inputs to a CPU oracle. */
int muse_group_read(muse_group *g, int64_t first, int64_t count, double *out);
/* The group's spectrum cache (muse_ctx_set_spectrum_cache): *rows_cached = the rows [0, *rows_cached) the next pass reads
 * from it (0: none), *bytes = the HBM it holds.  Any out pointer may be NULL.  _drop waits for the passes enqueued so far and
 * gives the HBM back; under mode 1 a later second pass builds it again. */
int muse_group_spectrum_cache(muse_group *g, int64_t *rows_cached, int64_t *bytes);
int muse_group_drop_spectrum_cache(muse_group *g);
int muse_group_free(muse_group *g);

/* -------------------------------------------------------------- batch */
/* NewBatch (muse_batch.go:23-52) / New (muse.go:23-42): validates
 * N == group length (MUSE_ERR_LENGTH), n = nextPowOf2(N), reference spectrum
 * FFT(zeroPad(zNormalize(ref)/(N-1), n)) computed on the device and kept
 * resident.  MUSE_ERR_ZERO_STD when sigma(ref) == 0; MUSE_ERR_EMPTY when
 * N < 1.  ref is copied, not mutated.
 * Divergence: N == 1 is rejected with MUSE_ERR_INVALID.  The reference accepts it (New / NewBatch divide by
 * N - 1 = 0: every score is NaN and never passes Results.passed), so the observable outcome -- no scores -- is the
 * same, but here it is an error at creation instead of an empty result. */
int muse_batch_create(muse_ctx *ctx, muse_group *g, const double *ref,
                      int32_t N, muse_batch **out);
/* A batch for another group against the SAME reference: shares src's
 * spectrum tables (reference-counted), so it costs no transform and two
 * small allocations.  Muse.Run (muse.go:46-92) scores one small group per
 * call against the Muse's one reference: create the template once in New,
 * then one _create_like + _run + _free per call.  MUSE_ERR_LENGTH when the
 * group's length differs from the reference's (muse.go:68-70). */
int muse_batch_create_like(muse_batch *src, muse_group *g, muse_batch **out);
/* Muse.Run (muse.go:46-92) in ONE call: the M rows of one label group, read from host memory (row_stride in doubles,
 * >= the reference's length: MUSE_ERR_LENGTH otherwise, muse.go:68-70), are scored against tmpl's reference -- tmpl is the
 * batch New made once (muse_batch_create over an empty group); its own group is not touched -- and the group's winner comes
 * back as muse_batch_run_groups reports it for G = 1: *out_winner = the member with the largest |clamped score| among the
 * members whose score is a number (series = its row index, -1 if none; the first one on ties, muse.go:86), *out_state = 1
 * the first member's score is a number (out_winner is the Score Muse.Run passes to Results.Update), 2 the first member
 * scores NaN (x > NaN never replaces it: the group's score is NaN and never passes Results.passed), 0 for M = 0
 * (muse.go:47-50).  abs_scores = 0: signed score clamped to [-1, 1] (Muse.Run); 1: |score| clamped to 1 (a Batch of one
 * label group).  rows are copied before the call returns and never mutated.
 * One host -> HBM copy, the fused kernel of the length, one reduction kernel that writes the record into pinned host
 * memory, one event: no allocation, no free and no device-wide synchronisation in steady state (a pool of slots per
 * context); any number of host threads may call it on one tmpl at the same time (muse_test.go:203-214). */
int muse_batch_run_rows(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride,
                        int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
/* The same with one pointer per row (rows[r] -> the N samples of row r): the comparison series of a Muse.Run are separate
 * slices (muse.go:46, compGraphs []*Series), gathered here straight into the call's pinned buffer instead of being packed
 * by the caller first.  (cgo: an array of Go pointers may only cross when the slices are pinned, runtime.Pinner;
 * INTEGRATION.md keeps the packed form for Go.) */
int muse_batch_run_row_ptrs(muse_batch *tmpl, const double *const *rows, int64_t M,
                            int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
/* Muse.Run (muse.go:46-92) over rows that are already resident in a group on tmpl's context: as muse_batch_run_rows, with
 * row i of the label group = src row rows[i] (any order, duplicates allowed); out_winner->series is the position in `rows`.
 * No sample crosses PCIe: the rows are gathered into the call's device buffer (float32-storage groups widened exactly), or,
 * when `rows` is one ascending contiguous run of a float64 group, scored where they lie.  Validation as
 * muse_group_append_from (MUSE_ERR_INVALID / MUSE_ERR_LENGTH for a length other than the reference's).  Any number of host
 * threads may call it at once on one tmpl and one src; appending to src while such calls are in flight is not allowed. */
int muse_batch_run_group_rows(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M,
                              int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
int muse_batch_fft_len(muse_batch *b, int32_t *n);
/* The batch's x (muse_batch.go:47): n/2+1 complex128, interleaved re,im. */
int muse_batch_spectrum(muse_batch *b, double *out);
/* The hot loop of Batch.scoreSingle / Muse.Run (muse_batch.go:68-73,
 * muse.go:64-71): one fused kernel launch computes, for every series of the
 * group, exactly what xCorrWithX returns (xcorr.go:160-197) minus the cc
 * slice: lag and signed max value; sigma==0 series give (0, 0.0).  Results
 * stay on the device (asynchronous; see muse_ctx_synchronize). */
int muse_batch_score(muse_batch *b);
/* Lag window, OPT-IN (off for every new batch; muse_batch_create_like does not inherit it).  Today's Run applies
 * Results.MaxLag the way the reference does (results.go:46-52): a series whose best lag over ALL n lags lies outside
 * +-MaxLag is dropped.  With a window set, every scoring pass of this batch (muse_batch_score, _scores, _run,
 * _run_shard, _run_groups) instead returns per series the best match INSIDE the window: with cc[0 .. n-1] the slice
 * xCorrWithX computes (xcorr.go:160-187) and lag(i) = i if i <= n/2 else i - n, maxAbsIndex (xcorr.go:39-50) runs over
 * the indices with |lag(i)| <= L only, in ascending index order (0 .. L, then n-L .. n-1), same start values, same
 * strict '>': the first index wins ties, a window of zeros / NaN gives (0, cc[0]), a NaN / Inf series (0, NaN),
 * sigma == 0 (0, 0.0).  L = min(max_lag, n/2); with L = n/2 the result is the unwindowed one, and whenever the
 * unwindowed winner lies inside the window the windowed result is that same (lag, value).  The pass is a direct
 * matrix product on the fp64 matrix pipe (xcorr_window.hip), one read of the rows, no transform; it is never screened
 * (muse_batch_last_run_path: MUSE_RUN_PATH_FP64).
 *   max_lag < 0                      : off -- the transform kernels, bit for bit as if never set
 *   0 <= max_lag <= MUSE_LAG_WINDOW_MAX : on
 * MUSE_LAG_WINDOW_MAX is the widest window of the DIRECT PRODUCT, the one mechanism behind this setting and behind the _windowed
 * entry points below; wider windows, and windows over float32-storage groups, are muse_batch_score_in_window's.
 * MUSE_ERR_UNSUPPORTED, the batch unchanged: max_lag > MUSE_LAG_WINDOW_MAX (beyond a few dozen lags the direct product
 * costs more than the transform); a float32-storage group; series longer than 65536 samples.  A batch with a window is
 * refused (MUSE_ERR_UNSUPPORTED) by muse_batch_score_many / _run_many (muse_batch_score_many_windowed is their windowed form) and as the template of muse_batch_run_rows /
 * _run_row_ptrs / _run_group_rows (their _windowed forms below take the window as an argument).  muse_batch_lag_window reads the
 * setting back (-1 = off). */
#define MUSE_LAG_WINDOW_MAX 63
int muse_batch_set_lag_window(muse_batch *b, int32_t max_lag);
int muse_batch_lag_window(muse_batch *b, int32_t *max_lag);
/* Muse.Run (muse.go:46-92) INSIDE A LAG WINDOW, in one call.  Each behaves as its unwindowed namesake (muse_batch_run_rows,
 * _run_row_ptrs, _run_group_rows): same validation, same out_winner / out_state rules, same abs_scores, M == 0 gives state 0, the
 * same pool of slots, any number of host threads on one tmpl.  The only difference is the per-row (lag, mv): the windowed one defined
 * at muse_batch_set_lag_window, with L = min(max_lag, n/2).  The window is an argument of the call: no batch's own lag_window setting
 * is touched, and the three unwindowed entry points go on refusing a windowed template.  Everything behind the per-row pair is
 * unchanged (signed clamp or |.|, the first member attaining the maximum wins, a NaN first member gives state 2).
 * Refused, every handle left as it was: max_lag < 0, or a template whose own window is on and differs from max_lag
 * (MUSE_ERR_INVALID); max_lag > MUSE_LAG_WINDOW_MAX, or series longer than 65536 samples (MUSE_ERR_UNSUPPORTED).  A float32-storage
 * src is accepted by _run_group_rows_windowed (the gather widens exactly).
 * Numerics: few rows of long series are scored by kernels that split the samples of a row over several workgroups and sum the
 * partial products in a fixed order (xcorr_window_split.hip; deterministic: two calls give the same bits).  Where that split is
 * not taken (one slice), a row's (lag, mv) is BIT-IDENTICAL to muse_batch_set_lag_window + muse_batch_score over the same rows;
 * where it is, the summation tree differs, and the result equals the definition at the project's tolerance (1e-6 relative),
 * not the unsplit kernel's bit for bit. */
int muse_batch_run_rows_windowed(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride,
                                 int32_t max_lag, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
int muse_batch_run_row_ptrs_windowed(muse_batch *tmpl, const double *const *rows, int64_t M,
                                     int32_t max_lag, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
int muse_batch_run_group_rows_windowed(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M,
                                       int32_t max_lag, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
/* THE SLIDE AND THE WINDOWED PASS IN ONE KERNEL (xcorr_window_slide.hip): one read and one write of the rows where the two calls
 * below move them three times.  muse_batch_slide_score_windowed is equivalent to
 *   muse_group_slide(the batch's group, 0, M, tails, k, tail_stride)  followed by  a windowed all-scores pass with window max_lag:
 * afterwards the group holds the slid rows -- BIT FOR BIT those of muse_group_slide -- and muse_batch_read_scores returns, BIT FOR
 * BIT, what muse_batch_set_lag_window(max_lag) + muse_batch_score give over them.  The whole group always slides (a row range would
 * leave scores of mixed age); everything muse_group_slide says about ordering (the call waits until the device is idle and returns
 * after its kernel has finished), about `tails` and about what goes with the old rows (the spectrum cache, kept statistics, kernel
 * selection) holds here.  The window is an argument of the call, as with the other _windowed entry points: the batch's own
 * lag_window must be off or equal to max_lag and is not touched; the window's tables are kept for the next call.
 * k == 0 or M == 0 is not an error: nothing moves and nothing is invalidated (with M > 0 the call is the windowed pass alone).
 * Refused, every handle left as it was (everything is checked before anything is enqueued): a NULL batch, k < 0, k > N,
 * tail_stride < k, NULL tails with M > 0 and k > 0, an open staging window, max_lag < 0, or a batch whose own window is on and
 * differs from max_lag (MUSE_ERR_INVALID); max_lag > MUSE_LAG_WINDOW_MAX, a float32-storage group, or series longer than 65536
 * samples (MUSE_ERR_UNSUPPORTED).
 * muse_batch_slide_run_windowed is that call followed by Batch.Run's selection over the scores, outputs as muse_batch_run; max_lag
 * is both the window and the Results.MaxLag of the selection (as in muse_batch_run_many_windowed).  A sign_filter outside -1 .. 1
 * or a negative G with group_id is refused before anything moves. */
int muse_batch_slide_score_windowed(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride, int32_t max_lag);
int muse_batch_slide_run_windowed(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                                  const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                                  int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                                  double *out_score, int32_t *out_count, double *out_mean_abs);
/* THE WINDOW AS AN ARGUMENT, ANY WIDTH.  muse_batch_score_in_window is an all-scores pass whose per-series (lag, mv) is the
 * windowed one defined at muse_batch_set_lag_window, with L = min(max_lag, n/2) -- for every max_lag >= 0, not only up to
 * MUSE_LAG_WINDOW_MAX, and for float32-storage groups too.  The window is an argument of the call, as with the other _windowed
 * entry points: the batch's own lag_window must be off or equal to max_lag and is not touched.  Results land in the batch's score
 * buffers (muse_batch_read_scores); the pass is exact fp64 and never screened (muse_batch_last_run_path: MUSE_RUN_PATH_FP64).
 * Which pass runs is decided from the length, the storage and L alone:
 *   L == n/2 (the window is every lag), any length, any storage     : muse_batch_score's pass with the window off, bit for bit
 *   float64 group, L <= MUSE_LAG_WINDOW_MAX, up to 65536 samples     : the direct product, bit for bit muse_batch_set_lag_window(L) +
 *                                                                      muse_batch_score
 *   FFT length 512, 1024, 2048 or 4096 (256 < N <= 4096) and
 *   L > MUSE_LAG_WINDOW_MAX or a float32-storage group               : the transform kernels of muse_batch_score with their argmax
 *                                                                      restricted to the window (every cc[i] outside it is replaced
 *                                                                      by +0.0 in front of maxAbsIndex): the cost of the unwindowed
 *                                                                      pass, constant in L.  It always reads the rows: the group's
 *                                                                      spectrum cache is neither used, built nor counted towards.
 *   anything else (L > MUSE_LAG_WINDOW_MAX with N <= 256 or N > 4096,
 *   a float32-storage group outside 256 < N <= 4096)                 : MUSE_ERR_UNSUPPORTED, nothing changed
 * MUSE_ERR_INVALID, nothing changed: a NULL batch, max_lag < 0, a batch whose own window is on and differs from max_lag.
 * muse_batch_run_in_window is that pass followed by Batch.Run's selection over the scores, outputs as muse_batch_run; max_lag is
 * both the window and the Results.MaxLag of the selection (as in muse_batch_slide_run_windowed).  A sign_filter outside -1 .. 1 or
 * a negative G with group_id is refused before anything is scored. */
int muse_batch_score_in_window(muse_batch *b, int32_t max_lag);
int muse_batch_run_in_window(muse_batch *b, const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n,
                             double threshold, int32_t sign_filter, int32_t abs_scores, int64_t *out_series,
                             int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
/* ONE-SIDED AND ASYMMETRIC WINDOWS.  muse_batch_score_in_lag_range is an all-scores pass whose per-series (lag, mv) is the best
 * match inside the lags lag_lo .. lag_hi, lag_lo <= 0 <= lag_hi.  A negative lag means the series trails the reference, a positive
 * one that it leads it (xcorr.go:103), so (lag_lo, 0) and (0, lag_hi) answer two different questions; filtering the symmetric
 * window's answer afterwards loses every series whose strongest peak lies on the other side.  Definition, per series, with n the FFT
 * length, hi = min(lag_hi, n/2), lo = max(lag_lo, -(n/2 - 1)), cc[0 .. n-1] the slice xCorrWithX computes and lag(i) as at
 * muse_batch_set_lag_window: maxAbsIndex runs over the indices 0 .. hi and then n + lo .. n - 1 in ascending order (no wrapped
 * index when lo == 0), from (0, 0.0), with the strict '>' -- the first index wins ties, a window of zeros or NaN gives (0, cc[0]), a
 * NaN / Inf series (0, NaN), a series with sigma == 0 (0, 0.0): the rules of the symmetric window.  hi == n/2 with lo == -(n/2 - 1)
 * is every lag: the unwindowed result.  lag_lo == -lag_hi is by definition muse_batch_score_in_window(b, lag_hi), bit for bit on
 * every path.  Results land in the batch's score buffers (muse_batch_read_scores); the pass is exact fp64 and never screened
 * (muse_batch_last_run_path: MUSE_RUN_PATH_FP64); the batch's own lag_window must be off, or on with lag_lo == -lag_hi equal to it,
 * and is not touched.  Which pass runs is decided from the length, the storage and the W = hi - lo + 1 lags of the clipped range:
 *   the range is every lag, any length, any storage                  : muse_batch_score's pass with the window off, bit for bit
 *   float64 group, W <= 2 MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples : the direct product over a table that starts at lag lo: W lag
 *                                                                      rows, ceil(W / 16) accumulator tiles (a one-sided window
 *                                                                      half those of the symmetric one, and up to 126 lags wide).
 *                                                                      The value at a lag has the bits the symmetric window's
 *                                                                      direct product gives at that lag
 *   FFT length 512, 1024, 2048 or 4096, W wider or float32 storage   : the transform kernels with their argmax restricted to the
 *                                                                      range (the two bounds set independently); always reads the
 *                                                                      rows: the group's spectrum cache is neither used, built
 *                                                                      nor counted towards
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * MUSE_ERR_INVALID, nothing changed (everything is checked before anything is enqueued; the scores of the last pass stay): a NULL
 * batch, lag_lo > 0 or lag_hi < 0 (a range that excludes lag 0: the (0, cc[0]) fallback needs index 0), a batch whose own window is
 * on and is not this range.
 * muse_batch_run_in_lag_range is that pass followed by Batch.Run's selection over the scores, outputs as muse_batch_run, with
 * Results.MaxLag = max(-lag_lo, lag_hi): every lag of the range passes the lag filter.  A sign_filter outside -1 .. 1 or a negative
 * G with group_id is refused before anything is scored.
 * Limits: ranges that exclude lag 0 (muse_batch_score_in_lag_band below scores them); the slide forms of a range (the Muse.Run-rows
 * forms: muse_batch_run_rows_in_lag_range below);
 * the multi-device layer; ranges of more than 127 lags, or float32 storage, outside FFT lengths 512 ... 4096; series longer than
 * 65536 samples (other than the whole range); narrow float64 ranges are never routed to the masked pass. */
int muse_batch_score_in_lag_range(muse_batch *b, int32_t lag_lo, int32_t lag_hi);
int muse_batch_run_in_lag_range(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                                int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                                int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
/* THE SIGNED BEST MATCH.  muse_batch_score_signed_in_lag_range is muse_batch_score_in_lag_range with the argmax restricted to the
 * values of one sign: sign = MUSE_SIGN_POS "where does the series move WITH the reference most", MUSE_SIGN_NEG "where AGAINST it".
 * The reference takes each series' argmax of |cc| and drops the series when the winner has the wrong sign (results.go:46-52): a
 * series whose anti-correlated peak is the larger one by magnitude is lost to a SignFilter_POS caller, because its positive peak
 * was never reported -- no filter brings it back.  Here the argmax is restricted instead of its answer filtered.  Definition, per
 * series, with n, lo, hi, cc[0 .. n-1] and the scan order exactly as at muse_batch_score_in_lag_range (indices 0 .. hi, then
 * n + lo .. n - 1):
 *   sign == MUSE_SIGN_ANY : by definition muse_batch_score_in_lag_range(b, lag_lo, lag_hi), bit for bit on every path, its
 *                           every-lag and MUSE_ERR_UNSUPPORTED outcomes included
 *   sign == MUSE_SIGN_POS : the scan starts from (0, 0.0) and takes index i when cc[i] > best (strict): the first index wins ties,
 *                           only values > 0 can win, a NaN never wins
 *   sign == MUSE_SIGN_NEG : takes i when -cc[i] > -best
 *   no value of the requested sign inside the range : (lag 0, mv +0.0) -- not cc[0], which would have the wrong sign; the selection's
 *                           sign filter (score > 0, score < 0) then drops the series, as it drops sigma == 0 rows
 *   a series with sigma == 0 : (0, 0.0);  a NaN / Inf series : (0, NaN), as the unsigned pass gives
 * Invariant: whenever the unsigned in-range winner has the requested sign, the signed result is that same (lag, value).
 * Which pass runs, for sign != 0 (W = hi - lo + 1 the lags of the clipped range):
 *   float64 group, W <= 2 MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples : the direct product of muse_batch_score_in_lag_range with the
 *                                                                      signed scan (key cc or -cc in place of |cc|): the same cc bits
 *   FFT length 512, 1024, 2048 or 4096, W wider or float32 storage   : the transform kernels' masked argmax with the sign in the mask
 *                                                                      (a value inside the range that has not the sign becomes +0.0
 *                                                                      in front of the unchanged maxAbsIndex), both storages
 *   the range is every lag, FFT length 512, 1024, 2048 or 4096       : the same masked kernels with both bounds at their widest
 *                                                                      ("the best positive match at any lag"); reads the rows
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * Results land in the batch's score buffers; the pass is exact fp64, never screened, and never uses, builds or counts towards the
 * group's spectrum cache; the batch's own lag_window rule is muse_batch_score_in_lag_range's.  MUSE_ERR_INVALID, nothing changed:
 * that call's cases, and a sign outside -1 .. 1.
 * muse_batch_run_signed_in_lag_range is that pass followed by Batch.Run's selection, outputs as muse_batch_run_in_lag_range:
 * sign_filter is both the argmax's sign and the selection's Results.SignFilter (as max_lag is both the window and Results.MaxLag of
 * muse_batch_run_in_window), Results.MaxLag = max(-lag_lo, lag_hi).  A label group's maximum is then taken over its members' best
 * values OF THE SIGN: a group whose first-by-magnitude member has the wrong sign is no longer dropped whole.  sign_filter == 0 is
 * muse_batch_run_in_lag_range.
 * Limits: the slide forms, the Muse.Run rows forms, the muse_batch_set_lag_window setting (a batch's own
 * window is unsigned), the multi-device and dist.py layers; signed passes where the table above says MUSE_ERR_UNSUPPORTED (every
 * lag, more than 127 lags or float32 storage outside FFT lengths 512 ... 4096). */
int muse_batch_score_signed_in_lag_range(muse_batch *b, int32_t lag_lo, int32_t lag_hi, int32_t sign);
int muse_batch_run_signed_in_lag_range(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                                       int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                                       int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
/* LAG BANDS: the best match inside lags lag_lo .. lag_hi that NEED NOT HOLD LAG 0 -- "which series lead the reference by 1 .. k
 * samples", "between 200 and 230 samples behind".  A range [0, k] answers another question: every co-moving series peaks at lag 0 or
 * next to it, lag 0 wins the argmax, and no later filter recovers the best lag inside 1 .. k.  Definition, per series, with n,
 * cc[0 .. n-1] and lag(i) as at muse_batch_score_in_lag_range; the band is clipped to hi = min(lag_hi, n/2),
 * lo = max(lag_lo, -(n/2 - 1)):
 *   lo <= 0 <= hi : by definition muse_batch_score_signed_in_lag_range(b, lag_lo, lag_hi, sign), bit for bit on every path, its
 *                   every-lag and MUSE_ERR_UNSUPPORTED outcomes included; no kernel of the bands runs
 *   0 < lo <= hi  : the scan runs over the indices lo .. hi in ascending order
 *   lo <= hi < 0  : the scan runs over the indices n + lo .. n + hi in ascending order
 * On both one-sided bands the scan starts from (0, 0.0) and uses strict '>', so the first index wins: sign == MUSE_SIGN_ANY compares
 * |cc[i]|, MUSE_SIGN_POS compares cc[i] (only values > 0 can win), MUSE_SIGN_NEG compares -cc[i] (only values < 0); a NaN never wins.
 *   nothing wins (the band holds only zeros or NaN, or no value of the sign) : (lag 0, mv +0.0) for every sign -- index 0 is not in the
 *                   band, so cc[0] is not an answer: the signed pass's "none" outcome
 *   a series with sigma == 0 : (0, 0.0);  a NaN / Inf series : (0, NaN), as everywhere else
 * Which pass runs for a band that excludes lag 0 (W = hi - lo + 1; such a band is never "every lag"):
 *   float64 group, W <= 2 MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples : the direct product over a table whose row v is lag lo + v:
 *                                                                      W rows, ceil(W / 16) accumulator tiles wherever the band lies
 *                                                                      (xcorr_window_band_mfma); the value at a lag has the bits
 *                                                                      muse_batch_score_in_lag_range's direct product gives there
 *   FFT length 512, 1024, 2048 or 4096, W wider or float32 storage   : the transform kernels with the argmax masked to the one index
 *                                                                      interval, the sign in the mask (their band builds)
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * Results land in the batch's score buffers; the pass is exact fp64, never screened, and never uses, builds or counts towards the
 * group's spectrum cache.  MUSE_ERR_INVALID, nothing changed (everything is checked before anything is enqueued): a NULL batch,
 * lag_lo > lag_hi, a band that is empty after clipping ((100, 226) at n = 64), a sign outside -1 .. 1, a batch whose own lag window
 * is on (unless the band is the symmetric range equal to it, as the range call allows).
 * muse_batch_run_in_lag_band is that pass followed by Batch.Run's selection, outputs as muse_batch_run_in_lag_range, with
 * Results.MaxLag = max(|lag_lo|, |lag_hi|); sign_filter is both the argmax's sign and the selection's filter, as in
 * muse_batch_run_signed_in_lag_range; the selection's own argument checks come first.
 * Limits: the Muse.Run rows and panels forms, the slide forms, the muse_batch_set_lag_window setting, the
 * multi-device and dist.py layers; bands where the table above says MUSE_ERR_UNSUPPORTED (more than 127 lags or float32 storage
 * outside FFT lengths 512 ... 4096, series longer than 65536 samples). */
int muse_batch_score_in_lag_band(muse_batch *b, int32_t lag_lo, int32_t lag_hi, int32_t sign);
int muse_batch_run_in_lag_band(muse_batch *b, const int32_t *group_id, int32_t G, int32_t lag_lo, int32_t lag_hi,
                               int32_t top_n, double threshold, int32_t sign_filter, int32_t abs_scores,
                               int64_t *out_series, int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
/* Muse.Run (muse.go:46-92) INSIDE A LAG RANGE of up to MUSE_RUN_ROWS_LAG_RANGE_MAX lags, in one call.  Each behaves as its _windowed
 * namesake (muse_batch_run_rows_windowed, _run_row_ptrs_windowed, _run_group_rows_windowed): same validation, same out_winner /
 * out_state rules, same abs_scores, M == 0 gives state 0, the same pool of slots, any number of host threads on one tmpl; a
 * float32-storage src is accepted by the _group_rows_ form, and groups too large for a slot take the same general path.  The only
 * difference is the per-row (lag, mv): the one defined at muse_batch_score_in_lag_range -- its clipping (hi = min(lag_hi, n/2),
 * lo = max(lag_lo, -(n/2 - 1))), its scan order (0 .. hi, then n + lo .. n - 1), its start values, strict '>' and outcome rules.  The
 * range is an argument of the call: the template's own lag_window must be off, or on with lag_lo == -lag_hi equal to it, and is not
 * touched.  Which pass runs is decided from M, N, the CUs of the device and the W = hi - lo + 1 lags of the clipped range:
 *   the range is every lag                     : the unwindowed namesake's pass, bit for bit (this row comes first: the _windowed
 *                                                forms keep the window kernels where +-max_lag covers every lag, n <= 126)
 *   W <= 127, up to 65536 samples              : the kernels of the _windowed forms over a table that starts at lag lo (unsplit, or
 *                                                split over the samples for few rows of long series); lag_lo == -lag_hi IS the
 *                                                _windowed call, bit for bit.  Unsplit, the value at a lag has the bits of
 *                                                muse_batch_score_in_lag_range's direct product over the same rows
 *   128 <= W <= 2048, up to 65536 samples      : the panel kernels (xcorr_window_panels.hip): the table cut into ceil(W / 128) panels
 *                                                of 128 lags, one workgroup per (16 rows, slice of the samples, panel), the panels
 *                                                merged by scan position.  2 M N W flops: few rows are what makes it cheap.  In one
 *                                                slice the value at a lag has the bits the direct product gives there; in several,
 *                                                the definition at the project's tolerance (1e-6 relative).  Two calls give the
 *                                                same bits
 *   anything else                              : MUSE_ERR_UNSUPPORTED, nothing changed
 * MUSE_ERR_INVALID, every handle left as it was (everything is checked before anything is enqueued): lag_lo > 0 or lag_hi < 0, a
 * template whose own window is on and is not this range, and the namesakes' own argument errors.
 * Limits: the slide form of a range; more than 2048 lags; ranges that exclude lag 0 (a resident group: muse_batch_score_in_lag_band);
 * series longer than 65536 samples (other than
 * every lag); float32 host rows; the multi-device layer. */
#define MUSE_RUN_ROWS_LAG_RANGE_MAX 2048   /* the most lags (hi - lo + 1, after clipping) a Muse.Run range may hold */
int muse_batch_run_rows_in_lag_range(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride,
                                     int32_t lag_lo, int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
int muse_batch_run_row_ptrs_in_lag_range(muse_batch *tmpl, const double *const *rows, int64_t M,
                                         int32_t lag_lo, int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
int muse_batch_run_group_rows_in_lag_range(muse_batch *tmpl, muse_group *src, const int64_t *rows, int64_t M,
                                           int32_t lag_lo, int32_t lag_hi, int32_t abs_scores, muse_record *out_winner, uint8_t *out_state);
/* THE SLIDE AND THE PASS OF ANY WINDOW IN ONE CALL.  muse_batch_slide_score_in_window is equivalent to
 *   muse_group_slide(the batch's group, 0, M, tails, k, tail_stride)  followed by  muse_batch_score_in_window(b, max_lag):
 * afterwards the group holds the slid rows -- BIT FOR BIT those of muse_group_slide -- and muse_batch_read_scores returns, BIT FOR
 * BIT, what muse_batch_score_in_window(max_lag) gives over them; max_lag >= n/2 is the unwindowed pass (the reference's own scoring).
 * Any window width and both storage types.  How the rows move is decided from the length, the storage and the window:
 *   float64 group, L <= MUSE_LAG_WINDOW_MAX, up to 65536 samples     : muse_batch_slide_score_windowed's kernel (one read, one write)
 *   FFT length 4096 (2048 < N <= 4096), any other window or storage  : the default transform kernel reads the new rows -- old row[k..N)
 *                                                                      and the tails -- and writes them back in place while it scores
 *                                                                      them: one read and one write of the rows instead of a read and
 *                                                                      a write for the slide and a read for the pass
 *   every other length both calls support                            : muse_group_slide's kernel and then the pass, inside the one
 *                                                                      call (one upload of the tails, one wait for the device)
 * Everything muse_group_slide says about ordering (the call waits until the device is idle and returns after its kernels have
 * finished), about `tails` and about what goes with the old rows holds here; the whole group always slides.  The pass is exact fp64
 * (muse_batch_last_run_path: MUSE_RUN_PATH_FP64) and always reads the rows: the group's spectrum cache is neither used, built nor
 * counted towards.  k == 0 or M == 0 is not an error: nothing moves and nothing is invalidated (with M > 0 the call is
 * muse_batch_score_in_window alone).  Refused with the codes of muse_batch_slide_score_windowed's slide arguments and of
 * muse_batch_score_in_window, every handle, the rows and the scores of the last pass left as they were (everything is checked before
 * anything is enqueued).
 * muse_batch_slide_run_in_window is that call followed by Batch.Run's selection over the scores, outputs as muse_batch_run; max_lag
 * is both the window and the Results.MaxLag.  muse_batch_slide_run is the reference's Run on the slid rows: the unwindowed pass (the
 * scoring of max_lag = n/2 above; the batch's own lag window must be off), then the selection with Results.MaxLag = max_lag -- the
 * records of muse_group_slide + muse_batch_run with screening off.  In both, a sign_filter outside -1 .. 1 or a negative G with
 * group_id is refused before anything moves. */
int muse_batch_slide_score_in_window(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride, int32_t max_lag);
int muse_batch_slide_run_in_window(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                                   const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                                   int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                                   double *out_score, int32_t *out_count, double *out_mean_abs);
int muse_batch_slide_run(muse_batch *b, const double *tails, int32_t k, int64_t tail_stride,
                         const int32_t *group_id, int32_t G, int32_t max_lag, int32_t top_n, double threshold,
                         int32_t sign_filter, int32_t abs_scores, int64_t *out_series, int32_t *out_lag,
                         double *out_score, int32_t *out_count, double *out_mean_abs);
/* muse_batch_score + D2H of the per-series results (lag[M], mv[M]). */
int muse_batch_scores(muse_batch *b, int32_t *lag, double *mv);
/* Batch.Run + Results.Update + Results.Fetch (muse_batch.go:99-130,
 * results.go:46-87); abs_scores = 0 gives the Muse.Run post-processing
 * (muse.go:72-90: signed score clamped to [-1,1], group max by |score|).
 *   group_id : host int32[M], label-group of each series in [0,G), or NULL =
 *              every series its own group (Run(nil) with distinct labels).
 *              Groups are fed to Results in group-id order; inside a group the
 *              first series (lowest index) wins ties (muse_batch.go:87).
 *   outputs  : up to top_n entries in Fetch order (descending |score|),
 *              out_series = index of each group's winning series;
 *              *out_mean_abs = mean |score| (NaN when empty, results.go:86). */
int muse_batch_run(muse_batch *b, const int32_t *group_id, int32_t G,
                   int32_t max_lag, int32_t top_n, double threshold,
                   int32_t sign_filter, int32_t abs_scores,
                   int64_t *out_series, int32_t *out_lag, double *out_score,
                   int32_t *out_count, double *out_mean_abs);
/* Sharded form of the same run: this context holds rows
 * [series_offset, series_offset + M) of a larger group and every label group
 * lives on ONE shard.  Returns this shard's top-N candidates (<= top_n
 * records, descending |score|); the host gathers the records of all shards
 * (RCCL all_gather of top_n * 24 B per rank) and passes them to
 * muse_merge_records.  group ids are global. */
int muse_batch_run_shard(muse_batch *b, const int32_t *group_id, int32_t G,
                         int64_t series_offset, int32_t max_lag, int32_t top_n,
                         double threshold, int32_t sign_filter,
                         int32_t abs_scores, muse_record *out_records,
                         int32_t *out_count);
/* Final Results.Update/Fetch over gathered shard candidates (host only, no
 * GPU): records in any order; they are fed to the top-N heap in group order. */
int muse_merge_records(const muse_record *records, int64_t count, int32_t top_n,
                       int64_t *out_series, int32_t *out_lag, double *out_score,
                       int32_t *out_count, double *out_mean_abs);
/* Sharded Run whose label groups may STRADDLE shards ("... or the per-group partial maxima are merged
 * before top-N"; e.g. Run(["graph"]) over a Group whose graphs are interleaved, cut into contiguous row ranges): every
 * shard reports, per label group and unfiltered, its winner among the members whose score is a number
 * (out_records[g].series = global index, -1 if none) and out_state[g] = 0 no member on this shard / 1 members, the first
 * one's score is a number / 2 the first member's score is NaN (muse_batch.go:87: x > NaN never replaces it, so a group
 * whose FIRST member overall scores NaN yields NaN).  G records and states per shard; group ids are global and
 * required (ungrouped Runs are exact with muse_batch_run_shard). */
int muse_batch_run_groups(muse_batch *b, const int32_t *group_id, int32_t G,
                          int64_t series_offset, int32_t abs_scores,
                          muse_record *out_records, uint8_t *out_state);
/* The per-group part of that merge alone (host only): records / state hold n_shards x G entries, shard-major, shards in
 * ascending row order; out_records[g] = the group's winner (the first shard with a member decides the NaN rule, the maximum by
 * |score| wins, the earlier shard on ties: muse_batch.go:87), out_state[g] = 0 the group has no member / 1 out_records[g] is its
 * Score / 2 its first member scores NaN, so its score is NaN.  This is what a host feeds through Results.Update, one Score per
 * label group in group order (muse_batch.go:124-128), to reproduce the reference's heap HISTORY and with it the order among
 * exactly tied scores -- also into a Results that earlier Runs have filled (results.go:55-72).  n_shards = 1 turns one
 * muse_batch_run_groups result into that feed. */
int muse_merge_group_winners(const muse_record *records, const uint8_t *state,
                             int32_t n_shards, int32_t G,
                             muse_record *out_records, uint8_t *out_state);
/* Merge of those per-shard records (host only): records / state hold n_shards x G entries, shard-major, shards in
 * ascending row order.  Per group: the first shard with a member decides the NaN rule, the maximum by |score| wins
 * (the earlier shard on ties: muse_batch.go:87 keeps the earlier series); then Results.passed, the top-N heap and
 * Fetch exactly as muse_merge_records. */
int muse_merge_group_records(const muse_record *records, const uint8_t *state,
                             int32_t n_shards, int32_t G, int32_t max_lag,
                             int32_t top_n, double threshold, int32_t sign_filter,
                             int64_t *out_series, int32_t *out_lag, double *out_score,
                             int32_t *out_count, double *out_mean_abs);
/* Many references against one resident group (the
 * README.md:10-13 use case iterates references and groupings over a fixed
 * set of series, i.e. one NewBatch + Run per reference against the same
 * Group).  The R batches must share the context and the group; each is
 * scored exactly as muse_batch_score would, but in ONE pass over the rows:
 * every pair of series is read and forward-transformed once and correlated
 * against all R reference spectra (FFT lengths 512 ... 16384, i.e.
 * 256 < N <= 16384, from two references on; FFT lengths 32768 and 65536 from
 * three references on: the row spectra stay in the workgroup's scratch slice
 * and every reference takes product, second transform and argmax from there;
 * float32-storage groups: FFT length 4096; shorter series and forced kernel
 * variants score the batches one after the other).  Results land in each
 * batch's own buffers (muse_batch_scores / _run on a batch re-score it). */
int muse_batch_score_many(muse_batch *const *batches, int32_t R);
/* Copies back the (lag, signed mv) of the last scoring pass WITHOUT re-scoring
 * (muse_batch_scores = muse_batch_score + this). */
int muse_batch_read_scores(muse_batch *b, int32_t *lag, double *mv);
/* muse_batch_score_many followed by Batch.Run's selection for every batch
 * with the same grouping and Results settings: outputs are R consecutive
 * blocks of top_n entries (out_series[r*top_n + i], ...), out_count[r] and
 * out_mean_abs[r] per reference.  Any output may be NULL. */
int muse_batch_run_many(muse_batch *const *batches, int32_t R,
                        const int32_t *group_id, int32_t G, int32_t max_lag,
                        int32_t top_n, double threshold, int32_t sign_filter,
                        int32_t abs_scores, int64_t *out_series,
                        int32_t *out_lag, double *out_score,
                        int32_t *out_count, double *out_mean_abs);
/* Many references INSIDE A LAG WINDOW in one pass over the rows: per batch and series the best match inside +-L,
 * L = min(max_lag, n/2), exactly as defined at muse_batch_set_lag_window -- but the window is an argument of the call, applied
 * to this pass only: no batch's own lag_window setting is changed, and every later pass of a batch is what it was before.  The
 * windows of the references are packed, reference after reference, into the A rows of one fp64 matrix product
 * (xcorr_window_many.hip: up to 128 (reference, lag) rows and a fixed budget of staged reference images per launch), so that
 * narrow windows share the accumulator tiles a single reference leaves empty and the rows are read once per launch; references
 * that do not fit one launch go to consecutive launches, and from 2 max_lag + 1 > 48 on (a window that fills four tiles by itself
 * is bound by the matrix pipe: packing two measured no faster) every reference has a launch of its own, the single-reference kernel's.  For every batch, mv and lag are BIT-IDENTICAL to muse_batch_set_lag_window(b, max_lag) +
 * muse_batch_score(b) on that batch alone, so a caller may switch between the two forms freely.  The pass is never screened
 * (muse_batch_last_run_path: MUSE_RUN_PATH_FP64) and never touches the spectrum cache.
 *   The list is checked as muse_batch_score_many checks it (one context, one group, no duplicate, no NULL: MUSE_ERR_INVALID);
 *   max_lag < 0, or a batch whose own window is on and differs from max_lag: MUSE_ERR_INVALID;
 *   max_lag > MUSE_LAG_WINDOW_MAX, a float32-storage group, series longer than 65536 samples: MUSE_ERR_UNSUPPORTED.
 * Every refusal leaves the handles as they were.  (muse_batch_score_many / _run_many go on refusing a batch with a window.) */
int muse_batch_score_many_windowed(muse_batch *const *batches, int32_t R, int32_t max_lag);
/* muse_batch_score_many_windowed followed by Batch.Run's selection for every batch, outputs as muse_batch_run_many;
 * max_lag is both the window and the Results.MaxLag of passed() (which every windowed score passes). */
int muse_batch_run_many_windowed(muse_batch *const *batches, int32_t R, const int32_t *group_id, int32_t G,
                                 int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                 int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                 int32_t *out_count, double *out_mean_abs);
/* Many references INSIDE A LAG WINDOW OF ANY WIDTH in one pass over the rows: per batch and series the (lag, mv) of
 * muse_batch_score_in_window(b, max_lag), L = min(max_lag, n/2) -- the window an argument of the call, one window for every
 * reference, no batch's own lag_window changed.  Which pass runs is decided from the length, the storage, L and R:
 *   L == n/2 (the window is every lag)                               : muse_batch_score_many, bit for bit
 *   float64 group, L <= MUSE_LAG_WINDOW_MAX, up to 65536 samples     : muse_batch_score_many_windowed, bit for bit
 *   FFT length 512, 1024, 2048 or 4096 (256 < N <= 4096), L >
 *   MUSE_LAG_WINDOW_MAX or a float32-storage group, R >= 2, and
 *   muse_batch_score_many's own one-pass conditions (FFT length 4096
 *   on either storage, 512 ... 2048 on float64; automatic kernel
 *   selection; the correction tables where N < 4096)                 : ONE pass of the many-references transform kernels -- every pair
 *                                                                      of series read and forward-transformed once -- with every
 *                                                                      reference's argmax restricted to the window (cc[i] outside
 *                                                                      it replaced by +0.0 in front of maxAbsIndex); pairs the
 *                                                                      FFT length 4096 kernel lists (NaN / Inf, sigmas far apart)
 *                                                                      are redone per reference with the same window.  Lags are
 *                                                                      those of muse_batch_score_in_window, scores agree to
 *                                                                      rounding (the arithmetic is muse_batch_score_many's)
 *   the same lengths where those conditions do not hold (R == 1,
 *   float32 storage below FFT length 4096, ...)                      : muse_batch_score_in_window(b, max_lag) batch after batch
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * The pass is exact fp64, never screened (muse_batch_last_run_path: MUSE_RUN_PATH_FP64), and neither reads, builds nor counts
 * towards the group's spectrum cache.  A kernel variant forced by a test hook that has no masked build is refused
 * (MUSE_ERR_UNSUPPORTED), never run unmasked.
 *   The list is checked as muse_batch_score_many checks it (one context, one group, no duplicate, no NULL: MUSE_ERR_INVALID);
 *   max_lag < 0, or a batch whose own window is on and differs from max_lag: MUSE_ERR_INVALID.
 * Every refusal leaves the handles as they were.
 * muse_batch_run_many_in_window is that pass followed by Batch.Run's selection for every batch, outputs as muse_batch_run_many;
 * max_lag is both the window and the Results.MaxLag of the selection (as in muse_batch_run_many_windowed).  A sign_filter outside
 * -1 .. 1 or a negative G with group_id is refused before anything is scored. */
int muse_batch_score_many_in_window(muse_batch *const *batches, int32_t R, int32_t max_lag);
int muse_batch_run_many_in_window(muse_batch *const *batches, int32_t R, const int32_t *group_id, int32_t G,
                                  int32_t max_lag, int32_t top_n, double threshold, int32_t sign_filter,
                                  int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                  int32_t *out_count, double *out_mean_abs);
/* Many references INSIDE A LAG RANGE in one pass over the rows: per batch and series the (lag, mv) of
 * muse_batch_score_in_lag_range(b, lag_lo, lag_hi) -- its definition, clipping, scan order and (0, cc[0]), NaN and sigma == 0
 * outcomes -- one range for every reference, lag_lo <= 0 <= lag_hi, no batch's own lag_window touched.  lag_lo == -lag_hi is by
 * definition muse_batch_score_many_in_window(batches, R, lag_hi).  Which pass runs is decided from the length, the storage, R and
 * the W = hi - lo + 1 lags of the clipped range:
 *   the range is every lag                                           : muse_batch_score_many, bit for bit
 *   float64 group, W <= 2 MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples : the direct product.  Up to 48 lags the references' W table
 *                                                                      rows are packed into the accumulator tiles of one launch
 *                                                                      (at most 128 rows: sixteen references at -7 .. 0 where +-7
 *                                                                      packs eight); wider ranges, and batches that do not share
 *                                                                      one length, take one launch per reference.  Per batch BIT
 *                                                                      FOR BIT muse_batch_score_in_lag_range, whose cached tables
 *                                                                      the pass shares
 *   FFT length 512 ... 4096 otherwise, R >= 2, and muse_batch_score_many's
 *   own one-pass conditions (as at muse_batch_score_many_in_window)  : ONE pass of the many-references transform kernels with every
 *                                                                      reference's argmax restricted to the range, the two bounds
 *                                                                      set independently; listed pairs are redone with the range
 *   the same lengths where those conditions do not hold              : muse_batch_score_in_lag_range(b, lag_lo, lag_hi) batch after batch
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * Exact fp64, never screened, the group's spectrum cache neither read nor built.  A kernel variant forced by a test hook that has no
 * masked build is refused (MUSE_ERR_UNSUPPORTED), never run unmasked.
 *   MUSE_ERR_INVALID: the list checks of muse_batch_score_many; lag_lo > 0 or lag_hi < 0; a batch whose own window is on (unless
 *   lag_lo == -lag_hi equals it).  Everything is checked before anything is enqueued: a refusal leaves every batch's scores and
 *   cached tables as they were.
 * muse_batch_run_many_in_lag_range is that pass followed by Batch.Run's selection for every batch, outputs as muse_batch_run_many,
 * with Results.MaxLag = max(-lag_lo, lag_hi).  A sign_filter outside -1 .. 1 or a negative G with group_id is refused before anything
 * is scored.
 * Limits: one range per reference; ranges that exclude lag 0 (muse_batch_score_many_in_lag_band below scores them); the multi-device
 * layer. */
int muse_batch_score_many_in_lag_range(muse_batch *const *batches, int32_t R, int32_t lag_lo, int32_t lag_hi);
int muse_batch_run_many_in_lag_range(muse_batch *const *batches, int32_t R, const int32_t *group_id, int32_t G,
                                     int32_t lag_lo, int32_t lag_hi, int32_t top_n, double threshold, int32_t sign_filter,
                                     int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                     int32_t *out_count, double *out_mean_abs);
/* Many references INSIDE A LAG BAND OR UNDER A SIGN in one pass over the rows: per batch and series the (lag, mv) of
 * muse_batch_score_in_lag_band(b, lag_lo, lag_hi, sign) -- its clipping, its ascending scan with strict '>', its key |cc| / cc / -cc
 * and its outcomes: (0, +0.0) where nothing wins, (0, 0.0) for sigma == 0, (0, NaN) for a NaN / Inf series -- one band and one sign
 * for every reference, no batch's own lag_window touched.  "What led each of my eight open alerts by 1 .. 15 samples", "what moved
 * WITH each of them".  sign == MUSE_SIGN_ANY with lag_lo <= 0 <= lag_hi is by definition muse_batch_score_many_in_lag_range (and so,
 * for lag_lo == -lag_hi, muse_batch_score_many_in_window), bit for bit on every path.  Otherwise, with W = hi - lo + 1 the lags of
 * the clipped band:
 *   float64 group, W <= 2 MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples : the direct product with the signed / band scan.  Up to 48 lags
 *                                                                      the references' W table rows are packed into the accumulator
 *                                                                      tiles of one launch (xcorr_window_many_signed_mfma: eight
 *                                                                      references at 1 .. 7 are 56 rows, four tiles), wherever the
 *                                                                      band lies; wider bands, and batches that do not share one
 *                                                                      length, take one launch per reference.  Per batch BIT FOR BIT
 *                                                                      muse_batch_score_in_lag_band, whose cached tables it shares
 *   FFT length 512 ... 4096 otherwise (every lag under a sign too), R >= 2, and muse_batch_score_many's own one-pass conditions (as at
 *   muse_batch_score_many_in_window: either storage at 4096, float64 below) : ONE pass of the many-references transform kernels with every
 *                                                                      reference's argmax masked to the band, the sign in the mask
 *                                                                      (xcorr_fused_n4096_fold_multi_band, xcorr_fused_small_many_band);
 *                                                                      listed pairs are redone with the band and the sign
 *   the same lengths where those conditions do not hold              : muse_batch_score_in_lag_band(b, lag_lo, lag_hi, sign) batch after batch
 *   anything else                                                    : MUSE_ERR_UNSUPPORTED, nothing changed
 * Exact fp64, never screened, the group's spectrum cache neither read nor built.  A kernel variant forced by a test hook that has no
 * masked build is refused (MUSE_ERR_UNSUPPORTED), never run unmasked.
 *   MUSE_ERR_INVALID: the list checks of muse_batch_score_many; lag_lo > lag_hi; a sign outside -1 .. 1; a band that is empty after
 *   clipping; a batch whose own window is on (unless the band is the symmetric range equal to it).  Everything is checked before
 *   anything is enqueued: a refusal leaves every batch's scores and cached tables as they were.
 * muse_batch_run_many_in_lag_band is that pass followed by Batch.Run's selection for every batch, outputs as muse_batch_run_many,
 * with Results.MaxLag = max(|lag_lo|, |lag_hi|); sign_filter is both the argmax's sign and the selection's filter, as in
 * muse_batch_run_in_lag_band; the selection's own argument checks come first.
 * Limits: one band and one sign per list; the Muse.Run rows and slide forms; the multi-device and dist.py layers. */
int muse_batch_score_many_in_lag_band(muse_batch *const *batches, int32_t R, int32_t lag_lo, int32_t lag_hi, int32_t sign);
int muse_batch_run_many_in_lag_band(muse_batch *const *batches, int32_t R, const int32_t *group_id, int32_t G,
                                    int32_t lag_lo, int32_t lag_hi, int32_t top_n, double threshold, int32_t sign_filter,
                                    int32_t abs_scores, int64_t *out_series, int32_t *out_lag, double *out_score,
                                    int32_t *out_count, double *out_mean_abs);
/* Many references, EACH INSIDE ITS OWN LAG BAND AND UNDER ITS OWN SIGN, in one pass over the rows: batch r is left exactly as
 * muse_batch_score_in_lag_band(batches[r], lag_lo[r], lag_hi[r], sign[r]) leaves it -- scores, lags, what muse_batch_kernel_name and
 * muse_test_last_in_window_path report -- and no batch's own lag_window is touched.  "What led alert A by 1 .. 7 samples, what
 * trailed alert B by up to 7, what moved against alert C inside +-3": (1, 7) / ANY, (-7, 0) / ANY, (-3, 3) / NEG, 15 + 8 + 7 table
 * rows in two accumulator tiles of one launch.  sign == NULL: MUSE_SIGN_ANY for every reference.
 *   the whole list shares one (lag_lo, lag_hi, sign)    : muse_batch_score_many_in_lag_band, bit for bit and kernel for kernel
 *   batches of one length, the references the single dispatch sends to the direct product (float64 group, at most
 *   2 MUSE_LAG_WINDOW_MAX + 1 lags after clipping, up to 65536 samples) : cut into launches in list order -- a reference of more than
 *                                                         48 lags has a launch to itself; the others join the open launch until one
 *                                                         more would pass 128 packed table rows or the launch's staged images their
 *                                                         LDS budget.  A launch whose members differ: xcorr_window_many_each_mfma,
 *                                                         every reference's shape, sign and image offset in a descriptor table in
 *                                                         device memory; one whose members share range and sign: the uniform packed
 *                                                         kernel of muse_batch_score_many_in_lag_band; a reference alone in its launch:
 *                                                         the single-reference kernel, named as the single call names it.  Per batch
 *                                                         BIT FOR BIT muse_batch_score_in_lag_band, whose cached tables it shares
 *   every other reference (more lags, float32 storage, every lag under a sign), and lists of mixed length : its own single pass, behind
 *                                                         the packed launches
 * Exact fp64, never screened, asynchronous; results land in each batch's own buffers.
 *   MUSE_ERR_INVALID: the list checks of muse_batch_score_many; NULL lag_lo / lag_hi; at any index lag_lo > lag_hi, a sign outside
 *   -1 .. 1, a band that is empty after clipping, a batch whose own window is on (unless the band is the symmetric range equal to it).
 *   MUSE_ERR_UNSUPPORTED: what the single call refuses for a reference that is not on the direct product.  Everything is checked
 *   before anything is enqueued: a refusal leaves every batch's scores and cached tables as they were.
 * muse_batch_run_many_in_lag_bands is that pass followed by Batch.Run's selection for every batch: batch r with Results.MaxLag =
 * max(|lag_lo[r]|, |lag_hi[r]|), top_n[r], threshold[r] and sign_filter[r], which is both the argmax's sign and the selection's filter,
 * as in muse_batch_run_in_lag_band (NULL: MUSE_SIGN_ANY).  Row r of out_series / out_lag / out_score starts at out_stride * r;
 * out_stride < top_n[r] at any index, NULL top_n / threshold: MUSE_ERR_INVALID.  The selection's own argument checks come first.
 * Limits: the masked many-references transform kernels take one mask per pass (those references take their single passes); the list is
 * packed in the order given; the Muse.Run rows, panels and slide forms; the multi-device and dist.py layers. */
int muse_batch_score_many_in_lag_bands(muse_batch *const *batches, int32_t R, const int32_t *lag_lo, const int32_t *lag_hi,
                                       const int32_t *sign);
int muse_batch_run_many_in_lag_bands(muse_batch *const *batches, int32_t R, const int32_t *group_id, int32_t G,
                                     const int32_t *lag_lo, const int32_t *lag_hi, const int32_t *top_n, const double *threshold,
                                     const int32_t *sign_filter, int32_t abs_scores, int32_t out_stride, int64_t *out_series,
                                     int32_t *out_lag, double *out_score, int32_t *out_count, double *out_mean_abs);
/* LAG PROFILES: the correlation itself, not its argmax.  For output row k, out[k * out_stride + v] = cc[(lag_lo + v) mod n],
 * v = 0 .. W - 1, W = lag_hi - lag_lo + 1: the slice xCorrWithX computes for that series against the batch's reference (xcorr.go:160-197),
 * n the FFT length.  series == NULL: every series of the group in order (K must be 0 or M); otherwise K host indices in 0 .. M - 1, any
 * order, duplicates allowed, output row k belonging to series[k].  The values are raw -- no clamp to +-1, no sign filter, no
 * threshold; a series with sigma == 0 gives a row of +0.0 and one that holds NaN or Inf a row of NaN (the rules of every lag-window
 * pass).  Columns W .. out_stride - 1 are never written.
 *   The pass is the direct product of muse_batch_score_in_lag_band with its scan replaced by a write-out (xcorr_window_profile.hip):
 *   the value at a lag is BIT FOR BIT the one the band, range and signed passes scan at that lag on the direct product, whatever band
 *   it was asked in.  More than 2 MUSE_LAG_WINDOW_MAX + 1 lags: consecutive launches of up to that many, each one read of the rows
 *   writing its own columns (muse_test_lag_profile_plan).  The tables of a launch are built into buffers of the call's own (a sibling
 *   of the cached window tables): the batch's score buffers, what names their pass, its own lag window, its cached window tables with
 *   their key and the spectrum cache are left as they were.
 *   muse_batch_lag_profile writes host memory and returns when the data is there.  It stages through a grow-on-demand device buffer
 *   in chunks of rows: at most MUSE_LAG_PROFILE_STAGE_BYTES of device memory however many rows are asked for.
 *   muse_batch_lag_profile_device writes caller-owned device memory of the batch's context (a torch tensor's data_ptr()); it is
 *   enqueued on the batch's stream like a score pass and does not wait.
 *   MUSE_ERR_INVALID: a NULL batch or output; lag_lo > lag_hi; a lag outside -(n / 2 - 1) .. n / 2 (the band calls clip, this one
 *   does not: clipping would change which column is which lag); out_stride < W; K < 0, series == NULL with K neither 0 nor M, an
 *   index outside 0 .. M - 1.  MUSE_ERR_UNSUPPORTED: a float32-storage group, series longer than 65536 samples, a batch without its
 *   time-domain reference (where the direct product is refused everywhere).  Everything is checked before anything is enqueued or
 *   written.  K == 0 with a list, or an empty group: MUSE_OK, nothing written. */
#define MUSE_LAG_PROFILE_STAGE_BYTES (64LL << 20)
int muse_batch_lag_profile(muse_batch *b, const int64_t *series, int64_t K, int32_t lag_lo, int32_t lag_hi, double *out,
                           int64_t out_stride);
int muse_batch_lag_profile_device(muse_batch *b, const int64_t *series, int64_t K, int32_t lag_lo, int32_t lag_hi, double *dev_out,
                                  int64_t out_stride);
int muse_batch_free(muse_batch *b);

/* ------------------------------------------- single-pair entry points */
/* xCorrWithX as exercised by xcorr_test.go:204-286: ref and y of length N,
 * FFT length n (any n >= N; n need not be a power of two -- then a direct
 * O(n^2) device kernel is used).  cc (n doubles, may be NULL) receives the
 * full correlation.  Returns MUSE_OK with *is_nil = 1 (lag 0, mv 0) where
 * the reference returns (nil, 0, 0). */
int muse_xcorr_with_x(muse_ctx *ctx, const double *ref, const double *y,
                      int32_t N, int32_t n, double *cc, int32_t *lag,
                      double *mv, int32_t *is_nil);
/* xCorr (xcorr.go:102-153): n is raised to max(n, lenx, leny); cc holds that
 * many doubles.  n is used as given (not rounded up: the reference transforms any length): powers of two up to 2^20 run
 * the batched kernels; any other n up to 8192 the direct kernel; any other n up to 2^19 is folded out of the correlation at
 * a power of two L >= 2 n, where nothing wraps around (cc_n[k] = r[k] + r[k - n]; the fold and the argmax run on the host). */
int muse_xcorr(muse_ctx *ctx, const double *x, int32_t lenx, const double *y,
               int32_t leny, int32_t n, int32_t normalize, double *cc,
               int32_t *lag, double *mv, int32_t *is_nil);
/* xCorr (xcorr.go:102-153) for M independent pairs in ONE launch: pair i = (row i of gx, row i of gy).
 * The two groups may hold series of different lengths (each is zero-padded on its own, xcorr.go:129-130); n is raised
 * to max(n, Nx, Ny) (xcorr.go:104-106).  Powers of two 2^17 ... 2^20 run the long-series kernels (xcorr_huge.hip: one series
 * per transform, every x its own multiplier table).  FFT lengths 512 ... 65536 that are powers of two run the batched kernels, in two
 * forms: n <= 4096 and n = 65536 -- z = (x read backwards) + i y, one forward transform, cc = Im FFT(Z^2) / 2n on the xCorrWithX
 * kernels' transforms (xcorr_small.hip; xcorr_two_sided.hip: n = 4096 and, on the four-step transform with one scratch slice per
 * workgroup, n = 65536); n = 8192, 16384, 32768 -- each series a REAL transform of n / 2 complex points, X parked in the
 * workgroup's scratch slice, cc = FFT_n(Y conj X) / n untangled and re-tangled at mirror pairs of bins (xcorr_real.hip);
 * scale 1 / (n (n - 1)) when normalized else 1 / n, exactly as xcorr.go:139-143.  At n = 65536 with Nx = Ny = n the rows are
 * read once and the spectrum squared unscaled; pairs whose series differ by more than 2^16 in scale (or whose magnitudes are
 * extreme) are listed on the device and redone by a second launch that takes the statistics first.  Finite samples whose SQUARES leave the float64 range (|x| >~ 1e154) are looked at again by a device
 * kernel and give what the reference's arithmetic gives: finite correlations (raw: the pair is recomputed at magnitude 1 and
 * scaled back by an exact power of two, so the results are numbers exactly as long as n max|x| max|y| stays inside the float64
 * range, as in xcorr.go:108-143), all zeros (normalized, sigma = +Inf) or NaN (the reference's own sums overflow).  Any other n (the reference's n = 5 tables, short series) goes pair by pair
 * through muse_xcorr's path.  The groups are not mutated (the reference's zNormalize mutates x and y in place).
 * Outputs (host): lag[M], mv[M]; is_nil[M] (may be NULL) = 1 where the reference returns (nil, 0, 0), i.e. normalize
 * and sigma(x) == 0 or sigma(y) == 0; cc (may be NULL): M x n correlations (rows of nil pairs are zero). */
int muse_xcorr_groups(muse_group *gx, muse_group *gy, int32_t n, int32_t normalize,
                      int32_t *lag, double *mv, int32_t *is_nil, double *cc);
/* The same from host memory: x_rows is M x lenx, y_rows M x leny, dense row-major; uploads, runs, frees. */
int muse_xcorr_batch(muse_ctx *ctx, const double *x_rows, const double *y_rows, int64_t M,
                     int32_t lenx, int32_t leny, int32_t n, int32_t normalize,
                     int32_t *lag, double *mv, int32_t *is_nil, double *cc);
/* nextPowOf2 (xcorr.go:19-24), same floating formula. */
int64_t muse_next_pow2(double val);

#ifdef __cplusplus
}
#endif
#endif
