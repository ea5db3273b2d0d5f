/*
 * muse_hip_test.h -- TEST AND MEASUREMENT HOOKS of libmuse_hip.so.  Not part of the drop-in boundary: nothing a
 * go-muse host binds lives here (INTEGRATION.md binds include/muse_hip.h only).  Used by tests/, tools/ and bench.py.
 */
#ifndef MUSE_HIP_TEST_H
#define MUSE_HIP_TEST_H

#include "muse_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forces the kernel of the all-scores pass (muse_batch_score): 0 = automatic (default), 1 = generic radix-2 kernel
 * (any power-of-two n), 7 = the n = 4096 kernel that rescales both series before the shared transform (the hand-off
 * target of the default kernel), 10 = the default n = 4096 kernel, 11 = round-1 radix-16 Stockham / four-step kernels
 * (n = 512 .. 2048, 8192 .. 65536), 12 = the pair-packed half-round kernels (n = 512 .. 2048: what auto takes; 8192, 16384; also the
 * two-sided xCorr at n = 16384), 13 = the four-step long-series kernel (n = 16384 .. 65536), 14 = one REAL series per workgroup
 * (n = 8192 .. 65536: what auto takes at 8192, 16384 and 65536), 15 = the same at n = 32768 with each 16384-point transform as
 * 16 x 1024 (wave-local 1024-point transforms around one workgroup transpose: what auto takes at 32768).  The parity tests run every kernel on the same inputs. */
int muse_ctx_set_kernel(muse_ctx *ctx, int32_t variant);
/* Scales the error bound the filter-and-refine Run assumes for its fp32 estimates (1.0 = the derived bound): the
 * guard test shrinks it a million-fold to force the fp64 re-run. */
int muse_test_set_screen_bound_scale(muse_ctx *ctx, double scale);
/* The bound itself, in the pass's scaled units, for FFT length n and max |X| (host only; docs/screen_error_bound.md). */
int muse_test_screen_bound(int32_t n, double xmax, double *Es);
/* Runs the screening pass of the filter-and-refine Run alone (MaxLag = max_lag, TopN = 1, no other filter) over a
 * batch of series of length 257 .. 65536 and returns, per series, the fp32 estimate of the signed score, the pass's
 * flag word (bit 0 / 1: a possible argmax has |lag| <= / > max_lag; bit 2 / 3: a possible argmax value is > 0 / < 0;
 * bit 4: fp32 not trusted, must be re-evaluated; bit 5: the exact score is NaN; bit 31: the row was re-evaluated and
 * `estimate` holds its fp64 score) and the bound *E (score units) that the selection assumes on
 * |estimate - exact score|.  Any out pointer may be NULL. */
int muse_batch_screen_estimates(muse_batch *b, int32_t max_lag, double *estimate, uint32_t *flags, double *E);

/* Shader clock held under load (bench.py's roofline.co_bounds): starts a one-wave kernel on a stream of its own that, for
 * total_ms, samples delta s_memtime / delta s_memrealtime x 100 MHz (MI355X_MICROARCH.md) in windows of window_ms while
 * the caller launches its kernels; _read waits for it and returns the clock of every window (MHz) in order.
 * _start returns once the probe is resident; _stop ends it within microseconds (a host flag), so that a device-wide
 * synchronisation behind the measured launches does not wait out the rest of total_ms. */
int muse_test_clock_probe_start(muse_ctx *ctx, double window_ms, double total_ms);
int muse_test_clock_probe_stop(muse_ctx *ctx);
int muse_test_clock_probe_read(muse_ctx *ctx, double *mhz, int32_t cap, int32_t *windows);

/* Device unit test of the n = 4096 kernels' argmax step (foldk_device.h, wave_argmax_store; maxAbsIndex of
 * xcorr.go:39-50): ccA / ccB are 4096 host doubles each, laid out in registers as the kernels hold a pair's correlations;
 * out24 receives, per wave w = 0..3, {max |cc|, signed value at the winning index (cc[0] of the wave's first lane when
 * nothing is above 0), winning index (2147483647 when nothing is above 0)} of series A, then of series B. */
int muse_test_wave_argmax(muse_ctx *ctx, const double *ccA, const double *ccB, double *out24);

/* muse_batch_run_rows lets the fused kernel read groups of up to 256 KB straight out of the pinned staging buffer (no copy
 * command); always_copy = 1 sends every group through the host -> HBM copy instead (A/B of the two, and the parity suite
 * runs both). */
int muse_test_rows_always_copy(muse_ctx *ctx, int32_t always_copy);

/* The context's allocation cache (muse_ctx_trim): bytes and blocks it holds idle, device and pinned host.  Any out
 * pointer may be NULL. */
int muse_test_pool_stats(muse_ctx *ctx, int64_t *dev_idle_bytes, int64_t *dev_idle_blocks, int64_t *host_idle_bytes,
                         int64_t *host_idle_blocks);
/* Measurement hook: muse_xcorr_groups launches its kernel `repeat` times back to back (same results) -- a sustained burst
 * for the clock probe and for HIP-event timing without the host's work between calls (tools/clock_trace_two_sided.py). */
int muse_test_xcorr_repeat(muse_ctx *ctx, int32_t repeat);

/* Measurement hook: the work buffer of one batch of the long-series pass (FFT lengths above 65 536; xcorr_huge.hip) in MB;
 * 0 = the built-in 128 MB (half the Infinity Cache).  tools/huge_bench.py, profiles/r06_long_series.txt. */
int muse_test_huge_batch_mb(muse_ctx *ctx, int32_t megabytes);

/* Measurement hook: the row gather of muse_group_append_from / muse_batch_run_group_rows (row_gather.hip) stores with
 * non-temporal stores (on = 1) or plain ones (0, the default): tools/resident_bench.py measures both. */
int muse_test_gather_nontemporal(muse_ctx *ctx, int32_t on);
/* The vector unit of muse_group_slide's kernel (row_slide.hip), a pure host function (no device needed): *unit_bytes = the widest
 * of 16 / 8 (/ 4 for float32 storage) bytes that divides both N x elem and k x elem -- float64 rows with odd k or odd N move in
 * 8-byte units.  MUSE_ERR_INVALID for N < 1 or k outside 0 .. N. */
int muse_test_slide_plan(int32_t N, int32_t k, int32_t f32_storage, int32_t *unit_bytes);

/* Spectrum cache (muse_ctx_set_spectrum_cache): the smallest group that is cached (default 65 536 rows; negative = default) and
 * a byte budget for a group's cache in place of half the free device memory (0 = always decline; negative = no override). */
int muse_test_spectrum_cache_limits(muse_ctx *ctx, int64_t min_rows, int64_t budget_bytes);
/* Which kernel scores from a valid cache: 0 (the default) = xcorr_cached_n4096, two workgroups per CU with the reference's table in
 * registers; 1 = xcorr_cached_n4096_occ4, the reader at four workgroups per CU it replaced (kept to compare against: results are
 * bit-identical).  Anything else: MUSE_ERR_INVALID. */
int muse_test_spectrum_cache_reader(muse_ctx *ctx, int32_t reader);
/* The cache's policy, a pure host function (no device needed): what the second pass over `rows` rows of length N decides with
 * free_bytes of device memory free -- *decision = 0 no cache, 1 build one of *bytes for rows [0, *rows_cached), 2 declined for
 * lack of memory.  min_rows / budget_bytes as in muse_test_spectrum_cache_limits. */
int muse_test_spectrum_cache_policy(int64_t rows, int32_t N, int32_t f32_storage, int32_t mode, int64_t min_rows,
                                    int64_t free_bytes, int64_t budget_bytes, int32_t *decision, int64_t *rows_cached,
                                    int64_t *bytes);
/* The pairs of series (row >> 1) the last all-scores pass of this batch at FFT length 4096 listed for the rescaling kernel (a NaN /
 * Inf series -- once per such series -- or sigmas too far apart), in list order: *count of them, the first min(*count, cap) in
 * pairs[].  Waits for the batch's stream. */
int muse_test_batch_redo_pairs(muse_batch *b, int64_t *pairs, int64_t cap, int64_t *count);
/* The planner of muse_batch_score_many_windowed, a pure host function (no device needed): R >= 1 references with window
 * 0 <= L <= MUSE_LAG_WINDOW_MAX are cut into *launches consecutive launches; launch_of[r] (R entries) = the launch of reference r,
 * tiles_of[l] (room for R entries) = the accumulator tiles of 16 packed rows of launch l.  *max_refs = the most references one
 * launch takes at this L (128 packed rows and the budget of staged images); img_of[l] / kc_of[l] (room for R entries each) = the
 * distance in doubles between the staged images of launch l and its chunk length in samples.  A launch of one reference is the
 * single-reference kernel's (xcorr_window_mfma).  Any out pointer but launches may be NULL. */
int muse_test_window_many_plan(int32_t R, int32_t L, int32_t *launches, int32_t *launch_of, int32_t *tiles_of, int32_t *max_refs,
                               int32_t *img_of, int32_t *kc_of);
/* The same planner in the rows 1 <= W <= 2 MUSE_LAG_WINDOW_MAX + 1 of a reference's table: a window +-L has W = 2 L + 1 (the hook
 * above), a lag range (muse_batch_score_many_in_lag_range) its W lags -- even W too.  Outputs as above. */
int muse_test_window_many_plan_rows(int32_t R, int32_t W, int32_t *launches, int32_t *launch_of, int32_t *tiles_of, int32_t *max_refs,
                                    int32_t *img_of, int32_t *kc_of);
/* The planner of the windowed Muse.Run (muse_batch_run_rows_windowed; xcorr_window_split.hip), a pure host function (no device
 * needed): M >= 1 rows of N >= 2 samples on num_cus CUs are scored in *S slices of whole 1024-sample chunks, slice s = chunks
 * [s chunks / S, (s + 1) chunks / S) of chunks = ceil(N / 1024); *chunks_per_slice = the largest slice.  *S == 1: the unsplit kernel. */
int muse_test_window_rows_plan(int64_t M, int32_t N, int32_t num_cus, int32_t *S, int32_t *chunks_per_slice);
/* Forces the slice count of the windowed Muse.Run on this context: 0 = the planner (default); S >= 1 = that many slices, clipped to
 * the chunks of the length (1 = the unsplit kernel) -- drives the split kernels at small shapes. */
int muse_test_window_rows_slices(muse_ctx *ctx, int32_t S);
/* muse_batch_run_rows_windowed's path (same checks, same slot, same kernels), and the slot's per-row (lag_out[M], mv_out[M]) copied
 * back before the slot is returned: without it only the winner is observable. */
int muse_test_run_rows_windowed_scores(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride, int32_t max_lag,
                                       int32_t *lag_out, double *mv_out);
/* The dispatch of muse_batch_run_rows_in_lag_range and its siblings, a pure host function (no device needed) of M >= 1 rows of
 * N >= 2 samples on num_cus CUs and the lags lag_lo .. lag_hi (lag_lo <= 0 <= lag_hi, clipped at the FFT length of N as
 * muse_batch_score_in_lag_range clips them; W = the lags that remain): *path = MUSE_ROWS_LAG_RANGE_PLAIN (every lag: the unwindowed
 * namesake's pass; *panels = *S = 0), _WINDOW / _SPLIT (W <= 127: the kernels of muse_batch_run_rows_windowed, unsplit / in the *S > 1
 * slices muse_test_window_rows_plan gives; *panels = 1), _PANELS (128 <= W <= MUSE_RUN_ROWS_LAG_RANGE_MAX: xcorr_window_panels.hip,
 * *panels = ceil(W / 128) panels in *S >= 1 slices) or _UNSUPPORTED (more lags, or series longer than 65536 samples).  panels and S
 * may be NULL. */
#define MUSE_ROWS_LAG_RANGE_UNSUPPORTED 0
#define MUSE_ROWS_LAG_RANGE_PLAIN 1
#define MUSE_ROWS_LAG_RANGE_WINDOW 2
#define MUSE_ROWS_LAG_RANGE_SPLIT 3
#define MUSE_ROWS_LAG_RANGE_PANELS 4
int muse_test_rows_lag_range_plan(int64_t M, int32_t N, int32_t num_cus, int32_t lag_lo, int32_t lag_hi, int32_t *path,
                                  int32_t *panels, int32_t *S);
/* muse_batch_run_rows_in_lag_range's path (same checks, same slot, same kernels; muse_test_window_rows_slices forces its slice count
 * too), and the slot's per-row (lag_out[M], mv_out[M]) copied back before the slot is returned. */
int muse_test_run_rows_in_lag_range_scores(muse_batch *tmpl, const double *rows, int64_t M, int64_t row_stride, int32_t lag_lo,
                                           int32_t lag_hi, int32_t *lag_out, double *mv_out);
/* The load / store widths of muse_batch_slide_score_windowed's kernel (xcorr_window_slide.hip), a pure host function (no device
 * needed): for rows of N samples slid by k, `wide` = the rows are 16-byte aligned (even N: the kernel's WIDE mapping) -- *load_bytes
 * = 16 iff wide and k is even (8 otherwise: the same samples from two loads), *store_bytes = 16 iff wide.  MUSE_ERR_INVALID for
 * N < 2, k outside 0 .. N, wide with an odd N, or a NULL out pointer. */
int muse_test_slide_score_plan(int32_t N, int32_t k, int32_t wide, int32_t *load_bytes, int32_t *store_bytes);

/* muse_batch_score_in_window's dispatch, a pure host function (no device needed): the pass that scores series of N >= 2 samples
 * (f32_storage: a float32-storage group) inside +-max_lag >= 0 -- *path = MUSE_IN_WINDOW_PLAIN (L == n/2: the unwindowed pass),
 * _MFMA (the direct product), _MASKED (the transform kernels with a masked argmax) or _UNSUPPORTED (the call returns
 * MUSE_ERR_UNSUPPORTED).  MUSE_ERR_INVALID for N < 2, max_lag < 0 or a NULL out pointer. */
#define MUSE_IN_WINDOW_UNSUPPORTED 0
#define MUSE_IN_WINDOW_PLAIN 1
#define MUSE_IN_WINDOW_MFMA 2
#define MUSE_IN_WINDOW_MASKED 3
int muse_test_in_window_plan(int32_t N, int32_t f32_storage, int32_t max_lag, int32_t *path);
/* on = 1: muse_batch_score_in_window sends float64 windows up to MUSE_LAG_WINDOW_MAX through the masked transform kernels too, where
 * the length has them (FFT lengths 512 ... 4096) -- cross-checks of the two mechanisms and tools/in_window_bench.py; 0 (default): the table. */
int muse_test_in_window_force_transform(muse_ctx *ctx, int32_t on);
/* The path (MUSE_IN_WINDOW_*) the batch's scores came by if its last scoring pass was muse_batch_score_in_window / _run_in_window
 * or muse_batch_score_in_lag_range / _run_in_lag_range; 0 after any other scoring pass. */
int muse_test_last_in_window_path(muse_batch *b, int32_t *path);
/* muse_batch_score_in_lag_range's dispatch, a pure host function (no device needed): the pass that scores series of N >= 2 samples
 * (f32_storage: a float32-storage group) inside the lags lag_lo .. lag_hi -- *path = MUSE_IN_WINDOW_PLAIN (the clipped range is
 * every lag), _MFMA (the direct product: float64, at most 2 MUSE_LAG_WINDOW_MAX + 1 lags, up to 65536 samples), _MASKED (the
 * transform kernels with a masked argmax) or _UNSUPPORTED.  For lag_lo == -lag_hi it is muse_test_in_window_plan(N, ., lag_hi).
 * MUSE_ERR_INVALID for N < 2, lag_lo > 0, lag_hi < 0 or a NULL out pointer. */
int muse_test_lag_range_plan(int32_t N, int32_t f32_storage, int32_t lag_lo, int32_t lag_hi, int32_t *path);
/* muse_batch_score_signed_in_lag_range's dispatch, a pure host function (no device needed).  sign == 0: muse_test_lag_range_plan.
 * sign == +-1: its _MFMA and _MASKED stand (the signed scan, the signed mask); where it says _PLAIN (the clipped range is every lag)
 * *path = MUSE_IN_WINDOW_MASKED at FFT lengths 512, 1024, 2048 and 4096 (the masked kernels with both bounds at their widest) and
 * _UNSUPPORTED elsewhere.  MUSE_ERR_INVALID for N < 2, lag_lo > 0, lag_hi < 0, a sign outside -1 .. 1 or a NULL out pointer.
 * muse_test_last_in_window_path reports the signed calls' passes too. */
int muse_test_signed_lag_range_plan(int32_t N, int32_t f32_storage, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t *path);
/* muse_batch_score_in_lag_band's dispatch, a pure host function (no device needed).  A band that holds lag 0:
 * muse_test_signed_lag_range_plan.  Otherwise, with W the lags of the clipped band: *path = MUSE_IN_WINDOW_MFMA (float64, W <= 2
 * MUSE_LAG_WINDOW_MAX + 1, up to 65536 samples: the direct product over W table rows), _MASKED (FFT lengths 512 ... 4096, W wider or
 * float32 storage: the transform kernels masked to the one index interval) or _UNSUPPORTED; never _PLAIN.  MUSE_ERR_INVALID for
 * N < 2, lag_lo > lag_hi, a band that is empty after clipping, a sign outside -1 .. 1 or a NULL out pointer.
 * muse_test_in_window_force_transform applies to bands as to ranges, muse_test_last_in_window_path reports the band pass. */
int muse_test_lag_band_plan(int32_t N, int32_t f32_storage, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t *path);
/* muse_batch_score_many_in_window's dispatch, a pure host function (no device needed): the pass that scores R >= 1 references against
 * series of N >= 2 samples (f32_storage: a float32-storage group) inside +-max_lag >= 0 -- *path = MUSE_IN_WINDOW_PLAIN
 * (muse_batch_score_many), _MFMA (muse_batch_score_many_windowed), _MASKED (ONE many-references pass of the transform kernels with a
 * masked argmax: R >= 2 at FFT length 4096, or at 512 ... 2048 on float64 storage), _MASKED_EACH (R single masked passes,
 * muse_batch_score_in_window per batch) or _UNSUPPORTED.  What only the handles know (a forced kernel variant, a missing correction
 * table) turns _MASKED into _MASKED_EACH when the call runs.  MUSE_ERR_INVALID for N < 2, max_lag < 0, R < 1 or a NULL out pointer. */
#define MUSE_IN_WINDOW_MASKED_EACH 4
int muse_test_many_in_window_plan(int32_t N, int32_t f32_storage, int32_t max_lag, int32_t R, int32_t *path);
/* muse_batch_score_many_in_lag_range's dispatch, a pure host function (no device needed): the pass that scores R >= 1 references
 * against series of N >= 2 samples inside the lags lag_lo .. lag_hi -- *path = MUSE_IN_WINDOW_PLAIN (the clipped range is every lag:
 * muse_batch_score_many), _MFMA (the direct product, packed where the planner packs: float64, at most 2 MUSE_LAG_WINDOW_MAX + 1 lags,
 * up to 65536 samples), _MASKED, _MASKED_EACH (as above, with muse_batch_score_in_lag_range per batch) or _UNSUPPORTED.  For
 * lag_lo == -lag_hi it is muse_test_many_in_window_plan(N, ., lag_hi, R).  MUSE_ERR_INVALID for N < 2, lag_lo > 0, lag_hi < 0, R < 1
 * or a NULL out pointer. */
int muse_test_many_lag_range_plan(int32_t N, int32_t f32_storage, int32_t lag_lo, int32_t lag_hi, int32_t R, int32_t *path);
/* muse_batch_score_many_in_lag_band's dispatch, a pure host function (no device needed): the pass that scores R >= 1 references
 * against series of N >= 2 samples inside the lags lag_lo .. lag_hi (lag 0 inside or not) under sign -1 .. 1.  sign == 0 with lag 0
 * inside: muse_test_many_lag_range_plan.  Otherwise, with the band clipped: *path = MUSE_IN_WINDOW_MFMA (float64, at most
 * 2 MUSE_LAG_WINDOW_MAX + 1 lags, up to 65536 samples: the direct product with the signed / band scan, packed where the planner
 * packs), _MASKED (ONE masked many-references pass: R >= 2 at FFT length 4096, or at 512 ... 2048 on float64 storage), _MASKED_EACH
 * (R single masked passes, muse_batch_score_in_lag_band per batch: R == 1, float32 storage at 512 ... 2048; a forced kernel variant
 * or a missing correction table turns _MASKED into it when the call runs) or _UNSUPPORTED; never _PLAIN (every lag under a sign is a
 * masked pass).  For
 * R == 1 it is muse_test_lag_band_plan with _MASKED_EACH for _MASKED.  MUSE_ERR_INVALID for N < 2, R < 1, lag_lo > lag_hi, a band
 * that is empty after clipping, a sign outside -1 .. 1 or a NULL out pointer. */
int muse_test_many_lag_band_plan(int32_t N, int32_t f32_storage, int32_t lag_lo, int32_t lag_hi, int32_t sign, int32_t R, int32_t *path);
/* muse_batch_score_many_in_lag_bands' planner for a list that does NOT share one (lag_lo, lag_hi, sign), a pure host function (no
 * device needed): R >= 1 references against series of N >= 2 samples, reference r inside lag_lo[r] .. lag_hi[r] under sign[r] (NULL:
 * MUSE_SIGN_ANY).  path[r] = the MUSE_IN_WINDOW_* value of the single dispatch (muse_test_lag_band_plan).  The references with
 * path[r] == MUSE_IN_WINDOW_MFMA are cut into *launches launches, numbered by their first member: launch_of[r] (-1 for every other
 * reference), tiles_of[l] and kc_of[l] per launch (a reference alone in its launch: the single-reference kernel's tiles and chunk of
 * 1024), img0[r] the LDS offset of the reference's staged image inside its launch (0 for a reference alone and for launch_of[r] == -1).
 * launch_of, path and img0 hold R entries, tiles_of and kc_of up to R.  MUSE_ERR_INVALID for N < 2, R < 1, a NULL array, and at any
 * index lag_lo > lag_hi, a sign outside -1 .. 1 or a band that is empty after clipping. */
int muse_test_many_lag_bands_plan(int32_t N, int32_t f32_storage, int32_t R, const int32_t *lag_lo, const int32_t *lag_hi,
                                  const int32_t *sign, int32_t *path, int32_t *launch_of, int32_t *launches, int32_t *tiles_of,
                                  int32_t *kc_of, int32_t *img0);
/* muse_batch_slide_score_in_window's dispatch, a pure host function (no device needed): how a group of series of N >= 2 samples
 * (f32_storage: a float32-storage group) is slid by 0 <= k <= N samples and scored inside +-max_lag >= 0 --
 *   _UNSUPPORTED : muse_test_in_window_plan says so (the call returns MUSE_ERR_UNSUPPORTED, nothing moves)
 *   _MFMA        : muse_test_in_window_plan says _MFMA: muse_batch_slide_score_windowed's kernel
 *   _FUSED       : the plain or masked transform pass at FFT length 4096 (2048 < N <= 4096): the SLIDE build of the default kernel
 *                  moves the rows while it scores them.  What only the handles know -- a forced kernel variant, a missing correction
 *                  table, a learned hand-off to the rescaling kernel -- turns it into _TWO_STEP when the call runs.
 *   _TWO_STEP    : everything else both calls support: muse_group_slide's kernel, then the pass, inside the one call
 * (k = 0 moves nothing whatever the path).  MUSE_ERR_INVALID for N < 2, max_lag < 0, k outside 0 .. N or a NULL out pointer. */
#define MUSE_SLIDE_IN_WINDOW_UNSUPPORTED 0
#define MUSE_SLIDE_IN_WINDOW_MFMA 1
#define MUSE_SLIDE_IN_WINDOW_FUSED 2
#define MUSE_SLIDE_IN_WINDOW_TWO_STEP 3
int muse_test_slide_in_window_plan(int32_t N, int32_t f32_storage, int32_t max_lag, int32_t k, int32_t *path);
/* mode = 1: muse_batch_slide_score_in_window takes _TWO_STEP wherever the table says _FUSED (the parent's kernels: cross-checks and
 * tools/slide_in_window_bench.py); 0 (default): the table.  Anything else: MUSE_ERR_INVALID. */
int muse_test_slide_in_window_force(muse_ctx *ctx, int32_t mode);
/* The path (MUSE_SLIDE_IN_WINDOW_*) the batch's last scoring pass took if it was a muse_batch_slide_score_in_window / _slide_run_in_window /
 * _slide_run that moved rows; 0 after any other scoring pass (k = 0 included). */
int muse_test_last_slide_path(muse_batch *b, int32_t *path);
/* muse_batch_lag_profile's planner and its lag checks, a pure host function (no device needed): the lags lag_lo .. lag_hi of series of
 * N >= 2 samples in *launches consecutive launches of up to 2 MUSE_LAG_WINDOW_MAX + 1 table rows -- lo_of[j] the first lag of launch
 * j, rows_of[j] its table rows; the first min(*launches, cap) entries are filled (NULL arrays with cap == 0: the count alone).
 * MUSE_ERR_INVALID for N < 2, lag_lo > lag_hi, a lag outside -(n / 2 - 1) .. n / 2 at the FFT length n of N, cap < 0 or a NULL
 * out pointer; MUSE_ERR_UNSUPPORTED for N > 65536: the entry points' own checks. */
int muse_test_lag_profile_plan(int32_t N, int32_t lag_lo, int32_t lag_hi, int32_t *launches, int32_t *lo_of, int32_t *rows_of,
                               int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
