// xcorr_window_many.hip -- the lag-window pass for MANY references (muse_batch_score_many_windowed): one read of the rows, the
// windows of all references of a launch PACKED into the accumulator tiles of one matrix product.
//
// xcorr_window.hip computes S[v][series] = sum_t d[t] e[t + v] with the 2L+1 window rows of ONE reference on the A rows of
// v_mfma_f64_16x16x4_f64 and leaves the rest of its last tile empty (L = 7: 15 of 16 rows; L = 3: 7 of 16; L = 1: 3 of 16).  Here
// the A rows are the packed list (reference r, table row v), A row index r W + v, cut into tiles of 16 wherever they fall: a
// tile may hold rows of several references.  W = origin + L + 1 is the rows of a reference's table, whose row v is lag v - origin
// (WindowShape): 2L+1 for a symmetric window (origin = L), the lags of a lag range whose table starts at its lowest lag (origin =
// Lneg; muse_batch_score_many_in_lag_range).  Everything that depends on the rows alone -- the loads, d = y - y[0], s1, s2 -- is done
// once per series for all references of the launch.
//
// Per chunk of `kc` samples the workgroup stages one image of e per reference in LDS, `img` doubles apart; lane (r, q) of tile i
// reads A from (image of its row's reference) + k + v: per lane and tile one offset, formed in front of the k loop.  img = W + 2
// mod 32 (window_many_img): modulo the 64 banks (32 doubles) reference j's row v on a k-lane that is koff doubles along lies at
// j (W + 2) + v + koff, as if every reference took W + 2 consecutive doubles.  The 32 lanes that one LDS cycle of a ds_read_b64
// serves are 16 rows x 2 k-lanes, koff <= 2 apart: the two doubles behind a reference's last row are what its second k-lane reads,
// and the next reference's row 0 begins behind them.  A tile with rows of m references so reads 16 + 2 m consecutive doubles modulo
// the banks (equal addresses -- the clamped empty rows -- are one broadcast): no conflict while m <= 8.  Nothing here asks W to be
// odd.  A tile of 16 packed rows holds rows of at most floor(14 / W) + 2 references: 6 at W = 3 (22 ... 28 doubles), 4 at W = 4, 5
// and 6, fewer beyond.  W = 2 (the ranges -1 .. 0 and 0 .. 1): the tiles start at multiples of 16, which 2 divides, so a tile holds
// the rows of exactly eight references, never nine: 32 doubles, every bank once.  Only W = 1 (the window +-0, 16 references in a
// tile, 48 doubles) wraps: its second k-lane meets the first one's banks two ways at six (8-byte loads: five) of the 32 addresses.
//
// Bit-identity with xcorr_window_mfma: an accumulator element sees the same A and B values in the same k slots of the same k-steps
// in the same order (kc is a multiple of 256 samples, so the 64-sample piece p still goes to wave p mod 4, pieces in rising
// order; the piece's load is that kernel's function and the k-loop its loop on the same mapping, window_device.h), the waves' tiles are summed in wave order by
// the same function, and the statistics, the scoring of a position, the candidate update and the outcome are that kernel's functions
// too; the scan is cut into parts differently, which strict '>' with the first index winning does not see.
#include "window_device.h"

namespace muse {

constexpr int WINM_STAGE = 3; // image samples per thread and reference in one batch of staging loads

// (xcorr_window_many_band.hip holds a copy of this body with the signed / band scan, xcorr_window_many_signed_mfma, kept apart so that this
// kernel keeps its symbols and its code: a fix to the staging, the k-loop or the scan's cut is made in both)
template <int TILES, bool WIDE>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_many_mfma(const WindowManyParams p)
{
    // [max(R img, TILES 256)] the e images, then the summed tiles [tile][row][series] | [4 waves][16 series][2] | [R parts][16 series][3]
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N, R = p.R, L = p.L, Lneg = p.Lneg, origin = p.origin, Wv = origin + L + 1, kc = p.kc, img = p.img, elen = kc + Wv - 1;
    const int STAT = p.buf, CAND = STAT + 128;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); nothing of them is written
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];

    v4d acc[TILES];
    int aoff[TILES]; // this lane's A row of tile i: image base of its reference + window row + the lane's k slot
#pragma unroll
    for (int i = 0; i < TILES; i++) {
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
        int rr = 16 * i + r;
        if (rr >= R * Wv) // the empty rows behind the last reference compute the last row again (one LDS address: a broadcast); nothing of them is read
            rr = R * Wv - 1;
        const int ref = rr / Wv;
        aoff[i] = ref * img + (rr - ref * Wv) + window_k<WIDE>(0, q);
    }
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = 0; T0 < N; T0 += kc) {
        if (T0 > 0)
            __syncthreads();
        // (the tables are padded with zeros to whole chunks of WIN_KC, which kc divides.)  Four references' loads of one batch are
        // in flight together: the images come out of L2, and one dependent load after the other would leave the workgroup waiting
        for (int ref0 = 0; ref0 < R; ref0 += 4) {
            const double *__restrict__ e[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                e[u] = p.e[ref0 + u < R ? ref0 + u : ref0] + T0;
            for (int v0 = t; v0 < elen; v0 += WINM_STAGE * WIN_THREADS) {
                double x[4][WINM_STAGE];
#pragma unroll
                for (int j = 0; j < WINM_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS < elen ? v0 + j * WIN_THREADS : v0;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        x[u][j] = e[u][v];
                }
#pragma unroll
                for (int j = 0; j < WINM_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (v < elen && ref0 + u < R)
                            lds[(ref0 + u) * img + v] = x[u][j];
                }
            }
        }
        __syncthreads();
        for (int s = wave; s < kc / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            double d[16];
            window_load_piece<WIDE>(d, y, y0, T, N, q);
            // (the k-loop of window_mac_piece, written out: called through the function these builds are 2 ... 3 % slower at 4 and 8
            // tiles -- the compiler spreads the accumulator copies through the MFMA run; profiles/window_refactor.txt)
            const double *a = lds + 64 * s;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                s1 += d[m];
                s2 = fma(d[m], d[m], s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[window_a<WIDE>(m) + aoff[i]], d[m], acc[i], 0, 0, 0);
            }
        }
    }
    window_sum_tiles<TILES>(lds, STAT, acc, s1, s2, wave, r, q);

    // the windowed maxAbsIndex per (series, reference): the scan positions of a reference cut into `parts` consecutive parts of
    // `plen` positions, one (reference, part) item per 16 threads at a time
    const int c = t & 15;
    const int parts = p.parts, plen = (L + 1 + Lneg + parts - 1) / parts;
    const WindowStats st = window_stats(window_wave_sum(lds, STAT, 2 * c), window_wave_sum(lds, STAT, 2 * c + 1), p.invN, p.invNm1);
    for (int item = t >> 4; item < R * parts; item += 16) {
        const int ref = item / parts, part = item - ref * parts;
        const double *__restrict__ pw = p.pw[ref];
        WindowBest best;
        for (int k = 0; k < plen; k++)
            window_scan_pos(best, lds, ref * Wv, part * plen + k, c, L, Lneg, origin, st, pw);
        window_put_best(lds + CAND + (item * 16 + c) * 3, best);
    }
    __syncthreads();
    if (row0 + c < p.M) {
        for (int ref = t >> 4; ref < R; ref += 16) {
            int lag;
            p.mv[ref][row0 + c] = window_outcome(lds, CAND, ref * parts, parts, ref * Wv, c, L, Lneg, origin, st, p.pw[ref], &lag);
            p.lag[ref][row0 + c] = lag;
        }
    }
}

// ---- the planner (pure host code: muse_test_window_many_plan, muse_test_window_many_plan_rows), in the rows W of a reference's table
// (a symmetric window +-L: W = 2 L + 1; a lag range: W = its lags)
int window_many_img(int W, int kc)
{
    const int want = (W + 2) & 31; // one reference's 16-lane read group ends where the next one's begins, modulo the banks
    int img = kc + W - 1;
    while ((img & 31) != want)
        img++;
    return img;
}

int window_many_max_refs(int W)
{
    // a reference that fills four tiles by itself (W > 48) is bound by the matrix pipe in its own pass: two of them in one launch
    // save no time (measured 0.97 ... 1.06 of two single passes at L = 31, profiles/window_many_bench.txt): one launch each
    if (W > WINM_PACK_MAX_ROWS)
        return 1;
    const int by_rows = (16 * WINM_MAX_TILES) / W, by_lds = WINM_IMG_DOUBLES / window_many_img(W, 256);
    return std::max(1, std::min(by_rows, by_lds));
}

int window_many_kc(int W, int refs)
{
    for (int kc = WIN_KC; kc > 256; kc /= 2)
        if ((long long)refs * window_many_img(W, kc) <= WINM_IMG_DOUBLES)
            return kc;
    return 256;
}

int window_many_plan(int R, int W, int *launch_of, int *tiles_of)
{
    const int per = window_many_max_refs(W);
    int launches = 0;
    for (int r0 = 0; r0 < R; r0 += per, launches++) {
        const int refs = std::min(per, R - r0);
        for (int r = r0; r < r0 + refs; r++)
            launch_of[r] = launches;
        tiles_of[launches] = (refs * W + 15) / 16;
    }
    return launches;
}

hipError_t launch_window_many(WindowManyParams p, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    // (every packed reference's table has the one shape: row v is lag v - origin, rows 0 .. origin + L; the shape check bounds
    // origin + L by 2 MUSE_LAG_WINDOW_MAX and Lneg by origin)
    const int W = p.origin + p.L + 1;
    if (window_launch_check(p, &blocks) != hipSuccess || p.R < 1 || p.R > window_many_max_refs(W))
        return hipErrorInvalidValue;
    const int tiles = (p.R * W + 15) / 16;
    p.kc = window_many_kc(W, p.R);
    p.img = window_many_img(W, p.kc);
    p.buf = std::max(p.R * p.img, tiles * 256);
    p.parts = std::max(1, 16 / p.R);
    const size_t lds_bytes = (size_t)(p.buf + 128 + p.R * p.parts * 16 * 3) * sizeof(double);
    if (tiles > WINM_MAX_TILES || lds_bytes > 64 * 1024)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
    window_with_tiles(tiles, [&](auto T) {
        if (wide)
            xcorr_window_many_mfma<T(), true><<<grid, block, lds_bytes, stream>>>(p);
        else
            xcorr_window_many_mfma<T(), false><<<grid, block, lds_bytes, stream>>>(p);
    });
    return hipGetLastError();
}

} // namespace muse
