// xcorr_window_many_each.hip -- the packed lag-window pass for MANY references, EACH inside its own lag range or band and under its own
// sign (muse_batch_score_many_in_lag_bands): xcorr_window_many.hip's product -- one read of the rows, the table rows of all references
// of a launch packed into the accumulator tiles of one matrix product -- where the references' tables need not have one shape.
//
// A kernel of its own, so that xcorr_window_many_mfma and xcorr_window_many_signed_mfma keep their symbols and their code.  The body is
// theirs: the staged images, a lane's A offset of tile i formed in front of the k-loop, the k-loop written out on the same mapping,
// the waves' tiles summed by window_sum_tiles, the scan of a reference cut into `parts`.  What those kernels take once per launch --
// L, Lneg, origin, W, the sign, band or not -- is here a descriptor per reference in device memory (WindowEachRef), with the
// reference's first packed row (row0, a prefix sum of the W) and the LDS offset of its image (img0).  A lane finds the reference that
// owns packed row 16 i + r by one pass over the at most R prefix sums for all its tiles, in front of the k-loop; the scan and the outcome
// of a (reference, part) item are window_scan_pos<SGN, BAND> / window_outcome<SGN, BAND>, chosen by a switch over the six builds.
// Items of different kinds in one wave diverge in the scan only, a few dozen instructions per position.
//
// Image placement (window_each_place).  img0[0] = 0, and img0[j + 1] is the smallest offset >= img0[j] + kc + W_j - 1 with
// img0[j + 1] - img0[j] = W_j + 2 (mod 32).  Modulo the 64 banks (32 doubles) reference j's row v on a k-lane that is koff doubles
// along lies at img0[j] + v + koff = (sum over i < j of (W_i + 2)) + v + koff: as if every reference took W_j + 2 consecutive doubles,
// its own W_j, not a shared one.  The 32 lanes that one LDS cycle of a ds_read_b64 serves are 16 rows x 2 k-lanes, koff <= 2 apart: the
// two doubles behind a reference's last row are what its second k-lane reads, and the next reference's row 0 begins behind them.  So
// the argument of xcorr_window_many.hip's header holds reference by reference: a tile with rows of m references reads 16 + 2 m
// consecutive doubles modulo the banks (equal addresses -- the clamped empty rows -- are one broadcast), no conflict while m <= 8.  A
// tile holds rows of more than 8 references only where W = 1 references follow each other; they wrap as they do in the uniform kernel.
//
// Bit-identity with the single kernels: an accumulator element sees the same A and B values in the same k slots of the same k-steps
// in the same order -- its A row is row v of ITS reference's own table (built under that reference's origin and row count, as the
// single pass builds it), kc is a multiple of 256 samples, so the 64-sample piece p still goes to wave p mod 4, pieces in rising
// order, the piece's load is window_load_piece and the k-loop the single kernels' loop on the same mapping -- the waves' tiles are
// summed in wave order by window_sum_tiles, and the statistics, the score of a position, the key and the outcome are the single
// kernels' functions under the reference's own (SGN, BAND); how the scan is cut into parts is invisible to strict '>' with the first
// position winning.  So a batch's packed result has the bits of its own muse_batch_score_in_lag_band(lo_r, hi_r, sign_r).
#include "window_device.h"

#include <algorithm>
#include <vector>

namespace muse {

constexpr int WINME_STAGE = 3; // image samples per thread and reference in one batch of staging loads (xcorr_window_many.hip's)

// the scan of one (reference, part) item and the outcome of a reference under the reference's own build
template <int SGN, bool BAND>
__device__ __forceinline__ void window_each_scan(WindowBest &best, const double *lds, const WindowEachRef &d, const int pos0, const int plen,
                                                 const int c, const WindowStats &st, const double *__restrict__ pw)
{
    for (int k = 0; k < plen; k++)
        window_scan_pos<SGN, BAND>(best, lds, d.row0, pos0 + k, c, d.L, d.Lneg, d.origin, st, pw);
}
// (sign + 1) + 3 band: the six builds
__device__ __forceinline__ int window_each_kind(const WindowEachRef &d) { return d.sign + 1 + (d.band ? 3 : 0); }

template <int TILES, bool WIDE>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_many_each_mfma(const WindowEachParams p)
{
    // [max(image doubles, TILES 256)] the e images, then the summed tiles [tile][row][series] | [4 waves][16 series][2] | [R parts][16 series][3]
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N, R = p.R, kc = p.kc;
    const WindowEachRef *__restrict__ ref = p.ref;
    const int STAT = p.buf, CAND = STAT + 128;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); nothing of them is written
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];

    v4d acc[TILES];
    int aoff[TILES]; // this lane's A row of tile i: image base of its reference + table row + the lane's k slot
#pragma unroll
    for (int i = 0; i < TILES; i++) {
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
        const int rr = 16 * i + r; // (the empty rows behind the last reference compute the last row again, one LDS address: a broadcast; nothing of them is read)
        aoff[i] = (rr < p.total ? rr : p.total - 1) + window_k<WIDE>(0, q);
    }
    // the reference that owns packed row rr is the last one whose first row is not behind rr (every W >= 1: the prefix sums rise
    // strictly; reference 0 has row0 = img0 = 0).  One pass over the descriptors -- wave-uniform loads -- serves every tile: the
    // lane's offset moves from (row) to (img0 + row - row0) of the owner
    for (int j = 1; j < R; j++) {
        const int first = ref[j].row0, shift = ref[j].img0 - first - (ref[j - 1].img0 - ref[j - 1].row0);
#pragma unroll
        for (int i = 0; i < TILES; i++) {
            const int rr = 16 * i + r < p.total ? 16 * i + r : p.total - 1;
            aoff[i] += first <= rr ? shift : 0;
        }
    }
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = 0; T0 < N; T0 += kc) {
        if (T0 > 0)
            __syncthreads();
        // (the tables are padded with zeros to whole chunks of WIN_KC, which kc divides, and hold WIN_E_TAIL >= W entries behind them;
        // four references' loads in flight together, each image kc + W_j - 1 doubles at its own offset)
        for (int ref0 = 0; ref0 < R; ref0 += 4) {
            const double *__restrict__ e[4];
            int elen[4], at[4], most = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = ref0 + u < R ? ref0 + u : ref0;
                e[u] = p.e[j] + T0;
                elen[u] = ref0 + u < R ? kc + ref[j].W - 1 : 0;
                at[u] = ref[j].img0;
                most = elen[u] > most ? elen[u] : most;
            }
            for (int v0 = t; v0 < most; v0 += WINME_STAGE * WIN_THREADS) {
                double x[4][WINME_STAGE];
#pragma unroll
                for (int j = 0; j < WINME_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        x[u][j] = e[u][v < elen[u] ? v : 0];
                }
#pragma unroll
                for (int j = 0; j < WINME_STAGE; j++) {
                    const int v = v0 + j * WIN_THREADS;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (v < elen[u])
                            lds[at[u] + v] = x[u][j];
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
            // (the k-loop of window_mac_piece, written out as in xcorr_window_many_mfma)
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

    // the scan per (series, reference) under the reference's own sign / over its own range or band: its positions cut into `parts`
    // consecutive parts of its own `plen` positions, one (reference, part) item per 16 threads at a time
    const int c = t & 15;
    const int parts = p.parts;
    const WindowStats st = window_stats(window_wave_sum(lds, STAT, 2 * c), window_wave_sum(lds, STAT, 2 * c + 1), p.invN, p.invNm1);
    for (int item = t >> 4; item < R * parts; item += 16) {
        const int j = item / parts, part = item - j * parts;
        const WindowEachRef d = ref[j];
        const double *__restrict__ pw = p.pw[j];
        const int plen = (d.L + 1 + d.Lneg + parts - 1) / parts;
        WindowBest best;
        switch (window_each_kind(d)) {
        case 0: window_each_scan<-1, false>(best, lds, d, part * plen, plen, c, st, pw); break;
        case 1: window_each_scan<0, false>(best, lds, d, part * plen, plen, c, st, pw); break; // (the zig-zag order of xcorr_window_many_mfma)
        case 2: window_each_scan<1, false>(best, lds, d, part * plen, plen, c, st, pw); break;
        case 3: window_each_scan<-1, true>(best, lds, d, part * plen, plen, c, st, pw); break;
        case 4: window_each_scan<0, true>(best, lds, d, part * plen, plen, c, st, pw); break;
        default: window_each_scan<1, true>(best, lds, d, part * plen, plen, c, st, pw); break;
        }
        window_put_best(lds + CAND + (item * 16 + c) * 3, best);
    }
    __syncthreads();
    if (row0 + c < p.M) {
        for (int j = t >> 4; j < R; j += 16) {
            const WindowEachRef d = ref[j];
            const double *__restrict__ pw = p.pw[j];
            int lag;
            double mv;
            switch (window_each_kind(d)) {
            case 0: mv = window_outcome<-1, false>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            case 1: mv = window_outcome<0, false>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            case 2: mv = window_outcome<1, false>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            case 3: mv = window_outcome<-1, true>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            case 4: mv = window_outcome<0, true>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            default: mv = window_outcome<1, true>(lds, CAND, j * parts, parts, d.row0, c, d.L, d.Lneg, d.origin, st, pw, &lag); break;
            }
            p.mv[j][row0 + c] = mv;
            p.lag[j][row0 + c] = lag;
        }
    }
}

// ---- the planner (pure host code: muse_test_many_lag_bands_plan)
int window_each_place(const int *W, int m, int kc, int *img0)
{
    int at = 0;
    for (int j = 0; j < m; j++) {
        if (img0)
            img0[j] = at;
        const int want = (W[j] + 2) & 31; // this reference's 16-lane read group ends where the next one's begins, modulo the banks
        int step = kc + W[j] - 1;
        while ((step & 31) != want)
            step++;
        at += step;
    }
    return at;
}

int window_each_plan(int R, const int *W, int *launch_of, int *tiles_of, int *kc_of, int *img0)
{
    int launches = 0, open = -1, open_rows = 0;
    std::vector<int> open_w; // the W of the open launch's members, in list order
    std::vector<std::vector<int>> members;
    for (int r = 0; r < R; r++) {
        launch_of[r] = -1;
        img0[r] = 0;
        if (W[r] <= 0)
            continue;
        if (W[r] > WINM_PACK_MAX_ROWS) { // four tiles by itself: a launch of its own (window_many_max_refs), the open launch stays open
            launch_of[r] = launches++;
            members.push_back({r});
            continue;
        }
        if (open >= 0) {
            open_w.push_back(W[r]);
            if (open_rows + W[r] > 16 * WINM_MAX_TILES || window_each_place(open_w.data(), (int)open_w.size(), 256, nullptr) > WINM_IMG_DOUBLES)
                open = -1;
        }
        if (open < 0) {
            open = launches++;
            members.push_back({});
            open_w.assign(1, W[r]);
            open_rows = 0;
        }
        launch_of[r] = open;
        members[(size_t)open].push_back(r);
        open_rows += W[r];
    }
    for (int l = 0; l < launches; l++) {
        const std::vector<int> &mem = members[(size_t)l];
        int rows = 0;
        std::vector<int> w;
        for (int r : mem) {
            w.push_back(W[r]);
            rows += W[r];
        }
        tiles_of[l] = (rows + 15) / 16;
        kc_of[l] = WIN_KC;
        if (mem.size() < 2) // (a reference alone in its launch: the single-reference kernel, its image at offset 0)
            continue;
        int kc = WIN_KC;
        while (kc > 256 && window_each_place(w.data(), (int)w.size(), kc, nullptr) > WINM_IMG_DOUBLES)
            kc /= 2;
        kc_of[l] = kc;
        std::vector<int> at(w.size());
        window_each_place(w.data(), (int)w.size(), kc, at.data());
        for (size_t k = 0; k < mem.size(); k++)
            img0[mem[k]] = at[k];
    }
    return launches;
}

// ref_host: the launch's descriptors as uploaded to p.ref.  Every one of them is checked here, and the launch is sized from them
hipError_t launch_window_many_each(WindowEachParams p, const WindowEachRef *ref_host, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    if (!ref_host || p.R < 1 || p.R > 16 * WINM_MAX_TILES || p.N < 2)
        return hipErrorInvalidValue;
    const long long blocks = (p.M + 15) / 16;
    if (blocks > 0x7fffffffLL)
        return hipErrorInvalidValue;
    std::vector<int> w((size_t)p.R), at((size_t)p.R);
    int rows = 0;
    for (int j = 0; j < p.R; j++) {
        const WindowEachRef &d = ref_host[j];
        WindowShape s{};
        s.M = p.M;
        s.N = p.N;
        s.L = d.L;
        s.Lneg = d.Lneg;
        s.origin = d.origin;
        long long b;
        if ((d.band ? window_launch_check_band(s, &b) : window_launch_check(s, &b)) != hipSuccess || d.W != d.origin + d.L + 1 || d.W < 1 ||
            d.W > WINM_PACK_MAX_ROWS || d.sign < -1 || d.sign > 1 || (d.band != 0) != (d.L < 0 || d.Lneg < 0) || d.row0 != rows)
            return hipErrorInvalidValue;
        w[(size_t)j] = d.W;
        rows += d.W;
    }
    const int tiles = (rows + 15) / 16;
    if (tiles > WINM_MAX_TILES)
        return hipErrorInvalidValue;
    int kc = WIN_KC;
    while (kc > 256 && window_each_place(w.data(), p.R, kc, nullptr) > WINM_IMG_DOUBLES)
        kc /= 2;
    const int img = window_each_place(w.data(), p.R, kc, at.data());
    for (int j = 0; j < p.R; j++)
        if (ref_host[j].img0 != at[(size_t)j])
            return hipErrorInvalidValue;
    p.total = rows;
    p.kc = kc;
    p.buf = std::max(img, tiles * 256);
    p.parts = std::max(1, 16 / p.R);
    const size_t lds_bytes = (size_t)(p.buf + 128 + p.R * p.parts * 16 * 3) * sizeof(double);
    if (img > WINM_IMG_DOUBLES || lds_bytes > 64 * 1024)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
    window_with_tiles(tiles, [&](auto T) {
        if (wide)
            xcorr_window_many_each_mfma<T(), true><<<grid, block, lds_bytes, stream>>>(p);
        else
            xcorr_window_many_each_mfma<T(), false><<<grid, block, lds_bytes, stream>>>(p);
    });
    return hipGetLastError();
}

} // namespace muse
