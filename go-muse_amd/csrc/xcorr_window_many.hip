// xcorr_window_many.hip -- the lag-window pass for MANY references (muse_batch_score_many_windowed): one read of the rows, the
// windows of all references of a launch PACKED into the accumulator tiles of one matrix product.
//
// xcorr_window.hip computes S[v][series] = sum_t d[t] e[t + v] with the 2L+1 window rows of ONE reference on the A rows of
// v_mfma_f64_16x16x4_f64 and leaves the rest of its last tile empty (L = 7: 15 of 16 rows; L = 3: 7 of 16; L = 1: 3 of 16).  Here
// the A rows are the packed list (reference r, window row v), A row index r (2L+1) + v, cut into tiles of 16 wherever they fall: a
// tile may hold rows of several references.  Everything that depends on the rows alone -- the loads, d = y - y[0], s1, s2 -- is done
// once per series for all references of the launch.
//
// Per chunk of `kc` samples the workgroup stages one image of e per reference in LDS, `img` doubles apart; lane (r, q) of tile i
// reads A from (image of its row's reference) + k + v: per lane and tile one offset, formed in front of the k loop.  img = 2L + 3
// mod 32 (window_many_img): the 32 lanes that one LDS cycle of a ds_read_b64 serves (16 rows x 2 k-lanes, at most two doubles
// apart in k) then read 16 + 2 (references in the tile) <= 32 consecutive doubles modulo the 64 banks -- a tile that straddles
// references collides no more than one that does not (2L+1 >= 3).
//
// Bit-identity with xcorr_window_mfma: an accumulator element sees the same A and B values in the same k slots of the same k-steps
// in the same order (kc is a multiple of 256 samples, so the 64-sample piece p still goes to wave p mod 4, pieces in rising
// order), the waves' tiles are summed in wave order, and the statistics and the scan are that kernel's expressions; the scan is
// cut into parts differently, which strict '>' with the first index winning does not see.
#include "xcorr_kernels.h"

namespace muse {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int WINM_THREADS = 256;
constexpr int WINM_STAGE = 3; // image samples per thread and reference in one batch of staging loads

template <int TILES, bool WIDE>
__global__ __launch_bounds__(WINM_THREADS) void xcorr_window_many_mfma(const WindowManyParams p)
{
    // [max(R img, TILES 256)] the e images, then the summed tiles [tile][row][series] | [4 waves][16 series][2] | [R parts][16 series][3]
    extern __shared__ double lds[];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N, R = p.R, L = p.L, Lneg = p.Lneg, Wv = 2 * L + 1, kc = p.kc, img = p.img, elen = kc + 2 * L;
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
        aoff[i] = ref * img + (rr - ref * Wv) + (WIDE ? 2 * q : q);
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
            for (int v0 = t; v0 < elen; v0 += WINM_STAGE * WINM_THREADS) {
                double x[4][WINM_STAGE];
#pragma unroll
                for (int j = 0; j < WINM_STAGE; j++) {
                    const int v = v0 + j * WINM_THREADS < elen ? v0 + j * WINM_THREADS : v0;
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        x[u][j] = e[u][v];
                }
#pragma unroll
                for (int j = 0; j < WINM_STAGE; j++) {
                    const int v = v0 + j * WINM_THREADS;
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
            // the k order of xcorr_window_mfma: WIDE, k-step m = 2 mp + h <-> sample T + 8 mp + 2 q + h; else m <-> T + 4 m + q
            double d[16];
            if (WIDE && T + 64 <= N) {
#pragma unroll
                for (int mp = 0; mp < 8; mp++) {
                    const double2 v = *reinterpret_cast<const double2 *>(y + T + 8 * mp + 2 * q);
                    d[2 * mp] = v.x - y0;
                    d[2 * mp + 1] = v.y - y0;
                }
            } else if (T + 64 <= N) {
#pragma unroll
                for (int m = 0; m < 16; m++)
                    d[m] = y[T + 4 * m + q] - y0;
            } else {
#pragma unroll
                for (int m = 0; m < 16; m++) {
                    const int tt = T + (WIDE ? 8 * (m >> 1) + 2 * q + (m & 1) : 4 * m + q);
                    d[m] = tt < N ? y[tt] - y0 : 0.0;
                }
            }
            const double *a = lds + 64 * s;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                s1 += d[m];
                s2 = fma(d[m], d[m], s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(WIDE ? 8 * (m >> 1) + (m & 1) : 4 * m) + aoff[i]], d[m], acc[i], 0, 0, 0);
            }
        }
    }
    // statistics: the four k-lanes of a series, then (below) the four waves
    s1 += __shfl_xor(s1, 16);
    s2 += __shfl_xor(s2, 16);
    s1 += __shfl_xor(s1, 32);
    s2 += __shfl_xor(s2, 32);
    if (q == 0) {
        lds[STAT + wave * 32 + 2 * r] = s1;
        lds[STAT + wave * 32 + 2 * r + 1] = s2;
    }
    __syncthreads(); // every wave is done with the e images
    // C/D of v_mfma_f64_16x16x4_f64: register j of lane (r, q) = [row q + 4 j][column r]
    for (int w = 0; w < 4; w++) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < TILES; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int at = i * 256 + (q + 4 * j) * 16 + r;
                    lds[at] = w == 0 ? acc[i][j] : lds[at] + acc[i][j];
                }
        }
        __syncthreads();
    }

    // the windowed maxAbsIndex per (series, reference): scan position pos = 0 .. W-1 <-> lag 0 .. L, -Lneg .. -1, cut into
    // `parts` consecutive parts of `plen` positions per reference
    const int c = t & 15;
    const int W = L + 1 + Lneg, parts = p.parts, plen = (W + parts - 1) / parts;
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        t1 += lds[STAT + w * 32 + 2 * c];
        t2 += lds[STAT + w * 32 + 2 * c + 1];
    }
    const double var = (t2 - t1 * t1 * p.invN) * p.invNm1;
    const bool nan = !__builtin_isfinite(var);
    const bool zero = !nan && !(var > 0.0);
    const double mean = t1 * p.invN;
    const double inv_sigma = 1.0 / sqrt(var);
    for (int item = t >> 4; item < R * parts; item += 16) {
        const int ref = item / parts, part = item - ref * parts;
        const double *__restrict__ pw = p.pw[ref];
        double best_abs = 0.0, best_val = 0.0, best_pos = -1.0;
        for (int k = 0; k < plen; k++) {
            const int pos = part * plen + k;
            if (pos < W) {
                const int v = pos <= L ? pos + L : pos - 1 - Lneg; // lag + L
                const int rr = ref * Wv + v;
                const double S = lds[(rr >> 4) * 256 + (rr & 15) * 16 + c];
                const double val = (S - mean * pw[v]) * inv_sigma;
                if (fabs(val) > best_abs) {
                    best_abs = fabs(val);
                    best_val = val;
                    best_pos = (double)pos;
                }
            }
        }
        lds[CAND + (item * 16 + c) * 3] = best_abs;
        lds[CAND + (item * 16 + c) * 3 + 1] = best_val;
        lds[CAND + (item * 16 + c) * 3 + 2] = best_pos;
    }
    __syncthreads();
    if (row0 + c < p.M) {
        for (int ref = t >> 4; ref < R; ref += 16) {
            double ba = 0.0, bv = 0.0;
            int bp = -1;
            for (int k = 0; k < parts; k++) {
                const int at = CAND + ((ref * parts + k) * 16 + c) * 3;
                const double a = lds[at];
                if (a > ba) {
                    ba = a;
                    bv = lds[at + 1];
                    bp = (int)lds[at + 2];
                }
            }
            int lag = 0;
            double mv;
            if (nan) {
                mv = __builtin_nan("");
            } else if (zero) {
                mv = 0.0; // sigma == 0: (nil, 0, 0), xcorr.go:165-168
            } else if (bp < 0) { // only zeros or NaN in the window: index 0 stands
                const int rr = ref * Wv + L;
                mv = (lds[(rr >> 4) * 256 + (rr & 15) * 16 + c] - mean * p.pw[ref][L]) * inv_sigma;
            } else {
                mv = bv;
                lag = bp <= L ? bp : bp - 1 - Lneg - L;
            }
            p.mv[ref][row0 + c] = mv;
            p.lag[ref][row0 + c] = lag;
        }
    }
}

// ---- the planner (pure host code: muse_test_window_many_plan)
int window_many_img(int L, int kc)
{
    const int want = (2 * L + 3) & 31; // one reference's 16-lane read group ends where the next one's begins, modulo the banks
    int img = kc + 2 * L;
    while ((img & 31) != want)
        img++;
    return img;
}

int window_many_max_refs(int L)
{
    // a reference that fills four tiles by itself (2L+1 > 48) is bound by the matrix pipe in its own pass: two of them in one launch
    // save no time (measured 0.97 ... 1.06 of two single passes at L = 31, profiles/window_many_bench.txt): one launch each
    if (2 * L + 1 > WINM_PACK_MAX_ROWS)
        return 1;
    const int by_rows = (16 * WINM_MAX_TILES) / (2 * L + 1), by_lds = WINM_IMG_DOUBLES / window_many_img(L, 256);
    return std::max(1, std::min(by_rows, by_lds));
}

int window_many_kc(int L, int refs)
{
    for (int kc = WIN_KC; kc > 256; kc /= 2)
        if ((long long)refs * window_many_img(L, kc) <= WINM_IMG_DOUBLES)
            return kc;
    return 256;
}

int window_many_plan(int R, int L, int *launch_of, int *tiles_of)
{
    const int per = window_many_max_refs(L);
    int launches = 0;
    for (int r0 = 0; r0 < R; r0 += per, launches++) {
        const int refs = std::min(per, R - r0);
        for (int r = r0; r < r0 + refs; r++)
            launch_of[r] = launches;
        tiles_of[launches] = (refs * (2 * L + 1) + 15) / 16;
    }
    return launches;
}

hipError_t launch_window_many(WindowManyParams p, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    if (p.L < 0 || p.L > MUSE_LAG_WINDOW_MAX || p.Lneg < 0 || p.Lneg > p.L || p.N < 2 || p.R < 1 || p.R > window_many_max_refs(p.L))
        return hipErrorInvalidValue;
    const long long blocks = (p.M + 15) / 16;
    if (blocks > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const int tiles = (p.R * (2 * p.L + 1) + 15) / 16;
    p.kc = window_many_kc(p.L, p.R);
    p.img = window_many_img(p.L, p.kc);
    p.buf = std::max(p.R * p.img, tiles * 256);
    p.parts = std::max(1, 16 / p.R);
    const size_t lds_bytes = (size_t)(p.buf + 128 + p.R * p.parts * 16 * 3) * sizeof(double);
    if (tiles > WINM_MAX_TILES || lds_bytes > 64 * 1024)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WINM_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
#define MUSE_WINDOW_MANY_LAUNCH(T)                                                        \
    do {                                                                                  \
        if (wide)                                                                         \
            xcorr_window_many_mfma<T, true><<<grid, block, lds_bytes, stream>>>(p);       \
        else                                                                              \
            xcorr_window_many_mfma<T, false><<<grid, block, lds_bytes, stream>>>(p);      \
    } while (0)
    switch (tiles) {
    case 1: MUSE_WINDOW_MANY_LAUNCH(1); break;
    case 2: MUSE_WINDOW_MANY_LAUNCH(2); break;
    case 3: MUSE_WINDOW_MANY_LAUNCH(3); break;
    case 4: MUSE_WINDOW_MANY_LAUNCH(4); break;
    case 5: MUSE_WINDOW_MANY_LAUNCH(5); break;
    case 6: MUSE_WINDOW_MANY_LAUNCH(6); break;
    case 7: MUSE_WINDOW_MANY_LAUNCH(7); break;
    default: MUSE_WINDOW_MANY_LAUNCH(8); break;
    }
#undef MUSE_WINDOW_MANY_LAUNCH
    return hipGetLastError();
}

} // namespace muse
