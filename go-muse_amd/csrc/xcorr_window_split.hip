// xcorr_window_split.hip -- the lag-window pass for FEW rows of LONG series (muse_batch_run_rows_windowed and its siblings): K split
// across workgroups.
//
// xcorr_window.hip gives 16 series to one workgroup and splits the samples over its four waves only, so a Muse.Run of 100 x 40 000
// samples is 7 workgroups on a 256-CU part.  Here the chunks of WIN_KC samples are cut into S slices of whole chunks and a grid of
// blocks x S workgroups (blocks = ceil(M / 16)) works on them; kernel boundaries are the only hand-off between workgroups:
//   xcorr_window_split_partial<TILES, WIDE>   grid blocks x S: the body of xcorr_window_mfma over the slice's chunks -- the same loads
//       (WIDE 16-byte and 8-byte forms), d = y - y[0], the same k-loop on v_mfma_f64_16x16x4_f64, the per-wave s1 / s2 and the sum
//       over the four waves in wave order -- then, instead of the scan, the summed tiles and the 16 series' (s1, s2) go out as one
//       slab of TILES * 256 + 32 doubles (plain vector stores) into slabs[(block * S + slice)];
//   window_split_finish<TILES>                grid blocks: sums the block's S slabs IN SLICE ORDER (deterministic: two calls give the
//       same bits) and runs xcorr_window_mfma's scan and write-out verbatim (NaN, sigma == 0 and all-zero-window rules, the
//       expression (S - mean pw[v]) inv_sigma).
// Numerics: S == 1 never comes here (launch_window_split refuses it: the caller takes launch_window, the existing kernel, untouched).
// At S > 1 the k-summation tree differs from xcorr_window_mfma's (partial sums per slice, then the slices), so a row's (lag, mv)
// equals the definition at the project's tolerance (1e-6 relative), not xcorr_window_mfma's result bit for bit.
//
// The planner (window_rows_plan, a pure host function) chooses S: see there.
#include "xcorr_kernels.h"

#include <algorithm>

namespace muse {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int WINS_THREADS = 256;
constexpr int WINS_ELDS = WIN_KC + WIN_E_TAIL; // doubles of e staged per chunk (as xcorr_window_mfma)

// the chunks of slice s of S: [s chunks / S, (s + 1) chunks / S) -- every slice floor(chunks / S) or one more
__host__ __device__ inline int window_slice_begin(int chunks, int S, int s) { return (int)((long long)s * chunks / S); }

int window_rows_plan(long long M, int N, int num_cus, int *chunks_per_slice)
{
    const long long blocks = (M + 15) / 16;
    const int chunks = (N + WIN_KC - 1) / WIN_KC;
    int S = 1;
    // the largest S that keeps blocks x S within the CUs (measured: 252 workgroups beat 126 at 63 blocks, 250 beat 125 at 25),
    // single-chunk slices up to WIN_ROWS_FULL_SPLIT of them, WIN_ROWS_MIN_CHUNKS chunks per slice beyond (xcorr_kernels.h)
    if (blocks >= 1 && blocks < num_cus && WIN_ROWS_SPLIT_ENABLED) {
        const int s_max = std::min(chunks, std::max(WIN_ROWS_FULL_SPLIT, chunks / WIN_ROWS_MIN_CHUNKS));
        S = (int)std::min<long long>(num_cus / blocks, s_max);
        if (S < 1)
            S = 1;
    }
    if (chunks_per_slice)
        *chunks_per_slice = (std::max(chunks, 1) + S - 1) / S;
    return S;
}

template <int TILES, bool WIDE>
__global__ __launch_bounds__(WINS_THREADS) void xcorr_window_split_partial(const WindowParams p, const int chunks, double *__restrict__ slabs)
{
    constexpr int RED = TILES * 256;                      // the summed accumulator tiles: [tile][lag row][series]
    constexpr int BUF = WINS_ELDS > RED ? WINS_ELDS : RED; // (the e image is dead when the tiles are summed: one region)
    constexpr int STAT = BUF;                             // [4 waves][16 series][2]
    __shared__ double lds[STAT + 128];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N;
    const int S = gridDim.y, slice = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); the finish kernel writes nothing of them
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];
    const int Tbeg = window_slice_begin(chunks, S, slice) * WIN_KC;
    const int Tlim = window_slice_begin(chunks, S, slice + 1) * WIN_KC;
    const int Tend = Tlim < N ? Tlim : N;

    v4d acc[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = Tbeg; T0 < Tend; T0 += WIN_KC) {
        if (T0 > Tbeg)
            __syncthreads();
        for (int v = t; v < WINS_ELDS; v += WINS_THREADS) // (the table is padded with zeros to whole chunks)
            lds[v] = p.e[T0 + v];
        __syncthreads();
        for (int s = wave; s < WIN_KC / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            // WIDE: k-step m = 2 mp + h <-> sample T + 8 mp + 2 q + h (one 16-byte load per two k-steps); else k-step m <-> sample
            // T + 4 m + q (8-byte loads: rows of any alignment) -- xcorr_window_mfma's piece, unchanged
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
            const double *a = lds + 64 * s + (WIDE ? 2 * q : q) + r;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                s1 += d[m];
                s2 = fma(d[m], d[m], s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(WIDE ? 8 * (m >> 1) + (m & 1) : 4 * m) + 16 * i], d[m], acc[i], 0, 0, 0);
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
    __syncthreads(); // every wave is done with the e image
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
    // the slab: [TILES][16 lag rows][16 series], then [16 series][s1, s2] (the waves in wave order)
    double *__restrict__ slab = slabs + ((long long)blockIdx.x * S + slice) * (RED + 32);
    for (int i = 2 * t; i < RED; i += 2 * WINS_THREADS)
        *reinterpret_cast<double2 *>(slab + i) = double2{lds[i], lds[i + 1]};
    if (t < 32) {
        double u = 0.0;
#pragma unroll
        for (int w = 0; w < 4; w++)
            u += lds[STAT + w * 32 + t];
        slab[RED + t] = u;
    }
}

template <int TILES>
__global__ __launch_bounds__(WINS_THREADS) void window_split_finish(const WindowParams p, const int S, const double *__restrict__ slabs)
{
    constexpr int RED = TILES * 256;
    constexpr int STAT = RED;        // [16 series][2]
    constexpr int CAND = STAT + 32;  // [16 parts][16 series][3]
    __shared__ double lds[CAND + 16 * 16 * 3];

    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 16;
    const double *__restrict__ slab = slabs + (long long)blockIdx.x * S * (RED + 32);
    for (int i = t; i < RED + 32; i += WINS_THREADS) {
        double u = slab[i];
        for (int s = 1; s < S; s++) // slice order
            u += slab[(long long)s * (RED + 32) + i];
        lds[i] = u;
    }
    __syncthreads();

    // the windowed maxAbsIndex: scan position pos = 0 .. W-1 <-> lag 0 .. L, -Lneg .. -1 (xcorr_window_mfma's, verbatim)
    const int c = t & 15, part = t >> 4;
    const int L = p.L, Lneg = p.Lneg, W = L + 1 + Lneg;
    const double t1 = lds[STAT + 2 * c], t2 = lds[STAT + 2 * c + 1];
    const double var = (t2 - t1 * t1 * p.invN) * p.invNm1;
    const bool nan = !__builtin_isfinite(var);
    const bool zero = !nan && !(var > 0.0);
    const double mean = t1 * p.invN;
    const double inv_sigma = 1.0 / sqrt(var);
    double best_abs = 0.0, best_val = 0.0, best_pos = -1.0;
#pragma unroll
    for (int k = 0; k < TILES; k++) {
        const int pos = part * TILES + k;
        if (pos < W) {
            const int v = pos <= L ? pos + L : pos - 1 - Lneg; // lag + L
            const double Sv = lds[(v >> 4) * 256 + (v & 15) * 16 + c];
            const double val = (Sv - mean * p.pw[v]) * inv_sigma;
            if (fabs(val) > best_abs) {
                best_abs = fabs(val);
                best_val = val;
                best_pos = (double)pos;
            }
        }
    }
    lds[CAND + (part * 16 + c) * 3] = best_abs;
    lds[CAND + (part * 16 + c) * 3 + 1] = best_val;
    lds[CAND + (part * 16 + c) * 3 + 2] = best_pos;
    __syncthreads();
    if (t < 16 && row0 + t < p.M) {
        double ba = 0.0, bv = 0.0;
        int bp = -1;
        for (int k = 0; k < 16; k++) {
            const double a = lds[CAND + (k * 16 + c) * 3];
            if (a > ba) {
                ba = a;
                bv = lds[CAND + (k * 16 + c) * 3 + 1];
                bp = (int)lds[CAND + (k * 16 + c) * 3 + 2];
            }
        }
        int lag = 0;
        double mv;
        if (nan) {
            mv = __builtin_nan("");
        } else if (zero) {
            mv = 0.0; // sigma == 0: (nil, 0, 0), xcorr.go:165-168
        } else if (bp < 0) { // only zeros or NaN in the window: index 0 stands
            mv = (lds[(L >> 4) * 256 + (L & 15) * 16 + c] - mean * p.pw[L]) * inv_sigma;
        } else {
            mv = bv;
            lag = bp <= L ? bp : bp - 1 - Lneg - L;
        }
        p.mv[row0 + t] = mv;
        p.lag[row0 + t] = lag;
    }
}

long long window_split_slab_doubles(int L) { return (long long)((2 * L + 1 + 15) / 16) * 256 + 32; }

hipError_t launch_window_split(const WindowParams &p, int S, double *slabs, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    const int chunks = (p.N + WIN_KC - 1) / WIN_KC;
    if (p.L < 0 || p.L > MUSE_LAG_WINDOW_MAX || p.Lneg < 0 || p.Lneg > p.L || p.N < 2 || S < 2 || S > chunks || !slabs)
        return hipErrorInvalidValue;
    const long long blocks = (p.M + 15) / 16;
    if (blocks > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)S), fgrid((unsigned)blocks), block(WINS_THREADS);
    const int W = 2 * p.L + 1; // lag + L runs up to 2 L whichever side the window drops
    const bool wide = window_wide(p.rows, p.stride);
#define MUSE_WINDOW_SPLIT_LAUNCH(T)                                                                     \
    do {                                                                                                \
        if (wide)                                                                                       \
            xcorr_window_split_partial<T, true><<<grid, block, 0, stream>>>(p, chunks, slabs);          \
        else                                                                                            \
            xcorr_window_split_partial<T, false><<<grid, block, 0, stream>>>(p, chunks, slabs);         \
        window_split_finish<T><<<fgrid, block, 0, stream>>>(p, S, slabs);                               \
    } while (0)
    switch ((W + 15) / 16) { // accumulator tiles of 16 lags
    case 1: MUSE_WINDOW_SPLIT_LAUNCH(1); break;
    case 2: MUSE_WINDOW_SPLIT_LAUNCH(2); break;
    case 3: MUSE_WINDOW_SPLIT_LAUNCH(3); break;
    case 4: MUSE_WINDOW_SPLIT_LAUNCH(4); break;
    case 5: MUSE_WINDOW_SPLIT_LAUNCH(5); break;
    case 6: MUSE_WINDOW_SPLIT_LAUNCH(6); break;
    case 7: MUSE_WINDOW_SPLIT_LAUNCH(7); break;
    default: MUSE_WINDOW_SPLIT_LAUNCH(8); break;
    }
#undef MUSE_WINDOW_SPLIT_LAUNCH
    return hipGetLastError();
}

} // namespace muse
