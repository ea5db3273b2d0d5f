// xcorr_window_split.hip -- the lag-window pass for FEW rows of LONG series (muse_batch_run_rows_windowed and its siblings): K split
// across workgroups.
//
// xcorr_window.hip gives 16 series to one workgroup and splits the samples over its four waves only, so a Muse.Run of 100 x 40 000
// samples is 7 workgroups on a 256-CU part.  Here the chunks of WIN_KC samples are cut into S slices of whole chunks and a grid of
// blocks x S workgroups (blocks = ceil(M / 16)) works on them; kernel boundaries are the only hand-off between workgroups:
//   xcorr_window_split_partial<TILES, WIDE>   grid blocks x S: the body of xcorr_window_mfma over the slice's chunks, out of the same
//       functions (window_device.h: the piece's loads in their WIDE 16-byte and 8-byte forms, d = y - y[0], the k-loop on
//       v_mfma_f64_16x16x4_f64, the per-wave s1 / s2 and the sum over the four waves in wave order) -- then, instead of the scan, the
//       summed tiles and the 16 series' (s1, s2) go out as one
//       slab of TILES * 256 + 32 doubles (plain vector stores) into slabs[(block * S + slice)];
//   window_split_finish<TILES>                grid blocks: sums the block's S slabs IN SLICE ORDER (deterministic: two calls give the
//       same bits) and calls window_scan_write, the scan and write-out xcorr_window_mfma calls (NaN, sigma == 0 and all-zero-window
//       rules, the expression (S - mean pw[v]) inv_sigma).
// Numerics: S == 1 never comes here (launch_window_split refuses it: the caller takes launch_window, the existing kernel, untouched).
// At S > 1 the k-summation tree differs from xcorr_window_mfma's (partial sums per slice, then the slices), so a row's (lag, mv)
// equals the definition at the project's tolerance (1e-6 relative), not xcorr_window_mfma's result bit for bit.
//
// The table may start at any lag (WindowShape::origin: a symmetric window's L, or the lowest lag of a lag range --
// muse_batch_run_rows_in_lag_range): the slabs are sized and TILES picked by window_tiles(const WindowShape &).
//
// The planner (window_rows_plan, a pure host function) chooses S: see there.
#include "window_device.h"

#include <algorithm>

namespace muse {

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
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_split_partial(const WindowParams p, const int chunks, double *__restrict__ slabs)
{
    constexpr int RED = WindowLds<TILES>::RED, STAT = WindowLds<TILES>::STAT; // (no scan here: nothing behind the statistics)
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
        window_stage_e(lds, p.e + T0, t);
        __syncthreads();
        for (int s = wave; s < WIN_KC / 64; s += 4) {
            const int T = T0 + 64 * s;
            if (T >= N)
                break;
            double d[16];
            window_load_piece<WIDE>(d, y, y0, T, N, q);
            window_mac_piece<TILES, WIDE>(acc, s1, s2, [&](int m) { return d[m]; }, lds, s, r, q);
        }
    }
    window_sum_tiles<TILES>(lds, STAT, acc, s1, s2, wave, r, q);
    // the slab: [TILES][16 lag rows][16 series], then [16 series][s1, s2] (the waves in wave order)
    double *__restrict__ slab = slabs + ((long long)blockIdx.x * S + slice) * (RED + 32);
    for (int i = 2 * t; i < RED; i += 2 * WIN_THREADS)
        *reinterpret_cast<double2 *>(slab + i) = double2{lds[i], lds[i + 1]};
    if (t < 32)
        slab[RED + t] = window_wave_sum(lds, STAT, t);
}

template <int TILES>
__global__ __launch_bounds__(WIN_THREADS) void window_split_finish(const WindowParams p, const int S, const double *__restrict__ slabs)
{
    constexpr int RED = TILES * 256;
    constexpr int STAT = RED;        // [16 series][2]
    constexpr int CAND = STAT + 32;  // [16 parts][16 series][3]
    __shared__ double lds[CAND + 16 * 16 * 3];

    const int t = threadIdx.x;
    const double *__restrict__ slab = slabs + (long long)blockIdx.x * S * (RED + 32);
    for (int i = t; i < RED + 32; i += WIN_THREADS) {
        double u = slab[i];
        for (int s = 1; s < S; s++) // slice order
            u += slab[(long long)s * (RED + 32) + i];
        lds[i] = u;
    }
    __syncthreads();
    // behind another way of filling LDS, the scan and the write-out of xcorr_window_mfma (window_finish calls the same function)
    const int c = t & 15;
    window_scan_write<TILES>(lds, CAND, lds[STAT + 2 * c], lds[STAT + 2 * c + 1], p, (long long)blockIdx.x * 16, t);
}

long long window_split_slab_doubles(const WindowShape &p) { return (long long)window_tiles(p) * 256 + 32; }

hipError_t launch_window_split(const WindowParams &p, int S, double *slabs, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    const int chunks = (p.N + WIN_KC - 1) / WIN_KC;
    long long blocks;
    // (a table of any origin: the slabs are sized by window_split_slab_doubles(p), the tiles of rows 0 .. origin + L)
    if (window_launch_check(p, &blocks) != hipSuccess || S < 2 || S > chunks || !slabs)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)S), fgrid((unsigned)blocks), block(WIN_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
    window_with_tiles(window_tiles(p), [&](auto tiles) {
        if (wide)
            xcorr_window_split_partial<tiles(), true><<<grid, block, 0, stream>>>(p, chunks, slabs);
        else
            xcorr_window_split_partial<tiles(), false><<<grid, block, 0, stream>>>(p, chunks, slabs);
        window_split_finish<tiles()><<<fgrid, block, 0, stream>>>(p, S, slabs);
    });
    return hipGetLastError();
}

} // namespace muse
