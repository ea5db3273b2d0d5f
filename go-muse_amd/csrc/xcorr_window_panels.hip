// xcorr_window_panels.hip -- the lag-range pass for FEW rows and MANY lags (muse_batch_run_rows_in_lag_range and its siblings,
// 128 ... MUSE_RUN_ROWS_LAG_RANGE_MAX lags): the lags split across workgroups as well as the samples.
//
// One workgroup holds eight accumulator tiles: 128 rows of the product table (row v = lag v - origin).  A wider table is cut into
// PANELS of 128 rows, panels = ceil(W / 128) <= 16, and the chunks of WIN_KC samples into S slices as in xcorr_window_split.hip; a
// grid of blocks x S x panels workgroups (blocks = ceil(M / 16)) works on them, kernel boundaries are the only hand-off:
//   xcorr_window_panel_partial<TILES, WIDE>   grid (blocks, S, panels): the body of xcorr_window_split_partial out of the same
//       functions (window_device.h), the staged image of panel z being e[T0 + 128 z .. + WIN_ELDS) -- the table's rows 128 z ..
//       128 z + 127 are the lags of that image's rows 0 .. 127.  Per (block, panel, slice) one slab of TILES * 256 + 32 doubles goes
//       out (plain vector stores): the summed tiles and the 16 series' (s1, s2).  S == 1 is a legal launch: the k-order of a lag row
//       is then xcorr_window_mfma's.  Every panel is built with all eight tiles; rows >= W are computed and never scanned.
//   window_panels_finish                      grid blocks: per panel, in panel order, the S slabs summed IN SLICE ORDER into LDS, then
//       16 parts per series scan the panel's rows with window_score (the expression and the window_stats of every window kernel).
//       Panels arrive in table order, not in the scan order of the definition (lags 0 .. hi, then lo .. -1, strict '>', first
//       index wins), so a candidate carries its scan position pos = lag >= 0 ? lag : hi + 1 + (lag - lo) and replaces the best iff
//       |val| > best.abs, or |val| == best.abs and pos < best.pos: a total order that picks what strict '>' picks in scan order.
//       NaN never wins.  cc[0] (row `origin`) is kept as its panel passes, for the "only zeros or NaN in the range" outcome; the
//       outcomes are window_outcome's.  (s1, s2) are panel 0's: every panel computes the same bits.
// Numerics: at S == 1 the value at a lag has the bits the direct product of muse_batch_score_in_lag_range gives at that lag for the
// same rows at the same alignment (the same k order, the same pw entry, the same statistics); at S > 1 the definition at the
// project's tolerance; two calls give the same bits at any S.
#include "window_device.h"

#include <algorithm>

namespace muse {

// the tables of a table of up to WIN_PANEL_MAX_ROWS rows: window_table_e / window_table_p of xcorr_window.hip restated (the same
// expressions and the same summation order, so pw[v] has the bits the narrow table has for the same lag), for an image that runs on
// behind the last chunk by the panels' offsets
__global__ __launch_bounds__(256) void window_panels_table_e(const double *__restrict__ xs, int N, int n, int origin, int W, long long len,
                                                             double *__restrict__ e)
{
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= len)
        return;
    double x = 0.0;
    if (v < (long long)N + W - 1) {
        long long idx = ((long long)(n - N) + v - origin) % n;
        if (idx < 0)
            idx += n;
        x = xs[idx];
    }
    e[v] = x;
}

__global__ __launch_bounds__(256) void window_panels_table_p(const double *__restrict__ e, int N, double *__restrict__ pw)
{
    __shared__ double part[256];
    const int v = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < N; i += 256)
        s += e[i + v];
    part[t] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            part[t] += part[t + h];
        __syncthreads();
    }
    if (t == 0)
        pw[v] = part[0];
}

int window_panels(int W) { return (W + WIN_PANEL_ROWS - 1) / WIN_PANEL_ROWS; }

long long window_panels_e_len(int N, int W)
{
    return (long long)((N + WIN_KC - 1) / WIN_KC) * WIN_KC + (long long)WIN_PANEL_ROWS * (window_panels(W) - 1) + WIN_E_TAIL;
}

hipError_t launch_window_tables_wide(const double *xs, int N, int n, int origin, int W, double *e, long long e_len, double *pw,
                                     hipStream_t stream)
{
    if (origin < 0 || W < origin + 1 || W > WIN_PANEL_MAX_ROWS || N < 2 || e_len < window_panels_e_len(N, W))
        return hipErrorInvalidValue;
    window_panels_table_e<<<dim3((unsigned)((e_len + 255) / 256)), dim3(256), 0, stream>>>(xs, N, n, origin, W, e_len, e);
    window_panels_table_p<<<dim3((unsigned)W), dim3(256), 0, stream>>>(e, N, pw);
    return hipGetLastError();
}

// the slice count of the panel pass (measured: xcorr_kernels.h, window_panels_plan): the partial kernel's time falls as chunks / S,
// the finish kernel adds a block's panels x S slabs one after the other -- the two balance at S ~ sqrt(WIN_PANEL_BALANCE chunks /
// panels), rounded: the largest S with (2 S - 1)^2 panels <= 4 WIN_PANEL_BALANCE chunks; never more workgroups than CUs
int window_panels_plan(long long M, int N, int num_cus, int W, int *panels_out)
{
    const long long blocks = (M + 15) / 16;
    const int chunks = (N + WIN_KC - 1) / WIN_KC;
    const int panels = window_panels(W);
    if (panels_out)
        *panels_out = panels;
    const long long wgs = blocks * panels;
    int S = 1;
    if (wgs >= 1 && wgs < num_cus && WIN_ROWS_SPLIT_ENABLED) {
        while (S < chunks && (long long)(2 * S + 1) * (2 * S + 1) * panels <= 4LL * WIN_PANEL_BALANCE * chunks)
            S++;
        S = (int)std::min<long long>(S, num_cus / wgs);
        if (S < 1)
            S = 1;
    }
    return S;
}

// the chunks of slice s of S, as xcorr_window_split.hip cuts them
__host__ __device__ inline int panel_slice_begin(int chunks, int S, int s) { return (int)((long long)s * chunks / S); }

template <int TILES, bool WIDE>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_panel_partial(const WindowParams p, const int chunks, double *__restrict__ slabs)
{
    constexpr int RED = WindowLds<TILES>::RED, STAT = WindowLds<TILES>::STAT; // (no scan here: nothing behind the statistics)
    __shared__ double lds[STAT + 128];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N;
    const int S = gridDim.y, slice = blockIdx.y;
    const int panels = gridDim.z, panel = blockIdx.z;
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    if (row >= p.M) // masked tail rows read the last row (valid memory); the finish kernel writes nothing of them
        row = p.M - 1;
    const double *__restrict__ y = p.rows + row * p.stride;
    const double y0 = y[0];
    const double *__restrict__ e = p.e + panel * WIN_PANEL_ROWS; // the panel's image: its row 0 is the table's row 128 panel
    const int Tbeg = panel_slice_begin(chunks, S, slice) * WIN_KC;
    const int Tlim = panel_slice_begin(chunks, S, slice + 1) * WIN_KC;
    const int Tend = Tlim < N ? Tlim : N;

    v4d acc[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = Tbeg; T0 < Tend; T0 += WIN_KC) {
        if (T0 > Tbeg)
            __syncthreads();
        window_stage_e(lds, e + T0, t);
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
    double *__restrict__ slab = slabs + (((long long)blockIdx.x * panels + panel) * S + slice) * (RED + 32);
    for (int i = 2 * t; i < RED; i += 2 * WIN_THREADS)
        *reinterpret_cast<double2 *>(slab + i) = double2{lds[i], lds[i + 1]};
    if (t < 32)
        slab[RED + t] = window_wave_sum(lds, STAT, t);
}

// candidate (a, val, pos) against the best: the total order of the header
__device__ __forceinline__ void panel_take(WindowBest &best, const double a, const double val, const double pos)
{
    if (a > best.abs || (a == best.abs && pos < best.pos)) { // (a == 0 never passes: best.pos starts at -1; NaN compares false)
        best.abs = a;
        best.val = val;
        best.pos = pos;
    }
}

__global__ __launch_bounds__(WIN_THREADS) void window_panels_finish(const WindowParams p, const int S, const int panels,
                                                                    const double *__restrict__ slabs)
{
    constexpr int TILES = WIN_PANEL_ROWS / 16;
    constexpr int RED = TILES * 256;
    constexpr int STAT = RED;                  // [16 series][2]
    constexpr int CAND = STAT + 32;            // [16 parts][16 series][3]
    constexpr int CC0 = CAND + 16 * 16 * 3;    // [16 series] cc at lag 0
    __shared__ double lds[CC0 + 16];

    const int t = threadIdx.x;
    const int c = t & 15, part = t >> 4;
    const int W = p.origin + p.L + 1;
    WindowStats st{};
    WindowBest best;
    for (int z = 0; z < panels; z++) {
        const double *__restrict__ slab = slabs + ((long long)blockIdx.x * panels + z) * S * (RED + 32);
        if (z > 0)
            __syncthreads(); // the scan of the panel before is done with the tiles
        for (int i = t; i < RED + 32; i += WIN_THREADS) {
            double u = slab[i];
            for (int s = 1; s < S; s++) // slice order
                u += slab[(long long)s * (RED + 32) + i];
            lds[i] = u;
        }
        __syncthreads();
        if (z == 0)
            st = window_stats(lds[STAT + 2 * c], lds[STAT + 2 * c + 1], p.invN, p.invNm1);
        const double *__restrict__ pw = p.pw + z * WIN_PANEL_ROWS;
#pragma unroll
        for (int k = 0; k < TILES; k++) {
            const int row = part * TILES + k;       // of the panel
            const int lag = z * WIN_PANEL_ROWS + row - p.origin;
            if (z * WIN_PANEL_ROWS + row < W && lag >= -p.Lneg) {
                const double val = window_score(lds, 0, row, c, st, pw);
                if (lag == 0)
                    lds[CC0 + c] = val;
                panel_take(best, fabs(val), val, (double)(lag >= 0 ? lag : p.L + 1 + lag + p.Lneg));
            }
        }
    }
    window_put_best(lds + CAND + (part * 16 + c) * 3, best);
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * 16;
    if (t < 16 && row0 + t < p.M) {
        WindowBest all;
        for (int k = 0; k < 16; k++) {
            const double *cand = lds + CAND + (k * 16 + c) * 3;
            if (cand[2] >= 0.0)
                panel_take(all, cand[0], cand[1], cand[2]);
        }
        int lag = 0;
        double mv;
        if (st.nan)
            mv = __builtin_nan("");
        else if (st.zero)
            mv = 0.0; // sigma == 0: (nil, 0, 0), xcorr.go:165-168
        else if (all.pos < 0.0) // only zeros or NaN in the range: index 0 stands
            mv = lds[CC0 + c];
        else {
            const int bp = (int)all.pos;
            lag = bp <= p.L ? bp : bp - 1 - p.Lneg - p.L;
            mv = all.val;
        }
        p.mv[row0 + t] = mv;
        p.lag[row0 + t] = lag;
    }
}

long long window_panels_slab_doubles() { return (long long)(WIN_PANEL_ROWS / 16) * 256 + 32; }

hipError_t launch_window_panels(const WindowParams &p, int S, double *slabs, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    const int chunks = (p.N + WIN_KC - 1) / WIN_KC;
    const int W = p.origin + p.L + 1;
    const long long blocks = (p.M + 15) / 16;
    // rows 0 .. W - 1 of the table: within pw, the panels and the images' tails (window_panels_e_len)
    if (p.L < 0 || p.Lneg < 0 || p.origin < p.Lneg || W > WIN_PANEL_MAX_ROWS || p.N < 2 || blocks > 0x7fffffffLL || S < 1 || S > chunks ||
        !slabs || !p.e || !p.pw)
        return hipErrorInvalidValue;
    const int panels = window_panels(W);
    const dim3 grid((unsigned)blocks, (unsigned)S, (unsigned)panels), fgrid((unsigned)blocks), block(WIN_THREADS);
    constexpr int TILES = WIN_PANEL_ROWS / 16;
    if (window_wide(p.rows, p.stride))
        xcorr_window_panel_partial<TILES, true><<<grid, block, 0, stream>>>(p, chunks, slabs);
    else
        xcorr_window_panel_partial<TILES, false><<<grid, block, 0, stream>>>(p, chunks, slabs);
    window_panels_finish<<<fgrid, block, 0, stream>>>(p, S, panels, slabs);
    return hipGetLastError();
}

} // namespace muse
