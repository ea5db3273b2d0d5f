// xcorr_window_slide.hip -- a resident group's rows moved forward in time AND scored inside a lag window in ONE pass over HBM
// (muse_batch_slide_score_windowed: capi_window.hip).  It is xcorr_window_mfma (xcorr_window.hip) over the NEW row
//     new row r [t]  =  old row r [t + k]            for t < N - k
//                       tails[r k + t - (N - k)]     otherwise       (the dense device tails buffer of muse_group_slide)
// and every sample a lane has loaded for the product is also stored to position t of the same row: 2 x 8 N M bytes cross HBM where
// muse_group_slide followed by the windowed pass moves 3 x.
//
// THE ARITHMETIC IS xcorr_window_mfma's, to the bit, because it is the same functions (window_device.h): 16 series per 256-thread
// workgroup, e staged per chunk of WIN_KC samples (window_stage_e), piece p of a chunk on wave p mod 4, the lane -> sample mapping of
// the WIDE / narrow build (window_k), d = y - y0, s1 / s2 and the MFMA order (the k-loop of window_mac_piece, written out below), and
// window_finish behind it.  The loader is this kernel's own: two sources, the raw values kept for the store, explicit waits.  WIDE is the MAPPING and follows window_wide() of the rows, so that a later stand-alone
// pass over the slid rows sums in the same order; LOAD16 is only the width of the loads (slide_score_plan): a WIDE lane's two
// consecutive samples come from one 16-byte load when k is even (row + k, every tail row r k and N - k are then even: aligned, and
// no pair straddles the kept / tail boundary), from two 8-byte loads otherwise.  Stores are 16-byte in WIDE builds (the destination
// is the aligned row itself), 8-byte in narrow ones.
//
// A row is shifted onto its own source and four waves share a row's pieces.  The rules that order it, by construction:
//   1. y0.  The new row's first sample is old row[k] (tails[r][0] when k == N).  EVERY wave loads it, and waits for it with an
//      explicit s_waitcnt vmcnt(0), ahead of the first workgroup barrier (the one behind the staging of the first chunk's e image).
//      No wave stores anything before that barrier: the store to piece 0 overwrites address k whenever k < 64.
//   2. ROUNDS.  The pieces are taken in rounds of four, one per wave, in the order xcorr_window_mfma takes them (round j of a chunk:
//      piece 4 j + wave).  In a round each wave issues every load of its piece, waits until ALL of them have returned (an explicit
//      s_waitcnt vmcnt(0), as row_slide.hip: not the per-register waits the compiler would put in front of each use), passes the
//      round's workgroup barrier, and only then stores its piece and feeds it to the matrix pipe.
//      So the store to destination piece p is issued only after the loads of every piece <= p, by every wave, have returned: piece p'
//      reads [64 p' + k, 64 p' + 64 + k), which overlaps only the destinations of pieces >= p'.
//   3. Loads of round j + 1 may be issued before or after the stores of round j: they read at or above 64 x 4 (j + 1) + k, which the
//      stores of rounds <= j (below 64 x 4 (j + 1)) never reach.  The barriers at chunk boundaries stay as they are.
//   4. HAND-OFFS.  Workgroup barriers and the kernel's boundaries are the only ones: no counters between workgroups, no fences.  A row
//      is touched by exactly one workgroup.
//   5. PARTIAL LAST BLOCK.  Lanes beyond the last row of a partial 16-row block read the LAST row of the range -- whose owner lane
//      is in the same workgroup and in the same load instruction, under the same rules -- and store nothing.
//   6. OUT OF BOUNDS.  Stores go to samples t < N of rows r < M only: the guard in front of row 0 and the memory behind row M are
//      never written.  A piece touching the tail selects per sample (per pair with 16-byte loads) between the row and the tails
//      buffer; a lane past N loads the start of its tail row (valid, never written), contributes 0.0 as in xcorr_window_mfma and
//      stores nothing.
// The raw samples stay in registers for the store (16 doubles); d is formed from them at use.  No build uses scratch memory
// (tools/kernel_resources.py).
#include "window_device.h"

namespace muse {

template <int TILES, bool WIDE, bool LOAD16>
__global__ __launch_bounds__(WIN_THREADS) void xcorr_window_slide_mfma(const WindowParams p, const double *__restrict__ tails, const int k)
{
    static_assert(WIDE || !LOAD16, "16-byte loads belong to the WIDE mapping");
    __shared__ double lds[WindowLds<TILES>::SIZE];

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int N = p.N;
    const int keep = N - k; // samples of the old row that stay (moved to its front)
    const long long row0 = (long long)blockIdx.x * 16;
    long long row = row0 + r;
    const bool owner = row < p.M;
    if (!owner) // rule 5
        row = p.M - 1;
    double *y = const_cast<double *>(p.rows) + row * p.stride; // (read AND written: no __restrict__)
    const double *__restrict__ tl = tails + row * k;
    const double y0 = keep > 0 ? y[k] : tl[0];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // rule 1: y0 has returned ahead of the first barrier

    v4d acc[TILES];
#pragma unroll
    for (int i = 0; i < TILES; i++)
        acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double s1 = 0.0, s2 = 0.0;

    for (int T0 = 0; T0 < N; T0 += WIN_KC) {
        if (T0 > 0)
            __syncthreads();
        window_stage_e(lds, p.e + T0, t);
        __syncthreads();
        for (int s0 = 0; s0 < WIN_KC / 64 && T0 + 64 * s0 < N; s0 += 4) { // a round: uniform over the workgroup
            const int s = s0 + wave;
            const int T = T0 + 64 * s;
            const bool active = T < N;         // (wave-uniform) the round's last pieces may lie behind the row
            const bool kept = T + 64 <= keep;  // (wave-uniform) the whole piece comes from the old row
            // k-step m of this lane <-> sample T + window_k<WIDE>(m, q) (window_device.h)
            double raw[16];
            if (active && kept) {
                const double *src = y + k + T;
                if (LOAD16) {
#pragma unroll
                    for (int mp = 0; mp < 8; mp++) {
                        const double2 v = *reinterpret_cast<const double2 *>(src + window_a<true>(2 * mp) + window_k<true>(0, q));
                        raw[2 * mp] = v.x;
                        raw[2 * mp + 1] = v.y;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 16; m++)
                        raw[m] = src[window_k<WIDE>(m, q)];
                }
            } else if (active) {
                if (LOAD16) { // N, k even: both samples of a pair lie on the same side of N - k and of N
#pragma unroll
                    for (int mp = 0; mp < 8; mp++) {
                        const int tt = T + window_k<true>(2 * mp, q);
                        const double *src = tt < keep ? y + tt + k : (tt < N ? tl + (tt - keep) : tl);
                        const double2 v = *reinterpret_cast<const double2 *>(src);
                        raw[2 * mp] = v.x;
                        raw[2 * mp + 1] = v.y;
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 16; m++) {
                        const int tt = T + window_k<WIDE>(m, q);
                        const double *src = tt < keep ? y + tt + k : (tt < N ? tl + (tt - keep) : tl);
                        raw[m] = *src;
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // rule 2: every load of the wave's piece has returned ...
            __syncthreads();                                 // ... and so has every load of every piece up to this round
            if (!active)
                continue;
            if (owner) {
                if (WIDE) { // (N is even: a pair is stored whole or not at all)
#pragma unroll
                    for (int mp = 0; mp < 8; mp++) {
                        const int tt = T + window_k<true>(2 * mp, q);
                        if (tt < N)
                            *reinterpret_cast<double2 *>(y + tt) = double2{raw[2 * mp], raw[2 * mp + 1]};
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 16; m++) {
                        const int tt = T + window_k<false>(m, q);
                        if (tt < N)
                            y[tt] = raw[m];
                    }
                }
            }
            const bool whole = T + 64 <= N;
            // (the k-loop of window_mac_piece, written out with d formed at use: through the function four shapes of
            // tools/slide_score_bench.py measured 1 ... 2 % slower; profiles/window_refactor.txt)
            const double *a = lds + 64 * s + window_k<WIDE>(0, q) + r;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                const double d = whole || T + window_k<WIDE>(m, q) < N ? raw[m] - y0 : 0.0;
                s1 += d;
                s2 = fma(d, d, s2);
#pragma unroll
                for (int i = 0; i < TILES; i++)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[window_a<WIDE>(m) + 16 * i], d, acc[i], 0, 0, 0);
            }
        }
    }
    window_finish<TILES>(lds, acc, s1, s2, p, row0, t, wave, r, q);
}

void slide_score_plan(int N, int k, bool wide, int *load_bytes, int *store_bytes)
{
    (void)N; // (WIDE rows have an even N: with an even k every pair of the new row has one aligned source)
    *load_bytes = wide && k % 2 == 0 ? 16 : 8;
    *store_bytes = wide ? 16 : 8;
}

hipError_t launch_window_slide(const WindowParams &p, const double *tails, int k, hipStream_t stream)
{
    if (p.M <= 0)
        return hipSuccess;
    long long blocks;
    if (window_launch_check(p, &blocks) != hipSuccess || p.origin != p.L || p.Lneg > p.L) // (its callers' windows are symmetric)
        return hipErrorInvalidValue;
    // dense rows (a group's: the slide is defined on them), 1 <= k <= N (k == 0 is launch_window's), tails 16-byte aligned
    if (p.stride != p.N || k < 1 || k > p.N || !tails || !p.rows || ((uintptr_t)tails & 15) != 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(WIN_THREADS);
    const bool wide = window_wide(p.rows, p.stride);
    int load_bytes = 8, store_bytes = 8;
    slide_score_plan(p.N, k, wide, &load_bytes, &store_bytes);
    window_with_tiles(window_tiles(p.L), [&](auto tiles) {
        if (wide && load_bytes == 16)
            xcorr_window_slide_mfma<tiles(), true, true><<<grid, block, 0, stream>>>(p, tails, k);
        else if (wide)
            xcorr_window_slide_mfma<tiles(), true, false><<<grid, block, 0, stream>>>(p, tails, k);
        else
            xcorr_window_slide_mfma<tiles(), false, false><<<grid, block, 0, stream>>>(p, tails, k);
    });
    return hipGetLastError();
}

} // namespace muse
