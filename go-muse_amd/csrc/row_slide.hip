// row_slide.hip -- rows of a resident group moved forward in time, in place in HBM (muse_group_slide: capi_group.hip):
//     row r  <-  old row r [k .. N)  followed by  tails[r][0 .. k),      r < count
//
// A left shift inside a row overlaps its own source.  The rules that make it free of races by construction:
//   1. ONE OWNER PER ROW.  A row is shifted by exactly one wave, from its first sample to its last; no other wave or workgroup
//      touches that row in the launch, and nothing is handed from one workgroup to another.  Rows are independent: the four
//      waves of a 256-thread workgroup take four rows, a grid of at most SLIDE_WGS_PER_CU workgroups per CU strides over the rows.
//   2. LOADS COMPLETE BEFORE THE OVERLAPPING STORES.  The owner walks its row left to right in pieces of P = 64 x SLIDE_UNROLL
//      vector units (the register gather of MI355X_MICROARCH.md § "Indexed rows", as row_gather.hip).  For piece p it issues every
//      load of the source range [pP + k, pP + P + k), waits until EVERY one of them has returned -- an explicit s_waitcnt vmcnt(0),
//      not the per-register waits the compiler puts in front of the first store's operand -- and only then issues the stores to
//      [pP, pP + P).
//   3. Piece p + 1 reads only addresses at or above (p + 1) P + k, which no store issued so far has touched (those lie below
//      (p + 1) P): nothing else needs ordering.  A lane behind the end of the kept samples loads the row's last unit instead of
//      branching around the load (that unit is not stored to before rule 4) and stores nothing.
//   4. After the last piece the owner writes the k tail samples from the device tails buffer (count x k, dense) into [N - k, N).
//   5. A row index at or beyond `count` ends the wave's loop: it is masked, never clamped onto a neighbouring row.  Nothing is
//      stored outside rows [0, count) of `rows`: the guard in front of row 0, the rows outside the range and the rows behind the
//      last one are never written.
//
// Vector width: row_gather.hip's rule with two offsets.  Rows lie N elements apart behind a 256-byte aligned base and the source
// of a store lies k elements further, so the unit is the widest of 16 / 8 (/ 4 for float32) bytes that divides both N x elem and
// k x elem (slide_unit_bytes, a pure host function): float64 rows with odd k or odd N move in 8-byte units.  The tails buffer is
// 256-byte aligned and row r's tail starts k elements x r into it: aligned for the same unit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "xcorr_kernels.h"

namespace muse {
namespace {

constexpr int SLIDE_UNROLL = 8;       // vector units per lane in flight: 8 KB per wave for 16-byte units
constexpr int SLIDE_WGS_PER_CU = 8;   // 32 waves per CU, 256 KB of reads in flight per CU

template <class T, int K> struct SlideVec { using type = T __attribute__((ext_vector_type(K))); };
template <class T> struct SlideVec<T, 1> { using type = T; };

// upr = N / K units per row, ku = k / K units of shift (1 <= ku <= upr)
template <class T, int K>
__global__ __launch_bounds__(256) void row_slide_kernel(T *rows, const T *__restrict__ tails, long long count, int upr, int ku)
{
    using V = typename SlideVec<T, K>::type;
    constexpr int P = 64 * SLIDE_UNROLL;
    const int lane = threadIdx.x & 63;
    const int keep = upr - ku; // units of the row that stay (moved to its front)
    const long long wstep = (long long)gridDim.x * 4;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < count; r += wstep) { // (wave-uniform)
        V *row = (V *)rows + r * upr;
        for (int u0 = 0; u0 < keep; u0 += P) {
            V v[SLIDE_UNROLL];
#pragma unroll
            for (int j = 0; j < SLIDE_UNROLL; j++)
                v[j] = row[min(u0 + j * 64 + lane + ku, upr - 1)];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every load of the piece has returned: rule 2
#pragma unroll
            for (int j = 0; j < SLIDE_UNROLL; j++) {
                const int u = u0 + j * 64 + lane;
                if (u < keep)
                    row[u] = v[j];
            }
        }
        const V *tail = (const V *)tails + r * ku;
        for (int u0 = 0; u0 < ku; u0 += P) {
            V v[SLIDE_UNROLL];
#pragma unroll
            for (int j = 0; j < SLIDE_UNROLL; j++)
                v[j] = tail[min(u0 + j * 64 + lane, ku - 1)];
#pragma unroll
            for (int j = 0; j < SLIDE_UNROLL; j++) {
                const int u = u0 + j * 64 + lane;
                if (u < ku)
                    row[keep + u] = v[j];
            }
        }
    }
}

template <class T, int K>
hipError_t slide_as(T *rows, const T *tails, long long count, int N, int k, int num_cus, hipStream_t stream)
{
    const long long wgs = std::min<long long>((count + 3) / 4, (long long)std::max(num_cus, 1) * SLIDE_WGS_PER_CU);
    hipLaunchKernelGGL((row_slide_kernel<T, K>), dim3((unsigned)wgs), dim3(256), 0, stream, rows, tails, count, N / K, k / K);
    return hipGetLastError();
}

} // namespace

int slide_unit_bytes(int N, int k, bool f32)
{
    const long long elem = f32 ? 4 : 8;
    for (long long u = 16; u > elem; u /= 2)
        if ((N * elem) % u == 0 && (k * elem) % u == 0)
            return (int)u;
    return (int)elem;
}

hipError_t launch_row_slide(void *rows, bool f32, long long count, int N, int k, const void *tails, int num_cus,
                            hipStream_t stream)
{
    if (count <= 0 || k == 0)
        return hipSuccess;
    if (N < 1 || k < 0 || k > N || !rows || !tails)
        return hipErrorInvalidValue;
    const int unit = slide_unit_bytes(N, k, f32);
    if (f32) {
        if (unit == 16)
            return slide_as<float, 4>((float *)rows, (const float *)tails, count, N, k, num_cus, stream);
        if (unit == 8)
            return slide_as<float, 2>((float *)rows, (const float *)tails, count, N, k, num_cus, stream);
        return slide_as<float, 1>((float *)rows, (const float *)tails, count, N, k, num_cus, stream);
    }
    if (unit == 16)
        return slide_as<double, 2>((double *)rows, (const double *)tails, count, N, k, num_cus, stream);
    return slide_as<double, 1>((double *)rows, (const double *)tails, count, N, k, num_cus, stream);
}

} // namespace muse
