// row_gather.hip -- rows of one resident group copied into another, HBM -> HBM, by an index list in device memory:
//     dst row i = src row idx[i], i < count      (muse_group_append_from, muse_batch_run_group_rows: capi_group.hip, capi_rows.hip)
//
// The register gather of MI355X_MICROARCH.md § "Indexed rows": one wave per destination piece of 64 x UNROLL vector units, all
// UNROLL loads issued before the first store, a grid of at most GATHER_WGS_PER_CU four-wave workgroups per CU that strides over
// the pieces.  Short rows put several rows into one piece (a lane finds its row by one 32-bit division), long rows (up to
// 2^20 samples) are cut into pieces, so every wave moves the same bytes whatever N is.
//
// Alignment: rows lie N elements apart behind a 256-byte aligned base, so a unit of K elements is aligned for every row as
// soon as K divides N.  K = 16 bytes of the source when N allows it, else 8, else one element (float64 rows of odd length
// move in 8-byte units: the parity of idx[i] and of the destination row never has to agree).  Nothing is written outside
// rows [0, count) of dst: the guard in front of row 0 and the rows behind the last one are never touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "xcorr_kernels.h"

namespace muse {
namespace {

constexpr int GATHER_UNROLL = 8;       // vector units per lane in flight: 8 KB per wave for 16-byte units
constexpr int GATHER_WGS_PER_CU = 8;   // 32 waves per CU, 256 KB of reads in flight per CU

template <class T, int K> struct Vec { using type = T __attribute__((ext_vector_type(K))); };
template <class T> struct Vec<T, 1> { using type = T; };

template <class VO, class VI> __device__ inline VO widen(VI v)
{
    if constexpr (std::is_same<VO, VI>::value || std::is_arithmetic<VI>::value)
        return (VO)v;
    else
        return __builtin_convertvector(v, VO);
}

template <class TI, class TO, int K, bool NT>
__global__ __launch_bounds__(256) void row_gather_kernel(const TI *__restrict__ src, TO *__restrict__ dst,
                                                         const long long *__restrict__ idx, long long count, int upr,
                                                         long long waves)
{
    using VI = typename Vec<TI, K>::type;
    using VO = typename Vec<TO, K>::type;
    const int lane = threadIdx.x & 63;
    const long long N = (long long)upr * K;
    const long long wstep = (long long)gridDim.x * 4;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < waves; w += wstep) {
        const long long u0 = w * (64 * GATHER_UNROLL); // first unit of the piece (wave-uniform)
        const long long r0 = u0 / upr;
        const unsigned c0 = (unsigned)(u0 - r0 * upr);
        // three phases and no branch between the loads: every index, then every row load (a unit past the last row
        // re-reads a row of the list and is not stored), then the stores -- UNROLL row loads in flight per lane
        long long d[GATHER_UNROLL], o[GATHER_UNROLL], s[GATHER_UNROLL];
#pragma unroll
        for (int j = 0; j < GATHER_UNROLL; j++) {
            const unsigned c = c0 + (unsigned)(j * 64 + lane);
            const unsigned dr = c / (unsigned)upr;
            const long long r = r0 + dr;
            o[j] = (long long)(c - dr * (unsigned)upr) * K;
            d[j] = r < count ? r * N + o[j] : -1;
            s[j] = idx[r < count ? r : count - 1];
        }
        VI v[GATHER_UNROLL];
#pragma unroll
        for (int j = 0; j < GATHER_UNROLL; j++)
            v[j] = *(const VI *)(src + s[j] * N + o[j]);
#pragma unroll
        for (int j = 0; j < GATHER_UNROLL; j++) {
            if (d[j] >= 0) {
                const VO x = widen<VO>(v[j]);
                if constexpr (NT)
                    __builtin_nontemporal_store(x, (VO *)(dst + d[j]));
                else
                    *(VO *)(dst + d[j]) = x;
            }
        }
    }
}

template <class TI, class TO, int K>
hipError_t gather_as(const TI *src, TO *dst, const long long *idx, long long count, int N, int num_cus, bool nt,
                     hipStream_t stream)
{
    const int upr = N / K;
    const long long units = count * (long long)upr;
    const long long waves = (units + 64 * GATHER_UNROLL - 1) / (64 * GATHER_UNROLL);
    const long long wgs = std::min<long long>((waves + 3) / 4, (long long)std::max(num_cus, 1) * GATHER_WGS_PER_CU);
    if (nt)
        hipLaunchKernelGGL((row_gather_kernel<TI, TO, K, true>), dim3((unsigned)wgs), dim3(256), 0, stream, src, dst, idx, count,
                           upr, waves);
    else
        hipLaunchKernelGGL((row_gather_kernel<TI, TO, K, false>), dim3((unsigned)wgs), dim3(256), 0, stream, src, dst, idx,
                           count, upr, waves);
    return hipGetLastError();
}

template <class TI, class TO>
hipError_t gather_typed(const TI *src, TO *dst, const long long *idx, long long count, int N, int num_cus, bool nt,
                        hipStream_t stream)
{
    constexpr int K16 = 16 / (int)sizeof(TI);
    if (N % K16 == 0)
        return gather_as<TI, TO, K16>(src, dst, idx, count, N, num_cus, nt, stream);
    if (K16 > 2 && N % 2 == 0)
        return gather_as<TI, TO, (K16 > 2 ? 2 : 1)>(src, dst, idx, count, N, num_cus, nt, stream);
    return gather_as<TI, TO, 1>(src, dst, idx, count, N, num_cus, nt, stream);
}

} // namespace

hipError_t launch_row_gather(const void *src, bool src_f32, void *dst, bool dst_f32, const long long *idx, long long count,
                             int N, int num_cus, bool nontemporal, hipStream_t stream)
{
    if (count <= 0)
        return hipSuccess;
    if (N < 1 || (!src_f32 && dst_f32))
        return hipErrorInvalidValue;
    if (src_f32 && dst_f32)
        return gather_typed((const float *)src, (float *)dst, idx, count, N, num_cus, nontemporal, stream);
    if (src_f32)
        return gather_typed((const float *)src, (double *)dst, idx, count, N, num_cus, nontemporal, stream);
    return gather_typed((const double *)src, (double *)dst, idx, count, N, num_cus, nontemporal, stream);
}

} // namespace muse
