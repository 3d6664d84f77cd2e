// Between the weight gradient and the optimizer, on the device: the sum of squares of a list of gradient tensors in float64, and from it
// the gradient norm, the clip coefficient that goes into step_scalars[3] and the flag that makes dga_adamw_cast.hip skip a step.
//   dga_grad_sumsq          tensors (fp32 / bf16, mixed) -> sumsq[0] = sum_i sum_e x_i[e]^2, float64; optionally added to what sumsq held
//   dga_grad_clip_scalars   sumsq -> norm, coef (fp32), step_scalars[3] = pre_scale * coef, skip = !isfinite(sumsq) (int32)
// Every product and every sum is float64: an fp32 or bf16 value converts exactly and its square has at most 48 significant bits, so the
// squares are exact, cannot overflow or underflow (|x| < 2^128 and >= 2^-149 give squares inside [2^-298, 2^256)), and the only roundings
// are those of the additions: |sumsq - exact| <= (n + 1) 2^-53 exact for n elements, in any order.  A NaN or an infinity anywhere makes
// sumsq non-finite (squares are non-negative: no inf - inf), and nothing else can.
// The order of the additions is fixed by the list of (numel, dtype) alone -- not by the pointers, their alignment, the number of CUs or
// the stream; no floating-point atomics, no last-arriver combine:
//   stage 1   one workgroup of 256 lanes per chunk of DGA_GRAD_SUMSQ_CHUNK = 16384 consecutive elements of ONE tensor (the last chunk of a
//             tensor is short; a chunk never spans two).  Lane t holds elements 8 (256 i + t) + j of its chunk, i, j = 0 .. 7: eight
//             accumulators a_j = sum over ascending i, then ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); the wave's 64 values by a
//             butterfly (lane ^ 1, 2, 4, 8, 16, 32: both partners form the same sum), the four waves as (r0 + r1) + (r2 + r3); one float64
//             partial per chunk, at the chunk's number in the list.
//   stage 2   one workgroup of 1024 lanes: lane t adds partials t, t + 1024, ... in ascending order, the same butterfly, the 16 waves in
//             ascending order; then out = fl(out + sum) if accumulating.
// A tensor whose pointer is short of 16 bytes, and the last chunk of any, takes the bounded loads for that tensor (chunk) alone with the
// same element-to-lane map: an element that is not there adds +0, so the bits are the same.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

constexpr int64_t kChunk = DGA_GRAD_SUMSQ_CHUNK;
constexpr int kMaxTensors = 64;        // list entries per stage-1 launch: the table is a kernel argument, 1536 bytes
constexpr int kFinalThreads = 1024;
static_assert(kChunk == 8 * 8 * 256, "lane t holds elements 8 (256 i + t) + j, i, j = 0 .. 7");

enum : uint32_t { GRAD_BF16 = 1, GRAD_VEC = 2 };

// The tensors of one stage-1 launch, list entries 64 l .. 64 l + 63, empty ones included; first[i] = the launch's first chunk of tensor i
// (ascending; an empty tensor shares its with the next)
struct GradTable {
    const void *ptr[kMaxTensors];
    int64_t numel[kMaxTensors];
    uint32_t first[kMaxTensors];
    uint32_t flags[kMaxTensors];
};

// a wave's 64 values: lane ^ 1, 2, 4, 8, 16, 32; the sum is commutative, so both partners of a step hold the same bits
__device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int msk = 1; msk < 64; msk <<= 1) s += __shfl_xor(s, msk, 64);
    return s;
}

// The lane's 64 elements of the chunk at element e0 of p, `left` >= 1 elements to the tensor's end: four groups of 8 loaded, then used,
// twice.  whole (uniform): all 16384 are there and p allows the 16-byte loads.
template <typename T>
__device__ __forceinline__ void chunk_squares(const void *p, int64_t e0, int64_t left, bool vec, int t, double (&acc)[8])
{
    const bool whole = vec && left >= kChunk;
#pragma unroll
    for (int h = 0; h < 8; h += 4) {
        float x[4][8];
        if (whole) {
            typename Elem<T>::Raw raw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[i] = Elem<T>::load8_raw(p, e0 + ((h + i) * 256 + t) * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) Elem<T>::unpack8(raw[i], x[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t off = ((h + i) * 256 + t) * 8;
                load8_bounded<T>(p, e0 + off, x[i], vec, off, left);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double d = (double)x[i][j];
                acc[j] = __builtin_fma(d, d, acc[j]);   // (the square is exact: one rounding, that of the sum)
            }
        }
    }
}

__global__ void __launch_bounds__(256) grad_sumsq_chunks_kernel(GradTable tab, int count, double *partials)
{
    __shared__ double red[4];
    const int t = threadIdx.x;
    const uint32_t blk = blockIdx.x;
    int lo = 0, hi = count - 1;   // (uniform) the last tensor whose first chunk is at or before blk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.first[mid] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const int64_t e0 = (int64_t)(blk - tab.first[lo]) * kChunk;
    const int64_t left = tab.numel[lo] - e0;
    const uint32_t flags = tab.flags[lo];
    const void *p = tab.ptr[lo];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (flags & GRAD_BF16) chunk_squares<Bf16Tag>(p, e0, left, (flags & GRAD_VEC) != 0, t, acc);
    else chunk_squares<float>(p, e0, left, (flags & GRAD_VEC) != 0, t, acc);
    const double s = wave_sum(((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) partials[blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(kFinalThreads) grad_sumsq_final_kernel(const double *partials, int64_t chunks, double *sumsq, int accumulate)
{
    __shared__ double red[kFinalThreads / 64];
    const int t = threadIdx.x;
    double s = 0.0;
#pragma unroll 4
    for (int64_t i = t; i < chunks; i += kFinalThreads) s += partials[i];
    s = wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int w = 0; w < kFinalThreads / 64; ++w) total += red[w];
        sumsq[0] = accumulate ? sumsq[0] + total : total;
    }
}

// One lane: everything in float64, rounded once to fp32 on store.  q < 1 ? q : 1 also answers a NaN quotient (0 / 0) with 1.
__global__ void __launch_bounds__(64) grad_clip_scalars_kernel(const double *sumsq, double max_norm, double pre_scale, double eps,
                                                               float *step_scalars, float *norm, float *coef, int32_t *skip)
{
    if (threadIdx.x != 0) return;
    const double ss = sumsq[0];
    const bool finite = __builtin_isfinite(ss);
    const double normd = pre_scale * __builtin_sqrt(ss);
    const double q = max_norm / (normd + eps);
    const double coefd = q < 1.0 ? q : 1.0;
    norm[0] = (float)normd;
    coef[0] = finite ? (float)coefd : 0.f;
    step_scalars[3] = finite ? (float)(pre_scale * coefd) : 0.f;
    skip[0] = finite ? 0 : 1;
}

// The list's chunks, or -1 where the entry refuses it by its sizes alone (count < 0, a negative numel, more than a 31-bit grid holds)
static int64_t chunks_of(int count, const int64_t *numel)
{
    int64_t total = 0;
    for (int i = 0; i < count; ++i) {
        if (numel[i] < 0) return -1;
        total += numel[i] / kChunk + (numel[i] % kChunk != 0);
        if (total > 0x7FFFFFFFll) return -1;
    }
    return total;
}

}  // namespace dga

extern "C" int64_t dga_grad_sumsq_workspace_bytes(int count, const int64_t *numel)
{
    if (count < 0 || (count > 0 && !numel)) return 0;
    const int64_t chunks = dga::chunks_of(count, numel);
    return chunks < 0 ? 0 : chunks * 8;
}

extern "C" int dga_grad_sumsq(const void *const *tensors, const int64_t *numel, const int *dtypes, int count, double *sumsq, int accumulate,
                              void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace dga;
    // run_cast's order: shape, pointers, dtypes, the ranges -- every code before the first launch; an empty list still writes sumsq
    if (count < 0) return DGA_E_SHAPE;
    if (count > 0 && !numel) return DGA_E_NULL;
    for (int i = 0; i < count; ++i)
        if (numel[i] < 0) return DGA_E_SHAPE;
    if (!sumsq || (count > 0 && (!tensors || !dtypes))) return DGA_E_NULL;
    bool any = false;
    for (int i = 0; i < count; ++i) {
        if (numel[i] > 0 && !tensors[i]) return DGA_E_NULL;
        any = any || numel[i] > 0;
    }
    if (any && !workspace) return DGA_E_NULL;
    for (int i = 0; i < count; ++i)
        if (dtypes[i] != DGA_DT_FP32 && dtypes[i] != DGA_DT_BF16) return DGA_E_DTYPE;
    const int64_t chunks = chunks_of(count, numel);
    if (chunks < 0 || workspace_bytes < chunks * 8 || reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return DGA_E_RANGE;
    double *partials = static_cast<double *>(workspace);
    GradTable tab;
    int held = 0;
    uint32_t in_launch = 0;
    int64_t done = 0;
    const auto flush = [&] {
        if (in_launch != 0)
            hipLaunchKernelGGL(grad_sumsq_chunks_kernel, dim3(in_launch), dim3(256), 0, static_cast<hipStream_t>(stream), tab, held,
                           partials + done);
        done += in_launch;
        held = 0;
        in_launch = 0;
    };
    for (int i = 0; i < count; ++i) {   // (an empty tensor holds a place in its table and no chunk: the kernel looks for the LAST tensor that starts at or before its chunk)
        tab.ptr[held] = tensors[i];
        tab.numel[held] = numel[i];
        tab.first[held] = in_launch;
        tab.flags[held] = (dtypes[i] == DGA_DT_BF16 ? GRAD_BF16 : 0u) | (reinterpret_cast<uintptr_t>(tensors[i]) % 16 == 0 ? GRAD_VEC : 0u);
        in_launch += static_cast<uint32_t>(numel[i] / kChunk + (numel[i] % kChunk != 0));
        if (++held == kMaxTensors) flush();
    }
    flush();
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(kFinalThreads), 0, static_cast<hipStream_t>(stream), partials, chunks, sumsq,
                       accumulate != 0);
    return record_hip(hipGetLastError());
}

extern "C" int dga_grad_clip_scalars(const double *sumsq, double max_norm, double pre_scale, double eps, float *step_scalars, float *norm,
                                     float *coef, int32_t *skip, void *stream)
{
    using namespace dga;
    if (!sumsq || !step_scalars || !norm || !coef || !skip) return DGA_E_NULL;
    // max_norm >= 0 (it may be +inf), pre_scale > 0 and finite, eps >= 0 and finite; each comparison is false for a NaN
    if (!(max_norm >= 0.0) || !(pre_scale > 0.0) || std::isinf(pre_scale) || !(eps >= 0.0) || std::isinf(eps)) return DGA_E_RANGE;
    hipLaunchKernelGGL(grad_clip_scalars_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sumsq, max_norm, pre_scale, eps,
                       step_scalars, norm, coef, skip);
    return record_hip(hipGetLastError());
}
