// Quantisers that sit immediately upstream of the fp8 GEMM in a MoE layer:
//   dga_cast_to_fp8_1x128    activations  x[rows,k] (fp32 / bf16 / fp16) -> e4m3fn bytes + fp32 scale per 1x128 block
//   dga_cast_to_fp8_128x128  weights      x[rows,k]                      -> e4m3fn bytes + fp32 scale per 128x128 block
// The reference has no fp8 data path (its inputs are fp16 files written by numpy, scripts/gen_data.py); the
// definition of record is the test oracle's quantiser (quant_1x128 / quant_128x128 in oracle/):
//   amax = max |x| over the block (NaN ignored), scale = amax / 448 (1 if amax == 0),
//   q = e4m3fn_rne_satfinite(x / scale)  with an IEEE fp32 division,
//   a block with an infinite amax: scale +inf, finite x -> the zero of its sign, +-inf and NaN -> sign(x) | 0x7F,
// and the results are byte-exact against it.  Both kernels are HBM streams (read 2 or 4 bytes, write 1 per element).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// 16 lanes share one 1x128 block, 8 consecutive elements per lane: a wave covers 4 blocks per pass, loads and stores
// are contiguous per 16-lane group (256 / 512 bytes in, 128 bytes out).
template <typename T>
__global__ void __launch_bounds__(256) cast_1x128_kernel(const void *x, uint8_t *q, float *sf, int64_t rows, int64_t k,
                                                         int64_t kb_n, bool vec_in, bool vec_out, int64_t ldq, bool ue8m0)
{
    const int64_t blk = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (blk >= rows * kb_n) return;  // whole 16-lane groups leave together
    const int sub = threadIdx.x & 15;
    const int64_t row = blk / kb_n, kb = blk - row * kb_n;
    const int64_t c0 = kb * 128 + sub * 8, base = row * k + c0;
    float v[8];
    load8_bounded<T>(x, base, v, vec_in, c0, k);
    float s;
    uint32_t w0, w1;
    quant_row_block(v, ue8m0, s, w0, w1);
    if (sub == 0) sf[blk] = s;
    // (columns at and beyond k were read as 0 and quantise to the zero byte: they fill the row's tail up to ldq)
    store_codes8(q + row * ldq + c0, w0, w1, vec_out, c0, ldq);
}

// The same, U blocks per 16-lane group with all U loads issued before the first is used: U x 16 (32) bytes in flight per lane
// instead of one load.  Block j of a group is blk + j * stride (stride = a U-th of the blocks), so that each of the U passes of
// the grid is the contiguous stream the one-block kernel reads.  Whole rows only on the fast path (vec_in, vec_out, K % 128 == 0).
template <typename T, int U>
__global__ void __launch_bounds__(256) cast_1x128_unrolled_kernel(const void *x, uint8_t *q, float *sf, int64_t blocks, int64_t stride, bool ue8m0)
{
    const int64_t blk0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (blk0 >= stride) return;
    const int sub = threadIdx.x & 15;
    float v[U][8];
    bool live[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const int64_t blk = blk0 + j * stride;
        live[j] = blk < blocks;
        if (live[j]) Elem<T>::load8(x, blk * 128 + sub * 8, v[j]);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
        if (!live[j]) continue;          // (uniform over the 16-lane group)
        const int64_t blk = blk0 + j * stride;
        float s;
        uint32_t w0, w1;
        quant_row_block(v[j], ue8m0, s, w0, w1);
        if (sub == 0) sf[blk] = s;
        *(v2i_c *)(q + blk * 128 + sub * 8) = v2i_c{(int)w0, (int)w1};
    }
}

// one workgroup per 128x128 block: thread t holds 64 elements of row t/2 (columns 64*(t&1) ..), the block amax goes
// through LDS, nothing is read twice.
template <typename T>
__global__ void __launch_bounds__(256) cast_128x128_kernel(const void *x, uint8_t *q, float *sf, int64_t rows, int64_t k,
                                                           int64_t kb_n, bool vec_in, bool vec_out, int64_t ldq, bool ue8m0)
{
    __shared__ float red[4];
    const int64_t rb = blockIdx.x / kb_n, kb = blockIdx.x - rb * kb_n;
    const int t = threadIdx.x;
    const int64_t row = rb * 128 + (t >> 1);
    const int64_t c0 = kb * 128 + (t & 1) * 64;
    const bool row_ok = row < rows;
    float v[64];
    float amax = 0.f;
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) {
        float e[8];
        const int64_t c = c0 + g8 * 8;
        load8_bounded<T>(x, row * k + c, e, vec_in, c, k, row_ok);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[g8 * 8 + j] = e[j];
            amax = __builtin_fmaxf(amax, abs_for_max(e[j]));
        }
    }
#pragma unroll
    for (int msk = 1; msk < 64; msk <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, msk, 64));
    if ((t & 63) == 0) red[t >> 6] = amax;
    __syncthreads();
    amax = __builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3]));
    const float s = block_scale(amax, ue8m0);
    if (t == 0) sf[blockIdx.x] = s;
    if (!row_ok) return;
#pragma unroll
    for (int g8 = 0; g8 < 8; ++g8) {
        const int64_t c = c0 + g8 * 8;
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = v[g8 * 8 + j];
        uint32_t w0, w1;
        quant8(e, s, w0, w1);
        store_codes8(q + row * ldq + c, w0, w1, vec_out, c, ldq);
    }
}

template <typename T>
static int launch_cast(int mode, const void *x, void *q, float *sf, int64_t rows, int64_t k, int64_t ldq, bool ue8m0, hipStream_t stream)
{
    const int64_t kb_n = (k + 127) / 128;
    // a lane's 8 elements start at element row*k + 8*j: 16-byte aligned for every row iff k % 8 == 0
    const bool vec_in = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (k % 8 == 0);
    const bool vec_out = (reinterpret_cast<uintptr_t>(q) % 8 == 0) && (ldq % 8 == 0);
    // 16-bit inputs, large problems: two blocks per 16-lane group (32 bytes in flight per lane): [32768, 7168] bf16 140.7 -> 124.2 us
    // (5.06 -> 5.73 TB/s; four blocks 129.8; fp32 inputs are faster one block at a time: 195 against 203 / 207 us; scripts/cast_ab.py)
    static const int unroll = [] { const char *e = std::getenv("DGA_CAST_UNROLL"); return e ? std::atoi(e) : 0; }();
    const bool two = unroll ? unroll >= 2 : (Elem<T>::kBytes == 2 && rows * kb_n >= 131072);
    if (mode == 0 && vec_in && vec_out && k % 128 == 0 && ldq == k && two) {
        const int64_t blocks = rows * kb_n;
        const int64_t stride = (blocks + 1) / 2;
        unsigned grid;
        if (int rc = grid_of_blocks(stride, 1, grid)) return rc;
        if (unroll >= 4)
            hipLaunchKernelGGL((cast_1x128_unrolled_kernel<T, 4>), dim3(static_cast<unsigned>(((blocks + 3) / 4 * 16 + 255) / 256)), dim3(256), 0,
                               stream, x, static_cast<uint8_t *>(q), sf, blocks, (blocks + 3) / 4, ue8m0);
        else
            hipLaunchKernelGGL((cast_1x128_unrolled_kernel<T, 2>), dim3(grid), dim3(256), 0, stream, x,
                               static_cast<uint8_t *>(q), sf, blocks, stride, ue8m0);
        return record_hip(hipGetLastError());
    }
    if (mode == 0) {
        unsigned grid;
        if (int rc = grid_of_blocks(rows, kb_n, grid)) return rc;
        hipLaunchKernelGGL(cast_1x128_kernel<T>, dim3(grid), dim3(256), 0, stream, x,
                           static_cast<uint8_t *>(q), sf, rows, k, kb_n, vec_in, vec_out, ldq, ue8m0);
    } else {
        const int64_t grid = ((rows + 127) / 128) * kb_n;
        if (grid > 0x7FFFFFFFll) return DGA_E_RANGE;
        hipLaunchKernelGGL(cast_128x128_kernel<T>, dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream, x,
                           static_cast<uint8_t *>(q), sf, rows, k, kb_n, vec_in, vec_out, ldq, ue8m0);
    }
    return record_hip(hipGetLastError());
}

static int run_cast(int mode, const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, void *stream, int flags = 0)
{
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    const bool ue8m0 = (flags & DGA_CAST_UE8M0) != 0;
    if (rows < 0 || k < 0 || ldq < k || ldq > (k + 127) / 128 * 128) return DGA_E_SHAPE;
    if (rows == 0 || k == 0) return DGA_OK;
    if (!x || !q || !sf) return DGA_E_NULL;
    return dispatch_dtype(x_dtype, [&](auto tag) {
        return launch_cast<decltype(tag)>(mode, x, q, sf, rows, k, ldq, ue8m0, static_cast<hipStream_t>(stream));
    });
}

}  // namespace dga

extern "C" {

int dga_cast_to_fp8_1x128(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, float *sf, void *stream)
{
    return dga::run_cast(0, x, x_dtype, rows, k, q, k, sf, stream);
}

int dga_cast_to_fp8_128x128(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, float *sf, void *stream)
{
    return dga::run_cast(1, x, x_dtype, rows, k, q, k, sf, stream);
}

int dga_cast_to_fp8_1x128_ld(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, void *stream)
{
    return dga::run_cast(0, x, x_dtype, rows, k, q, ldq, sf, stream);
}

int dga_cast_to_fp8_128x128_ld(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, void *stream)
{
    return dga::run_cast(1, x, x_dtype, rows, k, q, ldq, sf, stream);
}

int dga_cast_to_fp8_1x128_ex(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, int flags, void *stream)
{
    return dga::run_cast(0, x, x_dtype, rows, k, q, ldq, sf, stream, flags);
}

int dga_cast_to_fp8_128x128_ex(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, int flags, void *stream)
{
    return dga::run_cast(1, x, x_dtype, rows, k, q, ldq, sf, stream, flags);
}

}  // extern "C"
