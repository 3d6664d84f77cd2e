// The activation between the two forward GEMMs of a MoE expert MLP, fused into the quantiser that feeds the second one:
//   dga_silu_mul_cast_to_fp8_1x128   x[groups, rows, 2h] (bf16 / fp16 / fp32) -> e4m3fn bytes [groups, rows, h] + fp32 scale per 1x128
//   h = silu(gate) * up,  gate = x[..., :h],  up = x[..., h:],  silu(g) = g / (1 + exp(-g))
// in one pass over the valid rows: 4 bytes in and 1 out per element (bf16) where the torch activation followed by
// dga_cast_to_fp8_1x128 moves 9, on every padded row.  h lives in fp32 registers only; the quantiser proper is dga_cast.hip's
// (dga_cast_device.hpp), so (q, sf) are byte for byte what dga_cast_to_fp8_1x128_ex gives on the same fp32 h.
//
// Accuracy of h (DESIGN.md "Fused SiLU-and-multiply quantiser"):
//   gate >= 20       exp(-g) < 2^-24, 1 + exp(-g) rounds to 1, its reciprocal is 1 and stays 1 under the Newton step:
//                    h = fl32(gate * up) exactly (the product of two 16-bit inputs is itself exact) -- the oracle's bytes bit for bit.
//   |gate| <= 16     relative error <= (|g| + 4) 2^-24 <= 2^-19.7, stated as 2^-18: exp(-g) = v_exp_f32(g * -log2(e)) carries |g| 2^-24
//                    from rounding the argument and 1 ULP of its own; the add, the refined v_rcp_f32 and the two multiplies add
//                    at most three more.  The block amax alone is the correctly rounded fp32 of the real value (fp64, one element
//                    per lane: silu_mul_abs_rounded), so the scale is the one a float64 reference gives, to the bit.
//   gate <= -88.8    exp(-g) overflows, the reciprocal is 0 and h = +-0 (the real value is below 2^-126 |up|; at gate <= -120
//                    below the smallest subnormal).  Between -88.8 and -87 the reciprocal is subnormal and may flush: h is 0 or
//                    within the bound above.
//   NaN in gate or up gives a NaN h (code sign | 0x7F, ignored by the block amax); an infinite h is what dga_cast_to_fp8_1x128
//   makes of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// silu(g) * u.  r = 1 / (1 + 2^(g * -log2 e)): hardware exponential, hardware reciprocal, one Newton step.  With exp(-g) = inf the
// reciprocal is 0 and the Newton residual -inf * 0 + 1 is NaN: v_max_f32 drops the NaN (any ordinary residual is far above -1),
// and the step then returns the 0.  A NaN g still comes out NaN (r0 is NaN, and so is -1 * r0 + r0).
__device__ __forceinline__ float silu_mul(float g, float u)
{
    const float d = 1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f);
    const float r0 = __builtin_amdgcn_rcpf(d);
    const float r1 = __builtin_fmaf(__builtin_fmaxf(__builtin_fmaf(-d, r0, 1.f), -1.f), r0, r0);
    return (g * r1) * u;
}

// The lane's largest |h| once more, as the fp32 nearest to the real-number value: the block scale is amax / 448, and an amax that is
// within 2^-19.7 but a ULP or two off the correctly rounded one puts every dequantised value (code x scale) of its block the same
// ULP off.  fp64 exponential and division (error 2^-51, so the one rounding to fp32 is the right one but for 2^-27 of the inputs),
// one element per lane and block.  Where 1 + exp(-g) rounds to 1 in fp32 the value stays h32 = fl32(g * u): the contract for
// gate >= 20.  h32 = |silu_mul(g, u)|.
__device__ __forceinline__ float silu_mul_abs_rounded(float g, float u, float h32)
{
    const bool one = 1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f) == 1.f;
    const double gd = g;
    const float hd = (float)(gd / (1.0 + exp(-gd)) * (double)u);
    return one ? h32 : __builtin_fabsf(hd);
}

// a / b for 0 <= a, 0 < b: the 32-bit division when both fit (a quarter of the instructions of the 64-bit one)
__device__ __forceinline__ int64_t udiv(int64_t a, int64_t b, bool small)
{
    return small ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// cast_1x128_kernel's geometry: 16 lanes share one 1x128 block of h, 8 consecutive elements per lane (for bf16 one 16-byte load
// of gate and one of up: 32 bytes in flight per lane), DPP row max, no LDS.  `blocks` = rows_total * hb_n 16-lane groups over the
// rows of all groups; a group of lanes whose row the mask excludes leaves as a whole before it reads x.
template <typename T>
__global__ void __launch_bounds__(256) silu_mul_cast_1x128_kernel(const void *x, uint8_t *q, float *sf, int64_t blocks, int64_t mmax,
                                                                  int64_t h, int64_t hb_n, const int32_t *masked_m,
                                                                  const int32_t *m_indices, bool vec_in, bool vec_out, bool ue8m0,
                                                                  bool small)
{
    const int64_t blk = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (blk >= blocks) return;  // whole 16-lane groups leave together: the row max below never sees a lane of another block
    const int64_t row = udiv(blk, hb_n, small);
    if (masked_m) {
        const int64_t g = udiv(row, mmax, small);
        if (row - g * mmax >= masked_m[g]) return;
    } else if (m_indices) {
        if (m_indices[row] < 0) return;
    }
    const int sub = threadIdx.x & 15;
    const int64_t c0 = (blk - row * hb_n) * 128 + sub * 8, gbase = row * 2 * h + c0, ubase = gbase + h;
    float g8[8], u8[8];
    if (vec_in && c0 + 8 <= h) {
        Elem<T>::load8(x, gbase, g8);
        Elem<T>::load8(x, ubase, u8);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            g8[j] = (c0 + j < h) ? Elem<T>::load(x, gbase + j) : 0.f;
            u8[j] = (c0 + j < h) ? Elem<T>::load(x, ubase + j) : 0.f;   // (columns past h: silu(0) * 0 = 0 into the amax)
        }
    }
    float v[8];
    float amax = 0.f, gmax = 0.f, umax = 0.f;   // the lane's largest |h| (NaN never compares greater: ignored) and its inputs
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = silu_mul(g8[j], u8[j]);
        const float a = __builtin_fabsf(v[j]);
        const bool gt = a > amax;
        amax = gt ? a : amax;
        gmax = gt ? g8[j] : gmax;
        umax = gt ? u8[j] : umax;
    }
    amax = row16_max(silu_mul_abs_rounded(gmax, umax, amax));
    const float s = block_scale(amax, ue8m0);
    if (sub == 0) sf[blk] = s;
    uint32_t w0, w1;
    quant8(v, s, w0, w1);
    const int64_t qbase = row * h + c0;
    if (vec_out && c0 + 8 <= h) {
        *(v2i_c *)(q + qbase) = v2i_c{(int)w0, (int)w1};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < h) q[qbase + j] = (uint8_t)(((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xFF);
    }
}

template <typename T>
static int launch_silu_mul_cast(const void *x, int64_t rows_total, int64_t mmax, int64_t h, const int32_t *masked_m,
                                const int32_t *m_indices, void *q, float *sf, bool ue8m0, hipStream_t stream)
{
    const int64_t hb_n = (h + 127) / 128;
    if (rows_total > 0x7FFFFFFFll * 16 / hb_n) return DGA_E_RANGE;   // (also keeps rows_total * hb_n inside int64)
    const int64_t blocks = rows_total * hb_n;
    const int64_t grid = (blocks * 16 + 255) / 256;
    if (grid > 0x7FFFFFFFll) return DGA_E_RANGE;
    // gate starts at element row * 2h + 8j, up h elements later: both 16-byte aligned for every row iff h * sizeof(T) % 16 == 0
    const bool vec_in = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (h * Elem<T>::kBytes % 16 == 0);
    const bool vec_out = (reinterpret_cast<uintptr_t>(q) % 8 == 0) && (h % 8 == 0);
    const bool small = blocks <= 0xFFFFFFFFll && mmax <= 0xFFFFFFFFll;
    hipLaunchKernelGGL(silu_mul_cast_1x128_kernel<T>, dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream, x,
                       static_cast<uint8_t *>(q), sf, blocks, mmax, h, hb_n, masked_m, m_indices, vec_in, vec_out, ue8m0, small);
    return record_hip(hipGetLastError());
}

}  // namespace dga

extern "C" int dga_silu_mul_cast_to_fp8_1x128(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                              const int32_t *masked_m, const int32_t *m_indices, void *q, float *sf, int flags,
                                              void *stream)
{
    using namespace dga;
    // (run_cast's order: flags, shape, nothing to do, pointers, dtype, grid)
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (groups < 1 || rows < 0 || h < 0 || (masked_m && m_indices) || (m_indices && groups != 1)) return DGA_E_SHAPE;
    if (rows == 0 || h == 0) return DGA_OK;
    if (!x || !q || !sf) return DGA_E_NULL;
    if (x_dtype != DGA_DT_FP32 && x_dtype != DGA_DT_BF16 && x_dtype != DGA_DT_FP16) return DGA_E_DTYPE;
    if (groups > 0x7FFFFFFFFFFFFFFFll / rows) return DGA_E_RANGE;
    const bool ue8m0 = (flags & DGA_CAST_UE8M0) != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (x_dtype) {
        case DGA_DT_FP32: return launch_silu_mul_cast<float>(x, groups * rows, rows, h, masked_m, m_indices, q, sf, ue8m0, st);
        case DGA_DT_BF16: return launch_silu_mul_cast<Bf16Tag>(x, groups * rows, rows, h, masked_m, m_indices, q, sf, ue8m0, st);
        case DGA_DT_FP16: return launch_silu_mul_cast<F16Tag>(x, groups * rows, rows, h, masked_m, m_indices, q, sf, ue8m0, st);
        default: return DGA_E_DTYPE;
    }
}
