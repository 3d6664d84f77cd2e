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
    int64_t row, b;
    if (!locate_row(blk, hb_n, mmax, masked_m, m_indices, small, row, b)) return;
    const int sub = threadIdx.x & 15;
    const int64_t c0 = b * 128 + sub * 8, gbase = row * 2 * h + c0, ubase = gbase + h;
    float g8[8], u8[8];
    load8_bounded<T>(x, gbase, g8, vec_in, c0, h);
    load8_bounded<T>(x, ubase, u8, vec_in, c0, h);   // (columns past h read as 0: silu(0) * 0 = 0 into the amax)
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
    store_codes8(q + row * h + c0, w0, w1, vec_out, c0, h);
}

}  // namespace dga

extern "C" int dga_silu_mul_cast_to_fp8_1x128(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                              const int32_t *masked_m, const int32_t *m_indices, void *q, float *sf, int flags,
                                              void *stream)
{
    using namespace dga;
    return run_fused(flags, x_dtype, groups, rows, h, 1, masked_m, m_indices, x && q && sf, [&](auto tag, const FusedGeometry &g) {
        using T = decltype(tag);
        // gate starts at element row * 2h + 8j, up h elements later: both 16-byte aligned for every row iff h * sizeof(T) % 16 == 0
        const bool vec_in = (reinterpret_cast<uintptr_t>(x) % 16 == 0) && (h * Elem<T>::kBytes % 16 == 0);
        const bool vec_out = (reinterpret_cast<uintptr_t>(q) % 8 == 0) && (h % 8 == 0);
        hipLaunchKernelGGL(silu_mul_cast_1x128_kernel<T>, dim3(g.grid), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                           static_cast<uint8_t *>(q), sf, g.blocks, rows, h, g.hb_n, masked_m, m_indices, vec_in, vec_out, g.ue8m0, g.small);
        return record_hip(hipGetLastError());
    });
}
