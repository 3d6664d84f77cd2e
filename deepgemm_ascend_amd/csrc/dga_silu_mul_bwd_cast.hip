// The backward of the activation between the two GEMMs of a MoE expert MLP, fused into the quantiser that feeds the dgrad of the first:
//   dga_silu_mul_bwd_cast_to_fp8_1x128   x[groups, rows, 2h], grad_h[groups, rows, h] (bf16 / fp16 / fp32)
//                                        -> e4m3fn bytes [groups, rows, 2h] + fp32 scale per 1x128, optionally the gradient itself
//   dgate = d * u * silu'(g),  dup = d * silu(g),  g = x[..., :h], u = x[..., h:], d = grad_h,
//   silu(g) = g s,  silu'(g) = s + g s (1 - s),  s = 1 / (1 + exp(-g))
// in one pass over the valid rows: 6 bytes in and 2 out per (gate, up) pair (bf16), 4 more with grad_x.  Both gradients live in fp32
// registers only; the quantiser proper is dga_cast.hip's (dga_cast_device.hpp), so (dq, dsf) are byte for byte what
// dga_cast_to_fp8_1x128_ex gives on the same fp32 [dgate | dup].  h % 128 == 0: a 1x128 block of the [2h] axis is either gate's or up's.
//
// Accuracy (DESIGN.md "Fused SiLU-and-multiply backward quantiser"), e = exp(-g) from v_exp_f32, s from a refined v_rcp_f32
// (sigmoid_refined), 1 - s taken as e s (no cancellation for large g), silu' = fma(g s, e s, s):
//   gate >= 20       e < 2^-24: s = 1 and g e <= 20 e^-20 = 4.1e-8 < 2^-24, so silu' = 1 too: dgate = fl32(d u), dup = fl32(d g), the
//                    oracle's bytes on those products bit for bit (for 16-bit inputs the products are themselves exact).
//   |gate| <= 16     |dup32 - dup| <= 2^-18 |dup|;  |dgate32 - dgate| <= 2^-17 |d u| (s + |g| s (1 - s)) -- against the sum of the
//                    magnitudes of the two terms: silu' has a root at g = -1.2785 and no relative bound exists there.  The two block
//                    maxima alone are the correctly rounded fp32 of the real values (fp64, one element per lane and block:
//                    dgate_abs_rounded, dup_abs_rounded), so the scales are a float64 reference's, to the bit.
//   gate <= -88.8    e overflows, s = 0 and e s = inf * 0: v_min_f32 against 1 (the limit of 1 - s) drops the NaN; both results are +-0.
//   NaN in gate or grad gives NaN in both results, NaN in up in dgate alone (code sign | 0x7F, ignored by the block amax); an
//   infinite result is what dga_cast_to_fp8_1x128 makes of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// (silu_mul_bwd, dgate_abs_rounded and dup_abs_rounded live in dga_cast_device.hpp: dga_silu_mul_bwd_cast_transposed.hip shares them)
// silu_mul_cast_1x128_kernel's geometry: 16 lanes share column block b of a row, 8 consecutive elements per lane of gate, up and grad
// (for bf16 three 16-byte loads), and own the two output blocks b (dgate) and hb_n + b (dup) of that row: two DPP row maxima, two
// scales, two 8-byte code stores, no LDS.  `blocks` = rows_total * hb_n 16-lane groups; a group whose row the mask excludes leaves
// as a whole before it reads anything.  gx (may be null): the unquantised gradient, x's layout and type.  vec: every pointer is
// aligned for the 16-byte (codes: 8-byte) accesses; h % 128 == 0 keeps every row and half aligned with it.
template <typename T>
__global__ void __launch_bounds__(256) silu_mul_bwd_cast_1x128_kernel(const void *x, const void *grad, uint8_t *q, float *sf, void *gx,
                                                                      int64_t blocks, int64_t mmax, int64_t h, int64_t hb_n,
                                                                      const int32_t *masked_m, const int32_t *m_indices, bool vec,
                                                                      bool ue8m0, bool small)
{
    const int64_t blk = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (blk >= blocks) return;  // whole 16-lane groups leave together: the row maxima below never see a lane of another block
    int64_t row, b;
    if (!locate_row(blk, hb_n, mmax, masked_m, m_indices, small, row, b)) return;
    const int sub = threadIdx.x & 15;
    const int64_t c0 = b * 128 + sub * 8;
    const int64_t gbase = row * 2 * h + c0, ubase = gbase + h, dbase = row * h + c0;
    float g8[8], u8[8], d8[8];
    load8_bounded<T>(x, gbase, g8, vec, 0, 8);      // (0, 8): h % 128 == 0, all 8 are inside the row
    load8_bounded<T>(x, ubase, u8, vec, 0, 8);
    load8_bounded<T>(grad, dbase, d8, vec, 0, 8);
    float vg[8], vu[8];
    // each block's largest magnitude in this lane (NaN never compares greater: ignored) and the inputs it came from
    float amax_g = 0.f, gg = 0.f, ug = 0.f, dg = 0.f, amax_u = 0.f, gu = 0.f, du = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        silu_mul_bwd(g8[j], u8[j], d8[j], vg[j], vu[j]);
        const float ag = __builtin_fabsf(vg[j]), au = __builtin_fabsf(vu[j]);
        const bool wg = ag > amax_g, wu = au > amax_u;
        amax_g = wg ? ag : amax_g;
        gg = wg ? g8[j] : gg;
        ug = wg ? u8[j] : ug;
        dg = wg ? d8[j] : dg;
        amax_u = wu ? au : amax_u;
        gu = wu ? g8[j] : gu;
        du = wu ? d8[j] : du;
    }
    if (gx) {
        Store8<T>::run(gx, gbase, vg, vec);
        Store8<T>::run(gx, ubase, vu, vec);
    }
    const float sg = block_scale(row16_max(dgate_abs_rounded(gg, ug, dg, amax_g)), ue8m0);
    const float su = block_scale(row16_max(dup_abs_rounded(gu, du, amax_u)), ue8m0);
    if (sub == 0) {
        sf[row * 2 * hb_n + b] = sg;
        sf[row * 2 * hb_n + hb_n + b] = su;
    }
    uint32_t w0, w1;
    quant8(vg, sg, w0, w1);
    store_codes8(q + gbase, w0, w1, vec, 0, 8);
    quant8(vu, su, w0, w1);
    store_codes8(q + ubase, w0, w1, vec, 0, 8);
}

}  // namespace dga

extern "C" int dga_silu_mul_bwd_cast_to_fp8_1x128(const void *x, const void *grad_h, int dtype, int64_t groups, int64_t rows, int64_t h,
                                                  const int32_t *masked_m, const int32_t *m_indices, void *dq, float *dsf,
                                                  void *grad_x, int flags, void *stream)
{
    using namespace dga;
    return run_fused(flags, dtype, groups, rows, h, 128, masked_m, m_indices, x && grad_h && dq && dsf, [&](auto tag, const FusedGeometry &g) {
        using T = decltype(tag);
        // every access starts a multiple of 8 elements (codes: 8 bytes) into a row or half of h % 128 == 0 elements
        const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
        const bool vec = al(x, 16) && al(grad_h, 16) && al(dq, 8) && al(grad_x, 16);
        hipLaunchKernelGGL(silu_mul_bwd_cast_1x128_kernel<T>, dim3(g.grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, grad_h,
                           static_cast<uint8_t *>(dq), dsf, grad_x, g.blocks, rows, h, g.hb_n, masked_m, m_indices, vec, g.ue8m0, g.small);
        return record_hip(hipGetLastError());
    });
}
