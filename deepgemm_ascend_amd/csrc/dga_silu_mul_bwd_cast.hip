// The backward of the activation between the two GEMMs of a MoE expert MLP, fused into the quantiser that feeds the dgrad of the first:
//   dga_silu_mul_bwd_cast_to_fp8_1x128   x[groups, rows, 2h], grad_h[groups, rows, h] (bf16 / fp16 / fp32)
//                                        -> e4m3fn bytes [groups, rows, 2h] + fp32 scale per 1x128, optionally the gradient itself
//   dgate = d * u * silu'(g),  dup = d * silu(g),  g = x[..., :h], u = x[..., h:], d = grad_h,
//   silu(g) = g s,  silu'(g) = s + g s (1 - s),  s = 1 / (1 + exp(-g))
// in one pass over the valid rows: 6 bytes in and 2 out per (gate, up) pair (bf16), 4 more with grad_x.  Both gradients live in fp32
// registers only; the quantiser proper is dga_cast.hip's (dga_cast_device.hpp), so (dq, dsf) are byte for byte what
// dga_cast_to_fp8_1x128_ex gives on the same fp32 [dgate | dup].  h % 128 == 0: a 1x128 block of the [2h] axis is either gate's or up's.
//
// Accuracy (DESIGN.md "Fused SiLU-and-multiply backward quantiser"), e = exp(-g) from v_exp_f32, s from a refined v_rcp_f32 as in
// dga_silu_mul_cast.hip, 1 - s taken as e s (no cancellation for large g), silu' = fma(g s, e s, s):
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

// dgate = (d u) silu'(g) and dup = d (g s).  s as silu_mul's r1 (dga_silu_mul_cast.hip): with e = inf the reciprocal is 0, the Newton
// residual NaN, dropped by v_max_f32.  t = e s is 1 - s; e = inf gives inf * 0 = NaN there, dropped by v_min_f32 in favour of the 1
// that 1 - s tends to (e s <= 1 in real numbers, so the min changes nothing else).  A NaN g still gives NaN: s is NaN.
__device__ __forceinline__ void silu_mul_bwd(float g, float u, float d, float &dgate, float &dup)
{
    const float e = __builtin_amdgcn_exp2f(g * -1.4426950408889634f);
    const float dn = 1.f + e;
    const float r0 = __builtin_amdgcn_rcpf(dn);
    const float s = __builtin_fmaf(__builtin_fmaxf(__builtin_fmaf(-dn, r0, 1.f), -1.f), r0, r0);
    const float t = __builtin_fminf(e * s, 1.f);
    const float gs = g * s;
    dgate = (d * u) * __builtin_fmaf(gs, t, s);
    dup = d * gs;
}

// The lane's largest |dgate| and |dup| once more, as the fp32 nearest to the real-number value (silu_mul_abs_rounded's reasons: the
// block scale is amax / 448).  Where the fp32 factor is exactly 1 the value stays the fp32 product: the contract for gate >= 20.  An
// element whose fp32 value is 0 never is a lane's maximum, so g > -88.8 here and exp(-g) is finite in fp64.
__device__ __forceinline__ float dgate_abs_rounded(float g, float u, float d, float v32)
{
    const float e = __builtin_amdgcn_exp2f(g * -1.4426950408889634f);
    const bool one = 1.f + e == 1.f && __builtin_fmaf(g, e, 1.f) == 1.f;
    const double gd = g, ed = exp(-gd), sd = 1.0 / (1.0 + ed);
    const float vd = (float)((double)d * (double)u * (sd * (1.0 + gd * (ed * sd))));
    return one ? v32 : __builtin_fabsf(vd);
}
__device__ __forceinline__ float dup_abs_rounded(float g, float d, float v32)
{
    const bool one = 1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f) == 1.f;
    const double gd = g;
    const float vd = (float)((double)d * (gd / (1.0 + exp(-gd))));
    return one ? v32 : __builtin_fabsf(vd);
}

__device__ __forceinline__ int64_t udiv_bwd(int64_t a, int64_t b, bool small)
{
    return small ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// 8 fp32 values -> 8 elements of T at element index i: round to nearest even for the 16-bit types (v_cvt_pk_bf16_f32, v_cvt_f16_f32),
// as they are for fp32.  vec: 16-byte stores.
template <typename T> struct Store8;
template <> struct Store8<float> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        float *o = (float *)p + i;
        if (vec) {
            *(v4f_c *)o = v4f_c{v[0], v[1], v[2], v[3]};
            *(v4f_c *)(o + 4) = v4f_c{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = v[j];
        }
    }
};
template <> struct Store8<Bf16Tag> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        typedef float v2f __attribute__((ext_vector_type(2)));
        typedef __bf16 v2b __attribute__((ext_vector_type(2)));
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f{v[2 * j], v[2 * j + 1]}), v2b));
        uint16_t *o = (uint16_t *)p + i;
        if (vec) {
            *(v4i_c *)o = v4i_c{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
};
template <> struct Store8<F16Tag> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        typedef _Float16 v8h __attribute__((ext_vector_type(8)));
        _Float16 *o = (_Float16 *)p + i;
        if (vec) {
            *(v8h *)o = v8h{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                            (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (_Float16)v[j];
        }
    }
};

__device__ __forceinline__ void store_codes8(uint8_t *q, uint32_t w0, uint32_t w1, bool vec)
{
    if (vec) {
        *(v2i_c *)q = v2i_c{(int)w0, (int)w1};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (uint8_t)(((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xFF);
    }
}

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
    const int64_t row = udiv_bwd(blk, hb_n, small);
    if (masked_m) {
        const int64_t g = udiv_bwd(row, mmax, small);
        if (row - g * mmax >= masked_m[g]) return;
    } else if (m_indices) {
        if (m_indices[row] < 0) return;
    }
    const int sub = threadIdx.x & 15;
    const int64_t b = blk - row * hb_n, c0 = b * 128 + sub * 8;
    const int64_t gbase = row * 2 * h + c0, ubase = gbase + h, dbase = row * h + c0;
    float g8[8], u8[8], d8[8];
    if (vec) {
        Elem<T>::load8(x, gbase, g8);
        Elem<T>::load8(x, ubase, u8);
        Elem<T>::load8(grad, dbase, d8);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            g8[j] = Elem<T>::load(x, gbase + j);
            u8[j] = Elem<T>::load(x, ubase + j);
            d8[j] = Elem<T>::load(grad, dbase + j);
        }
    }
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
    store_codes8(q + gbase, w0, w1, vec);
    quant8(vu, su, w0, w1);
    store_codes8(q + ubase, w0, w1, vec);
}

template <typename T>
static int launch_silu_mul_bwd_cast(const void *x, const void *grad, int64_t rows_total, int64_t mmax, int64_t h,
                                    const int32_t *masked_m, const int32_t *m_indices, void *q, float *sf, void *gx, bool ue8m0,
                                    hipStream_t stream)
{
    const int64_t hb_n = h / 128;
    if (rows_total > 0x7FFFFFFFll * 16 / hb_n) return DGA_E_RANGE;   // (also keeps rows_total * hb_n inside int64)
    const int64_t blocks = rows_total * hb_n;
    const int64_t grid = (blocks * 16 + 255) / 256;
    if (grid > 0x7FFFFFFFll) return DGA_E_RANGE;
    // every access starts a multiple of 8 elements (codes: 8 bytes) into a row or half of h % 128 == 0 elements
    const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
    const bool vec = al(x, 16) && al(grad, 16) && al(q, 8) && al(gx, 16);
    const bool small = blocks <= 0xFFFFFFFFll && mmax <= 0xFFFFFFFFll;
    hipLaunchKernelGGL(silu_mul_bwd_cast_1x128_kernel<T>, dim3(static_cast<unsigned>(grid)), dim3(256), 0, stream, x, grad,
                       static_cast<uint8_t *>(q), sf, gx, blocks, mmax, h, hb_n, masked_m, m_indices, vec, ue8m0, small);
    return record_hip(hipGetLastError());
}

}  // namespace dga

extern "C" int dga_silu_mul_bwd_cast_to_fp8_1x128(const void *x, const void *grad_h, int dtype, int64_t groups, int64_t rows, int64_t h,
                                                  const int32_t *masked_m, const int32_t *m_indices, void *dq, float *dsf,
                                                  void *grad_x, int flags, void *stream)
{
    using namespace dga;
    // (dga_silu_mul_cast_to_fp8_1x128's order: flags, shape, nothing to do, pointers, dtype, grid)
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (groups < 1 || rows < 0 || h < 0 || h % 128 != 0 || (masked_m && m_indices) || (m_indices && groups != 1)) return DGA_E_SHAPE;
    if (rows == 0 || h == 0) return DGA_OK;
    if (!x || !grad_h || !dq || !dsf) return DGA_E_NULL;
    if (dtype != DGA_DT_FP32 && dtype != DGA_DT_BF16 && dtype != DGA_DT_FP16) return DGA_E_DTYPE;
    if (groups > 0x7FFFFFFFFFFFFFFFll / rows) return DGA_E_RANGE;
    const bool ue8m0 = (flags & DGA_CAST_UE8M0) != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t rt = groups * rows;
    switch (dtype) {
        case DGA_DT_FP32: return launch_silu_mul_bwd_cast<float>(x, grad_h, rt, rows, h, masked_m, m_indices, dq, dsf, grad_x, ue8m0, st);
        case DGA_DT_BF16: return launch_silu_mul_bwd_cast<Bf16Tag>(x, grad_h, rt, rows, h, masked_m, m_indices, dq, dsf, grad_x, ue8m0, st);
        case DGA_DT_FP16: return launch_silu_mul_bwd_cast<F16Tag>(x, grad_h, rt, rows, h, masked_m, m_indices, dq, dsf, grad_x, ue8m0, st);
        default: return DGA_E_DTYPE;
    }
}
