// The optimizer step of grouped expert weights fused into the quantiser of what the next step reads: AdamW on the fp32 master weights
// w [groups, n, k] with their moments and the fp32 (bf16) weight gradient, and both fp8 layouts of the updated weights, in one pass.
//   dga_adamw_cast_to_fp8_128x128_transposed   w, m, v (in place), grad, step_scalars {lr, bc1, bc2s, grad_scale} on the device
//                                              -> (qt, sft), optionally (q_row, sf_row): dga_cast_to_fp8_128x128_transposed of the w it
//                                                 leaves behind, byte for byte
//   dga_adamw_cast_to_fp8_128x128_transposed_skip   the same with a device flag (dga_grad_clip_scalars writes it): where skip[0] != 0 nothing
//                                              is stored to w, m and v, whatever grad holds, and the codes are those of the unchanged w
// 16 bytes in and 12 out per element for the update, 1 (2) out for the codes: 30 with fp32 moments and both layouts, 22 with bf16 moments;
// a separate optimizer and quantiser move 34.  Per element, every operation in fp32 and rounded on its own (this unit's text is compiled
// without contraction, the pragma below; division and square root are the correctly rounded ones, subnormals are kept):
//   g   = fl(grad * grad_scale)
//   m'  = fl(fl(beta1 * m) + fl(fl(1 - beta1) * g))
//   v'  = fl(fl(beta2 * v) + fl(fl(fl(1 - beta2) * g) * g))
//   den = fl(fl(sqrt(v') / bc2s) + eps)
//   w'  = fl(fl(w * fl(1 - fl(lr * weight_decay))) - fl(fl(lr / bc1) * fl(m' / den)))
// m' and v' are stored RNE in the moments' type; the update uses the unrounded ones.  The tile's maximum and the codes come from w' as it
// is stored, through dga_cast_transposed_block.hip's own text (quant_block_tile_transposed in dga_cast_device.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

#pragma clang fp contract(off)

namespace dga {

// which of the kernel's tensors take the 16-byte (codes: 8-byte) accesses; each decided on its own pointer
enum : uint32_t { ADAMW_VEC_W = 1, ADAMW_VEC_M = 2, ADAMW_VEC_V = 4, ADAMW_VEC_G = 8, ADAMW_VEC_QT = 16, ADAMW_VEC_ROW = 32 };

// What a step does not change per element: the launch arguments and the four device scalars, combined once per lane
struct AdamwStep {
    float grad_scale, beta1, omb1, beta2, omb2, bc2s, eps, decay, alpha;
};

__device__ __forceinline__ void adamw8(const AdamwStep &s, float (&w)[8], float (&m)[8], float (&v)[8], const float (&grad)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float g = grad[j] * s.grad_scale;
        const float a = s.beta1 * m[j], b = s.omb1 * g;
        m[j] = a + b;
        const float c = s.beta2 * v[j], d = (s.omb2 * g) * g;
        v[j] = c + d;
        const float den = __builtin_sqrtf(v[j]) / s.bc2s + s.eps;
        const float w1 = w[j] * s.decay, u = s.alpha * (m[j] / den);
        w[j] = w1 - u;
    }
}

// One workgroup per tile of 128 rows x 128 columns of one group, in cast_128x128_transposed_kernel's register shape: 16 lanes share a
// row, 8 consecutive columns per lane, and row group rg = t / 16 holds the 8 consecutive rows 8 rg .. 8 rg + 7, one per pass.  A pass
// loads the lane's 8 elements of w, m, v and grad -- all of them issued before the first is used --, forms and stores w', m', v', and
// keeps w' alone: 64 values per lane, the input of the existing tail.  Rows at and beyond n and columns at and beyond k are never loaded
// or stored; their place in the tile holds zeros.  TG: the gradient's type, TM: the moments'.
template <typename TG, typename TM, bool ROWWISE>
__global__ void __launch_bounds__(256) adamw_cast_128x128_transposed_kernel(float *w, void *m, void *v, const void *grad,
                                                                            const float *step_scalars, float beta1, float beta2, float eps,
                                                                            float weight_decay, uint8_t *qt, float *sft, uint8_t *q_row,
                                                                            float *sf_row, int64_t n, int64_t k, uint32_t nb_n,
                                                                            uint32_t kb_n, uint32_t vec, bool ue8m0, const int32_t *skip)
{
    const int t = threadIdx.x;
    const bool step = !skip || skip[0] == 0;   // (uniform) a skipped step stores nothing to w, m and v: the codes are those of w as it is
    const BlockTileAt at = block_tile_at(blockIdx.x, t, n, k, nb_n, kb_n);
    const int64_t c0 = at.c0, r0 = at.r0, g0 = at.g0;
    const float lr = step_scalars[0], bc1 = step_scalars[1];
    AdamwStep s;
    s.bc2s = step_scalars[2];
    s.grad_scale = step_scalars[3];
    s.beta1 = beta1;
    s.omb1 = 1.f - beta1;
    s.beta2 = beta2;
    s.omb2 = 1.f - beta2;
    s.eps = eps;
    const float lw = lr * weight_decay;
    s.decay = 1.f - lw;
    s.alpha = lr / bc1;
    const bool vec_w = vec & ADAMW_VEC_W, vec_m = vec & ADAMW_VEC_M, vec_v = vec & ADAMW_VEC_V, vec_g = vec & ADAMW_VEC_G;
    const bool all_vec = (vec & 15u) == 15u && (int64_t)at.kb * 128 + 128 <= k;   // (uniform) all 128 columns inside, every tensor aligned
    bool ok[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) ok[p] = r0 + p < n;
    float x[8][8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[p][j] = 0.f;
        if (!ok[p]) continue;   // (uniform over the 16 lanes of the row)
        const int64_t at_e = g0 + (r0 + p) * k + c0;
        float mm[8], vv[8], gg[8];
        if (all_vec) {
            const Elem<float>::Raw rw = Elem<float>::load8_raw(w, at_e);
            const typename Elem<TM>::Raw rm = Elem<TM>::load8_raw(m, at_e), rv = Elem<TM>::load8_raw(v, at_e);
            const typename Elem<TG>::Raw rg = Elem<TG>::load8_raw(grad, at_e);
            Elem<float>::unpack8(rw, x[p]);
            Elem<TM>::unpack8(rm, mm);
            Elem<TM>::unpack8(rv, vv);
            Elem<TG>::unpack8(rg, gg);
            if (step) {
                adamw8(s, x[p], mm, vv, gg);
                Store8<float>::run(w, at_e, x[p], true);
                Store8<TM>::run(m, at_e, mm, true);
                Store8<TM>::run(v, at_e, vv, true);
            }
        } else {
            load8_bounded<float>(w, at_e, x[p], vec_w, c0, k);
            load8_bounded<TM>(m, at_e, mm, vec_m, c0, k);
            load8_bounded<TM>(v, at_e, vv, vec_v, c0, k);
            load8_bounded<TG>(grad, at_e, gg, vec_g, c0, k);
            if (step) {
                adamw8(s, x[p], mm, vv, gg);
                store8_bounded<float>(w, at_e, x[p], vec_w, c0, k);
                store8_bounded<TM>(m, at_e, mm, vec_m, c0, k);
                store8_bounded<TM>(v, at_e, vv, vec_v, c0, k);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) x[p][j] = c0 + j < k ? x[p][j] : 0.f;   // (eps = 0 makes 0 / 0 of the zeros beyond k)
        }
    }
    quant_block_tile_transposed<ROWWISE>(x, ok, at, t, qt, sft, q_row, sf_row, n, k, nb_n, kb_n, (vec & ADAMW_VEC_QT) != 0,
                                         (vec & ADAMW_VEC_ROW) != 0, ue8m0);
}

}  // namespace dga

extern "C" int dga_adamw_cast_to_fp8_128x128_transposed_skip(void *w, void *m, void *v, int moment_dtype, const void *grad, int grad_dtype,
                                                             const float *step_scalars, float beta1, float beta2, float eps,
                                                             float weight_decay, int64_t groups, int64_t n, int64_t k, void *qt, float *sft,
                                                             void *q_row, float *sf_row, int flags, const int32_t *skip, void *stream)
{
    using namespace dga;
    // run_cast's order: flags, shape, nothing to do, pointers, dtypes, the ranges and the grid
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (groups < 0 || n < 0 || k < 0 || (q_row != nullptr) != (sf_row != nullptr)) return DGA_E_SHAPE;
    if (groups == 0 || n == 0 || k == 0) return DGA_OK;
    if (!w || !m || !v || !grad || !step_scalars || !qt || !sft) return DGA_E_NULL;
    const auto fp32_or_bf16 = [](int dt) { return dt == DGA_DT_FP32 || dt == DGA_DT_BF16; };
    if (!fp32_or_bf16(moment_dtype) || !fp32_or_bf16(grad_dtype)) return DGA_E_DTYPE;
    const auto beta_ok = [](float b) { return b >= 0.f && b < 1.f; };              // (false for a NaN)
    const auto term_ok = [](float x) { return x >= 0.f && !std::isinf(x); };
    if (!beta_ok(beta1) || !beta_ok(beta2) || !term_ok(eps) || !term_ok(weight_decay)) return DGA_E_RANGE;
    // one workgroup per tile, decided without a product or a sum that overflows
    const int64_t nb_n = n / 128 + (n % 128 != 0), kb_n = k / 128 + (k % 128 != 0);
    if (nb_n > 0x7FFFFFFFll / kb_n || groups > 0x7FFFFFFFll / (nb_n * kb_n)) return DGA_E_RANGE;
    const auto al = [](const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; };
    // as in dga_cast_to_fp8_128x128_transposed: with k % 8 == 0 (n % 8 == 0) every group and row starts on a multiple of 8 elements
    const bool k8 = k % 8 == 0;
    const uint32_t vec = (al(w, 16) && k8 ? ADAMW_VEC_W : 0) | (al(m, 16) && k8 ? ADAMW_VEC_M : 0) | (al(v, 16) && k8 ? ADAMW_VEC_V : 0) |
                         (al(grad, 16) && k8 ? ADAMW_VEC_G : 0) | (al(qt, 8) && n % 8 == 0 ? ADAMW_VEC_QT : 0) |
                         (al(q_row, 8) && k8 ? ADAMW_VEC_ROW : 0);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(groups * nb_n * kb_n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<float *>(w), m, v, grad, step_scalars, beta1, beta2, eps, weight_decay, static_cast<uint8_t *>(qt), sft,
                           static_cast<uint8_t *>(q_row), sf_row, n, k, static_cast<uint32_t>(nb_n), static_cast<uint32_t>(kb_n), vec,
                           (flags & DGA_CAST_UE8M0) != 0, skip);
    };
    const auto with_types = [&](auto tg, auto tm) {
        using TG = decltype(tg);
        using TM = decltype(tm);
        if (q_row) launch(adamw_cast_128x128_transposed_kernel<TG, TM, true>);
        else launch(adamw_cast_128x128_transposed_kernel<TG, TM, false>);
    };
    if (grad_dtype == DGA_DT_FP32 && moment_dtype == DGA_DT_FP32) with_types(float{}, float{});
    else if (grad_dtype == DGA_DT_FP32) with_types(float{}, Bf16Tag{});
    else if (moment_dtype == DGA_DT_FP32) with_types(Bf16Tag{}, float{});
    else with_types(Bf16Tag{}, Bf16Tag{});
    return record_hip(hipGetLastError());
}

extern "C" int dga_adamw_cast_to_fp8_128x128_transposed(void *w, void *m, void *v, int moment_dtype, const void *grad, int grad_dtype,
                                                        const float *step_scalars, float beta1, float beta2, float eps, float weight_decay,
                                                        int64_t groups, int64_t n, int64_t k, void *qt, float *sft, void *q_row,
                                                        float *sf_row, int flags, void *stream)
{
    return dga_adamw_cast_to_fp8_128x128_transposed_skip(w, m, v, moment_dtype, grad, grad_dtype, step_scalars, beta1, beta2, eps, weight_decay,
                                                         groups, n, k, qt, sft, q_row, sf_row, flags, nullptr, stream);
}
