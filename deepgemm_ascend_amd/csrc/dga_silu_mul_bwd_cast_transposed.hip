// The operand of the weight gradient of an expert MLP's FIRST GEMM, dW1[g] = dY1_g^T . x_g with dY1 = [dgate | dup] the backward of
// h = silu(gate) * up, from the tensors that backward reads: dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt runs K along the tokens and wants
// cast_to_fp8_1x128(dY1^T).
//   dga_silu_mul_bwd_cast_to_fp8_1x128_transposed   x [groups, rows, 2h] = [gate | up], grad_h [groups, rows, h] (fp32 / bf16 / fp16),
//                                                   T = groups * rows, optional row mask
//                                                   -> qt [2h, T], sft [2h, ceil(T/128)] of where(valid, [dgate | dup], 0)^T;
//                                                      optionally (q_row, sf_row) = dga_silu_mul_bwd_cast_to_fp8_1x128(x, grad_h) on the
//                                                      valid rows, from the same read
// One pass: 6 bytes in and 2 out per (gate, up) pair (bf16), 2 more with the row-wise output: 10.  dga_silu_mul_bwd_cast_to_fp8_1x128 with
// grad_x followed by dga_cast_to_fp8_1x128_transposed moves 18 and quantises a gradient rounded to 16 bits.  Here both gradients live in
// fp32 registers only, formed by dga_silu_mul_bwd_cast.hip's device text (silu_mul_bwd; the row-wise scales through dgate_abs_rounded /
// dup_abs_rounded) on dga_cast_transposed.hip's tile (rows_valid8; all in dga_cast_device.hpp).
// The contract is by composition: with G the fp32 grad_x that dga_silu_mul_bwd_cast_to_fp8_1x128 writes for the fp32 up-conversion of
// (x, grad_h), (qt, sft) are dga_cast_to_fp8_1x128_transposed(G, same mask) byte for byte, for every input type and on every input.  So the
// amax of a 128-token block is the plain fp32 maximum of the fp32 gradients, taken as cast_1x128_transposed_kernel takes it (no NaN of any
// kind enters) -- NOT re-evaluated in fp64 as silu_mul_cast_1x128_transposed_kernel does: that refinement lets a float64 reference predict
// the scales, and here the composition is an exact device-side oracle instead (and the three inputs per channel need no LDS parking).
// Rows a mask excludes are not read: their gradients are +0, their codes are 0, and a 128-token block without a valid token has scale 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// The end of a pass for the compiler: its 8 gradients are taken as computed here and no memory access moves across.  Without it the
// arithmetic is put off while the inputs (24 values a pass) wait, or the next batch's loads are gathered in front of it: neither fits
// beside the 64 gradients in 128 VGPRs.
__device__ __forceinline__ void bwd_pass_done(float (&v)[8])
{
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) : : "memory");
}

// One half (UP = false: dgate, channels 0 .. h - 1 of the result; UP = true: dup, channels h .. 2h - 1) of one tile of 128 tokens x 128
// channels, cast_1x128_transposed_kernel's tile: 16 lanes per row with 8 consecutive channels each, row group rg = t / 16 holds the 8
// consecutive tokens 8 rg .. 8 rg + 7, one per pass, 64 fp32 gradients per lane.  h % 128 == 0: all 128 channels are inside.
//   loads             gate at row * 2h + c, up h elements later (dgate alone reads it), grad_h at row * h + c: one 16-byte load each per
//                     pass (fp32: two).  The predicated raw loads of a batch of passes go out together before the first is used: 2 passes
//                     of the 16-bit types, 1 of fp32 -- 24 registers of raw words for three streams, what fits beside the 64 gradients.
//   row-wise output   (ROWWISE) per pass what silu_mul_bwd_cast_1x128_kernel does for its 16-lane block and this half, in its order: the
//                     lane's strict-> maximum with its inputs, dgate_abs_rounded / dup_abs_rounded, row16_max, block_scale, quant8 --
//                     that kernel's bits.
//   channel maxima, codes   cast_1x128_transposed_kernel's text on the fp32 gradients.
template <typename T, bool UP, bool ROWWISE>
__device__ __forceinline__ void silu_mul_bwd_half_tile(const void *x, const void *grad, uint8_t *qt, float *sft, uint8_t *q_row, float *sf_row,
                                                       int64_t t_n, int64_t h, uint32_t hb_n, uint32_t tb, uint32_t hb, int64_t tb_n,
                                                       int64_t ldqt, int64_t mmax, const int32_t *masked_m, const int32_t *m_indices,
                                                       bool vec_in, bool vec_qt, bool vec_row, bool ue8m0, bool small,
                                                       float (&red)[4][128], uint64_t (&tile)[128 * 16])
{
    constexpr int kBatch = Elem<T>::kBytes == 4 ? 1 : 2;
    const int t = threadIdx.x, sub = t & 15, rg = t >> 4;
    const int64_t c0 = (int64_t)hb * 128 + sub * 8;   // the lane's 8 channels of gate, up and grad_h
    const int64_t r0 = (int64_t)tb * 128 + rg * 8;    // ... and its 8 tokens
    const int64_t o0 = (UP ? h : 0) + c0;             // ... and its 8 channels of the result
    bool ok[8];
    rows_valid8(r0, t_n, mmax, masked_m, m_indices, small, ok);
    float v[8][8];
    // pass p with the lane's 8 gates, ups and grads in hand (zeros for a token that is not valid: both gradients are +0)
    const auto pass = [&](int p, const float (&g8)[8], const float (&u8)[8], const float (&d8)[8]) {
        float amax = 0.f, gm = 0.f, um = 0.f, dm = 0.f;   // silu_mul_bwd_cast_1x128_kernel's: the lane's largest magnitude and its inputs
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float vg, vu;
            silu_mul_bwd(g8[j], u8[j], d8[j], vg, vu);
            v[p][j] = UP ? vu : vg;
            if (ROWWISE) {
                const float a = __builtin_fabsf(v[p][j]);
                const bool gt = a > amax;
                amax = gt ? a : amax;
                gm = gt ? g8[j] : gm;
                um = gt ? u8[j] : um;
                dm = gt ? d8[j] : dm;
            }
        }
        if (ROWWISE) {
            // (the inputs are done with here: only the lane's maximum goes on into the fp64 text)
            asm volatile("" : "+v"(amax), "+v"(gm), "+v"(um), "+v"(dm) : : "memory");
            const float s = block_scale(row16_max(UP ? dup_abs_rounded(gm, dm, amax) : dgate_abs_rounded(gm, um, dm, amax)), ue8m0);
            uint32_t w0, w1;
            quant8(v[p], s, w0, w1);
            if (ok[p]) {   // (uniform over the 16 lanes of the row)
                const int64_t row = r0 + p;
                if (sub == 0) sf_row[row * 2 * hb_n + (UP ? hb_n : 0) + hb] = s;
                store_codes8(q_row + row * 2 * h + o0, w0, w1, vec_row, 0, 8);
            }
        }
    };
    if (vec_in) {   // (uniform) a batch's predicated raw loads, then their use
#pragma unroll
        for (int b = 0; b < 8; b += kBatch) {
            typename Elem<T>::Raw rawg[kBatch], rawu[kBatch], rawd[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                rawg[i] = rawu[i] = rawd[i] = typename Elem<T>::Raw{};
                if (ok[b + i]) {
                    const int64_t base = (r0 + b + i) * 2 * h + c0;
                    rawg[i] = Elem<T>::load8_raw(x, base);
                    if (!UP) rawu[i] = Elem<T>::load8_raw(x, base + h);
                    rawd[i] = Elem<T>::load8_raw(grad, (r0 + b + i) * h + c0);
                }
            }
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                float g8[8], u8[8], d8[8];
                Elem<T>::unpack8(rawg[i], g8);
                Elem<T>::unpack8(rawu[i], u8);
                Elem<T>::unpack8(rawd[i], d8);
                pass(b + i, g8, u8, d8);
                bwd_pass_done(v[b + i]);
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int64_t base = (r0 + p) * 2 * h + c0;
            float g8[8], u8[8], d8[8];
            load8_bounded<T>(x, base, g8, false, 0, 8, ok[p]);   // (0, 8): h % 128 == 0, all 8 are inside the row
            load8_bounded<T>(x, base + h, u8, false, 0, 8, ok[p] && !UP);
            load8_bounded<T>(grad, (r0 + p) * h + c0, d8, false, 0, 8, ok[p]);
            pass(p, g8, u8, d8);
            bwd_pass_done(v[p]);
        }
    }
    // (from here on cast_1x128_transposed_kernel's text)
    float cm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cm[j] = 0.f;
#pragma unroll
        for (int p = 0; p < 8; ++p)
            cm[j] = __builtin_fmaxf(cm[j], abs_for_max(v[p][j]));
        cm[j] = __builtin_fmaxf(cm[j], __shfl_xor(cm[j], 16, 64));
        cm[j] = __builtin_fmaxf(cm[j], __shfl_xor(cm[j], 32, 64));
    }
    if ((t & 48) == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[t >> 6][sub * 8 + j] = cm[j];
    }
    __syncthreads();
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = sub * 8 + j;
        s[j] = block_scale(__builtin_fmaxf(__builtin_fmaxf(red[0][c], red[1][c]), __builtin_fmaxf(red[2][c], red[3][c])), ue8m0);
        if (rg == 0) sft[(o0 + j) * tb_n + tb] = s[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float e[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) e[p] = v[p][j];
        uint32_t w0, w1;
        quant8(e, s[j], w0, w1);
        tile[(sub * 8 + j) * 16 + (rg ^ sub)] = (uint64_t)w0 | ((uint64_t)w1 << 32);
    }
    __syncthreads();
    const int64_t tc = (int64_t)tb * 128 + sub * 8;   // the first of the 8 tokens this lane stores, of channel rg + 16 i
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ch = rg + 16 * i;
        const int64_t c = (UP ? h : 0) + (int64_t)hb * 128 + ch;
        const uint64_t w = tile[ch * 16 + (sub ^ (ch >> 3))];
        store_codes8(qt + c * ldqt + tc, (uint32_t)w, (uint32_t)(w >> 32), vec_qt, tc, ldqt);
    }
}

// One workgroup per (tile, half): the two halves of 128 channels are 128 fp32 gradients per lane, which fit beside nothing.  The two
// workgroups of a tile are neighbours in block order (the half is the lowest bit), so the second read of gate and grad_h meets the L2; the
// dgate workgroup reads gate, up and grad_h, the dup workgroup gate and grad_h.  Tiles that follow each other share the tokens, as in
// cast_1x128_transposed_kernel.
// __launch_bounds__(256, 4): at most 128 VGPRs, four workgroups of 18 KB LDS per CU.
template <typename T, bool ROWWISE>
__global__ void __launch_bounds__(256, 4) silu_mul_bwd_cast_1x128_transposed_kernel(const void *x, const void *grad, uint8_t *qt, float *sft,
                                                                                 uint8_t *q_row, float *sf_row, int64_t t_n, int64_t h,
                                                                                 uint32_t hb_n, int64_t tb_n, int64_t ldqt, int64_t mmax,
                                                                                 const int32_t *masked_m, const int32_t *m_indices,
                                                                                 bool vec_in, bool vec_qt, bool vec_row, bool ue8m0,
                                                                                 bool small)
{
    __shared__ float red[4][128];
    __shared__ uint64_t tile[128 * 16];
    const uint32_t at = blockIdx.x >> 1;
    const uint32_t tb = at / hb_n, hb = at - tb * hb_n;
    if (blockIdx.x & 1)
        silu_mul_bwd_half_tile<T, true, ROWWISE>(x, grad, qt, sft, q_row, sf_row, t_n, h, hb_n, tb, hb, tb_n, ldqt, mmax, masked_m, m_indices,
                                                 vec_in, vec_qt, vec_row, ue8m0, small, red, tile);
    else
        silu_mul_bwd_half_tile<T, false, ROWWISE>(x, grad, qt, sft, q_row, sf_row, t_n, h, hb_n, tb, hb, tb_n, ldqt, mmax, masked_m, m_indices,
                                                  vec_in, vec_qt, vec_row, ue8m0, small, red, tile);
}

}  // namespace dga

extern "C" int dga_silu_mul_bwd_cast_to_fp8_1x128_transposed(const void *x, const void *grad_h, int dtype, int64_t groups, int64_t rows,
                                                             int64_t h, const int32_t *masked_m, const int32_t *m_indices, void *qt,
                                                             int64_t ldqt, float *sft, void *q_row, float *sf_row, int flags, void *stream)
{
    using namespace dga;
    const bool shape_ok = transposed_ldqt_ok(groups, rows, ldqt) && (q_row != nullptr) == (sf_row != nullptr);
    return run_fused(flags, dtype, groups, rows, h, 128, masked_m, m_indices, x && grad_h && qt && sft,
                     [&](auto tag, const FusedGeometry &g) -> int {
        using T = decltype(tag);
        const int64_t t_n = groups * rows, tb_n = (t_n + 127) / 128;
        if (tb_n * g.hb_n > 0x7FFFFFFFll / 2) return DGA_E_RANGE;   // one workgroup per tile and half
        const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
        // every input access starts a multiple of 8 elements into a row or half of h % 128 == 0 elements, every row-wise code store a
        // multiple of 8 bytes into a row of 2h
        const bool vec_in = al(x, 16) && al(grad_h, 16);
        const bool vec_qt = al(qt, 8) && ldqt % 8 == 0, vec_row = al(q_row, 8);
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tb_n * g.hb_n * 2)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                               grad_h, static_cast<uint8_t *>(qt), sft, static_cast<uint8_t *>(q_row), sf_row, t_n, h,
                               static_cast<uint32_t>(g.hb_n), tb_n, ldqt, rows, masked_m, m_indices, vec_in, vec_qt, vec_row, g.ue8m0, g.small);
        };
        if (q_row) launch(silu_mul_bwd_cast_1x128_transposed_kernel<T, true>);
        else launch(silu_mul_bwd_cast_1x128_transposed_kernel<T, false>);
        return record_hip(hipGetLastError());
    }, shape_ok);
}
