// The operand of the weight gradient of an expert MLP's SECOND GEMM, dW2[g] = dout_g^T . h_g with h = silu(gate) * up, from the tensor the
// forward's activation read: dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt runs K along the tokens and wants cast_to_fp8_1x128(h^T).
//   dga_silu_mul_cast_to_fp8_1x128_transposed   x [groups, rows, 2h] = [gate | up] (fp32 / bf16 / fp16), T = groups * rows, optional row mask
//                                               -> qt [h, T], sft [h, ceil(T/128)] of where(valid, silu(gate) * up, 0)^T;
//                                                  optionally (q_row, sf_row) = dga_silu_mul_cast_to_fp8_1x128(x) on the valid rows, from the
//                                                  same read
// One pass: 4 bytes in and 1 out per element of h (bf16), 1 more with the row-wise output; torch's silu * up in bf16 followed by
// dga_cast_to_fp8_1x128_transposed moves 13, on every padded row, and quantises an h rounded to 16 bits.  Here h lives in fp32 registers
// only, formed by dga_silu_mul_cast.hip's device text (silu_mul, silu_mul_abs_rounded: the accuracy stated there), on
// dga_cast_transposed.hip's tile (rows_valid8; all three in dga_cast_device.hpp).  Rows a mask excludes are not read: their h is +0, their
// codes are 0, and a 128-token block without a valid token has scale 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// The end of a pass for the compiler: the 8 running maxima are taken as computed here and no memory access moves across.  Without it the
// passes' loads are gathered in front of their arithmetic (the bounded path: all 8 passes'), and the inputs waiting there do not fit 128 VGPRs.
__device__ __forceinline__ void pass_done(float (&cm)[8])
{
    asm volatile("" : "+v"(cm[0]), "+v"(cm[1]), "+v"(cm[2]), "+v"(cm[3]), "+v"(cm[4]), "+v"(cm[5]), "+v"(cm[6]), "+v"(cm[7]) : : "memory");
}

// cast_1x128_transposed_kernel's tile: one workgroup per 128 tokens x 128 channels, 16 lanes per row with 8 consecutive channels each, row
// group rg = t / 16 holds the 8 consecutive tokens 8 rg .. 8 rg + 7, one per pass, 64 fp32 values of h per lane.
//   loads             gate at row * 2h + c, up h elements later: one 16-byte load each per pass (fp32: two).  The predicated raw loads of a
//                     batch of passes go out together before the first is used: 4 passes of the 16-bit types (32 registers of raw words,
//                     128 bytes in flight per lane), 1 of fp32 (16 registers, 64 bytes) -- what fits beside the 64 registers of h.
//   row-wise output   (ROWWISE) per pass what silu_mul_cast_1x128_kernel does for its 16-lane block, in its order: the lane's strict->
//                     maximum with its (gate, up), silu_mul_abs_rounded, row16_max, block_scale, quant8 -- that kernel's bits.
//   channel maxima    per lane and channel the strict-> maximum of |h| over the lane's 8 tokens in token order: a NaN never compares
//                     greater, so none enters.  The (gate, up) of the current maximum wait in LDS, in the 16 KB of the tile, which nothing
//                     else uses before the codes (8 bytes per lane and channel, [channel][lane]: a lane reads what it wrote, no barrier);
//                     in registers they would be 16 more than 128 allow.  After the passes the one value per channel is taken again as the
//                     fp32 nearest to the real-number value (silu_mul_abs_rounded, fp64) -- 8 evaluations per lane for 64 elements, the
//                     forward's 1 per 8 -- and then reduced as in cast_1x128_transposed_kernel: the scale is a float64 reference's.
//   codes             quant8 of the fp32 h with the channel's scale, through the swizzled tile: cast_1x128_transposed_kernel's text, which
//                     stays in both kernels (shared as a function it changes that kernel's registers and instructions).
// __launch_bounds__(256, 4): at most 128 VGPRs, four workgroups of 18 KB LDS per CU.
template <typename T, bool ROWWISE>
__global__ void __launch_bounds__(256, 4) silu_mul_cast_1x128_transposed_kernel(const void *x, uint8_t *qt, float *sft, uint8_t *q_row,
                                                                             float *sf_row, int64_t t_n, int64_t h, uint32_t hb_n,
                                                                             int64_t tb_n, int64_t ldqt, int64_t mmax,
                                                                             const int32_t *masked_m, const int32_t *m_indices, bool vec_in,
                                                                             bool vec_qt, bool vec_row, bool ue8m0, bool small)
{
    __shared__ float red[4][128];
    __shared__ uint64_t tile[128 * 16];
    constexpr int kBatch = Elem<T>::kBytes == 4 ? 1 : 4;   // 64 bytes of gate and up per lane and pass (fp32), 32 (16-bit types)
    const int t = threadIdx.x, sub = t & 15, rg = t >> 4;
    const uint32_t tb = blockIdx.x / hb_n, hb = blockIdx.x - tb * hb_n;
    const int64_t c0 = (int64_t)hb * 128 + sub * 8;   // the lane's 8 channels
    const int64_t r0 = (int64_t)tb * 128 + rg * 8;    // ... and its 8 tokens
    bool ok[8];
    rows_valid8(r0, t_n, mmax, masked_m, m_indices, small, ok);
    float v[8][8], cm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cm[j] = 0.f;
    // pass p with the lane's 8 gates and ups in hand (zeros for a token that is not valid: h = +0)
    const auto pass = [&](int p, const float (&g8)[8], const float (&u8)[8]) {
        float amax = 0.f, gmax = 0.f, umax = 0.f;   // silu_mul_cast_1x128_kernel's: the lane's largest |h| of this row and its inputs
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[p][j] = silu_mul(g8[j], u8[j]);
            const float a = __builtin_fabsf(v[p][j]);
            if (ROWWISE) {
                const bool gt = a > amax;
                amax = gt ? a : amax;
                gmax = gt ? g8[j] : gmax;
                umax = gt ? u8[j] : umax;
            }
            if (a > cm[j]) {   // ... and the same along the tokens, the inputs parked in the tile's LDS
                cm[j] = a;
                tile[j * 256 + t] = (uint64_t)__float_as_uint(g8[j]) | ((uint64_t)__float_as_uint(u8[j]) << 32);
            }
        }
        if (ROWWISE) {
            // (the gates and ups are done with here: only the lane's maximum goes on into the fp64 text)
            asm volatile("" : "+v"(amax), "+v"(gmax), "+v"(umax) : : "memory");
            pass_done(cm);
            const float s = block_scale(row16_max(silu_mul_abs_rounded(gmax, umax, amax)), ue8m0);
            uint32_t w0, w1;
            quant8(v[p], s, w0, w1);
            if (ok[p]) {   // (uniform over the 16 lanes of the row)
                const int64_t row = r0 + p;
                if (sub == 0) sf_row[row * hb_n + hb] = s;
                store_codes8(q_row + row * h + c0, w0, w1, vec_row, c0, h);
            }
        }
    };
    if (vec_in && (int64_t)hb * 128 + 128 <= h) {   // (uniform) all 128 channels inside: a batch's predicated raw loads, then their use
#pragma unroll
        for (int b = 0; b < 8; b += kBatch) {
            typename Elem<T>::Raw rawg[kBatch], rawu[kBatch];
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                rawg[i] = rawu[i] = typename Elem<T>::Raw{};
                if (ok[b + i]) {
                    const int64_t base = (r0 + b + i) * 2 * h + c0;
                    rawg[i] = Elem<T>::load8_raw(x, base);
                    rawu[i] = Elem<T>::load8_raw(x, base + h);
                }
            }
#pragma unroll
            for (int i = 0; i < kBatch; ++i) {
                float g8[8], u8[8];
                Elem<T>::unpack8(rawg[i], g8);
                Elem<T>::unpack8(rawu[i], u8);
                pass(b + i, g8, u8);
                pass_done(cm);
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int64_t base = (r0 + p) * 2 * h + c0;
            float g8[8], u8[8];
            load8_bounded<T>(x, base, g8, vec_in, c0, h, ok[p]);
            load8_bounded<T>(x, base + h, u8, vec_in, c0, h, ok[p]);   // (columns past h read as 0: silu(0) * 0 = 0)
            pass(p, g8, u8);
            pass_done(cm);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t w = tile[j * 256 + t];   // (never written while cm[j] is 0: not used then)
        const float r = silu_mul_abs_rounded(__uint_as_float((uint32_t)w), __uint_as_float((uint32_t)(w >> 32)), cm[j]);
        cm[j] = cm[j] > 0.f ? r : 0.f;
        asm volatile("" : "+v"(cm[j]) : : "memory");   // (one channel after the other, as the passes)
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cm[j] = __builtin_fmaxf(cm[j], __shfl_xor(cm[j], 16, 64));
        cm[j] = __builtin_fmaxf(cm[j], __shfl_xor(cm[j], 32, 64));
    }
    // (from here on cast_1x128_transposed_kernel's text)
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
        if (rg == 0 && c0 + j < h) sft[(c0 + j) * tb_n + tb] = s[j];
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
        const int64_t c = (int64_t)hb * 128 + ch;
        if (c >= h) break;
        const uint64_t w = tile[ch * 16 + (sub ^ (ch >> 3))];
        store_codes8(qt + c * ldqt + tc, (uint32_t)w, (uint32_t)(w >> 32), vec_qt, tc, ldqt);
    }
}

}  // namespace dga

extern "C" int dga_silu_mul_cast_to_fp8_1x128_transposed(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                                         const int32_t *masked_m, const int32_t *m_indices, void *qt, int64_t ldqt,
                                                         float *sft, void *q_row, float *sf_row, int flags, void *stream)
{
    using namespace dga;
    const bool shape_ok = transposed_ldqt_ok(groups, rows, ldqt) && (q_row != nullptr) == (sf_row != nullptr);
    return run_fused(flags, x_dtype, groups, rows, h, 1, masked_m, m_indices, x && qt && sft, [&](auto tag, const FusedGeometry &g) -> int {
        using T = decltype(tag);
        const int64_t t_n = groups * rows, tb_n = (t_n + 127) / 128;
        if (tb_n * g.hb_n > 0x7FFFFFFFll) return DGA_E_RANGE;   // one workgroup per tile
        const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
        // gate starts at element row * 2h + 8j, up h elements later: both 16-byte aligned for every row iff h * sizeof(T) % 16 == 0
        const bool vec_in = al(x, 16) && h * Elem<T>::kBytes % 16 == 0;
        const bool vec_qt = al(qt, 8) && ldqt % 8 == 0, vec_row = al(q_row, 8) && h % 8 == 0;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tb_n * g.hb_n)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                               static_cast<uint8_t *>(qt), sft, static_cast<uint8_t *>(q_row), sf_row, t_n, h, static_cast<uint32_t>(g.hb_n),
                               tb_n, ldqt, rows, masked_m, m_indices, vec_in, vec_qt, vec_row, g.ue8m0, g.small);
        };
        if (q_row) launch(silu_mul_cast_1x128_transposed_kernel<T, true>);
        else launch(silu_mul_cast_1x128_transposed_kernel<T, false>);
        return record_hip(hipGetLastError());
    }, shape_ok);
}
