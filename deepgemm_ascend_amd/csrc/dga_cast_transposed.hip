// The quantiser of the weight-gradient operands: activations live token-major, x [T, H], and both operands of dga_wgrad_gemm_fp8_fp8_fp32_nt /
// dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt are K-major along the tokens, cast_to_fp8_1x128(x^T): qt [H, T] e4m3fn bytes, sft [H, ceil(T/128)].
//   dga_cast_to_fp8_1x128_transposed   x [groups, rows, h] (fp32 / bf16 / fp16), T = groups * rows, optional row mask
//                                      -> qt, sft of where(valid, x, 0)^T, byte for byte dga_cast_to_fp8_1x128_ex on that transpose;
//                                         optionally (q_row, sf_row) = dga_cast_to_fp8_1x128_ex(x) on the valid rows, from the same read
// One pass: 2 bytes in and 1 out per element (bf16), 1 more with the row-wise output; the transpose-then-quantise pair moves 7 (10).
// Rows a mask excludes are not read: their codes are 0, and a 128-token block without a valid token has scale 1.  The quantiser proper
// is dga_cast.hip's (dga_cast_device.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// One workgroup per tile of 128 tokens x 128 channels; workgroups that follow each other share the tokens (whole rows of x are read side
// by side).  16 lanes share a row, 8 consecutive channels per lane (cast_1x128_kernel's loads: 256 contiguous bytes of bf16 per row), and
// row group rg = t / 16 holds the 8 CONSECUTIVE tokens 8 rg .. 8 rg + 7, one per pass: 64 fp32 values per lane, and the 8 codes of one
// channel in a lane are 8 neighbouring bytes of qt.
//   row-wise output (ROWWISE)   quant_row_block on each pass: the 16 lanes of a DPP row hold one 1x128 block of x.
//   channel maxima              in the lane over its 8 tokens; over the 4 row groups of a wave by two cross-lane moves; over the 4 waves
//                               through red (2 KB).  Every element is quieted first (abs_for_max), so no NaN of any kind reaches a maximum:
//                               there is no second pass.
//   codes                       quant8 on the lane's 8 tokens of each of its 8 channels, with the channel's scale, then one 8-byte LDS
//                               store per channel into the 16 KB tile [128 channels][16 slots of 8 tokens] and one 8-byte load per lane and
//                               output row: a 16-lane group stores 128 contiguous bytes of a row of qt.
// The tile is swizzled, not padded: slot k of channel ch lives at slot k ^ (ch / 8).  Store side (8-byte LDS stores go 16 lanes at a time,
// 32 banks of 4 bytes): the 16 lanes are the 16 values of ch / 8 at one k, so they hit 16 different slots = all 32 banks once; unswizzled they
// would be 1024 bytes apart, a 16-way conflict.  Load side (32 lanes at a time, 64 banks): two neighbouring channels, an even one (banks 0-31)
// and an odd one (banks 32-63), each with its 16 slots in some order: once each again.  Padding cannot serve the store side: its 16 lanes
// are 8 channel pitches apart, on 16 different bank pairs only for a pitch of an odd number of bytes, which no 8-byte store is aligned to.
// Tokens at and beyond t_n and tokens the mask excludes are zeros that were never loaded (a tile without a valid token loads nothing); the
// codes of the former fill a row of qt up to ldqt.
template <typename T, bool ROWWISE>
__global__ void __launch_bounds__(256) cast_1x128_transposed_kernel(const void *x, uint8_t *qt, float *sft, uint8_t *q_row, float *sf_row,
                                                                    int64_t t_n, int64_t h, uint32_t hb_n, int64_t tb_n, int64_t ldqt,
                                                                    int64_t mmax, const int32_t *masked_m, const int32_t *m_indices,
                                                                    bool vec_in, bool vec_qt, bool vec_row, bool ue8m0, bool small)
{
    __shared__ float red[4][128];
    __shared__ uint64_t tile[128 * 16];
    const int t = threadIdx.x, sub = t & 15, rg = t >> 4;
    const uint32_t tb = blockIdx.x / hb_n, hb = blockIdx.x - tb * hb_n;
    const int64_t c0 = (int64_t)hb * 128 + sub * 8;   // the lane's 8 channels
    const int64_t r0 = (int64_t)tb * 128 + rg * 8;    // ... and its 8 tokens
    bool ok[8];
    rows_valid8(r0, t_n, mmax, masked_m, m_indices, small, ok);
    float v[8][8];
    if (vec_in && (int64_t)hb * 128 + 128 <= h) {   // (uniform) all 128 channels inside: 8 predicated 16-byte loads in flight, then their use
        typename Elem<T>::Raw raw[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            raw[p] = typename Elem<T>::Raw{};
            if (ok[p]) raw[p] = Elem<T>::load8_raw(x, (r0 + p) * h + c0);
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) Elem<T>::unpack8(raw[p], v[p]);
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) load8_bounded<T>(x, (r0 + p) * h + c0, v[p], vec_in, c0, h, ok[p]);
    }
    if (ROWWISE) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            if (!ok[p]) continue;   // (uniform over the 16 lanes of the row)
            const int64_t row = r0 + p;
            float s;
            uint32_t w0, w1;
            quant_row_block(v[p], ue8m0, s, w0, w1);
            if (sub == 0) sf_row[row * hb_n + hb] = s;
            store_codes8(q_row + row * h + c0, w0, w1, vec_row, c0, h);
        }
    }
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

extern "C" int dga_cast_to_fp8_1x128_transposed(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                                const int32_t *masked_m, const int32_t *m_indices, void *qt, int64_t ldqt, float *sft,
                                                void *q_row, float *sf_row, int flags, void *stream)
{
    using namespace dga;
    const bool shape_ok = transposed_ldqt_ok(groups, rows, ldqt) && (q_row != nullptr) == (sf_row != nullptr);
    return run_fused(flags, x_dtype, groups, rows, h, 1, masked_m, m_indices, x && qt && sft, [&](auto tag, const FusedGeometry &g) -> int {
        using T = decltype(tag);
        const int64_t t_n = groups * rows, tb_n = (t_n + 127) / 128;
        if (tb_n * g.hb_n > 0x7FFFFFFFll) return DGA_E_RANGE;   // one workgroup per tile
        const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
        // a lane's 8 elements start 8 j elements into a row of h, its 8 codes 8 j bytes into a row of ldqt (qt) or of h (q_row)
        const bool vec_in = al(x, 16) && h % 8 == 0, vec_qt = al(qt, 8) && ldqt % 8 == 0, vec_row = al(q_row, 8) && h % 8 == 0;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tb_n * g.hb_n)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                               static_cast<uint8_t *>(qt), sft, static_cast<uint8_t *>(q_row), sf_row, t_n, h, static_cast<uint32_t>(g.hb_n),
                               tb_n, ldqt, rows, masked_m, m_indices, vec_in, vec_qt, vec_row, g.ue8m0, g.small);
        };
        if (q_row) launch(cast_1x128_transposed_kernel<T, true>);
        else launch(cast_1x128_transposed_kernel<T, false>);
        return record_hip(hipGetLastError());
    }, shape_ok);
}
