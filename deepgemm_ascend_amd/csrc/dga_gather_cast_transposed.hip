// The dispatch of an MoE layer fused into the quantiser of the weight-gradient operands: the tokens of x [S, h] reach the experts through a
// slot -> pair table (dga_route_slots' `inverse`), and what the step needs of the gathered rows is their fp8 form, never the rows themselves.
//   dga_gather_cast_to_fp8_1x128_transposed   src [S, h] (fp32 / bf16 / fp16), index int64 [groups, rows] with values in [0, S * index_div),
//                                             optional row_scale fp32 [S * index_div], optional masked_m
//                                             -> dga_cast_to_fp8_1x128_transposed's outputs on xg[r] = src[index[r] / index_div]
//                                                (with row_scale: fl32(row_scale[index[r]] * src[index[r] / index_div])), byte for byte
// Row r is valid iff the mask does not exclude it and 0 <= index[r] < S * index_div; an index the mask excludes is not read (dga_route_slots
// leaves stale values there), an index out of range dereferences nothing.  One pass: 2 bytes in and 1 out per element (bf16) plus one 8-byte
// index per 256-byte row segment, where the row copy in front of dga_cast_to_fp8_1x128_transposed moves 4 more.  The tile is
// dga_cast_transposed.hip's, kept as this unit's own text (dga_silu_mul_cast_transposed.hip says why); the quantiser proper is
// dga_cast.hip's (dga_cast_device.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// cast_1x128_transposed_kernel's tile (128 tokens x 128 channels per workgroup, 16 lanes per row, row group rg holds the 8 consecutive
// tokens 8 rg .. 8 rg + 7; the channel maxima, the swizzled 16 KB code tile and the stores are described there) with the rows read
// through the table: the lane's 8 mask answers go out together (rows_valid8), then its 8 predicated index reads and -- SCALED -- its 8
// predicated scale reads (gather_rows8), then the 8 predicated 16-byte row loads, each at its own row of src.  The 16 lanes of a row read
// the same index, so they agree on the row's validity and on its address.
template <typename T, bool ROWWISE, bool SCALED>
__global__ void __launch_bounds__(256) gather_cast_1x128_transposed_kernel(const void *src, const int64_t *index, const float *row_scale,
                                                                           int64_t pairs, int64_t index_div, uint8_t *qt, float *sft,
                                                                           uint8_t *q_row, float *sf_row, int64_t t_n, int64_t h, uint32_t hb_n,
                                                                           int64_t tb_n, int64_t ldqt, int64_t mmax, const int32_t *masked_m,
                                                                           bool vec_in, bool vec_qt, bool vec_row, bool ue8m0, bool small,
                                                                           bool small_pairs)
{
    __shared__ float red[4][128];
    __shared__ uint64_t tile[128 * 16];
    const int t = threadIdx.x, sub = t & 15, rg = t >> 4;
    const uint32_t tb = blockIdx.x / hb_n, hb = blockIdx.x - tb * hb_n;
    const int64_t c0 = (int64_t)hb * 128 + sub * 8;   // the lane's 8 channels
    const int64_t r0 = (int64_t)tb * 128 + rg * 8;    // ... and its 8 tokens
    bool ok[8];
    rows_valid8(r0, t_n, mmax, masked_m, nullptr, small, ok);
    int64_t at[8];   // element index of the lane's 8 channels in the row of src that token p names
    float sc[8];
    gather_rows8<SCALED>(index, row_scale, r0, pairs, index_div, small_pairs, h, c0, ok, at, sc);
    float v[8][8];
    if (vec_in && (int64_t)hb * 128 + 128 <= h) {   // (uniform) all 128 channels inside: 8 predicated 16-byte loads in flight, then their use
        typename Elem<T>::Raw raw[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            raw[p] = typename Elem<T>::Raw{};
            if (ok[p]) raw[p] = Elem<T>::load8_raw(src, at[p]);
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) Elem<T>::unpack8(raw[p], v[p]);
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) load8_bounded<T>(src, at[p], v[p], vec_in, c0, h, ok[p]);
    }
    if (SCALED) {   // one multiplication per element, no special cases (an excluded row: +0 * +0)
#pragma unroll
        for (int p = 0; p < 8; ++p) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[p][j] = sc[p] * v[p][j];
        }
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

extern "C" int dga_gather_cast_to_fp8_1x128_transposed(const void *src, int src_dtype, int64_t src_rows, int64_t h, const int64_t *index,
                                                       int64_t index_div, const float *row_scale, int64_t groups, int64_t rows,
                                                       const int32_t *masked_m, void *qt, int64_t ldqt, float *sft, void *q_row,
                                                       float *sf_row, int flags, void *stream)
{
    using namespace dga;
    const bool pairs_ok = index_div >= 1 && src_rows >= 0 && src_rows <= 0x7FFFFFFFFFFFFFFFll / index_div;
    const bool shape_ok = pairs_ok && (groups == 1 || masked_m) && transposed_ldqt_ok(groups, rows, ldqt) &&
                          (q_row != nullptr) == (sf_row != nullptr);
    // (src may be null when it has no row: every index is out of range then)
    const bool have_ptrs = (src || src_rows == 0) && index && qt && sft;
    return run_fused(flags, src_dtype, groups, rows, h, 1, masked_m, nullptr, have_ptrs, [&](auto tag, const FusedGeometry &g) -> int {
        using T = decltype(tag);
        const int64_t t_n = groups * rows, tb_n = (t_n + 127) / 128;
        if (tb_n * g.hb_n > 0x7FFFFFFFll) return DGA_E_RANGE;   // one workgroup per tile
        if (h > 0x7FFFFFFFFFFFFFFFll / (src_rows > 0 ? src_rows : 1)) return DGA_E_RANGE;   // element indices of src stay inside int64
        const int64_t pairs = src_rows * index_div;
        const auto al = [](const void *p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; };
        // a lane's 8 elements start 8 j elements into a row of h, its 8 codes 8 j bytes into a row of ldqt (qt) or of h (q_row)
        const bool vec_in = al(src, 16) && h % 8 == 0, vec_qt = al(qt, 8) && ldqt % 8 == 0, vec_row = al(q_row, 8) && h % 8 == 0;
        const bool small_pairs = pairs <= 0xFFFFFFFFll;   // (a valid index is below pairs: the 32-bit division)
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tb_n * g.hb_n)), dim3(256), 0, static_cast<hipStream_t>(stream), src, index,
                               row_scale, pairs, index_div, static_cast<uint8_t *>(qt), sft, static_cast<uint8_t *>(q_row), sf_row, t_n, h,
                               static_cast<uint32_t>(g.hb_n), tb_n, ldqt, rows, masked_m, vec_in, vec_qt, vec_row, g.ue8m0, g.small,
                               small_pairs);
        };
        if (row_scale) {
            if (q_row) launch(gather_cast_1x128_transposed_kernel<T, true, true>);
            else launch(gather_cast_1x128_transposed_kernel<T, false, true>);
        } else {
            if (q_row) launch(gather_cast_1x128_transposed_kernel<T, true, false>);
            else launch(gather_cast_1x128_transposed_kernel<T, false, false>);
        }
        return record_hip(hipGetLastError());
    }, shape_ok);
}
