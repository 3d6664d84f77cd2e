// The quantiser of grouped expert weights: fprop takes each expert's W [N, K] quantised 128x128, dgrad takes W^T [K, N] quantised 128x128, and
// a 128x128 block's amax does not change under transposition -- cast_to_fp8_128x128(W^T) is cast_to_fp8_128x128(W) with codes and scales
// transposed, bit for bit.
//   dga_cast_to_fp8_128x128_transposed   w [groups, n, k] (fp32 / bf16 / fp16)
//                                        -> qt [groups, k, n], sft [groups, ceil(k/128), ceil(n/128)]: per group byte for byte
//                                           dga_cast_to_fp8_128x128_ex on w[g]^T; optionally (q_row [groups, n, k], sf_row [groups,
//                                           ceil(n/128), ceil(k/128)]) = dga_cast_to_fp8_128x128_ex(w[g]) from the same read
// One pass: 2 (4) bytes in and 1 out per element, 1 more with the row-wise output; quantise, transpose, quantise moves 10 (18), per expert and
// in three launches each.  No scale block mixes two groups, whatever n is.  The quantiser proper is dga_cast.hip's (dga_cast_device.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

// One workgroup per tile of 128 rows x 128 columns of one group; workgroups that follow each other walk along k (whole rows of w are read
// side by side), then along n, then over the groups.  cast_1x128_transposed_kernel's register shape: 16 lanes share a row, 8 consecutive
// columns per lane (256 contiguous bytes of bf16 per row), and row group rg = t / 16 holds the 8 CONSECUTIVE rows 8 rg .. 8 rg + 7, one per
// pass: 64 fp32 values per lane, and the 8 codes of one column in a lane are 8 neighbouring bytes of qt.  From those 64 values on -- the
// tile maximum, the scale, the row-wise and the transposed codes -- the text is quant_block_tile_transposed's (dga_cast_device.hpp), which
// dga_adamw_cast.hip calls too.
// Rows at and beyond n and columns at and beyond k are zeros that are never loaded, and their codes are never stored.
template <typename T, bool ROWWISE>
__global__ void __launch_bounds__(256) cast_128x128_transposed_kernel(const void *w, uint8_t *qt, float *sft, uint8_t *q_row, float *sf_row,
                                                                      int64_t n, int64_t k, uint32_t nb_n, uint32_t kb_n, bool vec_in,
                                                                      bool vec_qt, bool vec_row, bool ue8m0)
{
    // block_tile_at's text, written out: through the helper the same arithmetic allocates 86 VGPRs instead of 77 in the builds without the
    // row-wise output (5 waves per SIMD instead of 6) and 110 instead of 108 in the fp32 row-wise one
    const int t = threadIdx.x, sub = t & 15, rg = t >> 4;
    const uint32_t per_group = nb_n * kb_n;   // (the grid, groups * per_group, fits 31 bits)
    const uint32_t g = blockIdx.x / per_group, in_g = blockIdx.x - g * per_group;
    const uint32_t nb = in_g / kb_n, kb = in_g - nb * kb_n;
    const int64_t c0 = (int64_t)kb * 128 + sub * 8;   // the lane's 8 columns
    const int64_t r0 = (int64_t)nb * 128 + rg * 8;    // ... and its 8 rows
    const int64_t g0 = (int64_t)g * n * k;            // the group's first element, in w and q_row (row-major [n, k]) and in qt ([k, n])
    const BlockTileAt at{g, nb, kb, c0, r0, g0};
    bool ok[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) ok[p] = r0 + p < n;
    float v[8][8];
    if (vec_in && (int64_t)kb * 128 + 128 <= k) {   // (uniform) all 128 columns inside: 8 predicated 16-byte loads in flight, then their use
        typename Elem<T>::Raw raw[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            raw[p] = typename Elem<T>::Raw{};
            if (ok[p]) raw[p] = Elem<T>::load8_raw(w, g0 + (r0 + p) * k + c0);
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) Elem<T>::unpack8(raw[p], v[p]);
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) load8_bounded<T>(w, g0 + (r0 + p) * k + c0, v[p], vec_in, c0, k, ok[p]);
    }
    quant_block_tile_transposed<ROWWISE>(v, ok, at, t, qt, sft, q_row, sf_row, n, k, nb_n, kb_n, vec_qt, vec_row, ue8m0);
}

}  // namespace dga

extern "C" int dga_cast_to_fp8_128x128_transposed(const void *w, int w_dtype, int64_t groups, int64_t n, int64_t k, void *qt, float *sft,
                                                  void *q_row, float *sf_row, int flags, void *stream)
{
    using namespace dga;
    // run_cast's order: flags, shape, nothing to do, pointers, dtype, the grid
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (groups < 0 || n < 0 || k < 0 || (q_row != nullptr) != (sf_row != nullptr)) return DGA_E_SHAPE;
    if (groups == 0 || n == 0 || k == 0) return DGA_OK;
    if (!w || !qt || !sft) return DGA_E_NULL;
    return dispatch_dtype(w_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        // one workgroup per tile, decided without a product or a sum that overflows
        const int64_t nb_n = n / 128 + (n % 128 != 0), kb_n = k / 128 + (k % 128 != 0);
        if (nb_n > 0x7FFFFFFFll / kb_n || groups > 0x7FFFFFFFll / (nb_n * kb_n)) return DGA_E_RANGE;
        const auto al = [](const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; };
        // a lane's 8 elements start g n k + r k + 8 j elements into w and q_row, its 8 transposed codes g n k + c n + 8 j bytes into qt:
        // with k % 8 == 0 (n % 8 == 0) every group starts on a multiple of 8 too
        const bool vec_in = al(w, 16) && k % 8 == 0, vec_qt = al(qt, 8) && n % 8 == 0, vec_row = al(q_row, 8) && k % 8 == 0;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(groups * nb_n * kb_n)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                               static_cast<uint8_t *>(qt), sft, static_cast<uint8_t *>(q_row), sf_row, n, k, static_cast<uint32_t>(nb_n),
                               static_cast<uint32_t>(kb_n), vec_in, vec_qt, vec_row, (flags & DGA_CAST_UE8M0) != 0);
        };
        if (q_row) launch(cast_128x128_transposed_kernel<T, true>);
        else launch(cast_128x128_transposed_kernel<T, false>);
        return record_hip(hipGetLastError());
    });
}
