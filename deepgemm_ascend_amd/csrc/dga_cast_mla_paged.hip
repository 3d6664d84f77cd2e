// The writer of sparse MLA's paged fp8 latent cache (the operand of dga_sparse_mla_fwd_fp8, dga_sparse_mla.hip):
//   dga_cast_mla_kv_to_fp8_paged   kv_c [tokens, 512], k_pe [tokens, 64] (fp32 / bf16 / fp16, one dtype), slot_mapping int64 [tokens] -> kv_cache
// A row of the cache is DGA_SPARSE_MLA_FP8_ROW_BYTES = 656 bytes: 512 e4m3fn codes, 4 fp32 scales (one per 128 codes), 64 bf16 rope values;
// row r lives at (r / page_size) block_stride + (r % page_size) 656.  Token t with 0 <= slot_mapping[t] < num_blocks page_size goes to row
// slot: the codes and scales are dga_cast_to_fp8_1x128's of kv_c's row t, byte for byte -- a wave takes a token, each of its four DPP rows
// one 1x128 block, and the loads and quant_row_block are that kernel's (dga_cast_device.hpp) -- and the rope part is RNE_bf16(k_pe[t]),
// eight lanes of the wave 8 values each (bf16 input: the 16 bytes as they are, whatever they hold).  Any other slot value (engines pad
// with -1) skips the token: its rows are not read and nothing is dereferenced through it.  No other byte of the cache is touched.  Two
// tokens with the same valid slot are the caller's error: each byte is then one of the writers'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

constexpr int MLA_ROW = DGA_SPARSE_MLA_FP8_ROW_BYTES;
constexpr int MLA_LATENT = DGA_SPARSE_MLA_D_V;                       // 512 codes, then their scales
constexpr int MLA_ROPE = DGA_SPARSE_MLA_D_QK - DGA_SPARSE_MLA_D_V;  // 64
constexpr int MLA_ROPE_AT = MLA_LATENT + 4 * (MLA_LATENT / 128);    // 528
static_assert(MLA_ROPE_AT + 2 * MLA_ROPE == MLA_ROW && MLA_LATENT == 4 * 128 && MLA_ROPE == 8 * 8, "the layout of a row: four blocks a wave, eight rope lanes");

// 64 lanes share one token: lane l holds elements 8 (l & 15) .. of 1x128 block l >> 4, and lanes 0 .. 7 the rope values 8 l ..
template <typename T>
__global__ void __launch_bounds__(256) cast_mla_kv_paged_kernel(const void *kv_c, int64_t ld_c, const void *k_pe, int64_t ld_pe, uint8_t *kv,
                                                                const int64_t *slot_mapping, int64_t tokens, int64_t slots, int64_t page_size,
                                                                int64_t block_stride, bool ue8m0)
{
    const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (t >= tokens) return;                                  // whole waves leave together, here and below
    const int64_t slot = slot_mapping[t];
    if ((uint64_t)slot >= (uint64_t)slots) return;
    const int lane = threadIdx.x & 63, blk = lane >> 4, sub = lane & 15;
    const int64_t page = slot / page_size;
    uint8_t *row = kv + page * block_stride + (slot - page * page_size) * MLA_ROW;
    float v[8];
    Elem<T>::load8(kv_c, t * ld_c + blk * 128 + sub * 8, v);
    if (lane < MLA_ROPE / 8) {
        if constexpr (std::is_same<T, Bf16Tag>::value) {
            *(v4i_c *)(row + MLA_ROPE_AT + 16 * lane) = Elem<T>::load8_raw(k_pe, t * ld_pe + lane * 8);
        } else {
            float r[8];
            Elem<T>::load8(k_pe, t * ld_pe + lane * 8, r);
            Store8<Bf16Tag>::run(row + MLA_ROPE_AT, lane * 8, r, true);
        }
    }
    float s;
    uint32_t w0, w1;
    quant_row_block(v, ue8m0, s, w0, w1);
    if (sub == 0) *(float *)(row + MLA_LATENT + 4 * blk) = s;
    *(v2i_c *)(row + 128 * blk + 8 * sub) = v2i_c{(int)w0, (int)w1};
}

}  // namespace dga

extern "C" int dga_cast_mla_kv_to_fp8_paged(const void *kv_c, int64_t ld_c, const void *k_pe, int64_t ld_pe, int x_dtype, int64_t tokens,
                                            void *kv_cache, int64_t num_blocks, int64_t page_size, int64_t block_stride,
                                            const int64_t *slot_mapping, int flags, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    // (block_stride / 656 < page_size says block_stride < 656 page_size without the product)
    if (tokens < 0 || num_blocks < 1 || page_size < 1 || block_stride / MLA_ROW < page_size || ld_c < MLA_LATENT || ld_pe < MLA_ROPE)
        return DGA_E_SHAPE;
    if (tokens == 0) return DGA_OK;
    if (!kv_c || !k_pe || !kv_cache || !slot_mapping) return DGA_E_NULL;
    return dispatch_dtype(x_dtype, [&](auto tag) -> int {
        // a lane reads 16 (fp32: twice 16) bytes and stores 8 or 16; a row's codes, scales and rope part sit at multiples of 16 from its start
        constexpr int64_t bytes = Elem<decltype(tag)>::kBytes;
        if (reinterpret_cast<uintptr_t>(kv_c) % 16 || reinterpret_cast<uintptr_t>(k_pe) % 16 || ld_c % (16 / bytes) || ld_pe % (16 / bytes) ||
            reinterpret_cast<uintptr_t>(kv_cache) % 16 || block_stride % 16 || reinterpret_cast<uintptr_t>(slot_mapping) % 8)
            return DGA_E_ALIGN;
        if (num_blocks > 0x7FFFFFFFll / page_size || block_stride > 0x7FFFFFFFFFFFFFFFll / num_blocks ||
            ld_c > 0x7FFFFFFFFFFFFFFFll / bytes / tokens || ld_pe > 0x7FFFFFFFFFFFFFFFll / bytes / tokens)
            return DGA_E_RANGE;
        unsigned grid;
        if (int rc = grid_of_blocks(tokens, 4, grid)) return rc;
        hipLaunchKernelGGL(cast_mla_kv_paged_kernel<decltype(tag)>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), kv_c, ld_c, k_pe,
                           ld_pe, static_cast<uint8_t *>(kv_cache), slot_mapping, tokens, num_blocks * page_size, page_size, block_stride,
                           (flags & DGA_CAST_UE8M0) != 0);
        return record_hip(hipGetLastError());
    });
}
