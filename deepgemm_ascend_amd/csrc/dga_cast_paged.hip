// The writer of the indexer's paged fp8 key cache (the operand of dga_fp8_paged_mqa_logits, dga_paged_mqa_logits.hip):
//   dga_cast_to_fp8_1x128_paged   x [tokens, 128] (fp32 / bf16 / fp16), slot_mapping int64 [tokens] -> kv_cache
// Block b of the cache is DGA_PAGED_MQA_LOGITS_BLOCK_BYTES = 8448 bytes at b * block_stride: the e4m3 codes of its 64 keys, key-major, then
// their 64 fp32 scales.  Token t with 0 <= slot_mapping[t] < 64 num_blocks goes to key slot % 64 of block slot / 64: its 128 codes to bytes
// 128 (slot % 64) .., its scale to bytes 8192 + 4 (slot % 64) .. -- dga_cast_to_fp8_1x128's codes and scale of row t, byte for byte: a key
// is one 1x128 block held by the 16 lanes of a DPP row, and the loads and quant_row_block are that kernel's (dga_cast_device.hpp).  Any
// other slot value (engines pad with -1) skips the token: its row of x is not read and nothing is dereferenced through it.  No other byte
// of the cache is touched.  Two tokens with the same valid slot are the caller's error: each byte is then one of the writers'.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

namespace dga {

constexpr int PAGED_KEYS = DGA_PAGED_MQA_LOGITS_BLOCK_KV;
constexpr int PAGED_SCALES = PAGED_KEYS * 128;     // byte offset of a block's scales
static_assert(PAGED_SCALES + 4 * PAGED_KEYS == DGA_PAGED_MQA_LOGITS_BLOCK_BYTES && DGA_MQA_LOGITS_HEAD_DIM == 128, "the layout of a block");

// 16 lanes share one token, 8 consecutive elements per lane (cast_1x128_kernel's geometry at k = 128)
template <typename T>
__global__ void __launch_bounds__(256) cast_1x128_paged_kernel(const void *x, uint8_t *kv, const int64_t *slot_mapping, int64_t tokens,
                                                               int64_t slots, int64_t block_stride, bool ue8m0)
{
    const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (t >= tokens) return;                                  // whole 16-lane groups leave together, here and below
    const int64_t slot = slot_mapping[t];
    if ((uint64_t)slot >= (uint64_t)slots) return;
    const int sub = threadIdx.x & 15;
    float v[8];
    Elem<T>::load8(x, t * 128 + sub * 8, v);
    float s;
    uint32_t w0, w1;
    quant_row_block(v, ue8m0, s, w0, w1);
    const int key = (int)(slot % PAGED_KEYS);
    uint8_t *b = kv + slot / PAGED_KEYS * block_stride;
    if (sub == 0) *(float *)(b + PAGED_SCALES + 4 * key) = s;
    *(v2i_c *)(b + 128 * key + 8 * sub) = v2i_c{(int)w0, (int)w1};
}

}  // namespace dga

extern "C" int dga_cast_to_fp8_1x128_paged(const void *x, int x_dtype, int64_t tokens, void *kv_cache, int64_t num_blocks, int64_t block_stride,
                                           const int64_t *slot_mapping, int flags, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (tokens < 0 || num_blocks < 1 || block_stride < DGA_PAGED_MQA_LOGITS_BLOCK_BYTES) return DGA_E_SHAPE;
    if (tokens == 0) return DGA_OK;
    if (!x || !kv_cache || !slot_mapping) return DGA_E_NULL;
    return dispatch_dtype(x_dtype, [&](auto tag) -> int {
        // a lane reads 16 (fp32: twice 16) bytes and stores 8; a block's codes and scales sit at multiples of 8 and 4 from its start
        if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(kv_cache) % 16 || block_stride % 16 ||
            reinterpret_cast<uintptr_t>(slot_mapping) % 8)
            return DGA_E_ALIGN;
        if (num_blocks > 0x7FFFFFFFFFFFFFFFll / block_stride) return DGA_E_RANGE;   // (block_stride >= 8448: 64 num_blocks fits as well)
        unsigned grid;
        if (int rc = grid_of_blocks(tokens, 1, grid)) return rc;
        hipLaunchKernelGGL(cast_1x128_paged_kernel<decltype(tag)>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                           static_cast<uint8_t *>(kv_cache), slot_mapping, tokens, num_blocks * PAGED_KEYS, block_stride,
                           (flags & DGA_CAST_UE8M0) != 0);
        return record_hip(hipGetLastError());
    });
}
