// The device text the sparse MLA attention units share (dga_sparse_mla.hip: the forward forms; dga_sparse_mla_bwd.hip: the backward): the
// geometry of a gathered tile and its LDS image, the vector types of the matrix instructions, and the bf16 row source.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"

namespace dga {

constexpr int SMLA_D = DGA_SPARSE_MLA_D_QK;                  // 576
constexpr int SMLA_DV = DGA_SPARSE_MLA_D_V;                  // 512
constexpr int SMLA_THREADS = 256;
constexpr int SMLA_TILE = 32;                                // positions of one gathered tile
constexpr int SMLA_ROW_BYTES = SMLA_D * 2 + 32;              // 1184: 296 dwords = 40 mod 64, both kinds of read are free of bank conflicts
constexpr int SMLA_CHUNKS = SMLA_D / 8;                      // 16-byte chunks of a row: 72
constexpr int SMLA_STAGE = SMLA_CHUNKS / 8;                  // chunks a thread gathers per tile: 9, of one row
constexpr int SMLA_KSTEPS = SMLA_D / 32;                     // 18
constexpr int SMLA_CTILES = SMLA_DV / 16;                    // 32
static_assert(SMLA_KSTEPS % 2 == 0 && SMLA_CTILES % 4 == 0 && SMLA_TILE * 8 == SMLA_THREADS && SMLA_CHUNKS == 8 * SMLA_STAGE && SMLA_D % 32 == 0 && SMLA_DV % 16 == 0, "the kernel's geometry");

typedef float smla_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 smla_v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 smla_v4bf __attribute__((ext_vector_type(4)));
typedef short smla_v4s __attribute__((ext_vector_type(4)));
typedef short smla_v8s __attribute__((ext_vector_type(8)));
typedef uint32_t smla_v4u __attribute__((ext_vector_type(4)));
typedef float smla_v2f __attribute__((ext_vector_type(2)));
typedef __bf16 smla_v2bf __attribute__((ext_vector_type(2)));

// What the kernel gathers from.  A cache says where thread gsub (of the eight a row has) starts in row r, what it loads from there
// (RAW uint4, all in flight together), and where chunk c of the nine it ends up with stands in the 1184-byte LDS row.
// bf16 rows: the nine chunks gsub + 8 c of the row as they are.
struct SmlaBf16Rows {
    static constexpr bool FP8 = false;
    static constexpr int RAW = SMLA_STAGE;
    const uint16_t *kv;
    int64_t kv_stride, s_rows;
    static __device__ __forceinline__ SmlaBf16Rows make(const void *kv, int64_t stride, int64_t s_rows, int, int)
    {
        return SmlaBf16Rows{static_cast<const uint16_t *>(kv), stride, s_rows};
    }
    __device__ __forceinline__ const unsigned char *at(int64_t r, int gsub) const
    {
        return reinterpret_cast<const unsigned char *>(kv + r * kv_stride + gsub * 8);
    }
    static __device__ __forceinline__ void load(const unsigned char *p, int gsub, uint4 (&v)[RAW])
    {
#pragma unroll
        for (int c = 0; c < RAW; ++c) v[c] = *reinterpret_cast<const uint4 *>(p + 128 * c);
    }
    static __device__ __forceinline__ int lds_at(int c, int gsub) { return gsub * 16 + 128 * c; }
};

// What the two backward units share (dga_sparse_mla_bwd.hip, dga_sparse_mla_bwd_det.hip): the geometry of a block of heads and its LDS
// images, and the reads of them.
constexpr int SMLB_HEADS = DGA_SPARSE_MLA_BWD_HEADS;         // heads of a workgroup: 32
constexpr int SMLB_DO_ROW_BYTES = SMLA_DV * 2 + 32;          // 1056
constexpr int SMLB_W_ROW_BYTES = SMLA_TILE * 2 + 16;         // 80: a head's 32 weights (p or dS) of the tile
constexpr int SMLB_DTILES = SMLA_D / 16;                     // column tiles of dq and dkv: 36
constexpr int SMLB_WAVE_TILES = SMLB_DTILES / 2;             // ... of one wave: 18
constexpr int SMLB_GROUP = 3;                                // column tiles whose LDS reads are in flight together
static_assert(SMLB_HEADS == SMLA_TILE && SMLB_WAVE_TILES % SMLB_GROUP == 0 && SMLB_HEADS * 8 == SMLA_THREADS && SMLA_DV % 64 == 0,
              "the backward's geometry");

typedef int32_t smlb_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float smlb_bf16(uint32_t bits) { return __uint_as_float(bits << 16); }
// the products of the eight bf16 pairs of two 16-byte chunks, added to `sum` in ascending order, nothing contracted
__device__ __forceinline__ float smlb_dot8(float sum, const uint4 &a, const uint4 &b)
{
#pragma clang fp contract(off)
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sum = sum + smlb_bf16(x[i] & 0xFFFFu) * smlb_bf16(y[i] & 0xFFFFu);
        sum = sum + smlb_bf16(x[i] >> 16) * smlb_bf16(y[i] >> 16);
    }
    return sum;
}
__device__ __forceinline__ uint32_t smlb_lds(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char *)p;
}
// one 16 x 32 (or 32 x 16) bf16 fragment by two transposed reads: the blocks at `addr` and sixteen image rows (`half` bytes) below it
__device__ __forceinline__ smla_v8bf smlb_read_tr(uint32_t addr, int half)
{
    const smla_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(addr));
    const smla_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(addr + half));
    return __builtin_bit_cast(smla_v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace dga
