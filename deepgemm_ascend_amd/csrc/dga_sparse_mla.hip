// What the lightning indexer selects for: sparse MLA attention (DeepSeek sparse attention, forward) over dga_indexer_topk's indices.
//   dga_sparse_mla_fwd   q bf16 [m, heads, 576], kv bf16 [s, 576] (rows kv_stride elements apart), indices int32 [m, topk] (rows
//                        idx_stride apart), offsets int32 [m] or null -> out bf16 [m, heads, 512], lse fp32 [m, heads]
//     row of position j     r_j = indices[t, j] + (offsets ? offsets[t] : 0), valid iff indices[t, j] >= 0 and 0 <= r_j < s
//     s_j                   sm_scale sum_d q[t, h, d] kv[r_j, d] over the valid positions;  lse = ln sum_j exp(s_j)
//     out[t, h, :]          sum_j exp(s_j - lse) kv[r_j, :512];  no valid position: out = +0, lse = -inf
// One workgroup of four waves owns one token and a block of up to 64 heads; wave w owns heads 16 w .. 16 w + 15 of the block and all 512
// value columns of them (128 fp32 accumulators a lane).  The block's slice of q goes to LDS once (64 rows of 1184 bytes).  The selected
// rows are gathered in tiles of 32 positions by 16-byte loads (eight threads a row) into registers while the tile before is computed on,
// and written to one LDS image of 1184-byte rows after it (invalid positions as zeros; the row, once gathered, serves every head of the
// block as key and as value).  The accumulators and the staged tile leave no room for q in registers beside LDS reads in flight, and with
// one wave a SIMD a read that is not in flight ahead of its MFMA costs its whole latency.  Per tile and wave:
//   S^T = K Q^T   two 16-key subtiles, each 18 chained v_mfma_f32_16x16x32_bf16 over d ascending from +0 (K and Q by ds_read_b128, Q the B operand):
//                 lane l holds head l & 15 of the wave and the keys 4 (l >> 4) + i and 16 + 4 (l >> 4) + i, i = 0 .. 3
//   x = S (sm_scale log2 e), -inf at invalid positions;  m' = max(m, max over the tile) (two lane exchanges);  m* = m' or 0 when m' = -inf;
//   alpha = exp2(m - m*);  p = exp2(x - m*);  l = l alpha + (the lane's eight p, fp32, unrounded, ascending key);  O = O alpha (skipped while
//   no lane of the wave has alpha != 1)
//   O^T += V^T P^T  32 column tiles, one v_mfma_f32_16x16x32_bf16 each: P rounded to bf16 (RNE) in the registers S left it in -- the
//                 product's k index runs over the lane's eight keys, and V's fragment is read to match by two ds_read_b64_tr_b16 of the
//                 blocks [keys 4 g .. 4 g + 3] and [keys 16 + 4 g ..] x [16 columns]
// and at the end l is summed over the four lane groups ((l_0 + l_1) + (l_2 + l_3)), out = O (1 / l) rounded to bf16, lse = ln 2 (m + log2 l).
// m* = 0 for a tile without a valid position while m is still -inf keeps -inf - -inf out of the exponent: alpha = exp2(-inf) = 0 on O = 0.
// A head's state lives in the 4 lanes l & 15 == h of one wave, every output has one writer, nothing is atomic: two runs give the same bits.
// Nothing is dereferenced for an invalid position, no kv row outside the list and no column >= 576 is read.
// Workgroup w of the grid takes the logical block (w % 8) chunk + w / 8, chunk = ceil(blocks / 8): workgroups go to the eight XCDs in
// turn, so consecutive tokens -- which select largely the same rows -- share one XCD's L2 (DGA_SPARSE_MLA_LINEAR_GRID turns it off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"

#pragma clang fp contract(off)

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

__global__ void __launch_bounds__(SMLA_THREADS) sparse_mla_fwd_kernel(const uint16_t *__restrict__ q, const uint16_t *__restrict__ kv,
                                                                      int64_t kv_stride, int64_t s_rows, const int32_t *__restrict__ indices,
                                                                      int64_t idx_stride, int topk, const int32_t *__restrict__ offsets,
                                                                      int heads, int head_blocks, int64_t blocks, int64_t chunk, float scale2,
                                                                      uint16_t *__restrict__ out, float *__restrict__ lse)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[SMLA_TILE * SMLA_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[64 * SMLA_ROW_BYTES];   // the block's q, one row a head
    __shared__ __attribute__((aligned(16))) int32_t live[SMLA_TILE];                      // 1 where the tile's position is valid
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the logical block of this workgroup (see the head of the file); chunk == 0: the grid is taken as it is
    int64_t block = blockIdx.x;
    if (chunk) block = (block & 7) * chunk + (block >> 3);
    if (block >= blocks) return;                             // (the whole workgroup alike, before any barrier)
    const int64_t t = block / head_blocks;
    const int h0 = (int)(block % head_blocks) * 64 + wave * 16;
    const bool computes = h0 < heads;                        // (a wave beyond the last head tile only gathers)

    const int32_t *irow = indices + t * idx_stride;
    const int64_t shift = offsets ? (int64_t)offsets[t] : 0;
    const int tiles = (topk + SMLA_TILE - 1) / SMLA_TILE;

    // The gather: eight threads a position (position tid / 8 of the tile), thread tid % 8 of them the 16-byte chunks tid % 8 + 8 c,
    // c = 0 .. 8, of the row -- 128 contiguous bytes of a row per eight lanes and step.  A position's index is read one tile ahead of its
    // row (ask: from a position clamped into the list, so that the load needs no branch and nothing waits for it) and turned into the
    // row's address, null for an invalid position, when the row is asked for (row_of).
    const int gpos = tid >> 3, gsub = tid & 7;
    auto ask = [&](int tl) -> int32_t {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        return irow[pos < topk ? pos : topk - 1];
    };
    auto row_of = [&](int tl, int32_t i) -> const uint16_t * {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        const int64_t r = (int64_t)i + shift;
        return (pos < topk && i >= 0 && r >= 0 && r < s_rows) ? kv + r * kv_stride + gsub * 8 : nullptr;
    };
    auto fetch = [&](const uint16_t *row, uint4 (&v)[SMLA_STAGE]) {
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) v[c] = uint4{0, 0, 0, 0};
        if (row) {
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(row + 64 * c);
        }
    };

    uint4 staged[SMLA_STAGE];
    const uint16_t *row = row_of(0, ask(0));
    fetch(row, staged);
    int32_t asked = ask(1);

    // the block's slice of q goes to LDS once, in the tile's row format (the first barrier of the loop stands between this and its use):
    // eight threads a head, 32 heads a pass
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int hb = pass * 32 + gpos, head = (int)(block % head_blocks) * 64 + hb;
        if (head < heads) {
            const uint16_t *qrow = q + ((t * heads + head) * SMLA_D + gsub * 8);
            uint4 v[SMLA_STAGE];
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + hb * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
        }
    }

    smla_v4f acc[SMLA_CTILES];
#pragma unroll
    for (int ct = 0; ct < SMLA_CTILES; ++ct) acc[ct] = smla_v4f{0.f, 0.f, 0.f, 0.f};
    float mx = -__builtin_inff(), sum = 0.f;                 // the running maximum (log2 domain) of head hl, the lane's share of l

    // LDS addresses of the lane's reads: K rows hl and 16 + hl at bytes 64 s + 16 g; V blocks by ds_read_b64_tr_b16 (lane 4 q + p of
    // a group gives row q, columns 4 p .. of the block)
    const uint32_t tile_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)tile;
    const uint32_t k_addr = tile_base + hl * SMLA_ROW_BYTES + 16 * g;
    const uint32_t v_addr = tile_base + (4 * g + (hl >> 2)) * SMLA_ROW_BYTES + 8 * (hl & 3);
    const uint32_t q_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)qimg + (wave * 16 + hl) * SMLA_ROW_BYTES + 16 * g;

#pragma unroll 1
    for (int tl = 0; tl < tiles; ++tl) {
        // the staged tile goes to LDS
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(tile + gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = staged[c];
        if (gsub == 0) live[gpos] = row != nullptr;
        __syncthreads();
        // the next tile's rows are asked for now and written after this tile's products; the indices of the one after it behind them
        row = row_of(tl + 1, asked);
        fetch(row, staged);
        asked = ask(tl + 2);

        if (computes) {
            // One wave a SIMD: nobody else hides an LDS read's latency, so the reads run one group ahead of the MFMAs that consume
            // them, in the order written here (the scheduling barriers keep it): two d steps a group for S, four column tiles for O.
            const smla_v4u lv0 = *reinterpret_cast<const smla_v4u *>(&live[4 * g]), lv1 = *reinterpret_cast<const smla_v4u *>(&live[16 + 4 * g]);
            smla_v4f s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
            smla_v4u ka[2][2], kb[2][2], qq[2][2];
            auto read_k = [&](int grp) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int s = 2 * grp + j;
                    ka[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(k_addr + 64 * s);
                    kb[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(k_addr + 16 * SMLA_ROW_BYTES + 64 * s);
                    qq[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(q_addr + 64 * s);
                }
            };
            smla_v4s vlo[2][4], vhi[2][4];
            auto read_v = [&](int grp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ct = 4 * grp + j;
                    vlo[grp & 1][j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(v_addr + 32 * ct));
                    vhi[grp & 1][j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(v_addr + 16 * SMLA_ROW_BYTES + 32 * ct));
                }
            };
            read_k(0);
#pragma unroll
            for (int grp = 0; grp < SMLA_KSTEPS / 2; ++grp) {
                if (grp + 1 < SMLA_KSTEPS / 2) read_k(grp + 1);
                else read_v(0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka[grp & 1][j]),
                                                                 __builtin_bit_cast(smla_v8bf, qq[grp & 1][j]), s0, 0, 0, 0);
                    s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, kb[grp & 1][j]),
                                                                 __builtin_bit_cast(smla_v8bf, qq[grp & 1][j]), s1, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            float x[8];
            float tmax = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float sv = i < 4 ? s0[i] : s1[i - 4];
                x[i] = (i < 4 ? lv0[i] : lv1[i - 4]) ? sv * scale2 : -__builtin_inff();
                tmax = __builtin_fmaxf(tmax, x[i]);          // (a NaN score is passed over here and reaches the result through p)
            }
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = __builtin_fmaxf(mx, tmax);
            const float muse = mnew == -__builtin_inff() ? 0.f : mnew;
            const float alpha = __builtin_amdgcn_exp2f(mx - muse);
            mx = mnew;
            float p[8];
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                p[i] = __builtin_amdgcn_exp2f(x[i] - muse);
                psum = psum + p[i];
            }
            sum = sum * alpha + psum;
            if (__ballot(alpha != 1.0f) != 0) {
#pragma unroll
                for (int ct = 0; ct < SMLA_CTILES; ++ct) acc[ct] = acc[ct] * alpha;
            }
            smla_v8bf pf;
#pragma unroll
            for (int i = 0; i < 8; ++i) pf[i] = (__bf16)p[i];
#pragma unroll
            for (int grp = 0; grp < SMLA_CTILES / 4; ++grp) {
                if (grp + 1 < SMLA_CTILES / 4) read_v(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const smla_v8s vf = __builtin_shufflevector(vlo[grp & 1][j], vhi[grp & 1][j], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[4 * grp + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, vf), pf, acc[4 * grp + j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }

    if (!computes) return;
    // l over the four lane groups that share a head: (l_0 + l_1) + (l_2 + l_3) in every one of them
    sum = sum + __shfl_xor(sum, 16, 64);
    sum = sum + __shfl_xor(sum, 32, 64);
    const bool empty = sum == 0.f;                           // no valid position (a NaN is not equal to 0 and goes through)
    const float inv = empty ? 0.f : 1.0f / sum;
    uint16_t *orow = out + ((t * heads + h0 + hl) * SMLA_DV + 4 * g);
#pragma unroll
    for (int ct = 0; ct < SMLA_CTILES; ++ct) {
        smla_v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)(empty ? 0.f : acc[ct][i] * inv);
        *reinterpret_cast<uint2 *>(orow + 16 * ct) = __builtin_bit_cast(uint2, o);
    }
    if (g == 0) lse[t * heads + h0 + hl] = empty ? -__builtin_inff() : (mx + __builtin_amdgcn_logf(sum)) * 0.693147180559945309f;
}

}  // namespace dga

extern "C" int dga_sparse_mla_fwd(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                  int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, void *out,
                                  float *lse, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_SPARSE_MLA_LINEAR_GRID) return DGA_E_RANGE;
    if (m < 0 || heads < 16 || heads > DGA_SPARSE_MLA_MAX_HEADS || heads % 16 || s < 1 || topk < 1 || kv_stride < SMLA_D || idx_stride < topk)
        return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !kv || !indices || !out || !lse) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(kv) % 16 || reinterpret_cast<uintptr_t>(out) % 16 ||
        reinterpret_cast<uintptr_t>(indices) % 4 || reinterpret_cast<uintptr_t>(index_offsets) % 4 || reinterpret_cast<uintptr_t>(lse) % 4 ||
        kv_stride % 8)
        return DGA_E_ALIGN;
    const int head_blocks = (heads + 63) / 64;
    if (s > 0x7FFFFFFFll || topk > 0x7FFFFFFFll - DGA_SPARSE_MLA_TILE || m > (0x7FFFFFFFll - 8) / head_blocks) return DGA_E_RANGE;
    if (kv_stride > 0x7FFFFFFFFFFFFFFFll / 2 / s || idx_stride > 0x7FFFFFFFFFFFFFFFll / 4 / m) return DGA_E_RANGE;
    const int64_t blocks = m * head_blocks;
    const bool linear = (flags & DGA_SPARSE_MLA_LINEAR_GRID) != 0;
    const int64_t chunk = linear ? 0 : (blocks + 7) / 8;
    const int64_t grid = linear ? blocks : chunk * 8;
    hipLaunchKernelGGL(sparse_mla_fwd_kernel, dim3(static_cast<unsigned>(grid)), dim3(SMLA_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(q), static_cast<const uint16_t *>(kv), kv_stride, s, indices, idx_stride,
                       static_cast<int>(topk), index_offsets, heads, head_blocks, blocks, chunk, static_cast<float>(sm_scale * 1.4426950408889634),
                       static_cast<uint16_t *>(out), lse);
    return record_hip(hipGetLastError());
}
