// dga_sparse_mla_bwd with a deterministic dkv and no floating-point atomic (dga_sparse_mla_bwd.hip is the atomic path and holds the
// formulas).  dq comes from that unit's kernel without its phase C (launch_sparse_mla_bwd(.., false)): the atomic path's bytes.  dkv, per
// chunk of C consecutive tokens (include/dga_hip.h has the rule for C and the order of summation):
//   row inverse  five small kernels that know nothing of attention: per kv row the list of the chunk's valid positions that name it, as
//                pair ids (m - m0) topk + j in ascending order.  clear count; count by int32 atomic adds (order-free); exclusive scan to
//                start (one workgroup); fill through an int32 cursor -- the order inside a row's segment races --; then every pair finds
//                its rank by counting the smaller ids of its segment and writes itself there: exact for every input, quadratic in the
//                length of a segment (an indexer's list names a row at most once a token: <= C entries)
//   dkv pass     one workgroup of four waves owns one token and ONE gathered tile of 32 positions, resident in LDS for the whole
//                workgroup, and loops over the token's head blocks of 32: per block the atomic kernel's prologue (q and d_out images,
//                delta, lse L2E: L2 hits, a token's workgroups run together) and its phase A (S^T, dP^T, p, dS into the bf16 images), then
//                phase C into 72 fp32 accumulators a lane HELD ACROSS the head blocks: dS^T Q, then P^T dO for columns < 512.  At the end
//                one plain store of T[m, j, :] per valid position into the staging buffer [C, topk, 576]; a tile without a valid
//                position leaves before the loop and an invalid position stores nothing.  LDS as the atomic kernel's: 115 072 B.
//   reduce       one workgroup of 144 threads a kv row, a float4 of columns a thread: walks the row's ordered segment four 2304-byte
//                rows in flight, adds them in order from +0, then stores fl32(dkv + acc) once, honouring dkv_stride
// Every output element has one writer and a fixed order of summation: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

// ---- the row inverse ----
// The lists of a chunk: pair = (token - m0) topk + j, `pairs` of them; the validity rule is the attention's (index >= 0, row in [0, s))
struct RowLists {
    const int32_t *indices, *offsets;
    int64_t idx_stride, s_rows, m0, pairs;
    int topk;
};
constexpr int ROWINV_THREADS = 256, ROWINV_SCAN_THREADS = 1024;

__device__ __forceinline__ int32_t rowinv_row(const RowLists &l, int64_t pair)
{
    const int64_t t = l.m0 + pair / l.topk;
    const int32_t i = l.indices[t * l.idx_stride + pair % l.topk];
    const int64_t r = (int64_t)i + (l.offsets ? (int64_t)l.offsets[t] : 0);
    return (i >= 0 && r >= 0 && r < l.s_rows) ? (int32_t)r : -1;
}

__global__ void __launch_bounds__(ROWINV_THREADS) rowinv_clear_kernel(int32_t *__restrict__ count, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * ROWINV_THREADS + threadIdx.x;
    if (i < n) count[i] = 0;
}

__global__ void __launch_bounds__(ROWINV_THREADS) rowinv_count_kernel(RowLists l, int32_t *__restrict__ count)
{
    const int64_t pair = (int64_t)blockIdx.x * ROWINV_THREADS + threadIdx.x;
    if (pair >= l.pairs) return;
    const int32_t r = rowinv_row(l, pair);
    if (r >= 0) atomicAdd(&count[r], 1);
}

// start[i] = cursor[i] = count[0] + .. + count[i - 1], i < n: thread t sums its slab, the slabs' sums are scanned in LDS
__global__ void __launch_bounds__(ROWINV_SCAN_THREADS) rowinv_scan_kernel(const int32_t *__restrict__ count, int32_t *__restrict__ start,
                                                                          int32_t *__restrict__ cursor, int64_t n)
{
    __shared__ int32_t part[ROWINV_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (n + ROWINV_SCAN_THREADS - 1) / ROWINV_SCAN_THREADS;
    const int64_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    int32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += count[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < ROWINV_SCAN_THREADS; d <<= 1) {
        const int32_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int32_t base = part[tid] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        start[i] = base;
        cursor[i] = base;
        base += count[i];
    }
}

__global__ void __launch_bounds__(ROWINV_THREADS) rowinv_fill_kernel(RowLists l, int32_t *__restrict__ cursor, int32_t *__restrict__ list)
{
    const int64_t pair = (int64_t)blockIdx.x * ROWINV_THREADS + threadIdx.x;
    if (pair >= l.pairs) return;
    const int32_t r = rowinv_row(l, pair);
    if (r >= 0) list[atomicAdd(&cursor[r], 1)] = (int32_t)pair;
}

// a pair's place in its row's segment is the number of smaller ids there (the ids of a segment are distinct)
__global__ void __launch_bounds__(ROWINV_THREADS) rowinv_order_kernel(RowLists l, const int32_t *__restrict__ start,
                                                                      const int32_t *__restrict__ count, const int32_t *__restrict__ list,
                                                                      int32_t *__restrict__ ordered)
{
    const int64_t pair = (int64_t)blockIdx.x * ROWINV_THREADS + threadIdx.x;
    if (pair >= l.pairs) return;
    const int32_t r = rowinv_row(l, pair);
    if (r < 0) return;
    const int32_t *seg = list + start[r];
    const int32_t n = count[r], id = (int32_t)pair;
    int32_t rank = 0;
    for (int32_t k = 0; k < n; ++k) rank += seg[k] < id ? 1 : 0;
    ordered[start[r] + rank] = id;
}

// ---- the dkv pass ----
__global__ void __launch_bounds__(SMLA_THREADS) sparse_mla_bwd_dkv_kernel(const uint16_t *__restrict__ q, const void *__restrict__ kv,
                                                                          int64_t kv_stride, int64_t s_rows, const int32_t *__restrict__ indices,
                                                                          int64_t idx_stride, int topk, const int32_t *__restrict__ offsets,
                                                                          int heads, int head_blocks, int64_t m0, int tiles, int64_t blocks,
                                                                          int64_t chunk, float scale2, float sm_scale,
                                                                          const uint16_t *__restrict__ out, const uint16_t *__restrict__ d_out,
                                                                          const float *__restrict__ lse, float *__restrict__ staging)
{
    const SmlaBf16Rows cache = SmlaBf16Rows::make(kv, kv_stride, s_rows, 0, 0);
    __shared__ __attribute__((aligned(16))) unsigned char tile[SMLA_TILE * SMLA_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[SMLB_HEADS * SMLA_ROW_BYTES];      // the head block's q, one row a head
    __shared__ __attribute__((aligned(16))) unsigned char doimg[SMLB_HEADS * SMLB_DO_ROW_BYTES];  // ... and its d_out
    __shared__ __attribute__((aligned(16))) unsigned char wimg[2][SMLB_HEADS * SMLB_W_ROW_BYTES]; // bf16 [head][key]: 0 the block's p, 1 its dS
    __shared__ __attribute__((aligned(16))) int32_t rowidx[SMLA_TILE];                            // the kv row of a position, -1: invalid
    __shared__ float delta_s[SMLB_HEADS], lse2_s[SMLB_HEADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the logical block, walked XCD by XCD as the atomic kernel's: a token's tiles are consecutive, its images stay in one L2
    int64_t block = blockIdx.x;
    if (chunk) block = (block & 7) * chunk + (block >> 3);
    if (block >= blocks) return;                             // (the whole workgroup alike, before any barrier)
    const int64_t tc = block / tiles, t = m0 + tc;
    const int tl = (int)(block % tiles);
    const int wlo = wave & 1, whi = wave >> 1;

    // the gather of the one tile: eight threads a position, an invalid position staged as zeros and marked -1
    const int gpos = tid >> 3, gsub = tid & 7;
    const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
    int32_t row = -1;
    if (pos < topk) {
        const int32_t i = indices[t * idx_stride + pos];
        const int64_t r = (int64_t)i + (offsets ? (int64_t)offsets[t] : 0);
        if (i >= 0 && r >= 0 && r < cache.s_rows) row = (int32_t)r;
    }
    {
        uint4 raw[SMLA_STAGE];
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) raw[c] = uint4{0, 0, 0, 0};
        if (row >= 0) SmlaBf16Rows::load(cache.at(row, gsub), gsub, raw);
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(tile + gpos * SMLA_ROW_BYTES + SmlaBf16Rows::lds_at(c, gsub)) = raw[c];
        if (gsub == 0) rowidx[gpos] = row;
    }
    if (!__syncthreads_or(row >= 0)) return;                 // no valid position: nothing is stored for this tile

    smla_v4f acc[SMLB_WAVE_TILES];
#pragma unroll
    for (int j = 0; j < SMLB_WAVE_TILES; ++j) acc[j] = smla_v4f{0.f, 0.f, 0.f, 0.f};

    // LDS addresses of the lane's reads, the atomic kernel's (A: rows of K, q and d_out at bytes 64 s + 16 g; C: transposed reads of the
    // q and d_out images and of the weight images)
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    const uint32_t ka_addr = smlb_lds(tile) + (16 * whi + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t qa_addr = smlb_lds(qimg) + (16 * wlo + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t da_addr = smlb_lds(doimg) + (16 * wlo + hl) * SMLB_DO_ROW_BYTES + 16 * g;
    const uint32_t wa_at = (16 * wlo + hl) * SMLB_W_ROW_BYTES + 2 * (16 * whi + 4 * g);          // A writes its four keys here
    const uint32_t qt_addr = smlb_lds(qimg) + trow * SMLA_ROW_BYTES + tcol + 32 * (SMLB_WAVE_TILES * whi);
    const uint32_t dt_addr = smlb_lds(doimg) + trow * SMLB_DO_ROW_BYTES + tcol + 32 * (SMLB_WAVE_TILES * whi);
    const uint32_t wt_at = trow * SMLB_W_ROW_BYTES + tcol + 2 * (16 * wlo);                      // C's P^T and dS^T: keys 16 (w & 1) ..

#pragma unroll 1
    for (int hb = 0; hb < head_blocks; ++hb) {
        const int hb0 = hb * SMLB_HEADS;
        const bool computes = hb0 + 16 * wlo < heads;        // (A: a head tile beyond the last head has nothing to compute)
        if (hb) __syncthreads();                             // (the images are free: C of the block before has read them)

        // the atomic kernel's prologue: head hb0 + gpos by the eight threads tid % 8
        {
            const int head = hb0 + gpos;
            const bool has = head < heads;
            uint4 v[SMLA_STAGE];
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = uint4{0, 0, 0, 0};
            if (has) {
                const uint16_t *qrow = q + ((t * heads + head) * SMLA_D + gsub * 8);
#pragma unroll
                for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
            }
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
            uint4 d[SMLA_DV / 64], o[SMLA_DV / 64];
#pragma unroll
            for (int c = 0; c < SMLA_DV / 64; ++c) d[c] = o[c] = uint4{0, 0, 0, 0};
            if (has) {
                const int64_t at = (t * heads + head) * SMLA_DV + gsub * 8;
#pragma unroll
                for (int c = 0; c < SMLA_DV / 64; ++c) {
                    d[c] = *reinterpret_cast<const uint4 *>(d_out + at + 64 * c);
                    o[c] = *reinterpret_cast<const uint4 *>(out + at + 64 * c);
                }
            }
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < SMLA_DV / 64; ++c) {
                *reinterpret_cast<uint4 *>(doimg + gpos * SMLB_DO_ROW_BYTES + gsub * 16 + 128 * c) = d[c];
                sum = smlb_dot8(sum, o[c], d[c]);
            }
            sum = sum + __shfl_xor(sum, 1, 64);
            sum = sum + __shfl_xor(sum, 2, 64);
            sum = sum + __shfl_xor(sum, 4, 64);
            if (gsub == 0) {
                delta_s[gpos] = sum;
                lse2_s[gpos] = has ? lse[t * heads + head] * 1.4426950408889634f : 0.f;
            }
        }
        __syncthreads();

        // ---- A ---- (the atomic kernel's; a head tile that computes nothing writes zeros over what the block before left)
        if (computes) {
            const float delta = delta_s[16 * wlo + hl], lse2 = lse2_s[16 * wlo + hl];
            smla_v4f sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            smla_v4u ka[2][2], qq[2][2], dd[2][2];
            auto read_a = [&](int grp) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int s = 2 * grp + j;
                    ka[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(ka_addr + 64 * s);
                    qq[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(qa_addr + 64 * s);
                    if (s < SMLA_DV / 32) dd[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(da_addr + 64 * s);
                }
            };
            read_a(0);
#pragma unroll
            for (int grp = 0; grp < SMLA_KSTEPS / 2; ++grp) {
                if (grp + 1 < SMLA_KSTEPS / 2) read_a(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka[grp & 1][j]),
                                                                 __builtin_bit_cast(smla_v8bf, qq[grp & 1][j]), sv, 0, 0, 0);
                    if (2 * grp + j < SMLA_DV / 32)
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka[grp & 1][j]),
                                                                     __builtin_bit_cast(smla_v8bf, dd[grp & 1][j]), dp, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            const smlb_v4i rv = *reinterpret_cast<const smlb_v4i *>(&rowidx[16 * whi + 4 * g]);
            smla_v4bf pb, db;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool live = rv[i] >= 0;
                const float x = sv[i] * scale2;
                const float p = __builtin_amdgcn_exp2f(x - lse2);
                const float ds = (sm_scale * p) * (dp[i] - delta);
                pb[i] = (__bf16)(live ? p : 0.f);
                db[i] = (__bf16)(live ? ds : 0.f);
            }
            *reinterpret_cast<uint2 *>(&wimg[0][wa_at]) = __builtin_bit_cast(uint2, pb);
            *reinterpret_cast<uint2 *>(&wimg[1][wa_at]) = __builtin_bit_cast(uint2, db);
        } else {
            *reinterpret_cast<uint2 *>(&wimg[0][wa_at]) = uint2{0, 0};
            *reinterpret_cast<uint2 *>(&wimg[1][wa_at]) = uint2{0, 0};
        }
        __syncthreads();

        // ---- C ---- (key subtile w & 1, column tiles 18 (w >> 1) ..): acc += dS^T Q, then += P^T dO for columns < 512
        {
            const smla_v8bf pa = smlb_read_tr(smlb_lds(&wimg[0][0]) + wt_at, 16 * SMLB_W_ROW_BYTES);
            const smla_v8bf dsa = smlb_read_tr(smlb_lds(&wimg[1][0]) + wt_at, 16 * SMLB_W_ROW_BYTES);
            smla_v8bf qt[2][SMLB_GROUP], dt[2][SMLB_GROUP];
            auto read_c = [&](int grp) {
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j) {
                    const int ct = SMLB_GROUP * grp + j;
                    qt[grp & 1][j] = smlb_read_tr(qt_addr + 32 * ct, 16 * SMLA_ROW_BYTES);
                    // (whi is wave-uniform: the column tiles 32 .. 35, the rope part, have no d_out)
                    if (SMLB_WAVE_TILES * whi + ct < SMLA_CTILES) dt[grp & 1][j] = smlb_read_tr(dt_addr + 32 * ct, 16 * SMLB_DO_ROW_BYTES);
                }
            };
            read_c(0);
#pragma unroll
            for (int grp = 0; grp < SMLB_WAVE_TILES / SMLB_GROUP; ++grp) {
                if (grp + 1 < SMLB_WAVE_TILES / SMLB_GROUP) read_c(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j) {
                    const int ct = SMLB_GROUP * grp + j;
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, qt[grp & 1][j], acc[ct], 0, 0, 0);
                    if (SMLB_WAVE_TILES * whi + ct < SMLA_CTILES)
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, dt[grp & 1][j], acc[ct], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // T[m, j, :]: the lane holds column 16 (18 whi + ct) + hl of the keys 16 wlo + 4 g + i; sixteen lanes store 64 contiguous bytes
    const smlb_v4i rv = *reinterpret_cast<const smlb_v4i *>(&rowidx[16 * wlo + 4 * g]);
    float *dst = staging + ((tc * topk + (int64_t)tl * SMLA_TILE + 16 * wlo + 4 * g) * SMLA_D + 16 * (SMLB_WAVE_TILES * whi) + hl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (rv[i] < 0) continue;                             // (a position beyond topk is marked -1 as well)
#pragma unroll
        for (int ct = 0; ct < SMLB_WAVE_TILES; ++ct) dst[(int64_t)i * SMLA_D + 16 * ct] = acc[ct][i];
    }
}

// ---- the reduction ----
constexpr int SMLD_REDUCE_THREADS = SMLA_D / 4;              // a float4 of columns a thread: 144
constexpr int SMLD_REDUCE_AHEAD = 4;                         // staged rows in flight

__global__ void __launch_bounds__(SMLD_REDUCE_THREADS) sparse_mla_bwd_reduce_kernel(const float *__restrict__ staging,
                                                                                    const int32_t *__restrict__ start,
                                                                                    const int32_t *__restrict__ count,
                                                                                    const int32_t *__restrict__ ordered, float *__restrict__ dkv,
                                                                                    int64_t dkv_stride)
{
    const int64_t r = blockIdx.x;
    const int32_t n = count[r];
    if (n == 0) return;                                      // (a row no position of the chunk names keeps its bytes)
    const int32_t *seg = ordered + start[r];
    const float4 *src = reinterpret_cast<const float4 *>(staging) + threadIdx.x;
    auto add = [](float4 &a, const float4 &v) {
        a.x = a.x + v.x;
        a.y = a.y + v.y;
        a.z = a.z + v.z;
        a.w = a.w + v.w;
    };
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    int32_t k = 0;
    for (; k + SMLD_REDUCE_AHEAD <= n; k += SMLD_REDUCE_AHEAD) {
        float4 v[SMLD_REDUCE_AHEAD];
#pragma unroll
        for (int u = 0; u < SMLD_REDUCE_AHEAD; ++u) v[u] = src[(int64_t)seg[k + u] * SMLD_REDUCE_THREADS];
#pragma unroll
        for (int u = 0; u < SMLD_REDUCE_AHEAD; ++u) add(acc, v[u]);
    }
    for (; k < n; ++k) add(acc, src[(int64_t)seg[k] * SMLD_REDUCE_THREADS]);
    float4 *dst = reinterpret_cast<float4 *>(dkv + r * dkv_stride) + threadIdx.x;
    float4 sum = *dst;
    add(sum, acc);
    *dst = sum;
}

// The workspace of a chunk of c tokens (c topk < 2^31): T, then count / start / cursor, then the two lists; every part 16-byte aligned
struct DetLayout {
    int64_t pairs, counts_at, lists_at, list_bytes, total;
};
static DetLayout det_layout(int64_t c, int64_t topk, int64_t s)
{
    DetLayout l;
    l.pairs = c * topk;
    l.counts_at = l.pairs * (SMLA_D * 4);
    l.lists_at = l.counts_at + (3 * (s + 1) * 4 + 15) / 16 * 16;
    l.list_bytes = (l.pairs * 4 + 15) / 16 * 16;
    l.total = l.lists_at + 2 * l.list_bytes;
    return l;
}
static int64_t det_rule(int64_t m, int64_t topk)
{
    const int64_t fit = DGA_SPARSE_MLA_BWD_DET_STAGING_BYTES / (topk * (SMLA_D * 4));
    const int64_t c = m < fit ? m : fit;
    return c > 1 ? c : 1;
}

}  // namespace dga

extern "C" int64_t dga_sparse_mla_bwd_det_workspace_bytes(int64_t m, int heads, int64_t topk, int64_t s)
{
    using namespace dga;
    if (m < 1 || heads < 16 || heads > DGA_SPARSE_MLA_MAX_HEADS || heads % 16 || topk < 1 || topk > 0x7FFFFFFFll - DGA_SPARSE_MLA_TILE || s < 1 ||
        s > 0x7FFFFFFFll)
        return 0;
    return det_layout(det_rule(m, topk), topk, s).total;
}

// dga_sparse_mla_bwd's checks in its order, then this entry's own in the same order: shape, null, alignment, workspace
extern "C" int dga_sparse_mla_bwd_det(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                      int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags,
                                      const void *out, const void *d_out, const float *lse, void *dq, float *dkv, int64_t dkv_stride,
                                      int64_t chunk_tokens, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace dga;
    const SmlaBwdCall b{{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream}, kv, s, kv_stride, out, d_out, lse, dq,
                        dkv, dkv_stride};
    bool launch;
    int rc = check_sparse_mla_bwd(b, &launch);
    if (!launch) return rc;
    if (chunk_tokens < 0) return DGA_E_SHAPE;
    const int64_t c = chunk_tokens ? (chunk_tokens < m ? chunk_tokens : m) : det_rule(m, topk);
    if (c > 0x7FFFFFFFll / topk) return DGA_E_SHAPE;
    if (!workspace) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return DGA_E_ALIGN;
    const DetLayout lay = det_layout(c, topk, s);
    if (workspace_bytes < lay.total) return DGA_E_WORKSPACE;

    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *staging = reinterpret_cast<float *>(ws);
    int32_t *count = reinterpret_cast<int32_t *>(ws + lay.counts_at), *start = count + (s + 1), *cursor = start + (s + 1);
    int32_t *list = reinterpret_cast<int32_t *>(ws + lay.lists_at), *ordered = reinterpret_cast<int32_t *>(ws + lay.lists_at + lay.list_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int head_blocks = (heads + SMLB_HEADS - 1) / SMLB_HEADS;
    const int tiles = static_cast<int>((topk + SMLA_TILE - 1) / SMLA_TILE);
    const bool linear = (flags & DGA_SPARSE_MLA_LINEAR_GRID) != 0;
    auto grid_of = [](int64_t n, int per) { return dim3(static_cast<unsigned>((n + per - 1) / per)); };

    rc = launch_sparse_mla_bwd(b, false);
    for (int64_t m0 = 0; m0 < m && rc == DGA_OK; m0 += c) {
        const int64_t mc = m - m0 < c ? m - m0 : c;
        const RowLists l{indices, index_offsets, idx_stride, s, m0, mc * topk, static_cast<int>(topk)};
        const dim3 by_pair = grid_of(l.pairs, ROWINV_THREADS);
        hipLaunchKernelGGL(rowinv_clear_kernel, grid_of(s + 1, ROWINV_THREADS), dim3(ROWINV_THREADS), 0, st, count, s + 1);
        hipLaunchKernelGGL(rowinv_count_kernel, by_pair, dim3(ROWINV_THREADS), 0, st, l, count);
        hipLaunchKernelGGL(rowinv_scan_kernel, dim3(1), dim3(ROWINV_SCAN_THREADS), 0, st, count, start, cursor, s + 1);
        hipLaunchKernelGGL(rowinv_fill_kernel, by_pair, dim3(ROWINV_THREADS), 0, st, l, cursor, list);
        hipLaunchKernelGGL(rowinv_order_kernel, by_pair, dim3(ROWINV_THREADS), 0, st, l, start, count, list, ordered);
        const int64_t blocks = mc * tiles;                   // (< 2^31 / 32)
        const int64_t chunk8 = linear ? 0 : (blocks + 7) / 8;
        hipLaunchKernelGGL(sparse_mla_bwd_dkv_kernel, dim3(static_cast<unsigned>(linear ? blocks : chunk8 * 8)), dim3(SMLA_THREADS), 0, st,
                           static_cast<const uint16_t *>(q), kv, kv_stride, s, indices, idx_stride, static_cast<int>(topk), index_offsets, heads,
                           head_blocks, m0, tiles, blocks, chunk8, static_cast<float>(sm_scale * 1.4426950408889634),
                           static_cast<float>(sm_scale), static_cast<const uint16_t *>(out), static_cast<const uint16_t *>(d_out), lse, staging);
        hipLaunchKernelGGL(sparse_mla_bwd_reduce_kernel, dim3(static_cast<unsigned>(s)), dim3(SMLD_REDUCE_THREADS), 0, st, staging, start, count,
                           ordered, dkv, dkv_stride);
        rc = record_hip(hipGetLastError());
    }
    return rc;
}
