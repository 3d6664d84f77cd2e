// The backward of the dense stage's main attention (dga_mla_dense.hip is the forward): dq and dkv from d_out, the forward's out and lse, over
// EVERY key of a token's range -- no list, no gather, no atomics.
//   dga_mla_bwd_dense   q bf16 [m, heads, 576], kv bf16 [s, 576] (rows kv_stride apart), ks / ke int32 [m] clamped to [0, s] as the forward
//                       clamps them; out, d_out bf16 [m, heads, 512], lse fp32 [m, heads]
//                       -> dq bf16 [m, heads, 576] (written), dkv fp32 [s, 576] (rows dkv_stride apart; added into)
//     over the keys n of [lo[t], hi[t]), L2E = (float)log2 e, scale2 = (float)(sm_scale L2E): dga_sparse_mla_bwd's formulas, key n = row n
//     p_n     = exp2(S_n scale2 - lse[t, h] L2E)           S_n = sum_d q[t, h, d] kv[n, d]
//     delta   = sum_c out[t, h, c] d_out[t, h, c]          dP_n = sum_c d_out[t, h, c] kv[n, c]           (c < 512)
//     dS_n    = ((float)sm_scale p_n) (dP_n - delta)
//     dq[t, h, :]   = sum_n bf16(dS_n) kv[n, :576]
//     dkv[n, :576] += sum_{t, h} bf16(dS_n) q[t, h, :]     dkv[n, :512] += sum_{t, h} bf16(p_n) d_out[t, h, :]
// With q, out and d_out contiguous the problem is regular: flat row r = t heads + h, and as heads is a multiple of 16 a 16-row tile never
// straddles a token.  Two passes each recompute the scores (dga_mqa_logits_bwd_dense.hip's answer), every output element has one writer.
// The per-tile arithmetic is phases A, B and C of dga_sparse_mla_bwd.hip, instruction order included; only who owns what changes.  All
// kernels: 256 threads, tiles of 32 consecutive kv rows in the 1184-byte-row LDS format, a block of 32 flat rows of q (1184-byte rows) and
// d_out (1056-byte rows), the bf16 images of P and dS [row][key] in rows of 80 B.  The images go through LDS as in the sparse backward: the
// wave that rounds a weight (row tile w & 1, key subtile w >> 1) is not the wave that consumes it (all 32 keys, or all 32 rows, of one MFMA).
//
// Row-owned pass (mdb_row_kernel: dq, and delta to the workspace).  A workgroup owns the flat rows 32 g .. 32 g + 31: two row tiles, at
// most two tokens and two ranges.  Prologue: q and d_out of the block to LDS once, delta by the sparse backward's fixed-order tree (eight
// threads a row, chunks i + 8 c ascending, lane ^ 1, ^ 2, ^ 4), also stored as fp32 [m heads] for the key-owned pass.  The walk is the
// forward's: ascending over the tiles that meet one of the two ranges, a row outside both staged as zeros, one tile ahead in registers, two
// tile images.  Per tile: A (S^T and dP^T from one ds_read_b128 of K; p, dS; +0 selected outside the row tile's range on a tile that
// straddles lo or hi) writes the dS image, a barrier, B (dQ^T += K^T dS^T, 72 fp32 accumulators a lane held across the whole walk).  A
// wave skips A and B of a tile that misses its row tile's range (wave-uniform; the barriers stay outside the branches): lse = -inf of an
// empty token never reaches an exp2.  Two barriers a tile: the dS image stands between A and B.  Epilogue: dq = RNE_bf16(acc).
//
// Key-owned pass (mdb_key_kernel: dkv's partial tiles).  A workgroup owns one tile of 32 keys, resident in LDS for its whole life (rows
// >= s as zeros), and one chunk of consecutive 32-row blocks.  It walks the blocks of its chunk with a row tile whose range meets the
// tile, found from the ranges as the indexer's key pass finds its tokens (lane i holds block i's two ranges, a ballot); the others are
// neither loaded nor multiplied.  A block's q and d_out rows (9 + 8 uint4 a thread), lse and delta come one block ahead in registers into
// a single image pair; the rows of a row tile that misses the tile are staged as zeros, so whatever an empty token's q, d_out, lse and
// delta hold reaches no product.  Per block: A (the P and dS images, zeros for a row tile that misses), a barrier, C (dKV [16 keys x 16
// columns] += dS^T Q over the 32 rows and, for columns < 512, P^T dO into the same accumulator), 18 column tiles a wave: 72 accumulators a
// lane that stay in registers across all blocks.  At the end the partial tile, and per key whether a range named it, go to the workspace.
// Causal ranges give low key tiles long walks and high ones short walks, so the blocks are split over `chunks` workgroups per key tile, a
// function of (m, heads, s) alone; the grid runs key tiles ascending, a tile's chunks descending: the longest walks first.
//
// mdb_reduce_kernel stores dkv[n, c] = fl(prior + ((p_0 + p_1) + ... + p_last)), chunks ascending, once per element of the named rows.
// A row no range names and a column >= 576 is not written.  dq and dkv are byte-reproducible: every sum's order follows from the shapes
// and the ranges.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int MDB_ROWS = SMLA_TILE;                          // flat rows of a block: 32, two row tiles
constexpr int MDB_TILE_BYTES = SMLA_TILE * SMLA_ROW_BYTES;   // 37 888: a key tile's image, and a block's q image
constexpr int MDB_DO_ROW_BYTES = SMLA_DV * 2 + 32;           // 1056
constexpr int MDB_W_ROW_BYTES = SMLA_TILE * 2 + 16;          // 80: a row's 32 weights (p or dS) of the tile
constexpr int MDB_W_BYTES = MDB_ROWS * MDB_W_ROW_BYTES;      // 2560
constexpr int MDB_DSTAGE = SMLA_DV / 64;                     // 16-byte chunks of a d_out row a thread brings: 8
constexpr int MDB_WAVE_TILES = SMLA_D / 32;                  // column tiles of dq and dkv of one wave: 18 of 36
constexpr int MDB_GROUP = 3;                                 // column tiles whose LDS reads are in flight together
constexpr int MDB_MAX_CHUNKS = 16, MDB_TARGET_GROUPS = 1024;
constexpr int MDB_END = 0x7FFFFFFF;                          // no further tile
static_assert(MDB_ROWS * 8 == SMLA_THREADS && MDB_WAVE_TILES % MDB_GROUP == 0 && SMLA_DV % 64 == 0 && SMLA_D % 4 == 0, "the backward's geometry");
static_assert(3 * MDB_TILE_BYTES + MDB_ROWS * MDB_DO_ROW_BYTES + 2 * MDB_W_BYTES + 1024 <= 160 * 1024, "q, d_out, two tile images and the weights in LDS");

typedef int32_t mdb_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int mdb_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
__device__ __forceinline__ float mdb_bf16(uint32_t bits) { return __uint_as_float(bits << 16); }
// the products of the eight bf16 pairs of two 16-byte chunks, added to `sum` in ascending order (the sparse backward's)
__device__ __forceinline__ float mdb_dot8(float sum, const uint4 &a, const uint4 &b)
{
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sum = sum + mdb_bf16(x[i] & 0xFFFFu) * mdb_bf16(y[i] & 0xFFFFu);
        sum = sum + mdb_bf16(x[i] >> 16) * mdb_bf16(y[i] >> 16);
    }
    return sum;
}
__device__ __forceinline__ uint32_t mdb_lds(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char *)p;
}
// one 16 x 32 (or 32 x 16) bf16 fragment by two transposed reads: the blocks at `addr` and sixteen image rows (`half` bytes) below it
__device__ __forceinline__ smla_v8bf mdb_read_tr(uint32_t addr, int half)
{
    const smla_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(addr));
    const smla_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(addr + half));
    return __builtin_bit_cast(smla_v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ void mdb_zero(uint4 *v, int n)
{
#pragma unroll
    for (int c = 0; c < n; ++c) v[c] = uint4{0, 0, 0, 0};
}

// Phase A's products for one (row tile, key subtile): S^T and dP^T [16 keys x 16 rows], 18 + 16 chained MFMAs, K the A operand (one
// ds_read_b128 serves both chains), q and d_out the B operands; the reads run one group of two d steps ahead of the MFMAs
__device__ __forceinline__ void mdb_scores(uint32_t ka_addr, uint32_t qa_addr, uint32_t da_addr, smla_v4f &sv, smla_v4f &dp)
{
    sv = dp = smla_v4f{0.f, 0.f, 0.f, 0.f};
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
}
// ... and its weights: p and dS of the lane's four keys first .. first + 3, +0 outside [lo, hi) by a select (whole: the tile lies inside
// the range and takes none), rounded to bf16 (RNE)
__device__ __forceinline__ void mdb_weights(const smla_v4f &sv, const smla_v4f &dp, float scale2, float sm_scale, float lse2, float delta,
                                            int first, int lo, int hi, bool whole, smla_v4bf &pb, smla_v4bf &db)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool live = whole || (first + i >= lo && first + i < hi);
        const float x = sv[i] * scale2;
        const float p = __builtin_amdgcn_exp2f(x - lse2);
        const float ds = (sm_scale * p) * (dp[i] - delta);
        pb[i] = (__bf16)(live ? p : 0.f);
        db[i] = (__bf16)(live ? ds : 0.f);
    }
}

// ---- the row-owned pass: dq, and delta to the workspace ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(SMLA_THREADS) mdb_row_kernel(const uint16_t *__restrict__ q, const uint16_t *__restrict__ kv, int64_t kv_stride,
                                                               int n_keys, const int32_t *__restrict__ ks_in, const int32_t *__restrict__ ke_in,
                                                               int heads, int64_t rows, int64_t blocks, float scale2, float sm_scale,
                                                               const uint16_t *__restrict__ out, const uint16_t *__restrict__ d_out,
                                                               const float *__restrict__ lse, uint16_t *__restrict__ dq,
                                                               float *__restrict__ delta_out)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][MDB_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[MDB_TILE_BYTES];                    // the block's q, one row a flat row
    __shared__ __attribute__((aligned(16))) unsigned char doimg[MDB_ROWS * MDB_DO_ROW_BYTES];      // ... and its d_out
    __shared__ __attribute__((aligned(16))) unsigned char dsimg[MDB_W_BYTES];                      // bf16 [row][key]: the tile's dS
    __shared__ float delta_s[MDB_ROWS], lse2_s[MDB_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int wlo = wave & 1, whi = wave >> 1;
    const int64_t block = blocks - 1 - (int64_t)blockIdx.x;  // (descending: under causal ranges the longest walks start first)
    const int64_t row0 = block * MDB_ROWS;

    // the two row tiles' ranges, clamped to [0, s] as the forward clamps them; an empty one (and a tile beyond the rows) is [0, 0)
    int lo[2], hi[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        lo[w] = hi[w] = 0;
        if (row0 + 16 * w < rows) {
            const int64_t t = (row0 + 16 * w) / heads;
            const int a = mdb_clamp(ks_in[t], n_keys), b = mdb_clamp(ke_in[t], n_keys);
            if (b > a) lo[w] = a, hi[w] = b;
        }
    }
    // the first tile >= tl that meets one of the ranges (the same in every thread)
    auto next_live = [&](int tl) -> int {
        int best = MDB_END;
#pragma unroll
        for (int w = 0; w < 2; ++w)
            if (hi[w] > lo[w] && tl * SMLA_TILE < hi[w]) {
                const int first = lo[w] / SMLA_TILE;
                const int cand = tl > first ? tl : first;
                best = cand < best ? cand : best;
            }
        return best;
    };
    const int mylo = wlo ? lo[1] : lo[0], myhi = wlo ? hi[1] : hi[0];

    // the staging: eight threads a row, thread tid % 8 of them the chunks tid % 8 + 8 c; a row outside both ranges (rows >= s among them) is zeros
    const int gpos = tid >> 3, gsub = tid & 7;
    uint4 staged[SMLA_STAGE];
    auto fetch = [&](int tl) {
        const int n = tl * SMLA_TILE + gpos;
        const bool in = (n >= lo[0] && n < hi[0]) || (n >= lo[1] && n < hi[1]);
        mdb_zero(staged, SMLA_STAGE);
        if (in) {
            const uint16_t *p = kv + ((int64_t)n * kv_stride + gsub * 8);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) staged[c] = *reinterpret_cast<const uint4 *>(p + 64 * c);
        }
    };
    int cur = next_live(0);
    if (cur != MDB_END) fetch(cur);

    // the prologue: flat row row0 + gpos by the eight threads tid % 8 (rows beyond m heads as zeros)
    {
        const int64_t row = row0 + gpos;
        const bool has = row < rows;
        uint4 v[SMLA_STAGE], d[MDB_DSTAGE], o[MDB_DSTAGE];
        mdb_zero(v, SMLA_STAGE), mdb_zero(d, MDB_DSTAGE), mdb_zero(o, MDB_DSTAGE);
        if (has) {
            const uint16_t *qrow = q + (row * SMLA_D + gsub * 8);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
            const int64_t at = row * SMLA_DV + gsub * 8;
#pragma unroll
            for (int c = 0; c < MDB_DSTAGE; ++c) {
                d[c] = *reinterpret_cast<const uint4 *>(d_out + at + 64 * c);
                o[c] = *reinterpret_cast<const uint4 *>(out + at + 64 * c);
            }
        }
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < MDB_DSTAGE; ++c) {
            *reinterpret_cast<uint4 *>(doimg + gpos * MDB_DO_ROW_BYTES + gsub * 16 + 128 * c) = d[c];
            sum = mdb_dot8(sum, o[c], d[c]);
        }
        sum = sum + __shfl_xor(sum, 1, 64);
        sum = sum + __shfl_xor(sum, 2, 64);
        sum = sum + __shfl_xor(sum, 4, 64);
        if (gsub == 0) {
            delta_s[gpos] = sum;
            lse2_s[gpos] = has ? lse[row] * 1.4426950408889634f : 0.f;
            if (has) delta_out[row] = sum;
        }
    }
    __syncthreads();
    const float delta = delta_s[16 * wlo + hl], lse2 = lse2_s[16 * wlo + hl];   // (A: the lane's row)

    smla_v4f accq[MDB_WAVE_TILES];
#pragma unroll
    for (int j = 0; j < MDB_WAVE_TILES; ++j) accq[j] = smla_v4f{0.f, 0.f, 0.f, 0.f};

    // LDS addresses of the lane's reads in tile image 0 (the sparse backward's): A the rows of K, q and d_out at bytes 64 s + 16 g; B the
    // transposed reads of the tile (lane 4 r + c of a group gives row r, columns 4 c .. of a block of 4 x 16)
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    const uint32_t ka_addr0 = mdb_lds(tile) + (16 * whi + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t qa_addr = mdb_lds(qimg) + (16 * wlo + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t da_addr = mdb_lds(doimg) + (16 * wlo + hl) * MDB_DO_ROW_BYTES + 16 * g;
    const uint32_t wa_at = (16 * wlo + hl) * MDB_W_ROW_BYTES + 2 * (16 * whi + 4 * g);           // A writes its four keys here
    const uint32_t kt_addr0 = mdb_lds(tile) + trow * SMLA_ROW_BYTES + tcol + 32 * (MDB_WAVE_TILES * whi);
    const uint32_t wb_at = (16 * wlo + hl) * MDB_W_ROW_BYTES + 8 * g;                            // B's dS^T: keys 4 g .. and, 32 bytes on, 16 + 4 g ..

    int step = 0;
#pragma unroll 1
    while (cur != MDB_END) {
        const int par = step & 1;
        // the staged tile goes to image `par`: it was last read by B two tiles ago, before both barriers of the previous tile
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(&tile[par][gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c]) = staged[c];
        __syncthreads();
        const int nxt = next_live(cur + 1);
        if (nxt != MDB_END) fetch(nxt);

        const int n0 = cur * SMLA_TILE;
        const bool mine = myhi > mylo && n0 < myhi && n0 + SMLA_TILE > mylo;    // (wave-uniform; the barriers stay outside)
        // ---- A ----
        if (mine) {
            smla_v4f sv, dp;
            mdb_scores(ka_addr0 + par * MDB_TILE_BYTES, qa_addr, da_addr, sv, dp);
            smla_v4bf pb, db;
            mdb_weights(sv, dp, scale2, sm_scale, lse2, delta, n0 + 16 * whi + 4 * g, mylo, myhi, n0 >= mylo && n0 + SMLA_TILE <= myhi, pb, db);
            *reinterpret_cast<uint2 *>(&dsimg[wa_at]) = __builtin_bit_cast(uint2, db);
        }
        __syncthreads();
        // ---- B ----
        if (mine) {
            const uint32_t kt_addr = kt_addr0 + par * MDB_TILE_BYTES;
            const uint2 w0 = *reinterpret_cast<const uint2 *>(&dsimg[wb_at]), w1 = *reinterpret_cast<const uint2 *>(&dsimg[wb_at + 32]);
            const smla_v8bf dsb = __builtin_bit_cast(smla_v8bf, (smla_v4u{w0.x, w0.y, w1.x, w1.y}));
            smla_v8bf kt[2][MDB_GROUP];
            auto read_b = [&](int grp) {
#pragma unroll
                for (int j = 0; j < MDB_GROUP; ++j) kt[grp & 1][j] = mdb_read_tr(kt_addr + 32 * (MDB_GROUP * grp + j), 16 * SMLA_ROW_BYTES);
            };
            read_b(0);
#pragma unroll
            for (int grp = 0; grp < MDB_WAVE_TILES / MDB_GROUP; ++grp) {
                if (grp + 1 < MDB_WAVE_TILES / MDB_GROUP) read_b(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < MDB_GROUP; ++j)
                    accq[MDB_GROUP * grp + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt[grp & 1][j], dsb, accq[MDB_GROUP * grp + j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        cur = nxt, ++step;
    }

    if (row0 + 16 * wlo >= rows) return;
    uint16_t *drow = dq + ((row0 + 16 * wlo + hl) * SMLA_D + 16 * (MDB_WAVE_TILES * whi) + 4 * g);
#pragma unroll
    for (int j = 0; j < MDB_WAVE_TILES; ++j) {
        smla_v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)accq[j][i];
        *reinterpret_cast<uint2 *>(drow + 16 * j) = __builtin_bit_cast(uint2, o);
    }
}

// ---- the key-owned pass: dkv's partial tiles ----------------------------------------------------------------------------------------------
struct MdbBlock {
    int b;                  // -1: none left
    int lo0, hi0, lo1, hi1; // its two row tiles' ranges; [0, 0) for one that misses the key tile
};

__global__ void __launch_bounds__(SMLA_THREADS) mdb_key_kernel(const uint16_t *__restrict__ q, const uint16_t *__restrict__ kv, int64_t kv_stride,
                                                               int n_keys, const int32_t *__restrict__ ks_in, const int32_t *__restrict__ ke_in,
                                                               int heads, int64_t rows, int blocks, int chunks, int blocks_per_chunk, float scale2,
                                                               float sm_scale, const uint16_t *__restrict__ d_out, const float *__restrict__ lse,
                                                               const float *__restrict__ delta_in, float *__restrict__ part,
                                                               int32_t *__restrict__ named_out, int64_t n_pad)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[MDB_TILE_BYTES];                    // the workgroup's 32 keys
    __shared__ __attribute__((aligned(16))) unsigned char qimg[MDB_TILE_BYTES];                    // a block's q, one row a flat row
    __shared__ __attribute__((aligned(16))) unsigned char doimg[MDB_ROWS * MDB_DO_ROW_BYTES];      // ... and its d_out
    __shared__ __attribute__((aligned(16))) unsigned char wimg[2][MDB_W_BYTES];                    // bf16 [row][key]: 0 the block's p, 1 its dS
    __shared__ float delta_s[MDB_ROWS], lse2_s[MDB_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int wlo = wave & 1, whi = wave >> 1;
    const int kt = blockIdx.x / chunks, chunk = chunks - 1 - blockIdx.x % chunks;
    const int n0 = kt * SMLA_TILE, n1 = n0 + SMLA_TILE;      // (s + 1024 fits an int; the ranges are clamped to s)
    const int gpos = tid >> 3, gsub = tid & 7;

    // the resident tile: eight threads a row, rows >= s as zeros (behind the first barrier of the walk, or the one before the store)
    {
        uint4 v[SMLA_STAGE];
        mdb_zero(v, SMLA_STAGE);
        if (n0 + gpos < n_keys) {
            const uint16_t *p = kv + ((int64_t)(n0 + gpos) * kv_stride + gsub * 8);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(p + 64 * c);
        }
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(tile + gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
    }

    // the walk over the chunk's blocks with a row tile whose range meets the tile (every wave computes the same sequence)
    int run = chunk * blocks_per_chunk;
    const int run_end = blocks - run < blocks_per_chunk ? blocks : run + blocks_per_chunk;
    uint64_t act = 0;
    int act_b0 = 0, l0 = 0, h0 = 0, l1 = 0, h1 = 0;
    auto range_of = [&](int64_t row, int &lo, int &hi) {
        lo = hi = 0;
        if (row < rows) {
            const int64_t t = row / heads;
            const int a = mdb_clamp(ks_in[t], n_keys), b = mdb_clamp(ke_in[t], n_keys);
            if (a < b && a < n1 && b > n0) lo = a, hi = b;
        }
    };
    auto next_block = [&]() -> MdbBlock {
        while (act == 0) {
            if (run >= run_end) return MdbBlock{-1, 0, 0, 0, 0};
            act_b0 = run;
            l0 = h0 = l1 = h1 = 0;
            if (run_end - run > lane) {
                const int64_t r = (int64_t)(run + lane) * MDB_ROWS;
                range_of(r, l0, h0);
                range_of(r + 16, l1, h1);
            }
            act = __ballot(h0 > l0 || h1 > l1);
            run = run_end - run > 64 ? run + 64 : run_end;
        }
        const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(act));
        act &= act - 1;
        return MdbBlock{act_b0 + i, __builtin_amdgcn_readlane(l0, i), __builtin_amdgcn_readlane(h0, i), __builtin_amdgcn_readlane(l1, i),
                        __builtin_amdgcn_readlane(h1, i)};
    };

    // the staging of a block: row gpos by the eight threads tid % 8; the rows of a row tile that misses the tile are zeros
    uint4 sq[SMLA_STAGE], sd[MDB_DSTAGE];
    float slse = 0.f, sdelta = 0.f;
    auto fetch = [&](const MdbBlock &bk) {
        const bool in = gpos < 16 ? bk.hi0 > bk.lo0 : bk.hi1 > bk.lo1;        // (a range that meets the tile belongs to a row < m heads)
        const int64_t row = (int64_t)bk.b * MDB_ROWS + gpos;
        mdb_zero(sq, SMLA_STAGE), mdb_zero(sd, MDB_DSTAGE);
        slse = sdelta = 0.f;
        if (in) {
            const uint16_t *qrow = q + (row * SMLA_D + gsub * 8);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) sq[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
            const uint16_t *drow = d_out + (row * SMLA_DV + gsub * 8);
#pragma unroll
            for (int c = 0; c < MDB_DSTAGE; ++c) sd[c] = *reinterpret_cast<const uint4 *>(drow + 64 * c);
            if (gsub == 0) slse = lse[row], sdelta = delta_in[row];
        }
    };

    smla_v4f acc[MDB_WAVE_TILES];
#pragma unroll
    for (int j = 0; j < MDB_WAVE_TILES; ++j) acc[j] = smla_v4f{0.f, 0.f, 0.f, 0.f};
    bool named = false;                                      // of key n0 + tid % 32
    const int my_n = n0 + (tid & 31);

    // LDS addresses of the lane's reads (the sparse backward's): A the rows of K, q and d_out at bytes 64 s + 16 g; C the transposed reads
    // of the q and d_out images and of the weight images (keys 16 (w & 1) ..)
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    const uint32_t ka_addr = mdb_lds(tile) + (16 * whi + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t qa_addr = mdb_lds(qimg) + (16 * wlo + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t da_addr = mdb_lds(doimg) + (16 * wlo + hl) * MDB_DO_ROW_BYTES + 16 * g;
    const uint32_t wa_at = (16 * wlo + hl) * MDB_W_ROW_BYTES + 2 * (16 * whi + 4 * g);
    const uint32_t qt_addr = mdb_lds(qimg) + trow * SMLA_ROW_BYTES + tcol + 32 * (MDB_WAVE_TILES * whi);
    const uint32_t dt_addr = mdb_lds(doimg) + trow * MDB_DO_ROW_BYTES + tcol + 32 * (MDB_WAVE_TILES * whi);
    const uint32_t wt_at = trow * MDB_W_ROW_BYTES + tcol + 2 * (16 * wlo);

    MdbBlock cur = next_block();
    if (cur.b >= 0) fetch(cur);
#pragma unroll 1
    while (cur.b >= 0) {
        // the staged block goes to the images: C of the previous block is behind the barrier that ended it
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = sq[c];
#pragma unroll
        for (int c = 0; c < MDB_DSTAGE; ++c) *reinterpret_cast<uint4 *>(doimg + gpos * MDB_DO_ROW_BYTES + gsub * 16 + 128 * c) = sd[c];
        if (gsub == 0) {
            delta_s[gpos] = sdelta;
            lse2_s[gpos] = slse * 1.4426950408889634f;
        }
        named = named || (my_n >= cur.lo0 && my_n < cur.hi0) || (my_n >= cur.lo1 && my_n < cur.hi1);
        __syncthreads();
        const MdbBlock nx = next_block();
        if (nx.b >= 0) fetch(nx);

        // ---- A ----  (row tile w & 1, key subtile w >> 1; a row tile that misses the tile writes zeros and computes nothing)
        {
            const int rlo = wlo ? cur.lo1 : cur.lo0, rhi = wlo ? cur.hi1 : cur.hi0;
            smla_v4bf pb = {(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f}, db = pb;
            if (rhi > rlo) {
                smla_v4f sv, dp;
                mdb_scores(ka_addr, qa_addr, da_addr, sv, dp);
                mdb_weights(sv, dp, scale2, sm_scale, lse2_s[16 * wlo + hl], delta_s[16 * wlo + hl], n0 + 16 * whi + 4 * g, rlo, rhi,
                            n0 >= rlo && n1 <= rhi, pb, db);
            }
            *reinterpret_cast<uint2 *>(&wimg[0][wa_at]) = __builtin_bit_cast(uint2, pb);
            *reinterpret_cast<uint2 *>(&wimg[1][wa_at]) = __builtin_bit_cast(uint2, db);
        }
        __syncthreads();

        // ---- C ----  (key subtile w & 1, column tiles 18 (w >> 1) ..)
        {
            const smla_v8bf pa = mdb_read_tr(mdb_lds(&wimg[0][0]) + wt_at, 16 * MDB_W_ROW_BYTES);
            const smla_v8bf dsa = mdb_read_tr(mdb_lds(&wimg[1][0]) + wt_at, 16 * MDB_W_ROW_BYTES);
            smla_v8bf qt[2][MDB_GROUP], dt[2][MDB_GROUP];
            auto read_c = [&](int grp) {
#pragma unroll
                for (int j = 0; j < MDB_GROUP; ++j) {
                    const int ct = MDB_GROUP * grp + j;
                    qt[grp & 1][j] = mdb_read_tr(qt_addr + 32 * ct, 16 * SMLA_ROW_BYTES);
                    // (whi is wave-uniform: the column tiles 32 .. 35, the rope part, have no d_out)
                    if (MDB_WAVE_TILES * whi + ct < SMLA_CTILES) dt[grp & 1][j] = mdb_read_tr(dt_addr + 32 * ct, 16 * MDB_DO_ROW_BYTES);
                }
            };
            read_c(0);
#pragma unroll
            for (int grp = 0; grp < MDB_WAVE_TILES / MDB_GROUP; ++grp) {
                if (grp + 1 < MDB_WAVE_TILES / MDB_GROUP) read_c(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < MDB_GROUP; ++j) {
                    const int ct = MDB_GROUP * grp + j;
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, qt[grp & 1][j], acc[ct], 0, 0, 0);
                    if (MDB_WAVE_TILES * whi + ct < SMLA_CTILES)
                        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, dt[grp & 1][j], acc[ct], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        cur = nx;
    }

    // the partial tile (lane l: keys 16 (w & 1) + 4 (l >> 4) + i, column 16 (18 (w >> 1) + j) + (l & 15)) and the keys' flags; rows up to
    // n_pad exist
    float *prow = part + (((int64_t)chunk * n_pad + n0 + 16 * wlo + 4 * g) * SMLA_D + 16 * (MDB_WAVE_TILES * whi) + hl);
#pragma unroll
    for (int j = 0; j < MDB_WAVE_TILES; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i * SMLA_D + 16 * j] = acc[j][i];
    if (tid < SMLA_TILE) named_out[(int64_t)chunk * n_pad + my_n] = named ? 1 : 0;
}

// dkv[n, :576] = fl(prior + ((p_0 + p_1) + ... )) for the rows a range named: 144 threads a row, four columns each
__global__ void __launch_bounds__(SMLA_THREADS) mdb_reduce_kernel(const float *__restrict__ part, const int32_t *__restrict__ named_in, int chunks,
                                                                  int64_t n_pad, int n_keys, float *__restrict__ dkv, int64_t dkv_stride)
{
    const int64_t idx = (int64_t)blockIdx.x * SMLA_THREADS + threadIdx.x;
    const int64_t row = idx / (SMLA_D / 4);
    const int c4 = (int)(idx % (SMLA_D / 4));
    if (row >= n_keys) return;
    bool named = false;
    for (int s = 0; s < chunks; ++s) named = named || named_in[s * n_pad + row] != 0;
    if (!named) return;
    smla_v4f v = *reinterpret_cast<const smla_v4f *>(part + (row * SMLA_D + 4 * c4));
    for (int s = 1; s < chunks; ++s) {
        const smla_v4f p = *reinterpret_cast<const smla_v4f *>(part + ((s * n_pad + row) * SMLA_D + 4 * c4));
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] + p[i];
    }
    float *o = dkv + (row * dkv_stride + 4 * c4);
    smla_v4f prior = *reinterpret_cast<const smla_v4f *>(o);
#pragma unroll
    for (int i = 0; i < 4; ++i) prior[i] = prior[i] + v[i];
    *reinterpret_cast<smla_v4f *>(o) = prior;
}

// the key-owned pass's split of the 32-row blocks: a function of m, heads and s alone
struct MdbSplit {
    int64_t key_tiles, blocks, blocks_per_chunk, chunks, n_pad;
};
static bool mdb_shape_ok(int64_t m, int heads, int64_t s)
{
    return m >= 0 && heads >= 16 && heads <= DGA_SPARSE_MLA_MAX_HEADS && heads % 16 == 0 && s >= 1;
}
static bool mdb_range_ok(int64_t m, int heads, int64_t s)
{
    return s <= 0x7FFFFFFFll - 1024 && m <= (0x7FFFFFFFll - 64) * MDB_ROWS / heads;   // (the blocks fit an int, 64 of a run beyond them too)
}
static MdbSplit mdb_split(int64_t m, int heads, int64_t s)
{
    MdbSplit p;
    p.key_tiles = (s + SMLA_TILE - 1) / SMLA_TILE;
    p.blocks = (m * heads + MDB_ROWS - 1) / MDB_ROWS;
    int64_t want = (MDB_TARGET_GROUPS + p.key_tiles - 1) / p.key_tiles;
    want = want > MDB_MAX_CHUNKS ? MDB_MAX_CHUNKS : want;
    want = want > p.blocks ? p.blocks : want;
    p.blocks_per_chunk = (p.blocks + want - 1) / want;
    p.chunks = (p.blocks + p.blocks_per_chunk - 1) / p.blocks_per_chunk;
    p.n_pad = p.key_tiles * SMLA_TILE;
    return p;
}
// partials, named flags, delta: [chunks][n_pad][576] fp32, [chunks][n_pad] int32, [m heads] fp32
static int64_t mdb_bytes(const MdbSplit &p, int64_t m, int heads) { return p.chunks * p.n_pad * (SMLA_D * 4 + 4) + m * heads * 4; }

}  // namespace dga

extern "C" int64_t dga_mla_bwd_dense_workspace_bytes(int64_t m, int heads, int64_t s)
{
    using namespace dga;
    if (m < 1 || !mdb_shape_ok(m, heads, s) || !mdb_range_ok(m, heads, s)) return 0;
    return mdb_bytes(mdb_split(m, heads, s), m, heads);
}

// The checks in the family's clause order: flags, shape, (m == 0), null, alignment, range, workspace
extern "C" int dga_mla_bwd_dense(const void *q, const void *kv, const int32_t *ks, const int32_t *ke, int64_t m, int heads, int64_t s,
                                 int64_t kv_stride, double sm_scale, int flags, const void *out, const void *d_out, const float *lse, void *dq,
                                 float *dkv, int64_t dkv_stride, void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace dga;
    if (flags) return DGA_E_RANGE;
    if (!mdb_shape_ok(m, heads, s) || kv_stride < SMLA_D || dkv_stride < SMLA_D) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !kv || !ks || !ke || !out || !d_out || !lse || !dq || !dkv || !workspace) return DGA_E_NULL;
    // a thread reads 16 bytes of q, out, d_out and of a kv row at once, a lane stores 8 bytes of dq, the reduce 16 bytes of dkv
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(kv) % 16 || reinterpret_cast<uintptr_t>(out) % 16 ||
        reinterpret_cast<uintptr_t>(d_out) % 16 || reinterpret_cast<uintptr_t>(dq) % 16 || reinterpret_cast<uintptr_t>(dkv) % 16 ||
        kv_stride % 8 || dkv_stride % 4 || reinterpret_cast<uintptr_t>(ks) % 4 || reinterpret_cast<uintptr_t>(ke) % 4 ||
        reinterpret_cast<uintptr_t>(lse) % 4)
        return DGA_E_ALIGN;
    if (!mdb_range_ok(m, heads, s) || kv_stride > 0x7FFFFFFFFFFFFFFFll / 2 / s || dkv_stride > 0x7FFFFFFFFFFFFFFFll / 4 / s) return DGA_E_RANGE;
    const MdbSplit sp = mdb_split(m, heads, s);
    if (sp.key_tiles * sp.chunks > 0x7FFFFFFFll || (s * (SMLA_D / 4) + SMLA_THREADS - 1) / SMLA_THREADS > 0x7FFFFFFFll) return DGA_E_RANGE;
    if (workspace_bytes < mdb_bytes(sp, m, heads) || reinterpret_cast<uintptr_t>(workspace) % 16) return DGA_E_WORKSPACE;
    float *part = static_cast<float *>(workspace);
    int32_t *named = reinterpret_cast<int32_t *>(part + sp.chunks * sp.n_pad * SMLA_D);
    float *delta = reinterpret_cast<float *>(named + sp.chunks * sp.n_pad);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *qc = static_cast<const uint16_t *>(q), *kc = static_cast<const uint16_t *>(kv), *dc = static_cast<const uint16_t *>(d_out);
    const int64_t rows = m * heads;
    const float scale2 = static_cast<float>(sm_scale * 1.4426950408889634), scale = static_cast<float>(sm_scale);
    const dim3 block(SMLA_THREADS);
    hipLaunchKernelGGL(mdb_row_kernel, dim3(static_cast<unsigned>(sp.blocks)), block, 0, st, qc, kc, kv_stride, static_cast<int>(s), ks, ke, heads,
                       rows, sp.blocks, scale2, scale, static_cast<const uint16_t *>(out), dc, lse, static_cast<uint16_t *>(dq), delta);
    hipLaunchKernelGGL(mdb_key_kernel, dim3(static_cast<unsigned>(sp.key_tiles * sp.chunks)), block, 0, st, qc, kc, kv_stride, static_cast<int>(s),
                       ks, ke, heads, rows, static_cast<int>(sp.blocks), static_cast<int>(sp.chunks), static_cast<int>(sp.blocks_per_chunk), scale2,
                       scale, dc, lse, delta, part, named, sp.n_pad);
    hipLaunchKernelGGL(mdb_reduce_kernel, dim3(static_cast<unsigned>((s * (SMLA_D / 4) + SMLA_THREADS - 1) / SMLA_THREADS)), block, 0, st, part,
                       named, static_cast<int>(sp.chunks), sp.n_pad, static_cast<int>(s), dkv, dkv_stride);
    return record_hip(hipGetLastError());
}
