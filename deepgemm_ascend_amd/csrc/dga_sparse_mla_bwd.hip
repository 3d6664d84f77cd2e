// The backward of sparse MLA attention (dga_sparse_mla.hip is the forward): dq and dkv from d_out, the forward's out and lse.
//   dga_sparse_mla_bwd   q, kv, indices, offsets as the forward's; out, d_out bf16 [m, heads, 512], lse fp32 [m, heads]
//                        -> dq bf16 [m, heads, 576] (written), dkv fp32 [s, 576] (rows dkv_stride apart; added into)
//     over the valid positions j of token t, r_j the row (the forward's rule), L2E = (float)log2 e, scale2 = (float)(sm_scale L2E):
//     p_j     = exp2(S_j scale2 - lse[t, h] L2E)           S_j = sum_d q[t, h, d] kv[r_j, d]
//     delta   = sum_c out[t, h, c] d_out[t, h, c]          dP_j = sum_c d_out[t, h, c] kv[r_j, c]         (c < 512)
//     dS_j    = ((float)sm_scale p_j) (dP_j - delta)
//     dq[t, h, :]     = sum_j bf16(dS_j) kv[r_j, :576]
//     dkv[r_j, :576] += sum_h bf16(dS_j) q[t, h, :]        dkv[r_j, :512] += sum_h bf16(p_j) d_out[t, h, :]
// One workgroup of four waves owns one token and a block of 32 heads (the forward's 64 do not fit: q and d_out of the block both have to
// stand in LDS, each read straight -- the B operand of S^T = K Q^T and dP^T = K dO^T -- and transposed -- the B operand of the products
// contracted over heads).  LDS: q 32 x 1184 B, d_out 32 x 1056 B (264 dwords = 8 mod 64: the same freedom of bank conflicts as the tile's
// 40), the gathered tile 32 x 1184 B, the bf16 images of P and dS [head][key] in rows of 80 B, the tile's rows and the block's delta and
// lse L2E: 115 072 B, one workgroup a CU.  The gather is the forward's: eight threads a row, one tile read ahead in registers, an invalid
// position staged as zeros and marked -1 in the list of rows.
// Prologue: q and d_out to LDS (rows of heads beyond `heads` as zeros, so that the products over 32 heads need no mask), delta by eight
// threads a head -- thread i of them the 16-byte chunks i + 8 c, c and the element ascending, fp32, nothing contracted -- and the lane tree
// (lane ^ 1, ^ 2, ^ 4): a fixed order.
// Per tile of 32 positions, wave w:
//   A  (head tile w & 1, key subtile w >> 1)  S^T and dP^T [16 keys x 16 heads]: 18 + 16 chained v_mfma_f32_16x16x32_bf16, K the A operand
//      (one ds_read_b128 serves both chains), q and d_out the B operands; lane l holds head l & 15 and keys 4 (l >> 4) + i: p and dS as above,
//      +0 at an invalid position whatever lse and delta hold (a select, not a product), rounded to bf16 (RNE), 8 bytes a lane into the images
//   B  (head tile w & 1, column tiles 18 (w >> 1) ..)  dQ^T += K^T dS^T: one MFMA a column tile over the 32 keys, K^T by the forward's two
//      ds_read_b64_tr_b16, dS^T from the image as it stands (keys 4 g .., 16 + 4 g ..); 72 fp32 accumulators a lane, held across tiles
//   C  (key subtile w & 1, column tiles 18 (w >> 1) ..)  dKV [16 keys x 16 columns] from +0: dS^T Q over the 32 heads and, for columns
//      < 512, P^T dO into the same accumulator -- dS^T and P^T by transposed reads of the images, Q and dO by transposed reads of theirs --
//      then global_atomic_add_f32 of the lane's four keys' values (sixteen lanes: 64 contiguous bytes of a row), none for a row of -1
// At the end dq = RNE_bf16(acc), 8 bytes a lane.  A wave whose head tile lies beyond `heads` (heads = 16, 48, ..) skips A, B and the store.
// dq has one writer per element and a fixed order of summation: two runs give the same bytes.  dkv does not: the order in which the
// atomic adds reach an element varies from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

// DKV: with phase C and its atomic adds onto dkv (dga_sparse_mla_bwd); without, dq alone by the same text in the same order
// (dga_sparse_mla_bwd_det's first pass: dkv is not looked at)
template <bool DKV>
__global__ void __launch_bounds__(SMLA_THREADS) sparse_mla_bwd_kernel(const uint16_t *__restrict__ q, const void *__restrict__ kv, int64_t kv_stride,
                                                                      int64_t s_rows, const int32_t *__restrict__ indices, int64_t idx_stride,
                                                                      int topk, const int32_t *__restrict__ offsets, int heads, int head_blocks,
                                                                      int64_t blocks, int64_t chunk, float scale2, float sm_scale,
                                                                      const uint16_t *__restrict__ out, const uint16_t *__restrict__ d_out,
                                                                      const float *__restrict__ lse, uint16_t *__restrict__ dq,
                                                                      float *__restrict__ dkv, int64_t dkv_stride)
{
    const SmlaBf16Rows cache = SmlaBf16Rows::make(kv, kv_stride, s_rows, 0, 0);
    __shared__ __attribute__((aligned(16))) unsigned char tile[SMLA_TILE * SMLA_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[SMLB_HEADS * SMLA_ROW_BYTES];      // the block's q, one row a head
    __shared__ __attribute__((aligned(16))) unsigned char doimg[SMLB_HEADS * SMLB_DO_ROW_BYTES];  // ... and its d_out
    __shared__ __attribute__((aligned(16))) unsigned char wimg[2][SMLB_HEADS * SMLB_W_ROW_BYTES]; // bf16 [head][key]: 0 the tile's p, 1 its dS
    __shared__ __attribute__((aligned(16))) int32_t rowidx[SMLA_TILE];                            // the kv row of a position, -1: invalid
    __shared__ float delta_s[SMLB_HEADS], lse2_s[SMLB_HEADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the logical block of this workgroup, as in the forward; chunk == 0: the grid is taken as it is
    int64_t block = blockIdx.x;
    if (chunk) block = (block & 7) * chunk + (block >> 3);
    if (block >= blocks) return;                             // (the whole workgroup alike, before any barrier)
    const int64_t t = block / head_blocks;
    const int hb0 = (int)(block % head_blocks) * SMLB_HEADS;
    const int wlo = wave & 1, whi = wave >> 1;
    const bool computes = hb0 + 16 * wlo < heads;            // (A and B: a head tile beyond the last head has nothing to compute)

    const int32_t *irow = indices + t * idx_stride;
    const int64_t shift = offsets ? (int64_t)offsets[t] : 0;
    const int tiles = (topk + SMLA_TILE - 1) / SMLA_TILE;

    // the forward's gather: eight threads a position, the index one tile ahead of its row
    const int gpos = tid >> 3, gsub = tid & 7;
    auto ask = [&](int tl) -> int32_t {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        return irow[pos < topk ? pos : topk - 1];
    };
    auto row_of = [&](int tl, int32_t i) -> int32_t {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        const int64_t r = (int64_t)i + shift;
        return (pos < topk && i >= 0 && r >= 0 && r < cache.s_rows) ? (int32_t)r : -1;   // (s_rows < 2^31)
    };
    auto fetch = [&](int32_t r, uint4 (&v)[SMLA_STAGE]) {
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) v[c] = uint4{0, 0, 0, 0};
        if (r >= 0) SmlaBf16Rows::load(cache.at(r, gsub), gsub, v);
    };

    uint4 raw[SMLA_STAGE];
    int32_t row = row_of(0, ask(0));
    fetch(row, raw);
    int32_t asked = ask(1);

    // the prologue: head hb0 + gpos by the eight threads tid % 8
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
        // the images of p and dS start as zeros: the rows of a head tile that computes nothing are never written
        for (int i = tid; i < (int)sizeof(wimg) / 16; i += SMLA_THREADS) reinterpret_cast<uint4 *>(&wimg[0][0])[i] = uint4{0, 0, 0, 0};
    }
    __syncthreads();
    const float delta = delta_s[16 * wlo + hl], lse2 = lse2_s[16 * wlo + hl];   // (A: the lane's head)

    smla_v4f accq[SMLB_WAVE_TILES];
#pragma unroll
    for (int j = 0; j < SMLB_WAVE_TILES; ++j) accq[j] = smla_v4f{0.f, 0.f, 0.f, 0.f};

    // LDS addresses of the lane's reads.  A: rows of K, q and d_out at bytes 64 s + 16 g.  Transposed reads (lane 4 r + c of a group gives
    // row r, columns 4 c .. of a block of 4 x 16; the fragment's k index 8 g + i stands for row 4 g + i, 8 g + 4 + i for row 16 + 4 g + i):
    // of the tile for B, of the q and d_out images and of the weight images for C.
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    const uint32_t ka_addr = smlb_lds(tile) + (16 * whi + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t qa_addr = smlb_lds(qimg) + (16 * wlo + hl) * SMLA_ROW_BYTES + 16 * g;
    const uint32_t da_addr = smlb_lds(doimg) + (16 * wlo + hl) * SMLB_DO_ROW_BYTES + 16 * g;
    const uint32_t wa_at = (16 * wlo + hl) * SMLB_W_ROW_BYTES + 2 * (16 * whi + 4 * g);          // A writes its four keys here
    const uint32_t kt_addr = smlb_lds(tile) + trow * SMLA_ROW_BYTES + tcol + 32 * (SMLB_WAVE_TILES * whi);
    const uint32_t wb_at = (16 * wlo + hl) * SMLB_W_ROW_BYTES + 8 * g;                           // B's dS^T: keys 4 g .. and, 32 bytes on, 16 + 4 g ..
    const uint32_t qt_addr = smlb_lds(qimg) + trow * SMLA_ROW_BYTES + tcol + 32 * (SMLB_WAVE_TILES * whi);
    const uint32_t dt_addr = smlb_lds(doimg) + trow * SMLB_DO_ROW_BYTES + tcol + 32 * (SMLB_WAVE_TILES * whi);
    const uint32_t wt_at = trow * SMLB_W_ROW_BYTES + tcol + 2 * (16 * wlo);                      // C's P^T and dS^T: keys 16 (w & 1) ..

#pragma unroll 1
    for (int tl = 0; tl < tiles; ++tl) {
        // the staged tile goes to LDS
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(tile + gpos * SMLA_ROW_BYTES + SmlaBf16Rows::lds_at(c, gsub)) = raw[c];
        if (gsub == 0) rowidx[gpos] = row;
        __syncthreads();
        // the next tile's rows are asked for now and written after this tile's products; the indices of the one after it behind them
        row = row_of(tl + 1, asked);
        fetch(row, raw);
        asked = ask(tl + 2);

        // ---- A ----
        if (computes) {
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
        }
        __syncthreads();

        // ---- B ----
        if (computes) {
            const uint2 w0 = *reinterpret_cast<const uint2 *>(&wimg[1][wb_at]), w1 = *reinterpret_cast<const uint2 *>(&wimg[1][wb_at + 32]);
            const smla_v8bf dsb = __builtin_bit_cast(smla_v8bf, (smla_v4u{w0.x, w0.y, w1.x, w1.y}));
            smla_v8bf kt[2][SMLB_GROUP];
            auto read_b = [&](int grp) {
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j) kt[grp & 1][j] = smlb_read_tr(kt_addr + 32 * (SMLB_GROUP * grp + j), 16 * SMLA_ROW_BYTES);
            };
            read_b(0);
#pragma unroll
            for (int grp = 0; grp < SMLB_WAVE_TILES / SMLB_GROUP; ++grp) {
                if (grp + 1 < SMLB_WAVE_TILES / SMLB_GROUP) read_b(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j)
                    accq[SMLB_GROUP * grp + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt[grp & 1][j], dsb, accq[SMLB_GROUP * grp + j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- C ----
        if constexpr (DKV) {
            const smla_v8bf pa = smlb_read_tr(smlb_lds(&wimg[0][0]) + wt_at, 16 * SMLB_W_ROW_BYTES);
            const smla_v8bf dsa = smlb_read_tr(smlb_lds(&wimg[1][0]) + wt_at, 16 * SMLB_W_ROW_BYTES);
            const smlb_v4i rv = *reinterpret_cast<const smlb_v4i *>(&rowidx[16 * wlo + 4 * g]);
            float *dst[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dst[i] = dkv + ((int64_t)(rv[i] >= 0 ? rv[i] : 0) * dkv_stride + 16 * (SMLB_WAVE_TILES * whi) + hl);
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
                smla_v4f r[SMLB_GROUP];
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j) {
                    r[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, qt[grp & 1][j], (smla_v4f{0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
                    if (SMLB_WAVE_TILES * whi + SMLB_GROUP * grp + j < SMLA_CTILES)
                        r[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, dt[grp & 1][j], r[j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < SMLB_GROUP; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (rv[i] >= 0) unsafeAtomicAdd(dst[i] + 16 * (SMLB_GROUP * grp + j), r[j][i]);
                }
            }
        }
        __syncthreads();
    }

    if (!computes) return;
    uint16_t *drow = dq + ((t * heads + hb0 + 16 * wlo + hl) * SMLA_D + 16 * (SMLB_WAVE_TILES * whi) + 4 * g);
#pragma unroll
    for (int j = 0; j < SMLB_WAVE_TILES; ++j) {
        smla_v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)accq[j][i];
        *reinterpret_cast<uint2 *>(drow + 16 * j) = __builtin_bit_cast(uint2, o);
    }
}

// The forward's call and its checks first (check_sparse_mla, in the documented order), then what a backward entry adds, in the same order
int check_sparse_mla_bwd(const SmlaBwdCall &b, bool *launch)
{
    const SmlaSource src{false, b.kv, b.s, 1, b.kv_stride};
    const int rc = check_sparse_mla(b.c, src, false, nullptr, nullptr, launch);
    if (!*launch) return rc;
    *launch = false;
    if (b.dkv_stride < SMLA_D) return DGA_E_SHAPE;
    if (!b.out || !b.d_out || !b.lse || !b.dq || !b.dkv) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(b.out) % 16 || reinterpret_cast<uintptr_t>(b.d_out) % 16 || reinterpret_cast<uintptr_t>(b.dq) % 16 ||
        reinterpret_cast<uintptr_t>(b.dkv) % 16 || reinterpret_cast<uintptr_t>(b.lse) % 4 || b.dkv_stride % 4)
        return DGA_E_ALIGN;
    const int head_blocks = (b.c.heads + SMLB_HEADS - 1) / SMLB_HEADS;
    if (b.c.m > (0x7FFFFFFFll - 8) / head_blocks || b.dkv_stride > 0x7FFFFFFFFFFFFFFFll / 4 / b.s) return DGA_E_RANGE;
    *launch = true;
    return DGA_OK;
}

int launch_sparse_mla_bwd(const SmlaBwdCall &b, bool with_dkv)
{
    const int head_blocks = (b.c.heads + SMLB_HEADS - 1) / SMLB_HEADS;
    const int64_t blocks = b.c.m * head_blocks;
    const bool linear = (b.c.flags & DGA_SPARSE_MLA_LINEAR_GRID) != 0;
    const int64_t chunk = linear ? 0 : (blocks + 7) / 8;
    const int64_t grid = linear ? blocks : chunk * 8;
    hipLaunchKernelGGL(with_dkv ? sparse_mla_bwd_kernel<true> : sparse_mla_bwd_kernel<false>, dim3(static_cast<unsigned>(grid)),
                       dim3(SMLA_THREADS), 0, static_cast<hipStream_t>(b.c.stream), static_cast<const uint16_t *>(b.c.q), b.kv, b.kv_stride, b.s,
                       b.c.indices, b.c.idx_stride, static_cast<int>(b.c.topk), b.c.index_offsets, b.c.heads, head_blocks, blocks, chunk,
                       static_cast<float>(b.c.sm_scale * 1.4426950408889634), static_cast<float>(b.c.sm_scale),
                       static_cast<const uint16_t *>(b.out), static_cast<const uint16_t *>(b.d_out), b.lse, static_cast<uint16_t *>(b.dq), b.dkv,
                       b.dkv_stride);
    return record_hip(hipGetLastError());
}

}  // namespace dga

extern "C" int dga_sparse_mla_bwd(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                  int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, const void *out,
                                  const void *d_out, const float *lse, void *dq, float *dkv, int64_t dkv_stride, void *stream)
{
    using namespace dga;
    const SmlaBwdCall b{{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream}, kv, s, kv_stride, out, d_out, lse, dq,
                        dkv, dkv_stride};
    bool launch;
    const int rc = check_sparse_mla_bwd(b, &launch);
    return launch ? launch_sparse_mla_bwd(b, true) : rc;
}
