// The backward of the lightning indexer's scoring over the selected keys (dga_mqa_logits.hip is the forward): dq, dk and d_weights from
// the derivative of a loss at the logits indexer_topk selected.
//   dga_fp8_mqa_logits_bwd   q [M, H, 128] e4m3, k [N, 128] e4m3, kscale [N], weights [M, H] as the forward's; indices int32 [M, topk]
//                            (+ offsets int32 [M]) by sparse MLA's validity rule; d_logits fp32 [M, topk]
//                            -> dq fp32 [M, H, 128] (written), d_weights fp32 [M, H] (written), dk fp32 [N, 128] (rows dk_stride apart; added into)
//     over the valid positions j of token m, r_j the row, s_hj = sum_d q[m,h,d] k[r_j,d] on the code values, mask_hj = s_hj > 0:
//     d_weights[m,h] = sum_j d_logits[m,j] kscale[r_j] (mask_hj ? s_hj : 0)
//     dq[m,h,:]      = sum_j Gq_hj k[r_j,:]       Gk_hj = mask_hj ? weights[m,h] d_logits[m,j] : +0,   Gq_hj = Gk_hj kscale[r_j]
//     dk[r_j,:]     += sum_h Gk_hj q[m,h,:]
// One workgroup of four waves owns one token and all its H heads (H a template parameter: 32 or 64).  LDS: the token's codes converted
// exactly to bf16 (mqa_cvt8) [H][128] in rows of 288 B (72 dwords = 8 mod 64: eight consecutive rows start on eight distinct multiples of
// eight banks, for the straight and for the transposed reads), the gathered tile of 64 positions [64][128] alike, the bf16 images of Gk,
// Gq and their residuals [head][key] in rows of 160 B (40 dwords), the tile's rows, d_logits and kscale, and the waves' head sums:
// 79 616 B at H = 64, 49 408 B at H = 32.  The gather is sparse MLA's: eight threads a row (16 of its 128 bytes each; here two rows a
// thread, positions p and p + 32 of the tile), one tile read ahead in registers, the index one tile further; an invalid position is staged
// as zero codes, row -1, d_logits and kscale +0 -- its d_logits element is never read.
// Per tile of 64 positions, wave w (a tile without a valid position is skipped by the whole workgroup):
//   A  key subtile w against every head tile: S^T [16 keys x 16 heads] = four chained v_mfma_f32_16x16x32_bf16 over d ascending from zero,
//      the key rows the A operand (read once), the q image the B operand; lane l holds head l & 15 and keys 4 (l >> 4) + i.  On the fp32
//      accumulator: mask = live && s > 0, c = d_logits kscale, g = weights d_logits; d_weights' share fma(c, mask ? s : 0, acc), keys
//      ascending; Gk = mask ? g : +0 and Gq = Gk kscale rounded to bf16 (RNE), 8 bytes a lane into the two images -- and their residuals
//      Gk - bf16(Gk), Gq - bf16(Gq) (exact in fp32), rounded to bf16 likewise, into two more: a bf16's rounding alone is 2^-8 of the value
//      in the worst case, twice what the operator's bounds give it (2^-9); with the residual the two products carry G to 2^-16
//   B  (head tile w % (H / 16), column tiles H / 8 (w / (H / 16)) ..)  dQ^T += K^T Gq^T: two MFMAs a column tile (keys 0 .. 31, 32 .. 63)
//      and two more for the residual, K^T by pairs of ds_read_b64_tr_b16 of the tile, Gq^T from the images as they stand; H / 2 fp32
//      accumulators a lane, held across tiles
//   C  key subtile w, the eight column tiles: dK [16 keys x 16 columns] from +0 = Gk^T Q over the H heads (one MFMA per 32 heads, and one
//      for the residual), both operands by transposed reads, then global_atomic_add_f32 of the lane's four keys' values (sixteen lanes:
//      64 contiguous bytes of a row), none for a row of -1
// At the end dq is the accumulators as they stand (weights is inside G), 16 bytes a lane; d_weights is reduced over the lane groups
// (lane ^ 16, lane ^ 32), then over the four waves through LDS as ((w0 + w1) + w2) + w3.
// dq and d_weights have one writer per element and a fixed order of summation: two runs give the same bytes.  dk does not: the order in
// which the atomic adds reach an element varies from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_mqa_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int MQB_THREADS = 256;
constexpr int MQB_D = DGA_MQA_LOGITS_HEAD_DIM;               // 128
constexpr int MQB_TILE = DGA_MQA_LOGITS_BWD_TILE;            // positions of one gathered tile: 64
constexpr int MQB_ROW_BYTES = MQB_D * 2 + 32;                // 288: a head's or a key's 128 bf16
constexpr int MQB_W_ROW_BYTES = MQB_TILE * 2 + 32;           // 160: a head's 64 weights (Gk or Gq) of the tile
constexpr int MQB_CTILES = MQB_D / 16;                       // column tiles of dq and dk: 8
static_assert(MQB_D == 128 && MQB_TILE == 64 && MQB_TILE * 4 == MQB_THREADS, "the kernel's geometry");

typedef short mqb_v4s __attribute__((ext_vector_type(4)));
typedef __bf16 mqb_v4bf __attribute__((ext_vector_type(4)));
typedef uint32_t mqb_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t mqb_lds(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char *)p;
}
// one 16 x 32 (or 32 x 16) bf16 fragment by two transposed reads: the blocks at `addr` and sixteen image rows (`half` bytes) below it
// (lane 4 r + c of a group gives row r, columns 4 c .. of a block of 4 x 16; the fragment's k index 8 g + i stands for row 4 g + i,
// 8 g + 4 + i for row 16 + 4 g + i)
__device__ __forceinline__ mqa_v8bf mqb_read_tr(uint32_t addr, int half)
{
    const mqb_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<mqb_v4s __attribute__((address_space(3))) *>(addr));
    const mqb_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<mqb_v4s __attribute__((address_space(3))) *>(addr + half));
    return __builtin_bit_cast(mqa_v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// 16 e4m3 codes -> 16 bf16 (exact), 32 bytes at dst
__device__ __forceinline__ void mqb_put16(unsigned char *dst, const uint4 &raw)
{
    reinterpret_cast<mqa_v4i *>(dst)[0] = mqa_cvt8(mqa_v2i{(int)raw.x, (int)raw.y});
    reinterpret_cast<mqa_v4i *>(dst)[1] = mqa_cvt8(mqa_v2i{(int)raw.z, (int)raw.w});
}

template <int H>
__global__ void __launch_bounds__(MQB_THREADS) mqa_logits_bwd_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ k,
                                                                     const float *__restrict__ kscale, const float *__restrict__ weights,
                                                                     const int32_t *__restrict__ indices, int64_t idx_stride,
                                                                     const int32_t *__restrict__ offsets, const float *__restrict__ d_logits,
                                                                     int64_t dl_stride, int topk, int64_t n_rows, int64_t tokens, int64_t chunk,
                                                                     float *__restrict__ dq, float *__restrict__ dk, int64_t dk_stride,
                                                                     float *__restrict__ d_weights)
{
    constexpr int HT = H / 16;                 // head tiles
    constexpr int NCT = 2 * HT;                // column tiles of dq one wave owns: 8 (H = 64) or 4
    constexpr int HK = H / 32;                 // k steps of a product contracted over the heads
    static_assert(H == 32 || H == 64, "the head counts of the indexer");
    __shared__ __attribute__((aligned(16))) unsigned char tile[MQB_TILE * MQB_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[H * MQB_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char wimg[4][H * MQB_W_ROW_BYTES];           // bf16 [head][key]: Gk, Gq, their residuals
    __shared__ __attribute__((aligned(16))) int32_t rowidx[MQB_TILE];                             // the k row of a position, -1: invalid
    __shared__ __attribute__((aligned(16))) float dl_s[MQB_TILE], ks_s[MQB_TILE];                 // its d_logits and kscale, +0 when invalid
    __shared__ float dw_s[4][H];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the token of this workgroup: the grid is walked XCD by XCD (workgroup i runs on XCD i % 8), as sparse MLA's
    int64_t t = blockIdx.x;
    t = (t & 7) * chunk + (t >> 3);
    if (t >= tokens) return;                                 // (the whole workgroup alike, before any barrier)

    const int32_t *irow = indices + t * idx_stride;
    const float *drow = d_logits + t * dl_stride;
    const int64_t shift = offsets ? (int64_t)offsets[t] : 0;
    const int tiles = (topk + MQB_TILE - 1) / MQB_TILE;

    // the gather: eight threads a position, two positions a thread (p and p + 32 of the tile), the index one tile ahead of its row
    const int gpos = tid >> 3, gsub = tid & 7;
    auto ask = [&](int tl, int half) -> int32_t {
        const int64_t pos = (int64_t)tl * MQB_TILE + 32 * half + gpos;
        return irow[pos < topk ? pos : topk - 1];
    };
    auto row_of = [&](int tl, int half, int32_t i) -> int32_t {
        const int64_t pos = (int64_t)tl * MQB_TILE + 32 * half + gpos;
        const int64_t r = (int64_t)i + shift;
        return (pos < topk && i >= 0 && r >= 0 && r < n_rows) ? (int32_t)r : -1;      // (n_rows < 2^31)
    };
    uint4 raw[2];
    float dlv[2], ksv[2];
    int32_t row[2], asked[2];
    auto fetch = [&](int tl) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            row[half] = row_of(tl, half, asked[half]);
            raw[half] = uint4{0, 0, 0, 0};
            dlv[half] = ksv[half] = 0.f;
            if (row[half] >= 0) {
                raw[half] = *reinterpret_cast<const uint4 *>(k + (int64_t)row[half] * MQB_D + gsub * 16);
                if (gsub == 0) {
                    ksv[half] = kscale[row[half]];
                    dlv[half] = drow[(int64_t)tl * MQB_TILE + 32 * half + gpos];
                }
            }
        }
    };
    asked[0] = ask(0, 0), asked[1] = ask(0, 1);
    fetch(0);
    asked[0] = ask(1, 0), asked[1] = ask(1, 1);

    // the prologue: the token's codes to bf16, 16 of them a thread and step
    for (int c = tid; c < H * 8; c += MQB_THREADS)
        mqb_put16(qimg + (c >> 3) * MQB_ROW_BYTES + (c & 7) * 32, *reinterpret_cast<const uint4 *>(q + (t * H + (c >> 3)) * MQB_D + (c & 7) * 16));
    float wr[HT], accw[HT];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
        wr[ht] = weights[t * H + 16 * ht + hl];              // (A: the lane's heads)
        accw[ht] = 0.f;
    }

    const int htb = wave % HT, ct0 = NCT * (wave / HT);     // B: the wave's head tile and its first column tile
    mqa_v4f accq[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j) accq[j] = mqa_v4f{0.f, 0.f, 0.f, 0.f};

    // LDS addresses of the lane's reads.  A: rows of K and q at bytes 64 s + 16 g.  Transposed reads: of the tile for B, of the Gk and the
    // q image for C.
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    const unsigned char *ka_at = tile + (16 * wave + hl) * MQB_ROW_BYTES + 16 * g;
    const unsigned char *qa_at = qimg + hl * MQB_ROW_BYTES + 16 * g;
    const int wa_at = hl * MQB_W_ROW_BYTES + 2 * (16 * wave + 4 * g);                               // A writes its four keys here
    const uint32_t kt_addr = mqb_lds(tile) + trow * MQB_ROW_BYTES + tcol + 32 * ct0;
    const int wb_at = (16 * htb + hl) * MQB_W_ROW_BYTES + 8 * g;                                    // B's Gq^T: keys 4 g .. and, 32 bytes on, 16 + 4 g ..
    const uint32_t qt_addr = mqb_lds(qimg) + trow * MQB_ROW_BYTES + tcol;
    const uint32_t gt_addr = mqb_lds(&wimg[0][0]) + trow * MQB_W_ROW_BYTES + tcol + 2 * (16 * wave);  // C's Gk^T: keys 16 w ..

#pragma unroll 1
    for (int tl = 0; tl < tiles; ++tl) {
        // the staged tile goes to LDS
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            mqb_put16(tile + (32 * half + gpos) * MQB_ROW_BYTES + gsub * 32, raw[half]);
            if (gsub == 0) {
                rowidx[32 * half + gpos] = row[half];
                dl_s[32 * half + gpos] = dlv[half];
                ks_s[32 * half + gpos] = ksv[half];
            }
        }
        __syncthreads();
        // the next tile's rows are asked for now and written after this tile's products; the indices of the one after it behind them
        fetch(tl + 1);
        asked[0] = ask(tl + 2, 0), asked[1] = ask(tl + 2, 1);

        if (__ballot(rowidx[lane] >= 0) != 0) {              // (the same 64 entries in every wave: the whole workgroup alike)
            // ---- A ----
            {
                const mqa_v4i rv = *reinterpret_cast<const mqa_v4i *>(&rowidx[16 * wave + 4 * g]);
                const mqa_v4f dl4 = *reinterpret_cast<const mqa_v4f *>(&dl_s[16 * wave + 4 * g]);
                const mqa_v4f ks4 = *reinterpret_cast<const mqa_v4f *>(&ks_s[16 * wave + 4 * g]);
                mqa_v4i ka[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) ka[s] = *reinterpret_cast<const mqa_v4i *>(ka_at + 64 * s);
                float c4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) c4[i] = dl4[i] * ks4[i];
#pragma unroll
                for (int ht = 0; ht < HT; ++ht) {
                    mqa_v4f sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const mqa_v4i qq = *reinterpret_cast<const mqa_v4i *>(qa_at + 16 * ht * MQB_ROW_BYTES + 64 * s);
                        sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mqa_v8bf, ka[s]), __builtin_bit_cast(mqa_v8bf, qq), sv, 0, 0, 0);
                    }
                    mqb_v4bf gk, gq, gkl, gql;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const bool mask = rv[i] >= 0 && sv[i] > 0.f;
                        accw[ht] = __builtin_fmaf(c4[i], mask ? sv[i] : 0.f, accw[ht]);
                        const float gg = wr[ht] * dl4[i];
                        const float gkf = mask ? gg : 0.f;
                        const float gqf = gkf * ks4[i];
                        gk[i] = (__bf16)gkf;
                        gq[i] = (__bf16)gqf;
                        gkl[i] = (__bf16)(gkf - (float)gk[i]);             // (the difference is exact in fp32)
                        gql[i] = (__bf16)(gqf - (float)gq[i]);
                    }
                    *reinterpret_cast<uint2 *>(&wimg[0][16 * ht * MQB_W_ROW_BYTES + wa_at]) = __builtin_bit_cast(uint2, gk);
                    *reinterpret_cast<uint2 *>(&wimg[1][16 * ht * MQB_W_ROW_BYTES + wa_at]) = __builtin_bit_cast(uint2, gq);
                    *reinterpret_cast<uint2 *>(&wimg[2][16 * ht * MQB_W_ROW_BYTES + wa_at]) = __builtin_bit_cast(uint2, gkl);
                    *reinterpret_cast<uint2 *>(&wimg[3][16 * ht * MQB_W_ROW_BYTES + wa_at]) = __builtin_bit_cast(uint2, gql);
                }
            }
            __syncthreads();

            // ---- B ----
            {
                mqa_v8bf gqb[2][2];                               // [Gq, its residual][keys 0 .. 31, 32 .. 63]
#pragma unroll
                for (int part = 0; part < 2; ++part) {
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const uint2 w0 = *reinterpret_cast<const uint2 *>(&wimg[1 + 2 * part][wb_at + 64 * half]);
                        const uint2 w1 = *reinterpret_cast<const uint2 *>(&wimg[1 + 2 * part][wb_at + 64 * half + 32]);
                        gqb[part][half] = __builtin_bit_cast(mqa_v8bf, (mqb_v4u{w0.x, w0.y, w1.x, w1.y}));
                    }
                }
#pragma unroll
                for (int j = 0; j < NCT; ++j) {
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const mqa_v8bf kt = mqb_read_tr(kt_addr + 32 * j + 32 * half * MQB_ROW_BYTES, 16 * MQB_ROW_BYTES);
                        accq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, gqb[0][half], accq[j], 0, 0, 0);
                        accq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, gqb[1][half], accq[j], 0, 0, 0);
                    }
                }
            }

            // ---- C ----
            {
                mqa_v8bf ga[2][HK];                               // [Gk, its residual][32 heads]
#pragma unroll
                for (int part = 0; part < 2; ++part) {
#pragma unroll
                    for (int kc = 0; kc < HK; ++kc)
                        ga[part][kc] = mqb_read_tr(gt_addr + 2 * part * (uint32_t)sizeof(wimg[0]) + 32 * kc * MQB_W_ROW_BYTES, 16 * MQB_W_ROW_BYTES);
                }
                const mqa_v4i rv = *reinterpret_cast<const mqa_v4i *>(&rowidx[16 * wave + 4 * g]);
                float *dst[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[i] = dk + ((int64_t)(rv[i] >= 0 ? rv[i] : 0) * dk_stride + hl);
#pragma unroll
                for (int ct = 0; ct < MQB_CTILES; ++ct) {
                    mqa_v4f r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kc = 0; kc < HK; ++kc) {
                        const mqa_v8bf qt = mqb_read_tr(qt_addr + 32 * kc * MQB_ROW_BYTES + 32 * ct, 16 * MQB_ROW_BYTES);
                        r = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[0][kc], qt, r, 0, 0, 0);
                        r = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[1][kc], qt, r, 0, 0, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (rv[i] >= 0) unsafeAtomicAdd(dst[i] + 16 * ct, r[i]);
                }
            }
        }
        __syncthreads();
    }

    float *orow = dq + ((t * H + 16 * htb + hl) * MQB_D + 16 * ct0 + 4 * g);
#pragma unroll
    for (int j = 0; j < NCT; ++j) *reinterpret_cast<mqa_v4f *>(orow + 16 * j) = accq[j];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
        float v = accw[ht];
        v = v + __shfl_xor(v, 16, 64);
        v = v + __shfl_xor(v, 32, 64);
        if (g == 0) dw_s[wave][16 * ht + hl] = v;
    }
    __syncthreads();
    if (tid < H) d_weights[t * H + tid] = ((dw_s[0][tid] + dw_s[1][tid]) + dw_s[2][tid]) + dw_s[3][tid];
}

}  // namespace dga

// The checks in the documented clause order: shape, (m == 0), null, alignment, range
extern "C" int dga_fp8_mqa_logits_bwd(const void *q, const void *k, const float *kscale, const float *weights, const int32_t *indices,
                                      const int32_t *index_offsets, const float *d_logits, int64_t m, int64_t n, int heads, int head_dim,
                                      int64_t topk, int64_t idx_stride, int64_t dl_stride, float *dq, float *dk, int64_t dk_stride,
                                      float *d_weights, void *stream)
{
    using namespace dga;
    if (m < 0 || n < 1 || head_dim != MQB_D || (heads != 32 && heads != 64) || topk < 1 || idx_stride < topk || dl_stride < topk ||
        dk_stride < MQB_D)
        return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !k || !kscale || !weights || !indices || !d_logits || !dq || !dk || !d_weights) return DGA_E_NULL;
    // a thread reads 16 codes at once and stores four values of dq; the rows of dk must keep a lane's column 4-byte aligned
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(k) % 16 || reinterpret_cast<uintptr_t>(dq) % 16 ||
        reinterpret_cast<uintptr_t>(dk) % 16 || dk_stride % 4 || reinterpret_cast<uintptr_t>(kscale) % 4 ||
        reinterpret_cast<uintptr_t>(weights) % 4 || reinterpret_cast<uintptr_t>(indices) % 4 || reinterpret_cast<uintptr_t>(d_logits) % 4 ||
        reinterpret_cast<uintptr_t>(d_weights) % 4 || (index_offsets && reinterpret_cast<uintptr_t>(index_offsets) % 4))
        return DGA_E_ALIGN;
    if (n > 0x7FFFFFFFll || topk > 0x7FFFFFFFll - MQB_TILE || dk_stride > 0x7FFFFFFFFFFFFFFFll / 4 / n || m > 0x7FFFFFFFll - 8)
        return DGA_E_RANGE;
    const int64_t chunk = (m + 7) / 8;
    const dim3 grid(static_cast<unsigned>(chunk * 8)), block(MQB_THREADS);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(q),
                           static_cast<const uint8_t *>(k), kscale, weights, indices, idx_stride, index_offsets, d_logits, dl_stride,
                           static_cast<int>(topk), n, m, chunk, dq, dk, dk_stride, d_weights);
    };
    if (heads == 64) launch(mqa_logits_bwd_kernel<64>);
    else launch(mqa_logits_bwd_kernel<32>);
    return record_hip(hipGetLastError());
}
