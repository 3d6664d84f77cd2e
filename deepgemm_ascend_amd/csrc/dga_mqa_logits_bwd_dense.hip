// The backward of the lightning indexer's scoring over ALL keys of a token's range (the dense warm-up stage; dga_mqa_logits_bwd.hip is the
// sparse stage's, over the selected keys): dq, dk and d_weights from the derivative of a loss at fp8_mqa_logits' in-range logits.
//   dga_fp8_mqa_logits_bwd_dense   q [M, H, 128] e4m3, k [N, 128] e4m3, kscale [N], weights [M, H], ks / ke int32 [M] as the forward's;
//                                  d_logits fp32 [M, N] (rows dl_stride apart) -> dq fp32 [M, H, 128] (written), d_weights fp32 [M, H]
//                                  (written), dk fp32 [N, 128] (rows dk_stride apart; added into)
//     over the keys n of token m's range [clamp(ks[m]), clamp(ke[m])), s_hn = sum_d q[m,h,d] k[n,d] on the code values, mask_hn = s_hn > 0:
//     d_weights[m,h] = sum_n d_logits[m,n] kscale[n] (mask_hn ? s_hn : 0)
//     dq[m,h,:]      = sum_n Gq_hn k[n,:]        Gk_hn = mask_hn ? weights[m,h] d_logits[m,n] : +0,   Gq_hn = Gk_hn kscale[n]
//     dk[n,:]       += sum_m sum_h Gk_hn q[m,h,:]
// The arithmetic is the sparse backward's: codes to bf16 exactly (mqa_cvt8), a score four chained v_mfma_f32_16x16x32_bf16 over d ascending
// from zero, the mask on the fp32 accumulator, Gk a select, Gk and Gq carried into the products as two bf16 terms (the RNE value and the
// rounded residual, exact in fp32).  The split of the work is not: the problem is a regular [M H, 128] x [128, N] GEMM problem, so two
// passes each recompute the scores and every output has exactly one owner -- no atomics, every sum in an order the shapes and the ranges
// fix, all three outputs byte-reproducible.  256 threads (four waves), key tiles of 64, bf16 images in rows of 288 B (72 dwords = 8 mod 64,
// the sparse backward's rule for the straight and the transposed reads).  G never goes through LDS: in both passes the wave that masks a
// score owns the product that consumes it, and the accumulator's layout is the next product's operand layout once the contraction index is
// permuted the way ds_read_b64_tr_b16 permutes the other operand (k index 8 g + i stands for row 4 g + i, 8 g + 4 + i for row 16 + 4 g + i).
//
// Token-owned pass (mqd_token_kernel: dq, d_weights).  A workgroup owns DGA_MQA_LOGITS_BWD_DENSE_RUN = 2 consecutive tokens.  Wave w owns
// head tile w % (H / 16) of both and the key subtiles (16 keys) H / 16 (w / (H / 16)) .. of every tile: all four at H = 64, one half of the
// tile at H = 32.  Its q codes, converted once, stay in registers as B fragments (16 VGPRs a token) with its heads' weights; its dq
// accumulators (16 heads x 128 columns, 32 VGPRs a token) live in registers for the whole walk.  The walk visits the key tiles that meet a
// token's range, ascending; a tile outside both ranges is neither loaded nor multiplied.  A tile's codes (16 bytes a thread, two rows),
// kscale and the two tokens' d_logits segments are read once per run, one tile ahead in registers, and written (codes converted) into one of
// two LDS buffers: one barrier a tile.  Per tile and key subtile the key rows are read once (A operand) for both tokens: S^T [16 keys x 16
// heads], lane l holding head l & 15 and keys 4 (l >> 4) + i; d_weights' share fma(d_logits kscale, mask ? s : 0, acc) with keys ascending;
// Gq and its residual rounded to bf16 into the registers that are, subtile pair by subtile pair, the B operand of dQ^T += K^T Gq^T, whose
// K^T comes by pairs of transposed reads, once for both tokens.  An element outside its token's range is staged as +0 and never read.
// Epilogue: dq is the accumulators as they stand at H = 64; at H = 32 the two waves of a head tile add their halves (keys 0 .. 31 of every
// tile + keys 32 .. 63) through LDS.  d_weights over the lane groups (lane ^ 16, lane ^ 32), then over the waves of a head tile ascending.
//
// Key-owned pass (mqd_key_kernel: dk).  A workgroup owns a tile of 64 keys, wave w its subtile w as B fragments in registers (converted
// once), and a chunk of consecutive token runs of 64 (the workspace below).  It walks them as the forward does: lane i holds token i's
// clamped range, a ballot selects the tokens whose range meets the tile, the others are neither loaded nor multiplied.  Per token: the q
// image [H][128] and the weights go to one of two LDS buffers (the next token's loads in flight: one barrier a token); S [16 heads x 16
// keys] per head tile, lane l holding key l & 15 and heads 4 (l >> 4) + i; Gk and its residual in bf16 -- as they stand the A operand of
// dK [16 keys x 16 columns] += Gk^T Q over the H heads, Q by transposed reads of the image; 8 column tiles: 32 fp32 accumulators a lane.
// Causal ranges leave the key tiles unequal work, so the tokens are split over `splits` workgroups per tile (a function of M and N alone)
// and each writes its partial tile and, per key, whether a range named it, to the workspace; mqd_reduce_kernel then stores
// fl(prior + ((p_0 + p_1) + ... + p_last)) once per element of the named rows.  A row no range names and a column >= 128 is not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_mqa_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int MQD_THREADS = 256;
constexpr int MQD_D = DGA_MQA_LOGITS_HEAD_DIM;               // 128
constexpr int MQD_TILE = DGA_MQA_LOGITS_BWD_DENSE_TILE;      // keys of a tile: 64
constexpr int MQD_RUN = DGA_MQA_LOGITS_BWD_DENSE_RUN;        // tokens of a workgroup of the token-owned pass: 2
constexpr int MQD_BM = DGA_MQA_LOGITS_BLOCK_M;               // tokens of a run of the key-owned pass: one per lane (the ballot)
constexpr int MQD_ROW_BYTES = MQD_D * 2 + 32;                // 288: a head's or a key's 128 bf16
constexpr int MQD_CTILES = MQD_D / 16;                       // column tiles of dq and dk: 8
constexpr int MQD_MAX_SPLITS = 16, MQD_TARGET_GROUPS = 2048;
constexpr int MQD_NONE = 0x7FFFFFFF;
static_assert(MQD_D == 128 && MQD_TILE == 64 && MQD_BM == 64 && MQD_RUN >= 1 && MQD_RUN <= 4, "the kernels' geometry");

typedef short mqd_v4s __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int mqd_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
__device__ __forceinline__ uint32_t mqd_lds(const void *p)
{
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const unsigned char *)p;
}
// one 16 x 32 (or 32 x 16) bf16 fragment by two transposed reads: the blocks at `addr` and sixteen image rows (`half` bytes) below it
__device__ __forceinline__ mqa_v8bf mqd_read_tr(uint32_t addr, int half)
{
    const mqd_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<mqd_v4s __attribute__((address_space(3))) *>(addr));
    const mqd_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<mqd_v4s __attribute__((address_space(3))) *>(addr + half));
    return __builtin_bit_cast(mqa_v8bf, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// 16 e4m3 codes -> 16 bf16 (exact), 32 bytes at dst
__device__ __forceinline__ void mqd_put16(unsigned char *dst, const uint4 &raw)
{
    reinterpret_cast<mqa_v4i *>(dst)[0] = mqa_cvt8(mqa_v2i{(int)raw.x, (int)raw.y});
    reinterpret_cast<mqa_v4i *>(dst)[1] = mqa_cvt8(mqa_v2i{(int)raw.z, (int)raw.w});
}
// g as two bf16 terms: element e of `val` the RNE value, of `res` the rounded residual (g - bf16(g) is exact in fp32)
__device__ __forceinline__ void mqd_two_terms(float gf, mqa_v8bf &val, mqa_v8bf &res, int e)
{
    const __bf16 b = (__bf16)gf;
    val[e] = b;
    res[e] = (__bf16)(gf - (float)b);
}

// ---- the token-owned pass: dq and d_weights ---------------------------------------------------------------------------------------------
template <int H>
__global__ void __launch_bounds__(MQD_THREADS) mqd_token_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ k,
                                                                const float *__restrict__ kscale, const float *__restrict__ weights,
                                                                const int32_t *__restrict__ ks_in, const int32_t *__restrict__ ke_in,
                                                                const float *__restrict__ d_logits, int64_t dl_stride, int64_t m_n, int n_n,
                                                                float *__restrict__ dq, float *__restrict__ d_weights)
{
    constexpr int HT = H / 16;                 // head tiles; also the key subtiles of a wave
    constexpr int NH = HT / 2;                 // ... which are this many halves of a tile (32 keys: one k step of the second product)
    static_assert(H == 32 || H == 64, "the head counts of the indexer");
    static_assert(HT == 4 || 2 * MQD_RUN * MQD_CTILES * 64 * 16 <= 2 * MQD_TILE * MQD_ROW_BYTES, "the H = 32 epilogue reuses the tile buffers");
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][MQD_TILE * MQD_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) float dl_s[2][MQD_RUN][MQD_TILE], ks_s[2][MQD_TILE];   // +0 outside the range / beyond N
    __shared__ float dw_s[4][MQD_RUN][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int htb = wave % HT, kt0 = (wave / HT) * HT;       // the wave's head tile and its first key subtile
    const int64_t m0 = (int64_t)blockIdx.x * MQD_RUN;

    // the run's ranges, clamped to [0, N] as the forward clamps them; an empty one (and a token beyond M) is [0, 0)
    int lo[MQD_RUN], hi[MQD_RUN];
#pragma unroll
    for (int t = 0; t < MQD_RUN; ++t) {
        lo[t] = hi[t] = 0;
        if (m0 + t < m_n) {
            const int a = mqd_clamp(ks_in[m0 + t], n_n), b = mqd_clamp(ke_in[m0 + t], n_n);
            if (a < b) lo[t] = a, hi[t] = b;
        }
    }
    // the first tile at or behind `from` that meets a range (n_n <= DGA_MQA_LOGITS_MAX_N: 64 (from + 1) fits an int)
    auto next_tile = [&](int from) -> int {
        int best = MQD_NONE;
#pragma unroll
        for (int t = 0; t < MQD_RUN; ++t) {
            if (hi[t] > from * MQD_TILE) {
                const int first = lo[t] / MQD_TILE;
                const int c = first < from ? from : first;
                best = c < best ? c : best;
            }
        }
        return best;
    };

    // the wave's q fragments (B operand of S^T: lane l holds head 16 htb + (l & 15), codes 32 s + 8 (l >> 4) ..) and its heads' weights
    mqa_v4i qf[MQD_RUN][4];
    float wr[MQD_RUN], accw[MQD_RUN];
    mqa_v4f accq[MQD_RUN][MQD_CTILES];
#pragma unroll
    for (int t = 0; t < MQD_RUN; ++t) {
        const bool ok = m0 + t < m_n;
        const int64_t row = (m0 + t) * H + 16 * htb + hl;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            mqa_v2i raw = {0, 0};
            if (ok) raw = *reinterpret_cast<const mqa_v2i *>(q + row * MQD_D + 32 * s + 8 * g);
            qf[t][s] = mqa_cvt8(raw);
        }
        wr[t] = ok ? weights[row] : 0.f;
        accw[t] = 0.f;
#pragma unroll
        for (int j = 0; j < MQD_CTILES; ++j) accq[t][j] = mqa_v4f{0.f, 0.f, 0.f, 0.f};
    }

    // the staging: eight threads a key row, two rows a thread (p and p + 32 of the tile); wave t brings token t's d_logits segment, wave 0
    // kscale as well
    const int gpos = tid >> 3, gsub = tid & 7;
    uint4 raw[2];
    float dlv = 0.f, ksv = 0.f;
    auto fetch = [&](int tl) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int n = tl * MQD_TILE + 32 * half + gpos;
            raw[half] = uint4{0, 0, 0, 0};
            if (n < n_n) raw[half] = *reinterpret_cast<const uint4 *>(k + (int64_t)n * MQD_D + gsub * 16);
        }
        const int n = tl * MQD_TILE + lane;
        ksv = (wave == 0 && n < n_n) ? kscale[n] : 0.f;
        dlv = 0.f;
#pragma unroll
        for (int t = 0; t < MQD_RUN; ++t)
            if (wave == t && n >= lo[t] && n < hi[t]) dlv = d_logits[(m0 + t) * dl_stride + n];      // (hi <= N, token < M: inside the tensor)
    };

    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    int tl = next_tile(0), par = 0;
    if (tl != MQD_NONE) fetch(tl);
#pragma unroll 1
    while (tl != MQD_NONE) {
        unsigned char *tb = tile[par];
#pragma unroll
        for (int half = 0; half < 2; ++half) mqd_put16(tb + (32 * half + gpos) * MQD_ROW_BYTES + gsub * 32, raw[half]);
        if (wave < MQD_RUN) dl_s[par][wave][lane] = dlv;
        if (wave == 0) ks_s[par][lane] = ksv;
        // one barrier a tile: the buffer written here was last read two tiles ago, before every wave's previous barrier
        __syncthreads();
        const int nx = next_tile(tl + 1);
        if (nx != MQD_NONE) fetch(nx);

        const int base = tl * MQD_TILE;
        bool meets[MQD_RUN];
#pragma unroll
        for (int t = 0; t < MQD_RUN; ++t) meets[t] = hi[t] > base && lo[t] < base + MQD_TILE;       // (workgroup-uniform)
        mqa_v8bf gq[MQD_RUN][NH][2];                             // [token][half of the wave's keys][Gq, its residual]
#pragma unroll
        for (int t = 0; t < MQD_RUN; ++t)
#pragma unroll
            for (int hh = 0; hh < NH; ++hh) gq[t][hh][0] = gq[t][hh][1] = __builtin_bit_cast(mqa_v8bf, mqa_v4i{0, 0, 0, 0});

        // S^T, the mask, d_weights' share and Gq: key subtile by key subtile, the key rows read once for the run
#pragma unroll
        for (int kk = 0; kk < HT; ++kk) {
            const int kt = kt0 + kk;
            mqa_v4i ka[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) ka[s] = *reinterpret_cast<const mqa_v4i *>(tb + (16 * kt + hl) * MQD_ROW_BYTES + 64 * s + 16 * g);
            const mqa_v4f ks4 = *reinterpret_cast<const mqa_v4f *>(&ks_s[par][16 * kt + 4 * g]);
#pragma unroll
            for (int t = 0; t < MQD_RUN; ++t) {
                if (!meets[t]) continue;
                const mqa_v4f dl4 = *reinterpret_cast<const mqa_v4f *>(&dl_s[par][t][16 * kt + 4 * g]);
                mqa_v4f sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mqa_v8bf, ka[s]), __builtin_bit_cast(mqa_v8bf, qf[t][s]), sv, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = base + 16 * kt + 4 * g + i;
                    const bool mask = n >= lo[t] && n < hi[t] && sv[i] > 0.f;
                    const float c = dl4[i] * ks4[i];
                    accw[t] = __builtin_fmaf(c, mask ? sv[i] : 0.f, accw[t]);
                    const float gg = wr[t] * dl4[i];
                    const float gkf = mask ? gg : 0.f;
                    const float gqf = gkf * ks4[i];
                    mqd_two_terms(gqf, gq[t][kk >> 1][0], gq[t][kk >> 1][1], 4 * (kk & 1) + i);
                }
            }
        }
        // dQ^T += K^T Gq^T: a column tile's K^T read once for the run; keys 0 .. 31 before 32 .. 63, the value before its residual
        const uint32_t kt_addr = mqd_lds(tb) + (trow + 16 * kt0) * MQD_ROW_BYTES + tcol;
#pragma unroll
        for (int j = 0; j < MQD_CTILES; ++j) {
#pragma unroll
            for (int hh = 0; hh < NH; ++hh) {
                const mqa_v8bf kf = mqd_read_tr(kt_addr + 32 * j + 32 * hh * MQD_ROW_BYTES, 16 * MQD_ROW_BYTES);
#pragma unroll
                for (int t = 0; t < MQD_RUN; ++t) {
                    if (!meets[t]) continue;
                    accq[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, gq[t][hh][0], accq[t][j], 0, 0, 0);
                    accq[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, gq[t][hh][1], accq[t][j], 0, 0, 0);
                }
            }
        }
        tl = nx;
        par ^= 1;
    }

    // d_weights: the lane groups, then (below) the waves of a head tile
#pragma unroll
    for (int t = 0; t < MQD_RUN; ++t) {
        float v = accw[t];
        v = v + __shfl_xor(v, 16, 64);
        v = v + __shfl_xor(v, 32, 64);
        if (g == 0) dw_s[wave][t][hl] = v;
    }
    if constexpr (HT == 2) {
        // the upper waves' halves of dq go through the tile buffers, which every wave has finished reading behind this barrier
        __syncthreads();
        mqa_v4f *red = reinterpret_cast<mqa_v4f *>(&tile[0][0]);
        if (wave >= 2) {
#pragma unroll
            for (int t = 0; t < MQD_RUN; ++t)
#pragma unroll
                for (int j = 0; j < MQD_CTILES; ++j) red[(((wave - 2) * MQD_RUN + t) * MQD_CTILES + j) * 64 + lane] = accq[t][j];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int t = 0; t < MQD_RUN; ++t)
#pragma unroll
                for (int j = 0; j < MQD_CTILES; ++j) {
                    const mqa_v4f up = red[((wave * MQD_RUN + t) * MQD_CTILES + j) * 64 + lane];
#pragma unroll
                    for (int i = 0; i < 4; ++i) accq[t][j][i] = accq[t][j][i] + up[i];
                }
        }
    } else {
        __syncthreads();
    }
    if (wave < HT) {
#pragma unroll
        for (int t = 0; t < MQD_RUN; ++t) {
            if (m0 + t >= m_n) continue;
            float *orow = dq + (((m0 + t) * H + 16 * htb + hl) * MQD_D + 4 * g);
#pragma unroll
            for (int j = 0; j < MQD_CTILES; ++j) *reinterpret_cast<mqa_v4f *>(orow + 16 * j) = accq[t][j];
        }
    }
    if (tid < MQD_RUN * H) {
        const int t = tid / H, h = tid % H;
        float v = dw_s[h >> 4][t][h & 15];
        if constexpr (HT == 2) v = v + dw_s[(h >> 4) + 2][t][h & 15];
        if (m0 + t < m_n) d_weights[(m0 + t) * H + h] = v;
    }
}

// ---- the key-owned pass: dk's partial tiles -----------------------------------------------------------------------------------------------
struct MqdToken {
    int64_t m;      // -1: none left
    int lo, hi;
};

template <int H>
__global__ void __launch_bounds__(MQD_THREADS) mqd_key_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ k,
                                                              const float *__restrict__ weights, const int32_t *__restrict__ ks_in,
                                                              const int32_t *__restrict__ ke_in, const float *__restrict__ d_logits,
                                                              int64_t dl_stride, int64_t m_n, int n_n, int key_tiles, int runs, int runs_per_split,
                                                              float *__restrict__ part, int32_t *__restrict__ named_out, int64_t n_pad)
{
    constexpr int HT = H / 16;                 // head tiles
    constexpr int HK = H / 32;                 // k steps of the product contracted over the heads
    constexpr int QL = H * 8 / MQD_THREADS;    // 16-byte pieces of a token's codes a thread brings: 2 or 1
    static_assert(H == 32 || H == 64, "the head counts of the indexer");
    __shared__ __attribute__((aligned(16))) unsigned char qimg[2][H * MQD_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) float w_s[2][H];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int kt = blockIdx.x % key_tiles, split = blockIdx.x / key_tiles;
    const int n0 = kt * MQD_TILE;                                           // (n_n <= DGA_MQA_LOGITS_MAX_N: no overflow)
    const int n1 = n_n - n0 < MQD_TILE ? n_n : n0 + MQD_TILE;               // the tile's keys: [n0, n1)
    const int my_n = n0 + 16 * wave + hl;                                   // the lane's key in S

    // the wave's key fragments (B operand of S: lane l holds key 16 w + (l & 15), codes 32 s + 8 (l >> 4) ..), zero codes beyond N
    mqa_v4i kb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        mqa_v2i raw = {0, 0};
        if (my_n < n_n) raw = *reinterpret_cast<const mqa_v2i *>(k + (int64_t)my_n * MQD_D + 32 * s + 8 * g);
        kb[s] = mqa_cvt8(raw);
    }

    // the walk over the chunk's tokens whose range meets the tile (every wave computes the same sequence)
    int run = split * runs_per_split;
    const int run_end = run + runs_per_split < runs ? run + runs_per_split : runs;
    uint64_t act = 0;
    int64_t act_m0 = 0;
    int lo_v = 0, hi_v = 0;
    auto next_token = [&]() -> MqdToken {
        while (act == 0) {
            if (run >= run_end) return MqdToken{-1, 0, 0};
            act_m0 = (int64_t)run * MQD_BM;
            lo_v = hi_v = 0;
            if (act_m0 + lane < m_n) {
                lo_v = mqd_clamp(ks_in[act_m0 + lane], n_n);
                hi_v = mqd_clamp(ke_in[act_m0 + lane], n_n);
            }
            act = __ballot(lo_v < hi_v && lo_v < n1 && hi_v > n0);
            ++run;
        }
        const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(act));
        act &= act - 1;
        return MqdToken{act_m0 + i, __builtin_amdgcn_readlane(lo_v, i), __builtin_amdgcn_readlane(hi_v, i)};
    };

    uint4 raw[QL];
    float wv = 0.f, dlv = 0.f;
    auto fetch = [&](const MqdToken &tk) {
#pragma unroll
        for (int j = 0; j < QL; ++j) {
            const int c = tid + MQD_THREADS * j;
            raw[j] = *reinterpret_cast<const uint4 *>(q + (tk.m * H + (c >> 3)) * MQD_D + (c & 7) * 16);
        }
        if (tid < H) wv = weights[tk.m * H + tid];
        dlv = (my_n >= tk.lo && my_n < tk.hi) ? d_logits[tk.m * dl_stride + my_n] : 0.f;      // (hi <= N: inside the tensor)
    };

    mqa_v4f acc[MQD_CTILES];
#pragma unroll
    for (int ct = 0; ct < MQD_CTILES; ++ct) acc[ct] = mqa_v4f{0.f, 0.f, 0.f, 0.f};
    bool named = false;
    const int trow = 4 * g + (hl >> 2), tcol = 8 * (hl & 3);
    MqdToken cur = next_token();
    int par = 0;
    if (cur.m >= 0) fetch(cur);
#pragma unroll 1
    while (cur.m >= 0) {
        unsigned char *qi = qimg[par];
#pragma unroll
        for (int j = 0; j < QL; ++j) {
            const int c = tid + MQD_THREADS * j;
            mqd_put16(qi + (c >> 3) * MQD_ROW_BYTES + (c & 7) * 32, raw[j]);
        }
        if (tid < H) w_s[par][tid] = wv;
        const float dl = dlv;
        const bool live = my_n >= cur.lo && my_n < cur.hi;
        named = named || live;
        // one barrier a token: the buffer written here was last read two tokens ago, before every wave's previous barrier
        __syncthreads();
        const MqdToken nx = next_token();
        if (nx.m >= 0) fetch(nx);

        // S, the mask and Gk with its residual: head tile pair by head tile pair the A operand of the product over the heads
        mqa_v8bf ga[2][HK];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            mqa_v4f sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const mqa_v4i qa = *reinterpret_cast<const mqa_v4i *>(qi + (16 * ht + hl) * MQD_ROW_BYTES + 64 * s + 16 * g);
                sv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mqa_v8bf, qa), __builtin_bit_cast(mqa_v8bf, kb[s]), sv, 0, 0, 0);
            }
            const mqa_v4f w4 = *reinterpret_cast<const mqa_v4f *>(&w_s[par][16 * ht + 4 * g]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool mask = live && sv[i] > 0.f;
                const float gg = w4[i] * dl;
                mqd_two_terms(mask ? gg : 0.f, ga[0][ht >> 1], ga[1][ht >> 1], 4 * (ht & 1) + i);
            }
        }
        // dK += Gk^T Q: heads 0 .. 31 before 32 .. 63, the value before its residual
        const uint32_t qt_addr = mqd_lds(qi) + trow * MQD_ROW_BYTES + tcol;
#pragma unroll
        for (int ct = 0; ct < MQD_CTILES; ++ct) {
#pragma unroll
            for (int kc = 0; kc < HK; ++kc) {
                const mqa_v8bf qt = mqd_read_tr(qt_addr + 32 * kc * MQD_ROW_BYTES + 32 * ct, 16 * MQD_ROW_BYTES);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[0][kc], qt, acc[ct], 0, 0, 0);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[1][kc], qt, acc[ct], 0, 0, 0);
            }
        }
        cur = nx;
        par ^= 1;
    }

    // the partial tile (lane l: keys 16 w + 4 (l >> 4) + i, column 16 ct + (l & 15)) and the keys' flags; rows up to n_pad exist
    float *prow = part + (((int64_t)split * n_pad + n0 + 16 * wave + 4 * g) * MQD_D + hl);
#pragma unroll
    for (int ct = 0; ct < MQD_CTILES; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i * MQD_D + 16 * ct] = acc[ct][i];
    if (g == 0) named_out[(int64_t)split * n_pad + my_n] = named ? 1 : 0;
}

// dk[n, :] = fl(prior + ((p_0 + p_1) + ... )) for the rows a range named: 32 threads a row, four columns each
__global__ void __launch_bounds__(MQD_THREADS) mqd_reduce_kernel(const float *__restrict__ part, const int32_t *__restrict__ named_in, int splits,
                                                                 int64_t n_pad, int n_n, float *__restrict__ dk, int64_t dk_stride)
{
    const int64_t idx = (int64_t)blockIdx.x * MQD_THREADS + threadIdx.x;
    const int64_t row = idx >> 5;
    const int c4 = (int)(idx & 31);
    if (row >= n_n) return;
    bool named = false;
    for (int s = 0; s < splits; ++s) named = named || named_in[s * n_pad + row] != 0;
    if (!named) return;
    mqa_v4f v = *reinterpret_cast<const mqa_v4f *>(part + (row * MQD_D + 4 * c4));
    for (int s = 1; s < splits; ++s) {
        const mqa_v4f p = *reinterpret_cast<const mqa_v4f *>(part + ((s * n_pad + row) * MQD_D + 4 * c4));
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] + p[i];
    }
    float *o = dk + (row * dk_stride + 4 * c4);
    mqa_v4f prior = *reinterpret_cast<const mqa_v4f *>(o);
#pragma unroll
    for (int i = 0; i < 4; ++i) prior[i] = prior[i] + v[i];
    *reinterpret_cast<mqa_v4f *>(o) = prior;
}

// the key-owned pass's split of the tokens: a function of m and n alone
struct MqdSplit {
    int64_t key_tiles, runs, runs_per_split, splits, n_pad;
};
static MqdSplit mqd_split(int64_t m, int64_t n)
{
    MqdSplit s;
    s.key_tiles = (n + MQD_TILE - 1) / MQD_TILE;
    s.runs = (m + MQD_BM - 1) / MQD_BM;
    int64_t want = (MQD_TARGET_GROUPS + s.key_tiles - 1) / s.key_tiles;
    want = want > MQD_MAX_SPLITS ? MQD_MAX_SPLITS : want;
    want = want > s.runs ? s.runs : want;
    s.runs_per_split = (s.runs + want - 1) / want;
    s.splits = (s.runs + s.runs_per_split - 1) / s.runs_per_split;
    s.n_pad = s.key_tiles * MQD_TILE;
    return s;
}

}  // namespace dga

extern "C" int64_t dga_fp8_mqa_logits_bwd_dense_workspace_bytes(int64_t m, int64_t n)
{
    using namespace dga;
    if (m < 1 || n < 1 || n > DGA_MQA_LOGITS_MAX_N) return 0;
    const MqdSplit s = mqd_split(m, n);
    return s.splits * s.n_pad * (MQD_D * 4 + 4);
}

// The checks in the documented clause order: shape, (m == 0), null, alignment, range, workspace
extern "C" int dga_fp8_mqa_logits_bwd_dense(const void *q, const void *k, const float *kscale, const float *weights, const int32_t *ks,
                                            const int32_t *ke, const float *d_logits, int64_t m, int64_t n, int heads, int head_dim,
                                            int64_t dl_stride, float *dq, float *dk, int64_t dk_stride, float *d_weights, void *workspace,
                                            int64_t workspace_bytes, void *stream)
{
    using namespace dga;
    if (m < 0 || n < 1 || head_dim != MQD_D || (heads != 32 && heads != 64) || dl_stride < n || dk_stride < MQD_D) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !k || !kscale || !weights || !ks || !ke || !d_logits || !dq || !dk || !d_weights || !workspace) return DGA_E_NULL;
    // a thread reads 16 codes at once and stores four values of dq and dk
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(k) % 16 || reinterpret_cast<uintptr_t>(dq) % 16 ||
        reinterpret_cast<uintptr_t>(dk) % 16 || dk_stride % 4 || reinterpret_cast<uintptr_t>(kscale) % 4 ||
        reinterpret_cast<uintptr_t>(weights) % 4 || reinterpret_cast<uintptr_t>(ks) % 4 || reinterpret_cast<uintptr_t>(ke) % 4 ||
        reinterpret_cast<uintptr_t>(d_logits) % 4 || reinterpret_cast<uintptr_t>(d_weights) % 4)
        return DGA_E_ALIGN;
    if (n > DGA_MQA_LOGITS_MAX_N || dl_stride > 0x7FFFFFFFFFFFFFFFll / 4 / m || dk_stride > 0x7FFFFFFFFFFFFFFFll / 4 / n ||
        (m + MQD_RUN - 1) / MQD_RUN > 0x7FFFFFFFll)
        return DGA_E_RANGE;
    const MqdSplit sp = mqd_split(m, n);                     // (key_tiles * splits <= 2^25 + 2048 * 16: a grid)
    if (workspace_bytes < sp.splits * sp.n_pad * (MQD_D * 4 + 4) || reinterpret_cast<uintptr_t>(workspace) % 16) return DGA_E_WORKSPACE;
    float *part = static_cast<float *>(workspace);
    int32_t *named = reinterpret_cast<int32_t *>(part + sp.splits * sp.n_pad * MQD_D);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t *qc = static_cast<const uint8_t *>(q), *kc = static_cast<const uint8_t *>(k);
    const dim3 block(MQD_THREADS);
    auto launch = [&](auto token_kernel, auto key_kernel) {
        hipLaunchKernelGGL(token_kernel, dim3(static_cast<unsigned>((m + MQD_RUN - 1) / MQD_RUN)), block, 0, s, qc, kc, kscale, weights, ks, ke,
                           d_logits, dl_stride, m, static_cast<int>(n), dq, d_weights);
        hipLaunchKernelGGL(key_kernel, dim3(static_cast<unsigned>(sp.key_tiles * sp.splits)), block, 0, s, qc, kc, weights, ks, ke, d_logits,
                           dl_stride, m, static_cast<int>(n), static_cast<int>(sp.key_tiles), static_cast<int>(sp.runs),
                           static_cast<int>(sp.runs_per_split), part, named, sp.n_pad);
    };
    if (heads == 64) launch(mqd_token_kernel<64>, mqd_key_kernel<64>);
    else launch(mqd_token_kernel<32>, mqd_key_kernel<32>);
    hipLaunchKernelGGL(mqd_reduce_kernel, dim3(static_cast<unsigned>((n + 7) / 8)), block, 0, s, part, named, static_cast<int>(sp.splits), sp.n_pad,
                       static_cast<int>(n), dk, dk_stride);
    return record_hip(hipGetLastError());
}
