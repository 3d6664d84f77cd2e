// What trains the lightning indexer in the sparse stage of DeepSeek sparse attention: the KL loss between the main attention's head-summed
// probabilities over the selected keys and the indexer's softmax over the same keys, and its derivative at the selected logits.
//   dga_indexer_kl_loss   q, kv, indices, offsets, sm_scale as dga_sparse_mla_fwd's (and its validity rule); lse fp32 [m, heads] (normally
//                         the forward's); logits fp32 [m, s] (rows logits_stride apart: dga_fp8_mqa_logits' output, key column = kv row)
//                         -> loss fp32 [m], d_logits fp32 [m, topk], target fp32 [m, topk] (optional)
//     over the valid positions j of token t, r_j the row:
//     p_hj = exp(sm_scale sum_d q[t,h,d] kv[r_j,d] - lse[t,h]);  t_j = (1 / heads) sum_h p_hj;  L = ln sum_j exp(logits[t,r_j]);
//     a_j = logits[t,r_j] - L;  y_j = exp(a_j);  loss[t] = sum_j (t_j > 0 ? t_j (ln t_j - a_j) : 0);  d_logits[t,j] = grad_scale (y_j - t_j)
//     an invalid position: d_logits = target = +0; a token without a valid position: loss = +0 whatever its lse holds
// One workgroup of four waves owns one token and all its heads (HT = heads / 16 head tiles, a template parameter).  There is no value
// product and so no output accumulator: q does not go to LDS but stays in registers as ready B-operand fragments -- 18 uint4 (72 VGPRs) a
// head tile, read once from global memory --, and LDS holds two buffers of the gathered tile (SMLA_TILE positions in the 1184-byte rows of
// dga_sparse_mla_device.hpp) and 1.3 KB of exchange.  Who computes what, wave w:
//   HT >= 4   head tiles w and w + 4 (when there is one), both key subtiles of 16
//   HT == 3   head tile w (wave 3 only gathers), both key subtiles
//   HT == 2   head tile w / 2, key subtile w % 2
//   HT == 1   head tile 0, key subtile w (waves 2 and 3 only gather)
// Prologue: the token's valid logits[t, r_j] are read twice by the whole workgroup (position tid, tid + 256, ..): their maximum, then
// sum_j exp2((logit - max) log2 e) per thread over its positions ascending, the lanes by xor 32, 16, .. 1, the waves through LDS as
// ((w0 + w1) + w2) + w3; L = max + ln 2 log2(sum).
// The gather is sparse MLA's (eight threads a row, nine 16-byte chunks each, one tile read ahead in registers, the index one tile further;
// thread 0 of a row also brings logits[t, r_j]; an invalid position is staged as zeros).  Per tile, one barrier:
//   tile tl goes to buffer tl % 2, barrier, the rows of tile tl + 1 are asked for
//   the positions of tile tl - 1 are finished (below) by the threads that brought them: thread 0 of each row, eight a wave
//   unless no position of tile tl is valid (a ballot over the 32 staged flags, the same in every wave):
//     S^T = K Q^T per head tile and key subtile: 18 chained v_mfma_f32_16x16x32_bf16 over d ascending from +0, key rows the A operand by
//     ds_read_b128, exactly the forward's chain: lane l holds head l & 15 and keys 4 (l >> 4) + i
//     p = exp2(S (sm_scale log2 e) - lse log2 e) in fp32; the lane's head tiles added ascending; the sixteen lanes of a key by xor 1, 2, 4, 8;
//     lane 0 of each key group stores its four keys' sums to psum[tl % 2][w]
// Finishing position j (after the next barrier): the waves' sums in the fixed order of the table above (ascending wave), once times
// 1 / heads: t_j; a_j, y_j, the loss term added to the thread's own sum (tiles ascending), d_logits and target stored -- +0 for an invalid
// position, which reads nothing of psum.  What a buffer of parity b holds at tile tl is next written at tl + 2, behind the barrier of
// tl + 1, which every reader of it has reached: one barrier a tile serves the tile, the flags and the sums.
// Epilogue: the threads' loss sums over the lanes by xor 32 .. 1 and the waves as ((w0 + w1) + w2) + w3.
// Every output has one writer and a fixed order of summation, nothing is atomic: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr float IKL_L2E = 1.4426950408889634f, IKL_LN2 = 0.693147180559945309f;
constexpr int IKL_TILE_BYTES = SMLA_TILE * SMLA_ROW_BYTES;

// log2 of x > 0, subnormal x included (v_log_f32 alone takes them for zero): x 2^64 is exact
__device__ __forceinline__ float ikl_log2(float x)
{
    const bool tiny = x < 0x1p-100f;
    const float l = __builtin_amdgcn_logf(tiny ? x * 0x1p64f : x);
    return tiny ? l - 64.f : l;
}
// the fixed tree over the 64 lanes, every lane gets the sum
__device__ __forceinline__ float ikl_lane_sum(float v)
{
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) v = v + __shfl_xor(v, x, 64);
    return v;
}

template <int HT>
__global__ void __launch_bounds__(SMLA_THREADS) indexer_kl_kernel(const uint16_t *__restrict__ q, const void *__restrict__ kv, int64_t kv_stride,
                                                                  int64_t s_rows, const int32_t *__restrict__ indices, int64_t idx_stride,
                                                                  int topk, const int32_t *__restrict__ offsets, int64_t tokens, int64_t chunk,
                                                                  float scale2, const float *__restrict__ lse, const float *__restrict__ logits,
                                                                  int64_t lg_stride, float grad_scale, float inv_heads, float *__restrict__ loss,
                                                                  float *__restrict__ d_logits, float *__restrict__ target)
{
    constexpr int H = 16 * HT;
    constexpr int NKS = HT <= 2 ? 1 : 2;                     // key subtiles a computing wave takes
    constexpr int MAXNH = HT > 4 ? 2 : 1;                    // head tiles a wave may own
    const SmlaBf16Rows cache = SmlaBf16Rows::make(kv, kv_stride, s_rows, 0, 0);
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][IKL_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) float psum[2][4][SMLA_TILE];                  // a wave's head sums of the tile's positions
    __shared__ __attribute__((aligned(16))) int32_t live[2][SMLA_TILE];                   // 1 where the tile's position is valid
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the token of this workgroup: the grid is walked XCD by XCD as sparse MLA's; chunk == 0: the grid is taken as it is
    int64_t t = blockIdx.x;
    if (chunk) t = (t & 7) * chunk + (t >> 3);
    if (t >= tokens) return;                                 // (the whole workgroup alike, before any barrier)

    // the wave's share (the table at the head of the file), wave-uniform
    const int nh = HT >= 4 ? 1 + (wave + 4 < HT ? 1 : 0) : HT == 3 ? (wave < 3 ? 1 : 0) : HT == 2 ? 1 : (wave < 2 ? 1 : 0);
    const int ht0 = HT >= 3 ? wave : HT == 2 ? wave >> 1 : 0;
    const int ks0 = HT <= 2 ? wave & 1 : 0;

    const int32_t *irow = indices + t * idx_stride;
    const float *lrow = logits + t * lg_stride;
    const int64_t shift = offsets ? (int64_t)offsets[t] : 0;
    const int tiles = (topk + SMLA_TILE - 1) / SMLA_TILE;

    // the gather (dga_sparse_mla.hip): eight threads a position, the index one tile ahead of its row; -1: an invalid position
    const int gpos = tid >> 3, gsub = tid & 7;
    auto ask = [&](int tl) -> int32_t {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        return irow[pos < topk ? pos : topk - 1];
    };
    auto row_of = [&](int64_t pos, int32_t i) -> int64_t {
        const int64_t r = (int64_t)i + shift;
        return (pos < topk && i >= 0 && r >= 0 && r < s_rows) ? r : -1;
    };
    uint4 raw[SMLA_STAGE];
    int64_t row;
    float lg_next;
    auto fetch = [&](int tl, int32_t i) {
        row = row_of((int64_t)tl * SMLA_TILE + gpos, i);
        lg_next = 0.f;
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) raw[c] = uint4{0, 0, 0, 0};
        if (row >= 0) {
            SmlaBf16Rows::load(cache.at(row, gsub), gsub, raw);
            if (gsub == 0) lg_next = lrow[row];
        }
    };
    fetch(0, ask(0));
    int32_t asked = ask(1);

    // the wave's q as B-operand fragments: head 16 ht + (l & 15), the eight d at 32 s + 8 (l >> 4); and its heads' lse in the log2 domain
    smla_v4u qf[MAXNH][SMLA_KSTEPS];
    float lseb[MAXNH];
#pragma unroll
    for (int hi = 0; hi < MAXNH; ++hi) {
        lseb[hi] = 0.f;
#pragma unroll
        for (int s = 0; s < SMLA_KSTEPS; ++s) qf[hi][s] = smla_v4u{0, 0, 0, 0};
        if (hi < nh) {
            const int64_t head = t * H + 16 * (ht0 + 4 * hi) + hl;
            const uint16_t *qrow = q + (head * SMLA_D + 8 * g);
#pragma unroll
            for (int s = 0; s < SMLA_KSTEPS; ++s) qf[hi][s] = *reinterpret_cast<const smla_v4u *>(qrow + 32 * s);
            lseb[hi] = lse[head] * IKL_L2E;
        }
    }

    // the prologue: L = ln sum_j exp(logits[t, r_j]) over the valid positions
    float mx = -__builtin_inff();
    for (int64_t pos = tid; pos < topk; pos += SMLA_THREADS) {
        const int64_t r = row_of(pos, irow[pos]);
        if (r >= 0) mx = __builtin_fmaxf(mx, lrow[r]);
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, x, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = __builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3]));
    __syncthreads();
    float esum = 0.f;
    for (int64_t pos = tid; pos < topk; pos += SMLA_THREADS) {
        const int64_t r = row_of(pos, irow[pos]);
        if (r >= 0) esum = esum + __builtin_amdgcn_exp2f((lrow[r] - mx) * IKL_L2E);
    }
    esum = ikl_lane_sum(esum);
    if (lane == 0) red[wave] = esum;
    __syncthreads();
    const float big_l = mx + __builtin_amdgcn_logf(((red[0] + red[1]) + red[2]) + red[3]) * IKL_LN2;   // (unused when nothing is valid)

    const uint32_t tile_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)&tile[0][0];
    const uint32_t k_addr = tile_base + (16 * ks0 + hl) * SMLA_ROW_BYTES + 16 * g;

    // S^T, p and the head sums of one tile for a wave of NH head tiles
    auto compute = [&](auto nh_c, int par) {
        constexpr int NH = decltype(nh_c)::value;
        smla_v4f acc[NH][NKS];
#pragma unroll
        for (int hi = 0; hi < NH; ++hi)
#pragma unroll
            for (int k = 0; k < NKS; ++k) acc[hi][k] = smla_v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < SMLA_KSTEPS; ++s) {
#pragma unroll
            for (int k = 0; k < NKS; ++k) {
                const smla_v4u ka = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(
                    k_addr + par * IKL_TILE_BYTES + k * 16 * SMLA_ROW_BYTES + 64 * s);
#pragma unroll
                for (int hi = 0; hi < NH; ++hi)
                    acc[hi][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka), __builtin_bit_cast(smla_v8bf, qf[hi][s]),
                                                                         acc[hi][k], 0, 0, 0);
            }
        }
#pragma unroll
        for (int k = 0; k < NKS; ++k) {
            smla_v4f v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = __builtin_amdgcn_exp2f(acc[0][k][i] * scale2 - lseb[0]);
                if constexpr (NH == 2) v[i] = v[i] + __builtin_amdgcn_exp2f(acc[1][k][i] * scale2 - lseb[1]);
            }
#pragma unroll
            for (int x = 1; x <= 8; x <<= 1)
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] + __shfl_xor(v[i], x, 64);
            if (hl == 0) *reinterpret_cast<smla_v4f *>(&psum[par][wave][16 * (ks0 + k) + 4 * g]) = v;
        }
    };

    // position gpos of tile tl, by thread 0 of its row: ok and lg are what that thread staged for it
    float loss_acc = 0.f;
    auto finish = [&](int tl, bool ok, float lg) {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        if (gsub != 0 || pos >= topk) return;
        float tv = 0.f, dl = 0.f;
        if (ok) {
            const float *ps = &psum[tl & 1][0][gpos];
            const int ks = gpos >> 4;
            float hs;
            if constexpr (HT >= 4) hs = ((ps[0] + ps[SMLA_TILE]) + ps[2 * SMLA_TILE]) + ps[3 * SMLA_TILE];
            else if constexpr (HT == 3) hs = (ps[0] + ps[SMLA_TILE]) + ps[2 * SMLA_TILE];
            else if constexpr (HT == 2) hs = ps[ks * SMLA_TILE] + ps[(ks + 2) * SMLA_TILE];
            else hs = ps[ks * SMLA_TILE];
            tv = hs * inv_heads;
            const float a = lg - big_l;
            const float y = __builtin_amdgcn_exp2f(a * IKL_L2E);
            dl = grad_scale * (y - tv);
            if (tv > 0.f) loss_acc = loss_acc + tv * (ikl_log2(tv) * IKL_LN2 - a);
        }
        d_logits[t * topk + pos] = dl;
        if (target) target[t * topk + pos] = tv;
    };

    bool ok_cur = false, ok_prev = false;
    float lg_cur = 0.f, lg_prev = 0.f;
#pragma unroll 1
    for (int tl = 0; tl < tiles; ++tl) {
        const int par = tl & 1;
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(&tile[par][gpos * SMLA_ROW_BYTES + SmlaBf16Rows::lds_at(c, gsub)]) = raw[c];
        if (gsub == 0) live[par][gpos] = row >= 0;
        ok_prev = ok_cur, lg_prev = lg_cur;
        ok_cur = row >= 0, lg_cur = lg_next;
        __syncthreads();
        fetch(tl + 1, asked);
        asked = ask(tl + 2);
        if (tl > 0) finish(tl - 1, ok_prev, lg_prev);
        if (__ballot(live[par][lane & (SMLA_TILE - 1)] != 0) != 0) {      // (the same 32 flags in every wave: the whole workgroup alike)
            if constexpr (MAXNH == 2) {
                if (nh == 2) compute(std::integral_constant<int, 2>{}, par);
                else compute(std::integral_constant<int, 1>{}, par);
            } else {
                if (nh == 1) compute(std::integral_constant<int, 1>{}, par);
            }
        }
    }
    __syncthreads();
    finish(tiles - 1, ok_cur, lg_cur);

    loss_acc = ikl_lane_sum(loss_acc);
    if (lane == 0) red[wave] = loss_acc;
    __syncthreads();
    if (tid == 0) loss[t] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace dga

// The checks in the family's order: dga_sparse_mla_fwd's (its outputs apart), then this entry's shape, null, alignment and range clauses
extern "C" int dga_indexer_kl_loss(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                   int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, const float *lse,
                                   const float *logits, int64_t logits_stride, double grad_scale, float *loss, float *d_logits, float *target,
                                   void *stream)
{
    using namespace dga;
    const SmlaCall c{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream};
    const SmlaSource src{false, kv, s, 1, kv_stride};
    bool launch;
    const int rc = check_sparse_mla(c, src, false, nullptr, nullptr, &launch);
    if (!launch) return rc;
    if (logits_stride < s) return DGA_E_SHAPE;
    if (!lse || !logits || !loss || !d_logits) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(lse) % 4 || reinterpret_cast<uintptr_t>(logits) % 4 || reinterpret_cast<uintptr_t>(loss) % 4 ||
        reinterpret_cast<uintptr_t>(d_logits) % 4 || reinterpret_cast<uintptr_t>(target) % 4)
        return DGA_E_ALIGN;
    if (logits_stride > 0x7FFFFFFFFFFFFFFFll / 4 / m) return DGA_E_RANGE;
    const bool linear = (flags & DGA_SPARSE_MLA_LINEAR_GRID) != 0;
    const int64_t chunk = linear ? 0 : (m + 7) / 8;
    const dim3 grid(static_cast<unsigned>(linear ? m : chunk * 8)), block(SMLA_THREADS);
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(q), kv, kv_stride, s, indices,
                           idx_stride, static_cast<int>(topk), index_offsets, m, chunk, static_cast<float>(sm_scale * 1.4426950408889634), lse,
                           logits, logits_stride, static_cast<float>(grad_scale), static_cast<float>(1.0 / heads), loss, d_logits, target);
    };
    switch (heads / 16) {
    case 1: run(indexer_kl_kernel<1>); break;
    case 2: run(indexer_kl_kernel<2>); break;
    case 3: run(indexer_kl_kernel<3>); break;
    case 4: run(indexer_kl_kernel<4>); break;
    case 5: run(indexer_kl_kernel<5>); break;
    case 6: run(indexer_kl_kernel<6>); break;
    case 7: run(indexer_kl_kernel<7>); break;
    default: run(indexer_kl_kernel<8>); break;
    }
    return record_hip(hipGetLastError());
}
