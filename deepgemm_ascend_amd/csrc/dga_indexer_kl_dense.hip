// What trains the lightning indexer in the dense warm-up stage of DeepSeek sparse attention, before any top-k exists: the KL loss between the
// main attention's head-summed probabilities over ALL keys of a token's range and the indexer's softmax over the same keys, its derivative
// at the logits (what dga_fp8_mqa_logits_bwd_dense takes), and the main attention's lse over the range, which nothing else here supplies.
//   dga_indexer_kl_loss_dense   q bf16 [m, heads, 576], kv bf16 [s, 576] (rows kv_stride apart), ks / ke int32 [m] clamped to [0, s] as
//                               dga_fp8_mqa_logits clamps them, logits fp32 [m, s] (key column = kv row), lse fp32 [m, heads] or null
//                               -> loss fp32 [m], d_logits fp32 [m, s], target fp32 [m, s] (optional), lse_out fp32 [m, heads] (lse null)
//     over the keys n of [lo[t], hi[t]): dga_indexer_kl.hip's formulas with "valid position j" replaced by "key n inside the range", and
//     lse[t, h] = ln sum_n exp(sm_scale sum_d q[t,h,d] kv[n,d]); outside the range d_logits = target = +0; an empty token: loss = +0, lse = -inf
// One kernel template, ikd_kernel<HT, LSE>, is the walk over the key tiles; it is launched as the lse pass (LSE, skipped when lse is given) and
// then as the loss pass.  Both form a score with the same instructions in the same order, so the loss pass's S is the lse pass's bit for bit.
// A workgroup of eight waves owns a run of two consecutive tokens and all their heads (HT = heads / 16 head tiles).  There is no gather: a
// tile is SMLA_TILE = 32 consecutive kv rows, tile tl the rows 32 tl .. 32 tl + 31, read by 16-byte loads that follow one another through a
// row (thread tid brings chunks tid, tid + 512, .. of the tile's 2304, a row is 72 chunks), one tile ahead in registers, and written into one
// of two LDS buffers in the 1184-byte rows of dga_sparse_mla_device.hpp (rows >= s as zeros).  The walk visits, ascending, the tiles that
// meet one of the run's two clamped ranges; the next one is found from the ranges, a tile outside both is neither loaded nor multiplied.
// q never goes to LDS: a wave holds its head tile's q as ready B-operand fragments, 18 uint4 (72 VGPRs) a token.  Who computes what, wave w:
//   HT >= 5   head tile w of both tokens, both key subtiles of 16: a key fragment is read from LDS once for two MFMAs (waves >= HT only load)
//   HT 3, 4   head tile w % HT of both tokens, key subtile w / HT (HT == 3: waves 6 and 7 only load)
//   HT == 2   head tile w % 2, key subtile (w / 2) % 2, token w / 4
//   HT == 1   head tile 0, key subtile w % 2, token (w / 2) % 2 (waves 4 .. 7 only load)
// Per tile, one barrier: the tile goes to buffer step % 2, barrier, the next live tile is asked for, the previous tile is finished (loss
// pass), then S^T = K Q^T per token and key subtile: 18 chained v_mfma_f32_16x16x32_bf16 over d ascending from +0, key rows the A operand by
// ds_read_b128 -- the sparse forward's chain; lane l holds head l & 15 and keys 4 (l >> 4) + i.
// The lse pass: per lane and token a running maximum m and sum l in the log2 domain, x = S (sm_scale log2 e); per tile the lane's keys inside
// the token's range (a select on the accumulator) give the new maximum, l = l exp2(m_old - m_new) once, then + exp2(x - m_new) keys
// ascending.  At the end every lane stores (m, l) to LDS (the tile buffers, after a barrier) and one thread a (token, head) takes the
// maximum of its head's pairs -- four lane groups times the waves that share the head tile -- and adds l_i exp2(m_i - max) ascending:
// lse = LN2 (max + log2 sum), -inf for an empty token.
// The loss pass.  Prologue: L = ln sum_n exp(logits[t, n]) per token over its range by the whole workgroup, in the two-pass form of
// dga_indexer_kl.hip (maximum, then sum_n exp2((logit - max) log2 e): thread, lanes by xor 32 .. 1, waves ascending through LDS); and +0
// into d_logits and target at every column of a tile the walk does not visit.  Per tile p = exp2(S (sm_scale log2 e) - lse log2 e) in fp32,
// the sixteen lanes of a key by xor 1, 2, 4, 8, lane 0 of each key group stores four keys' sums to psum[step % 2][token][head tile].
// Finishing a tile, one step later behind the next barrier, by wave 7 (lane l: token l >> 5, key l & 31; its logit was asked for a tile
// ahead): the head tiles' sums ascending, once times 1 / heads: t; a, y, the loss term added to the lane's own sum (tiles ascending),
// d_logits and target stored, 128 contiguous bytes a token -- a selected +0 where the key is outside the token's range.  Epilogue: the loss
// sums over the 32 lanes of a token by xor 16 .. 1.
// Every output has one writer and a fixed order of summation, nothing is atomic: two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr float IKD_L2E = 1.4426950408889634f, IKD_LN2 = 0.693147180559945309f;
constexpr int IKD_THREADS = 512, IKD_WAVES = IKD_THREADS / 64, IKD_RUN = DGA_INDEXER_KL_DENSE_RUN;
constexpr int IKD_TILE_BYTES = SMLA_TILE * SMLA_ROW_BYTES;
constexpr int IKD_TILE_CHUNKS = SMLA_TILE * SMLA_CHUNKS;                                   // 2304 16-byte chunks
constexpr int IKD_STAGE = (IKD_TILE_CHUNKS + IKD_THREADS - 1) / IKD_THREADS;               // 5 a thread, the last one of half the threads
constexpr int IKD_END = 0x7FFFFFFF;                                                        // no further tile
static_assert(IKD_RUN == 2 && IKD_WAVES == 8 && IKD_RUN * SMLA_TILE == 64 && IKD_RUN * DGA_SPARSE_MLA_MAX_HEADS <= IKD_THREADS, "the kernel's geometry");

__device__ __forceinline__ int ikd_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }
// log2 of x > 0, subnormal x included (v_log_f32 alone takes them for zero): x 2^64 is exact
__device__ __forceinline__ float ikd_log2(float x)
{
    const bool tiny = x < 0x1p-100f;
    const float l = __builtin_amdgcn_logf(tiny ? x * 0x1p64f : x);
    return tiny ? l - 64.f : l;
}

template <int HT, bool LSE>
__global__ void __launch_bounds__(IKD_THREADS) ikd_kernel(const uint16_t *__restrict__ q, const uint16_t *__restrict__ kv, int64_t kv_stride, int n_keys,
                                                          const int32_t *__restrict__ ks_in, const int32_t *__restrict__ ke_in, int64_t tokens,
                                                          float scale2, const float *__restrict__ lse, const float *__restrict__ logits,
                                                          int64_t lg_stride, float grad_scale, float inv_heads, float *__restrict__ loss,
                                                          float *__restrict__ d_logits, int64_t dl_stride, float *__restrict__ target,
                                                          int64_t tg_stride, float *__restrict__ lse_out)
{
    constexpr int H = 16 * HT;
    constexpr int NKS = HT >= 5 ? 2 : 1;                     // key subtiles a computing wave takes
    constexpr int NT = HT >= 3 ? 2 : 1;                      // tokens a computing wave takes
    constexpr int SLOTS = 4 * (2 / NKS);                     // (m, l) pairs a (token, head) ends the lse pass with
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][IKD_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) float psum[LSE ? 1 : 2][IKD_RUN][HT][SMLA_TILE];   // a head tile's sums of the tile's keys
    __shared__ float red[IKD_RUN][IKD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int64_t m0 = (int64_t)blockIdx.x * IKD_RUN;

    // the run's ranges, clamped to [0, s] as the indexer's forward clamps them; an empty one (and a token beyond m) is [0, 0)
    int lo[IKD_RUN], hi[IKD_RUN];
#pragma unroll
    for (int t = 0; t < IKD_RUN; ++t) {
        lo[t] = hi[t] = 0;
        if (m0 + t < tokens) {
            const int a = ikd_clamp(ks_in[m0 + t], n_keys), b = ikd_clamp(ke_in[m0 + t], n_keys);
            if (b > a) lo[t] = a, hi[t] = b;
        }
    }
    // the first tile >= tl that meets one of the ranges (the same in every thread)
    auto next_live = [&](int tl) -> int {
        int best = IKD_END;
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t)
            if (hi[t] > lo[t] && tl * SMLA_TILE < hi[t]) {
                const int first = lo[t] / SMLA_TILE;
                const int cand = tl > first ? tl : first;
                best = cand < best ? cand : best;
            }
        return best;
    };

    // the wave's share (the table at the head of the file), wave-uniform
    const int ht0 = wave % HT, r1 = wave / HT;
    const int ks0 = NKS == 2 ? 0 : r1 % 2, r2 = NKS == 2 ? r1 : r1 / 2;
    const int tk0 = NT == 2 ? 0 : r2 % 2, r3 = NT == 2 ? r2 : r2 / 2;
    const bool active = r3 == 0;

    // the wave's q as B-operand fragments: head 16 ht0 + (l & 15), the eight d at 32 s + 8 (l >> 4); and its heads' lse in the log2 domain
    smla_v4u qf[NT][SMLA_KSTEPS];
    float lseb[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        lseb[ti] = 0.f;
#pragma unroll
        for (int s = 0; s < SMLA_KSTEPS; ++s) qf[ti][s] = smla_v4u{0, 0, 0, 0};
        if (active && m0 + tk0 + ti < tokens) {
            const int64_t head = (m0 + tk0 + ti) * H + 16 * ht0 + hl;
            const uint16_t *qrow = q + (head * SMLA_D + 8 * g);
#pragma unroll
            for (int s = 0; s < SMLA_KSTEPS; ++s) qf[ti][s] = *reinterpret_cast<const smla_v4u *>(qrow + 32 * s);
            if constexpr (!LSE) lseb[ti] = lse[head] * IKD_L2E;
        }
    }

    // the finisher of the loss pass: wave 7, lane l token l >> 5 and key l & 31 of a tile
    const int fk = lane >> 5, fj = lane & 31;
    const bool finisher = !LSE && wave == IKD_WAVES - 1 && m0 + fk < tokens;
    const int flo = fk ? lo[1] : lo[0], fhi = fk ? hi[1] : hi[0];
    float big_l = 0.f;

    if constexpr (!LSE) {
        // L = ln sum_n exp(logits[t, n]) over each token's range
        float mx[IKD_RUN], esum[IKD_RUN];
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t) {
            const float *lrow = logits + (m0 + t) * lg_stride;
            mx[t] = -__builtin_inff();
            for (int n = lo[t] + tid; n < hi[t]; n += IKD_THREADS) mx[t] = __builtin_fmaxf(mx[t], lrow[n]);
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) mx[t] = __builtin_fmaxf(mx[t], __shfl_xor(mx[t], x, 64));
            if (lane == 0) red[t][wave] = mx[t];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t) {
            mx[t] = red[t][0];
#pragma unroll
            for (int w = 1; w < IKD_WAVES; ++w) mx[t] = __builtin_fmaxf(mx[t], red[t][w]);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t) {
            const float *lrow = logits + (m0 + t) * lg_stride;
            esum[t] = 0.f;
            for (int n = lo[t] + tid; n < hi[t]; n += IKD_THREADS) esum[t] = esum[t] + __builtin_amdgcn_exp2f((lrow[n] - mx[t]) * IKD_L2E);
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) esum[t] = esum[t] + __shfl_xor(esum[t], x, 64);
            if (lane == 0) red[t][wave] = esum[t];
        }
        __syncthreads();
        float bl[IKD_RUN];
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t) {
            float sum = red[t][0];
#pragma unroll
            for (int w = 1; w < IKD_WAVES; ++w) sum = sum + red[t][w];
            bl[t] = mx[t] + __builtin_amdgcn_logf(sum) * IKD_LN2;                          // (unused for an empty token)
        }
        big_l = fk ? bl[1] : bl[0];

        // +0 at every column of a tile the walk does not visit (those of a visited tile are the finisher's)
#pragma unroll
        for (int t = 0; t < IKD_RUN; ++t) {
            if (m0 + t >= tokens) continue;
            for (int n = tid; n < n_keys; n += IKD_THREADS) {
                const int tl = n / SMLA_TILE;
                bool live = false;
#pragma unroll
                for (int u = 0; u < IKD_RUN; ++u) live = live || (hi[u] > lo[u] && tl * SMLA_TILE < hi[u] && (tl + 1) * SMLA_TILE > lo[u]);
                if (!live) {
                    d_logits[(m0 + t) * dl_stride + n] = 0.f;
                    if (target) target[(m0 + t) * tg_stride + n] = 0.f;
                }
            }
        }
    }

    // the tile's chunks of this thread, one tile ahead in registers; the finisher's logit with them
    uint4 raw[IKD_STAGE];
    float lg_next = 0.f;
    auto fetch = [&](int tl) {
#pragma unroll
        for (int c = 0; c < IKD_STAGE; ++c) {
            const int chunk = tid + c * IKD_THREADS, row = chunk / SMLA_CHUNKS, col = chunk % SMLA_CHUNKS;
            const int n = tl * SMLA_TILE + row;
            raw[c] = uint4{0, 0, 0, 0};
            if (chunk < IKD_TILE_CHUNKS && n < n_keys) raw[c] = *reinterpret_cast<const uint4 *>(kv + ((int64_t)n * kv_stride + col * 8));
        }
        if constexpr (!LSE) {
            const int n = tl * SMLA_TILE + fj;
            lg_next = 0.f;
            if (finisher && n >= flo && n < fhi) lg_next = logits[(m0 + fk) * lg_stride + n];
        }
    };

    const uint32_t tile_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)&tile[0][0];
    const uint32_t k_addr = tile_base + (16 * ks0 + hl) * SMLA_ROW_BYTES + 16 * g;

    // S^T of one tile: the wave's head tile against its key subtiles, for its tokens
    smla_v4f acc[NT][NKS];
    auto scores = [&](int par) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int k = 0; k < NKS; ++k) acc[ti][k] = smla_v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < SMLA_KSTEPS; ++s) {
#pragma unroll
            for (int k = 0; k < NKS; ++k) {
                const smla_v4u ka = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(
                    k_addr + par * IKD_TILE_BYTES + k * 16 * SMLA_ROW_BYTES + 64 * s);
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
                    acc[ti][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka), __builtin_bit_cast(smla_v8bf, qf[ti][s]),
                                                                         acc[ti][k], 0, 0, 0);
            }
        }
    };

    // the lse pass: the lane's running maximum and sum per token, in the log2 domain
    float m_run[NT], l_run[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) m_run[ti] = -__builtin_inff(), l_run[ti] = 0.f;
    auto online = [&](int tl) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const int a = (tk0 + ti) ? lo[1] : lo[0], b = (tk0 + ti) ? hi[1] : hi[0];
            float x[NKS][4], top = -__builtin_inff();
#pragma unroll
            for (int k = 0; k < NKS; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = tl * SMLA_TILE + 16 * (ks0 + k) + 4 * g + i;
                    x[k][i] = (n >= a && n < b) ? acc[ti][k][i] * scale2 : -__builtin_inff();
                    top = __builtin_fmaxf(top, x[k][i]);
                }
            const float nm = __builtin_fmaxf(m_run[ti], top);
            const bool any = nm > -__builtin_inff();
            float sum = l_run[ti] * __builtin_amdgcn_exp2f(any ? m_run[ti] - nm : 0.f);
#pragma unroll
            for (int k = 0; k < NKS; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) sum = sum + __builtin_amdgcn_exp2f(any ? x[k][i] - nm : -__builtin_inff());
            l_run[ti] = sum, m_run[ti] = nm;
        }
    };

    // the loss pass: p and the head tile's sums of one tile
    auto head_sums = [&](int par) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int k = 0; k < NKS; ++k) {
                smla_v4f v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = __builtin_amdgcn_exp2f(acc[ti][k][i] * scale2 - lseb[ti]);
#pragma unroll
                for (int x = 1; x <= 8; x <<= 1)
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = v[i] + __shfl_xor(v[i], x, 64);
                if (hl == 0) *reinterpret_cast<smla_v4f *>(&psum[par % (LSE ? 1 : 2)][tk0 + ti][ht0][16 * (ks0 + k) + 4 * g]) = v;
            }
    };

    // key fj of tile tl for token fk, by the finisher: lg is what it asked for with the tile
    float loss_acc = 0.f;
    auto finish = [&](int tl, int par, float lg) {
        const int n = tl * SMLA_TILE + fj;
        if (!finisher || n >= n_keys) return;
        float tv = 0.f, dl = 0.f;
        if (n >= flo && n < fhi) {
            const float *ps = &psum[par % (LSE ? 1 : 2)][fk][0][fj];
            float hs = ps[0];
#pragma unroll
            for (int h = 1; h < HT; ++h) hs = hs + ps[h * SMLA_TILE];
            tv = hs * inv_heads;
            const float a = lg - big_l;
            const float y = __builtin_amdgcn_exp2f(a * IKD_L2E);
            dl = grad_scale * (y - tv);
            if (tv > 0.f) loss_acc = loss_acc + tv * (ikd_log2(tv) * IKD_LN2 - a);
        }
        d_logits[(m0 + fk) * dl_stride + n] = dl;
        if (target) target[(m0 + fk) * tg_stride + n] = tv;
    };

    int cur = next_live(0), prev = 0, step = 0;
    float lg_cur = 0.f, lg_prev = 0.f;
    if (cur != IKD_END) fetch(cur);
#pragma unroll 1
    while (cur != IKD_END) {
        const int par = step & 1;
#pragma unroll
        for (int c = 0; c < IKD_STAGE; ++c) {
            const int chunk = tid + c * IKD_THREADS, row = chunk / SMLA_CHUNKS, col = chunk % SMLA_CHUNKS;
            if (chunk < IKD_TILE_CHUNKS) *reinterpret_cast<uint4 *>(&tile[par][row * SMLA_ROW_BYTES + col * 16]) = raw[c];
        }
        lg_prev = lg_cur, lg_cur = lg_next;
        __syncthreads();
        const int nxt = next_live(cur + 1);
        if (nxt != IKD_END) fetch(nxt);
        if constexpr (!LSE)
            if (step > 0) finish(prev, par ^ 1, lg_prev);
        if (active) {
            scores(par);
            if constexpr (LSE) online(cur);
            else head_sums(par);
        }
        prev = cur, cur = nxt, ++step;
    }
    __syncthreads();

    if constexpr (LSE) {
        // every lane's (m, l) to LDS, then one thread a (token, head): the maximum of the pairs, the rescaled sums ascending
        float2 *pairs = reinterpret_cast<float2 *>(&tile[0][0]);                           // [IKD_RUN][H][SLOTS]
        if (active) {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
                pairs[((tk0 + ti) * H + 16 * ht0 + hl) * SLOTS + (NKS == 2 ? 0 : 4 * ks0) + g] = float2{m_run[ti], l_run[ti]};
        }
        __syncthreads();
        if (tid < IKD_RUN * H && m0 + tid / H < tokens) {
            const float2 *mine = pairs + tid * SLOTS;
            float top = mine[0].x;
#pragma unroll
            for (int i = 1; i < SLOTS; ++i) top = __builtin_fmaxf(top, mine[i].x);
            const bool any = top > -__builtin_inff();
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) sum = sum + mine[i].y * __builtin_amdgcn_exp2f(any ? mine[i].x - top : 0.f);
            lse_out[(m0 + tid / H) * H + tid % H] = any ? (top + __builtin_amdgcn_logf(sum)) * IKD_LN2 : -__builtin_inff();
        }
    } else {
        if (step > 0) finish(prev, (step - 1) & 1, lg_cur);
#pragma unroll
        for (int x = 16; x >= 1; x >>= 1) loss_acc = loss_acc + __shfl_xor(loss_acc, x, 64);
        if (finisher && fj == 0) loss[m0 + fk] = loss_acc;
    }
}

}  // namespace dga

// The checks in the family's clause order: shape, (m == 0), null, alignment, range
extern "C" int dga_indexer_kl_loss_dense(const void *q, const void *kv, const int32_t *ks, const int32_t *ke, int64_t m, int heads, int64_t s,
                                         int64_t kv_stride, double sm_scale, const float *lse, const float *logits, int64_t logits_stride,
                                         double grad_scale, float *loss, float *d_logits, int64_t dl_stride, float *target,
                                         int64_t target_stride, float *lse_out, void *stream)
{
    using namespace dga;
    if (m < 0 || heads < 16 || heads > DGA_SPARSE_MLA_MAX_HEADS || heads % 16 || s < 1 || kv_stride < SMLA_D || logits_stride < s ||
        dl_stride < s || (target && target_stride < s))
        return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !kv || !ks || !ke || !logits || !loss || !d_logits || (!lse && !lse_out)) return DGA_E_NULL;
    // a thread reads 16 bytes of q and of a kv row at once
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(kv) % 16 || kv_stride % 8 || reinterpret_cast<uintptr_t>(ks) % 4 ||
        reinterpret_cast<uintptr_t>(ke) % 4 || reinterpret_cast<uintptr_t>(lse) % 4 || reinterpret_cast<uintptr_t>(logits) % 4 ||
        reinterpret_cast<uintptr_t>(loss) % 4 || reinterpret_cast<uintptr_t>(d_logits) % 4 || reinterpret_cast<uintptr_t>(target) % 4 ||
        (!lse && reinterpret_cast<uintptr_t>(lse_out) % 4))
        return DGA_E_ALIGN;
    const int64_t widest = target && target_stride > dl_stride ? target_stride : dl_stride;
    if (s > 0x7FFFFFFFll - 1024 || logits_stride > 0x7FFFFFFFFFFFFFFFll / 4 / m || widest > 0x7FFFFFFFFFFFFFFFll / 4 / m ||
        kv_stride > 0x7FFFFFFFFFFFFFFFll / 2 / s || (m + IKD_RUN - 1) / IKD_RUN > 0x7FFFFFFFll)
        return DGA_E_RANGE;
    const dim3 grid(static_cast<unsigned>((m + IKD_RUN - 1) / IKD_RUN)), block(IKD_THREADS);
    const float *lse_read = lse ? lse : lse_out;
    auto run = [&](auto lse_kernel, auto loss_kernel) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(q),
                               static_cast<const uint16_t *>(kv), kv_stride, static_cast<int>(s), ks, ke, m,
                               static_cast<float>(sm_scale * 1.4426950408889634), lse_read, logits, logits_stride, static_cast<float>(grad_scale),
                               static_cast<float>(1.0 / heads), loss, d_logits, dl_stride, target, target_stride, lse_out);
        };
        if (!lse) go(lse_kernel);
        go(loss_kernel);
    };
    switch (heads / 16) {
    case 1: run(ikd_kernel<1, true>, ikd_kernel<1, false>); break;
    case 2: run(ikd_kernel<2, true>, ikd_kernel<2, false>); break;
    case 3: run(ikd_kernel<3, true>, ikd_kernel<3, false>); break;
    case 4: run(ikd_kernel<4, true>, ikd_kernel<4, false>); break;
    case 5: run(ikd_kernel<5, true>, ikd_kernel<5, false>); break;
    case 6: run(ikd_kernel<6, true>, ikd_kernel<6, false>); break;
    case 7: run(ikd_kernel<7, true>, ikd_kernel<7, false>); break;
    default: run(ikd_kernel<8, true>, ikd_kernel<8, false>); break;
    }
    return record_hip(hipGetLastError());
}
