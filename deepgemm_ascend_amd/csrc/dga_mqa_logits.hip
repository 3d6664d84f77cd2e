// The scoring kernel of the lightning indexer (DeepSeek sparse attention): upstream DeepGEMM's fp8_mqa_logits.
//   dga_fp8_mqa_logits   q [M, H, 128] e4m3, k [N, 128] e4m3, kscale [N], weights [M, H], ks / ke int32 [M] -> logits fp32 [M, N]
//     s[m,h,n]    = sum_d q[m,h,d] k[n,d]
//     logits[m,n] = kscale[n] * sum_h weights[m,h] * relu(s[m,h,n])      for clamp(ks[m]) <= n < clamp(ke[m]),   -inf elsewhere
// A GEMM of [M H, 128] x [128, N] whose epilogue folds the H heads away.  Arithmetic: the library's default policy -- codes converted to
// bf16 exactly (v_cvt_scalef32_pk_bf16_fp8 at scale 1), s = four chained v_mfma_f32_16x16x32_bf16 over d ascending, fp32 accumulation.
//
// Tile: a workgroup of four waves owns MQA_BN = 256 keys and a run of MQA_BM = 64 consecutive tokens.  Wave w owns the 64 keys
// 64 w .. 64 w + 63 of the block: their B fragments (four 16-key tiles x four k steps, 64 VGPRs) are read from global memory and converted
// once and stay in registers for the workgroup's life.  The tokens of the run are walked one at a time: a token's H x 128 codes are read
// once per workgroup, 8 bytes a lane, in the order the A fragments want them -- fragment (head tile ht, k step ks) is 512 contiguous bytes
// of LDS, lane l's 8 codes q[m, 16 ht + (l & 15), 32 ks + 8 (l >> 4) ..] at byte 8 l, so that writes and reads are both linear in the
// lane -- into one of two LDS images; the next token's loads are in flight while this one is multiplied (one barrier a token).
// The heads are the accumulator's rows (C/D: col = lane & 15, row = 4 (lane >> 4) + reg), so a lane holds four heads of one key per
// 16 x 16 tile and the head sum needs no LDS.  Its order, fixed by H alone: lane group g = lane >> 4 forms
//     P_g = fma chain over (ht ascending, reg ascending) of weights[m, 16 ht + 4 g + reg] * relu(s), starting from +0,
// then the groups are added as (P_0 + P_2) + (P_1 + P_3) by a two-step exchange (lane ^ 32, then lane ^ 16) that halves what a lane keeps
// at each step, so that lane l ends with key 16 (l >> 4) + (l & 15) = l of the wave's 64: one dword store a lane, 256 contiguous bytes a
// wave.  kscale[n] multiplies once, after the sum.  relu is s < 0 ? 0 : s, which keeps a NaN (a NaN code in q poisons its row, one in k
// its column, inside the ranges).  No atomics; every element of logits is written by exactly one lane.
// Ranges are read on the device (lane i of every wave holds token i's clamped pair; a ballot gives the run's active tokens).  A token whose
// range misses the key block is neither loaded nor multiplied, by any wave, and a wave whose 64 keys miss the range skips its MFMAs
// (both branches are wave-uniform); such elements are stored as -inf.  A workgroup whose whole run misses the block never reads k.
// Nothing at or beyond row N of k / kscale or row M of q / weights / ks / ke is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_mqa_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int MQA_THREADS = 256;
constexpr int MQA_BN = DGA_MQA_LOGITS_BLOCK_N;   // keys of a workgroup
constexpr int MQA_BM = DGA_MQA_LOGITS_BLOCK_M;   // tokens of a workgroup's run: one per lane of a wave (the ballot below)
constexpr int MQA_D = DGA_MQA_LOGITS_HEAD_DIM;
static_assert(MQA_BM == 64 && MQA_BN == 64 * (MQA_THREADS / 64) && MQA_D == 128, "the kernel's geometry");

__device__ __forceinline__ int mqa_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }

template <int H>
__global__ void __launch_bounds__(MQA_THREADS) mqa_logits_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ k,
                                                                 const float *__restrict__ kscale, const float *__restrict__ weights,
                                                                 const int32_t *__restrict__ ks_in, const int32_t *__restrict__ ke_in,
                                                                 float *__restrict__ out, int64_t m_n, int n_n, int key_blocks)
{
    constexpr int HT = H / 16;        // head tiles
    constexpr int FR = HT * 4;        // A fragments of a token: (head tile, k step), 512 bytes each
    constexpr int FPW = FR / 4;       // ... staged by one wave
    __shared__ mqa_v2i image[2][FR * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    // key blocks fastest, so that the workgroups in flight share a few token runs; rotated by the run, so that under a causal mask the
    // skipped pairs fall on every XCD alike (workgroup i runs on XCD i % 8: unrotated, an XCD would own the same key blocks in every run)
    const int run = blockIdx.x / key_blocks;
    const int kb =(blockIdx.x % key_blocks + run % key_blocks) % key_blocks;
    const int64_t m0 = (int64_t)run * MQA_BM;
    const int cnt = m_n - m0 < MQA_BM ? (int)(m_n - m0) : MQA_BM;
    const int n0 = kb * MQA_BN;                                          // (n_n <= DGA_MQA_LOGITS_MAX_N: no overflow below)
    const int n1 = n_n - n0 < MQA_BN ? n_n : n0 + MQA_BN;                // the block's keys: [n0, n1)
    const int nw0 = n0 + 64 * wave;
    const int nw1 = nw0 + 64 < n1 ? nw0 + 64 : n1;                       // the wave's keys: [nw0, nw1), empty in a ragged last block
    const int my_n = nw0 + lane;
    const bool my_ok = my_n < n_n;
    const float ninf = -__builtin_inff();

    // lane i: token m0 + i's range, clamped to [0, N]
    int lo_v = 0, hi_v = 0;
    if (lane < cnt) {
        lo_v = mqa_clamp(ks_in[m0 + lane], n_n);
        hi_v = mqa_clamp(ke_in[m0 + lane], n_n);
    }
    const uint64_t active = __ballot(lo_v < hi_v && lo_v < n1 && hi_v > n0);   // tokens whose range meets the block (the same in every wave)
    float *orow = out + m0 * n_n + my_n;
    if (active == 0) {
        if (my_ok)
            for (int i = 0; i < cnt; ++i) orow[(int64_t)i * n_n] = ninf;
        return;
    }

    // the wave's B fragments: lane l holds k[nw0 + 16 nt + (l & 15)][32 ks + 8 (l >> 4) ..]
    mqa_v4i bf[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = nw0 + 16 * nt + c;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            mqa_v2i raw = {0, 0};
            if (n < n_n) raw = *(const mqa_v2i *)(k + (int64_t)n * MQA_D + 32 * s + 8 * g);
            bf[nt][s] = mqa_cvt8(raw);
        }
    }
    const float scale = my_ok ? kscale[my_n] : 0.f;

    mqa_v2i qr[FPW];
    mqa_v4f wr[HT];
    auto fetch = [&](int i) {
        const int64_t m = m0 + i;
#pragma unroll
        for (int j = 0; j < FPW; ++j) {
            const int f = wave * FPW + j;
            qr[j] = *(const mqa_v2i *)(q + (m * H + (f >> 2) * 16 + c) * MQA_D + 32 * (f & 3) + 8 * g);
        }
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) wr[ht] = *(const mqa_v4f *)(weights + m * H + 16 * ht + 4 * g);
    };
    fetch(__builtin_ctzll(active));

    int par = 0;
    for (int i = 0; i < cnt; ++i) {
        if (!((active >> i) & 1)) {                     // the whole workgroup alike
            if (my_ok) orow[(int64_t)i * n_n] = ninf;
            continue;
        }
        mqa_v2i *img = image[par];
        par ^= 1;
#pragma unroll
        for (int j = 0; j < FPW; ++j) img[(wave * FPW + j) * 64 + lane] = qr[j];
        mqa_v4f w[HT];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) w[ht] = wr[ht];
        // one barrier a token: the image written here was last read two active tokens ago, before every wave's previous barrier
        __syncthreads();
        const uint64_t rest = i < 63 ? active >> (i + 1) : 0;
        if (rest) fetch(i + 1 + __builtin_ctzll(rest));

        const int lo = __builtin_amdgcn_readlane(lo_v, i), hi = __builtin_amdgcn_readlane(hi_v, i);
        float val = ninf;
        if (lo < nw1 && hi > nw0) {                     // wave-uniform; false for a wave without keys (nw1 <= nw0 <= lo or hi <= nw0)
            float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) {
                mqa_v4i af[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) af[s] = mqa_cvt8(img[(ht * 4 + s) * 64 + lane]);
                mqa_head_tile(af, bf, w[ht], p);
            }
            const float v = mqa_exchange(p, g);
            if (my_n >= lo && my_n < hi) val = v * scale;
        }
        if (my_ok) orow[(int64_t)i * n_n] = val;
    }
}

}  // namespace dga

extern "C" int dga_fp8_mqa_logits(const void *q, const void *k, const float *kscale, const float *weights, const int32_t *ks, const int32_t *ke,
                                  int64_t m, int64_t n, int heads, int head_dim, float *logits, void *stream)
{
    using namespace dga;
    if (m < 0 || n < 1 || head_dim != MQA_D || (heads != 32 && heads != 64)) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !k || !kscale || !weights || !ks || !ke || !logits) return DGA_E_NULL;
    // a lane reads 8 codes and four weights at once
    if (reinterpret_cast<uintptr_t>(q) % 8 || reinterpret_cast<uintptr_t>(k) % 8 || reinterpret_cast<uintptr_t>(weights) % 16 ||
        reinterpret_cast<uintptr_t>(kscale) % 4 || reinterpret_cast<uintptr_t>(logits) % 4)
        return DGA_E_ALIGN;
    if (n > DGA_MQA_LOGITS_MAX_N) return DGA_E_RANGE;
    const int64_t key_blocks = (n + MQA_BN - 1) / MQA_BN, runs = (m + MQA_BM - 1) / MQA_BM;
    if (runs > 0x7FFFFFFFll / key_blocks) return DGA_E_RANGE;
    const dim3 grid(static_cast<unsigned>(runs * key_blocks)), block(MQA_THREADS);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<const uint8_t *>(q), static_cast<const uint8_t *>(k), kscale, weights, ks, ke,
                           logits, m, static_cast<int>(n), static_cast<int>(key_blocks));
    };
    if (heads == 64) launch(mqa_logits_kernel<64>);
    else launch(mqa_logits_kernel<32>);
    return record_hip(hipGetLastError());
}
