// The main attention of the dense stage: MLA attention (absorbed, MQA form, forward) over EVERY key of a token's range -- no list, no gather.
//   dga_mla_fwd_dense   q bf16 [m, heads, 576], kv bf16 [s, 576] (rows kv_stride elements apart), ks / ke int32 [m] clamped to [0, s] as
//                       dga_fp8_mqa_logits clamps them -> out bf16 [m, heads, 512], lse fp32 [m, heads]
//     over the keys n of [lo[t], hi[t]):  s_n = sm_scale sum_d q[t, h, d] kv[n, d];  lse = ln sum_n exp(s_n);
//     out[t, h, :] = sum_n exp(s_n - lse) kv[n, :512];  an empty token (hi <= lo): out = +0, lse = -inf
// With q contiguous this is flash attention of the matrix [m heads, 576] against kv: flat row r = t heads + h, and as heads is a multiple
// of 16 a 16-row tile never straddles a token.  Workgroup g (four waves, one a SIMD) owns the flat rows 64 g .. 64 g + 63, wave w the row
// tile 64 g + 16 w .. + 15 and all 512 value columns of it (128 fp32 accumulators a lane); the wave's token, and with it its range, is
// (64 g + 16 w) / heads -- a workgroup spans one to four consecutive tokens and no wave idles at any head count (a wave beyond m heads,
// in the last workgroup alone, only loads).  The workgroup's q block, 64 contiguous rows, goes to LDS once (rows of 1184 bytes).
// A tile is SMLA_TILE = 32 consecutive kv rows, tile tl the rows 32 tl .. 32 tl + 31.  The walk visits, ascending, the tiles that meet the
// range of one of the four waves; the next one is found from the ranges (dga_indexer_kl_dense.hip's next_live over four ranges), a tile
// outside all of them is neither loaded nor multiplied.  A row is brought by eight threads, 16-byte loads of the chunks tid % 8 + 8 c,
// c = 0 .. 8, one tile ahead in registers; a row outside every range of the workgroup is not read and staged as zeros.  Two LDS images:
// per tile the staged rows go to image step % 2, ONE barrier, the next live tile is asked for, the products run on image step % 2 -- a
// wave can only write image (step + 1) % 2 behind barrier `step`, which every wave reaches after its products of step - 1 on that image.
// Per tile and wave (the arithmetic of dga_sparse_mla.hip's tile, whose bounds carry over):
//   the wave skips both products of a tile that does not meet its own range (wave-uniform; the barrier stays outside the branch)
//   S^T = K Q^T   two 16-key subtiles, each 18 chained v_mfma_f32_16x16x32_bf16 over d ascending from +0 (K the A operand by ds_read_b128):
//                 lane l holds row l & 15 of the wave and the keys 4 (l >> 4) + i and 16 + 4 (l >> 4) + i, i = 0 .. 3
//   x = S (sm_scale log2 e); on a tile that straddles lo or hi, and only there, -inf selected at the keys outside [lo, hi)
//   m' = max(m, max over the tile);  m* = m' or 0 when m' = -inf;  alpha = exp2(m - m*);  p = exp2(x - m*);
//   l = l alpha + (the lane's eight p, fp32, unrounded, ascending key);  O = O alpha (skipped while no lane has alpha != 1)
//   O^T += V^T P^T  32 column tiles, one MFMA each, P rounded to bf16 (RNE) in place, V's fragments by ds_read_b64_tr_b16
// and at the end l over the four lane groups ((l_0 + l_1) + (l_2 + l_3)), out = O (1 / l) rounded to bf16, lse = ln 2 (m + log2 l).
// A key outside the wave's range on a straddling tile has the selected weight 0, which a NaN in its value columns would not survive:
// rows inside one of the call's ranges must be finite, rows outside all of them are never read.
// Every output has one writer, nothing is atomic, the order of every sum follows from the shapes and the ranges: two runs give the same bytes.
// The grid runs the workgroups in descending g (under causal ranges the longest walks start first); DGA_MLA_DENSE_LINEAR_GRID: ascending.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_sparse_mla_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int MLD_WAVES = SMLA_THREADS / 64;                 // 4: the row tiles, and the ranges, of a workgroup
constexpr int MLD_ROWS = 16 * MLD_WAVES;                     // 64 flat rows a workgroup
constexpr int MLD_TILE_BYTES = SMLA_TILE * SMLA_ROW_BYTES;   // 37 888
constexpr int MLD_END = 0x7FFFFFFF;                          // no further tile
static_assert(MLD_WAVES == 4 && MLD_ROWS * SMLA_ROW_BYTES + 2 * MLD_TILE_BYTES <= 160 * 1024, "q and two tile images in LDS");

__device__ __forceinline__ int mld_clamp(int v, int n) { return v < 0 ? 0 : (v > n ? n : v); }

__global__ void __launch_bounds__(SMLA_THREADS) mla_dense_fwd_kernel(const uint16_t *__restrict__ q, const uint16_t *__restrict__ kv,
                                                                     int64_t kv_stride, int n_keys, const int32_t *__restrict__ ks_in,
                                                                     const int32_t *__restrict__ ke_in, int heads, int64_t rows, int64_t blocks,
                                                                     int linear, float scale2, uint16_t *__restrict__ out,
                                                                     float *__restrict__ lse)
{
    __shared__ __attribute__((aligned(16))) unsigned char tile[2][MLD_TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[MLD_ROWS * SMLA_ROW_BYTES];   // the workgroup's q, one row a flat row
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;
    const int64_t block = linear ? (int64_t)blockIdx.x : blocks - 1 - (int64_t)blockIdx.x;
    const int64_t row0 = block * MLD_ROWS;

    // the four waves' ranges, clamped to [0, s] as the indexer's forward clamps them; an empty one (and a wave beyond the rows) is [0, 0)
    int lo[MLD_WAVES], hi[MLD_WAVES];
#pragma unroll
    for (int w = 0; w < MLD_WAVES; ++w) {
        lo[w] = hi[w] = 0;
        if (row0 + 16 * w < rows) {
            const int64_t t = (row0 + 16 * w) / heads;
            const int a = mld_clamp(ks_in[t], n_keys), b = mld_clamp(ke_in[t], n_keys);
            if (b > a) lo[w] = a, hi[w] = b;
        }
    }
    // the first tile >= tl that meets one of the ranges (the same in every thread)
    auto next_live = [&](int tl) -> int {
        int best = MLD_END;
#pragma unroll
        for (int w = 0; w < MLD_WAVES; ++w)
            if (hi[w] > lo[w] && tl * SMLA_TILE < hi[w]) {
                const int first = lo[w] / SMLA_TILE;
                const int cand = tl > first ? tl : first;
                best = cand < best ? cand : best;
            }
        return best;
    };
    const bool computes = row0 + 16 * wave < rows;            // (a wave beyond the last row tile only loads)
    const int mylo = wave == 0 ? lo[0] : wave == 1 ? lo[1] : wave == 2 ? lo[2] : lo[3];
    const int myhi = wave == 0 ? hi[0] : wave == 1 ? hi[1] : wave == 2 ? hi[2] : hi[3];

    // The staging: eight threads a row (row tid / 8 of the tile), thread tid % 8 of them the 16-byte chunks tid % 8 + 8 c of it -- 128
    // contiguous bytes of a row per eight lanes and step.  A row outside every range of the workgroup (rows >= s among them) is zeros.
    const int gpos = tid >> 3, gsub = tid & 7;
    uint4 staged[SMLA_STAGE];
    auto fetch = [&](int tl) {
        const int n = tl * SMLA_TILE + gpos;
        bool in = false;
#pragma unroll
        for (int w = 0; w < MLD_WAVES; ++w) in = in || (n >= lo[w] && n < hi[w]);
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c) staged[c] = uint4{0, 0, 0, 0};
        if (in) {
            const uint16_t *p = kv + ((int64_t)n * kv_stride + gsub * 8);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) staged[c] = *reinterpret_cast<const uint4 *>(p + 64 * c);
        }
    };

    int cur = next_live(0);
    if (cur != MLD_END) fetch(cur);

    // the workgroup's q block, 64 contiguous rows cut off at m heads, goes to LDS once in the tile's row format (the first barrier of
    // the loop stands between this and its use): eight threads a row, 32 rows a pass
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int rb = pass * 32 + gpos;
        if (row0 + rb < rows) {
            const uint16_t *qrow = q + ((row0 + rb) * SMLA_D + gsub * 8);
            uint4 v[SMLA_STAGE];
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + rb * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
        }
    }

    smla_v4f acc[SMLA_CTILES];
#pragma unroll
    for (int ct = 0; ct < SMLA_CTILES; ++ct) acc[ct] = smla_v4f{0.f, 0.f, 0.f, 0.f};
    float mx = -__builtin_inff(), sum = 0.f;                 // the running maximum (log2 domain) of row hl, the lane's share of l

    // LDS addresses of the lane's reads in image 0: K rows hl and 16 + hl at bytes 64 s + 16 g; V blocks by ds_read_b64_tr_b16 (lane
    // 4 q + p of a group gives row q, columns 4 p .. of the block)
    const uint32_t tile_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)&tile[0][0];
    const uint32_t k_addr0 = tile_base + hl * SMLA_ROW_BYTES + 16 * g;
    const uint32_t v_addr0 = tile_base + (4 * g + (hl >> 2)) * SMLA_ROW_BYTES + 8 * (hl & 3);
    const uint32_t q_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)qimg + (wave * 16 + hl) * SMLA_ROW_BYTES + 16 * g;

    int step = 0;
#pragma unroll 1
    while (cur != MLD_END) {
        const int par = step & 1;
        // the staged tile goes to image `par`
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(&tile[par][gpos * SMLA_ROW_BYTES + gsub * 16 + 128 * c]) = staged[c];
        __syncthreads();
        // the next live tile's rows are asked for now and written at the top of the next step
        const int nxt = next_live(cur + 1);
        if (nxt != MLD_END) fetch(nxt);

        const int n0 = cur * SMLA_TILE;
        if (computes && myhi > mylo && n0 < myhi && n0 + SMLA_TILE > mylo) {
            // One wave a SIMD: nobody else hides an LDS read's latency, so the reads run one group ahead of the MFMAs that consume
            // them, in the order written here (the scheduling barriers keep it): two d steps a group for S, four column tiles for O.
            const uint32_t k_addr = k_addr0 + par * MLD_TILE_BYTES, v_addr = v_addr0 + par * MLD_TILE_BYTES;
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
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = (i < 4 ? s0[i] : s1[i - 4]) * scale2;
            if (n0 < mylo || n0 + SMLA_TILE > myhi) {          // the tile straddles an end of the range: an interior one takes no select
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int n = n0 + (i < 4 ? 0 : 16) + 4 * g + (i & 3);
                    x[i] = (n >= mylo && n < myhi) ? x[i] : -__builtin_inff();
                }
            }
            float tmax = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < 8; ++i) tmax = __builtin_fmaxf(tmax, x[i]);   // (a NaN score is passed over here and reaches the result through p)
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
        cur = nxt, ++step;
    }

    if (!computes) return;
    // l over the four lane groups that share a row: (l_0 + l_1) + (l_2 + l_3) in every one of them
    sum = sum + __shfl_xor(sum, 16, 64);
    sum = sum + __shfl_xor(sum, 32, 64);
    const bool empty = sum == 0.f;                           // an empty range (a NaN is not equal to 0 and goes through)
    const float inv = empty ? 0.f : 1.0f / sum;
    const int64_t row = row0 + 16 * wave + hl;
    uint16_t *orow = out + (row * SMLA_DV + 4 * g);
#pragma unroll
    for (int ct = 0; ct < SMLA_CTILES; ++ct) {
        smla_v4bf o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (__bf16)(empty ? 0.f : acc[ct][i] * inv);
        *reinterpret_cast<uint2 *>(orow + 16 * ct) = __builtin_bit_cast(uint2, o);
    }
    if (g == 0) lse[row] = empty ? -__builtin_inff() : (mx + __builtin_amdgcn_logf(sum)) * 0.693147180559945309f;
}

}  // namespace dga

// The checks in the family's clause order: flags, shape, (m == 0), null, alignment, range
extern "C" int dga_mla_fwd_dense(const void *q, const void *kv, const int32_t *ks, const int32_t *ke, int64_t m, int heads, int64_t s,
                                 int64_t kv_stride, double sm_scale, int flags, void *out, float *lse, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_MLA_DENSE_LINEAR_GRID) return DGA_E_RANGE;
    if (m < 0 || heads < 16 || heads > DGA_SPARSE_MLA_MAX_HEADS || heads % 16 || s < 1 || kv_stride < SMLA_D) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !kv || !ks || !ke || !out || !lse) return DGA_E_NULL;
    // a thread reads 16 bytes of q and of a kv row at once, and a lane stores 8 bytes of out at a multiple of 8
    if (reinterpret_cast<uintptr_t>(q) % 16 || reinterpret_cast<uintptr_t>(kv) % 16 || reinterpret_cast<uintptr_t>(out) % 16 || kv_stride % 8 ||
        reinterpret_cast<uintptr_t>(ks) % 4 || reinterpret_cast<uintptr_t>(ke) % 4 || reinterpret_cast<uintptr_t>(lse) % 4)
        return DGA_E_ALIGN;
    if (s > 0x7FFFFFFFll - 1024 || m > 0x7FFFFFFFFFFFFFFFll / 2 / SMLA_D / heads || kv_stride > 0x7FFFFFFFFFFFFFFFll / 2 / s) return DGA_E_RANGE;
    const int64_t rows = m * heads, blocks = (rows + MLD_ROWS - 1) / MLD_ROWS;
    if (blocks > 0x7FFFFFFFll) return DGA_E_RANGE;
    hipLaunchKernelGGL(mla_dense_fwd_kernel, dim3(static_cast<unsigned>(blocks)), dim3(SMLA_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(q), static_cast<const uint16_t *>(kv), kv_stride, static_cast<int>(s), ks, ke, heads, rows,
                       blocks, (flags & DGA_MLA_DENSE_LINEAR_GRID) ? 1 : 0, static_cast<float>(sm_scale * 1.4426950408889634),
                       static_cast<uint16_t *>(out), lse);
    return record_hip(hipGetLastError());
}
