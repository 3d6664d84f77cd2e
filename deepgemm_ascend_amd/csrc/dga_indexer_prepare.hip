// What produces the operands of the indexer (dga_fp8_mqa_logits, dga_fp8_paged_mqa_logits) from the projections' outputs, and carries the
// indexer's gradients back to them:
//   dga_indexer_prepare_q     q [m, heads, 128] -> RoPE, Hadamard rotation, 1x128 quantiser: codes, q_scale [m, heads], folded weights
//   dga_indexer_prepare_k     k [n, 128] -> (LayerNorm,) RoPE, rotation, quantiser: codes + kscale and / or the paged key cache; mean, rstd
//   dga_indexer_prepare_bwd   grad fp32 [rows, 128] (/ row_div) -> rotation, transposed RoPE -> grad_in; d_weights_raw
// All three in the quantisers' geometry: 256 threads, the sixteen lanes of a DPP row on one row of 128 values, lane `sub` holding the 8
// consecutive elements 8 sub .. 8 sub + 7, 16 rows a workgroup.  A row never leaves its sixteen lanes: no LDS allocation, no barrier.
// Element index = 8 sub + j, so bits 0 .. 2 of it are in-lane and bits 3 .. 6 are the lane's: the rotation's strides 1, 2, 4 are 24
// in-lane add / sub, its strides 8, 16, 32, 64 exchange with lane sub ^ 1, 2, 4, 8 (quad_perm, quad_perm, ds_swizzle in bit-mask mode,
// row_ror:8).  The lane whose bit is set computes partner - own, so the butterfly comes out in natural (Sylvester) order.  The RoPE's
// non-interleaved pairs (x[i], x[i + 32]) sit in lanes sub and sub ^ 4 (sub < 8) at the same j; interleaved pairs are in-lane.  The
// LayerNorm's two sums are the lane's 8 terms ascending, then the tree over sub ^ 1, 2, 4, 8 (every lane ends with the same bits).
// Every operation below is one float32 rounding: the unit is compiled without contraction (the pragma below, and -ffp-contract=off in the
// Makefile), and numpy float32 reproduces every value that reaches the quantiser to the bit (tests/indexer_prepare_ref.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr float PREP_C = 0x1.6a09e6p-4f;   // the float32 nearest 128^-1/2 (0x3DB504F3)
constexpr int PREP_PAGED_KEYS = DGA_PAGED_MQA_LOGITS_BLOCK_KV;
constexpr int PREP_PAGED_SCALES = PREP_PAGED_KEYS * 128;
static_assert(PREP_PAGED_SCALES + 4 * PREP_PAGED_KEYS == DGA_PAGED_MQA_LOGITS_BLOCK_BYTES && DGA_MQA_LOGITS_HEAD_DIM == 128, "the layout of a block");

// the value lane sub ^ BIT of the same DPP row holds, in every lane
template <int BIT> __device__ __forceinline__ float row_partner(float x)
{
    const int xi = __builtin_bit_cast(int, x);
    if constexpr (BIT == 1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0xB1, 0xF, 0xF, false));        // quad_perm [1,0,3,2]
    else if constexpr (BIT == 2) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    else if constexpr (BIT == 4) return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(xi, 0x101F));   // bit-mask mode: and 0x1F, or 0, xor 4
    else return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, xi, 0x128, 0xF, 0xF, false));                         // row_ror:8
}

// the sum of p over the 16 lanes of the row as the tree ((l, l^1), ^2, ^4, ^8): the same bits in every lane (fp32 addition commutes)
__device__ __forceinline__ float row16_sum(float p)
{
    p = p + row_partner<1>(p);
    p = p + row_partner<2>(p);
    p = p + row_partner<4>(p);
    p = p + row_partner<8>(p);
    return p;
}

// one cross-lane stage of the rotation: the pair (u, v) held by lanes (l, l ^ BIT), u in the lane whose bit is clear, becomes
// (fl(u + v), fl(u - v)).  The lane with the bit set computes partner - own = partner + (-own): the negation is exact.
template <int BIT> __device__ __forceinline__ void butterfly_lanes(float (&v)[8], int sub)
{
    const bool upper = (sub & BIT) != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float p = row_partner<BIT>(v[j]);
        v[j] = p + (upper ? -v[j] : v[j]);
    }
}

// y = C H x, H the 128-point Walsh-Hadamard matrix in natural order: strides 1, 2, 4 in the lane, 8 .. 64 across the row, then one product
__device__ __forceinline__ void hadamard128(float (&v)[8], int sub)
{
#pragma unroll
    for (int h = 1; h < 8; h <<= 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i & h) continue;
            const float u = v[i], w = v[i + h];
            v[i] = u + w;
            v[i + h] = u - w;
        }
    }
    butterfly_lanes<1>(v, sub);
    butterfly_lanes<2>(v, sub);
    butterfly_lanes<4>(v, sub);
    butterfly_lanes<8>(v, sub);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] * PREP_C;
}

// RoPE on elements 0 .. 63 of the row (lanes sub < 8); cs = the token's 64 table entries, cos of frequency i at [i], sin at [32 + i].
// Forward a' = fl(fl(a c) - fl(b s)), b' = fl(fl(a s) + fl(b c)); transposed a' = fl(fl(a c) + fl(b s)), b' = fl(fl(b c) - fl(a s)):
// the forward with -s, and negating s is exact.  Lanes 8 .. 15 read nothing of the table and keep their values.
template <bool INTER> __device__ __forceinline__ void rope64(float (&v)[8], int sub, const float *cs, bool transposed)
{
    if constexpr (INTER) {
        if (sub < 8) {   // pairs (x[2 i], x[2 i + 1]), i = 4 sub .. 4 sub + 3: in the lane
            const v4f_c c = *(const v4f_c *)(cs + 4 * sub), s = *(const v4f_c *)(cs + 32 + 4 * sub);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = v[2 * i], b = v[2 * i + 1], sn = transposed ? -s[i] : s[i];
                v[2 * i] = a * c[i] - b * sn;
                v[2 * i + 1] = a * sn + b * c[i];
            }
        }
    } else {
        // pairs (x[i], x[i + 32]): a in lane i / 8 (sub < 4), b in lane sub ^ 4 at the same j; both need frequency 8 (sub & 3) + j
        float c[8], s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = s[j] = 0.f;
        if (sub < 8) {
            const float *t = cs + 8 * (sub & 3);
            const v4f_c c0 = *(const v4f_c *)t, c1 = *(const v4f_c *)(t + 4), s0 = *(const v4f_c *)(t + 32), s1 = *(const v4f_c *)(t + 36);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = c0[j]; c[j + 4] = c1[j];
                s[j] = s0[j]; s[j + 4] = s1[j];
            }
        }
        // the lane that holds a takes -s (forward), the one that holds b takes +s; transposed the other way round
        const bool plus = ((sub & 4) != 0) != transposed;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = row_partner<4>(v[j]);        // (every lane of the row: the exchange is outside the branch)
            const float r = v[j] * c[j] + p * (plus ? s[j] : -s[j]);
            v[j] = sub < 8 ? r : v[j];
        }
    }
}

// the token's position, int32 or int64 as the caller holds it
__device__ __forceinline__ int64_t position_of(const void *positions, bool pos64, int64_t tok)
{
    return pos64 ? ((const int64_t *)positions)[tok] : (int64_t)((const int32_t *)positions)[tok];
}

// 8 values of a [128] vector that is of type T or fp32, decided by a uniform flag (the LayerNorm's weight and bias)
template <typename T> __device__ __forceinline__ void load8_vec(const void *p, bool f32, int i, float (&v)[8])
{
    if (f32) Elem<float>::load8(p, i, v);
    else Elem<T>::load8(p, i, v);
}

// One row of q per 16 lanes: row = token * heads + head.  The row is asked for before the position is known (it is inside the tensor
// either way); a token whose position lies outside [0, table_rows) leaves here, before the table is touched and before any store.
template <typename T, bool INTER>
__global__ void __launch_bounds__(256) indexer_prepare_q_kernel(const void *q, const void *positions, bool pos64, const float *cos_sin,
                                                                int64_t table_rows, const void *weights, bool w_bf16, float weight_scale,
                                                                int64_t rows, int64_t heads, bool small, uint8_t *q_fp8, float *q_scale,
                                                                float *weights_out, bool ue8m0)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (row >= rows) return;                                  // whole 16-lane groups leave together, here and below
    const int sub = threadIdx.x & 15;
    const typename Elem<T>::Raw raw = Elem<T>::load8_raw(q, row * 128 + sub * 8);
    const int64_t pos = position_of(positions, pos64, udiv(row, heads, small));
    if ((uint64_t)pos >= (uint64_t)table_rows) return;
    float v[8];
    Elem<T>::unpack8(raw, v);
    rope64<INTER>(v, sub, cos_sin + pos * 64, false);
    hadamard128(v, sub);
    float s;
    uint32_t w0, w1;
    quant_row_block(v, ue8m0, s, w0, w1);
    store_codes8(q_fp8 + row * 128 + sub * 8, w0, w1, true, 0, 8);
    if (sub == 0) {
        q_scale[row] = s;
        if (weights) {
            const float w = w_bf16 ? Elem<Bf16Tag>::load(weights, row) : ((const float *)weights)[row];
            weights_out[row] = (w * weight_scale) * s;
        }
    }
}

// One key per 16 lanes.  NORM: LayerNorm first, its statistics in one order -- the lane's 8 terms ascending, then row16_sum's tree --
// mean = fl(sum x / 128), var = fl(sum fl(fl(x - mean)^2) / 128) (a product by 2^-7: the same rounding), rstd = fl(1 / fl(sqrt(fl(var +
// eps)))) by the correctly rounded square root and division; z = fl(fl(fl(fl(x - mean) rstd) gamma) + beta) (no beta: no addition).
// A slot outside [0, slots) skips the cache write only.
template <typename T, bool INTER, bool NORM>
__global__ void __launch_bounds__(256) indexer_prepare_k_kernel(const void *k, const void *positions, bool pos64, const float *cos_sin,
                                                                int64_t table_rows, const void *gamma, const void *beta, bool w_f32, float eps,
                                                                int64_t n, uint8_t *k_fp8, float *kscale, float *mean_out, float *rstd_out,
                                                                uint8_t *kv, const int64_t *slot_mapping, int64_t slots, int64_t block_stride,
                                                                bool ue8m0)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (row >= n) return;
    const int sub = threadIdx.x & 15;
    const typename Elem<T>::Raw raw = Elem<T>::load8_raw(k, row * 128 + sub * 8);
    const int64_t pos = position_of(positions, pos64, row);
    if ((uint64_t)pos >= (uint64_t)table_rows) return;
    float v[8];
    Elem<T>::unpack8(raw, v);
    if constexpr (NORM) {
        float g[8], b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        load8_vec<T>(gamma, w_f32, sub * 8, g);
        if (beta) load8_vec<T>(beta, w_f32, sub * 8, b);
        float p = v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) p = p + v[j];
        const float mean = row16_sum(p) * 0x1p-7f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] - mean;
        p = v[0] * v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) p = p + v[j] * v[j];
        const float var = row16_sum(p) * 0x1p-7f;
        const float rstd = 1.f / __builtin_sqrtf(var + eps);
        if (sub == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = (v[j] * rstd) * g[j];
            if (beta) v[j] = v[j] + b[j];
        }
    }
    rope64<INTER>(v, sub, cos_sin + pos * 64, false);
    hadamard128(v, sub);
    float s;
    uint32_t w0, w1;
    quant_row_block(v, ue8m0, s, w0, w1);
    if (k_fp8) {
        store_codes8(k_fp8 + row * 128 + sub * 8, w0, w1, true, 0, 8);
        if (sub == 0) kscale[row] = s;
    }
    if (kv) {
        const int64_t slot = slot_mapping[row];
        if ((uint64_t)slot < (uint64_t)slots) {
            const int key = (int)(slot % PREP_PAGED_KEYS);
            uint8_t *blk = kv + slot / PREP_PAGED_KEYS * block_stride;
            if (sub == 0) *(float *)(blk + PREP_PAGED_SCALES + 4 * key) = s;
            *(v2i_c *)(blk + 128 * key + 8 * sub) = v2i_c{(int)w0, (int)w1};
        }
    }
}

// One gradient row per 16 lanes, rows `stride` floats apart: g = fl(grad / row_div[row]) (IEEE division), the rotation (its own
// transpose), the transposed RoPE, one rounding to O.  d_weights_raw = fl(fl(d_weights weight_scale) row_div).
template <typename O, bool INTER>
__global__ void __launch_bounds__(256) indexer_prepare_bwd_kernel(const float *grad, int64_t stride, const void *positions, bool pos64,
                                                                  const float *cos_sin, int64_t table_rows, const float *row_div,
                                                                  const float *d_weights, float weight_scale, int64_t rows, int64_t heads,
                                                                  bool small, void *grad_in, float *d_weights_raw)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (row >= rows) return;
    const int sub = threadIdx.x & 15;
    const Elem<float>::Raw raw = Elem<float>::load8_raw(grad, row * stride + sub * 8);
    const int64_t pos = position_of(positions, pos64, udiv(row, heads, small));
    if ((uint64_t)pos >= (uint64_t)table_rows) return;
    float v[8];
    Elem<float>::unpack8(raw, v);
    float div = 1.f;
    if (row_div) {
        div = row_div[row];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] / div;
    }
    hadamard128(v, sub);
    rope64<INTER>(v, sub, cos_sin + pos * 64, true);
    Store8<O>::run(grad_in, row * 128 + sub * 8, v, true);
    if (d_weights && sub == 0) d_weights_raw[row] = (d_weights[row] * weight_scale) * div;
}

inline bool prep_aligned(const void *p, unsigned a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// What the three entries ask of the flags, the positions and the table, in one order: DGA_E_RANGE for an unknown flag is the caller's
// first clause; here DGA_E_NULL, then DGA_E_ALIGN (cos_sin 16 bytes, positions their own width), then DGA_E_RANGE (a table beyond int64)
inline int prep_table_check(const void *positions, int pos_i64, const float *cos_sin, int64_t table_rows)
{
    if (!positions || !cos_sin) return DGA_E_NULL;
    if (!prep_aligned(cos_sin, 16) || !prep_aligned(positions, pos_i64 ? 8 : 4)) return DGA_E_ALIGN;
    if (table_rows > 0x7FFFFFFFFFFFFFFFll / 256) return DGA_E_RANGE;
    return DGA_OK;
}

constexpr int PREP_FLAGS = DGA_CAST_UE8M0 | DGA_INDEXER_PREPARE_INTERLEAVED;

}  // namespace dga

extern "C" int dga_indexer_prepare_q(const void *q, int q_dtype, int64_t m, int64_t heads, const void *positions, int pos_i64,
                                     const float *cos_sin, int64_t table_rows, const void *weights, int w_dtype, float weight_scale,
                                     void *q_fp8, float *q_scale, float *weights_out, int flags, void *stream)
{
    using namespace dga;
    if (flags & ~PREP_FLAGS) return DGA_E_RANGE;
    if (m < 0 || heads < 1 || table_rows < 0) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!q || !q_fp8 || !q_scale || !weights != !weights_out) return DGA_E_NULL;
    if (int rc = prep_table_check(positions, pos_i64, cos_sin, table_rows)) return rc;
    return dispatch_dtype(q_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (weights && w_dtype != DGA_DT_FP32 && w_dtype != DGA_DT_BF16) return DGA_E_DTYPE;
        if (!prep_aligned(q, 16) || !prep_aligned(q_fp8, 8) || !prep_aligned(q_scale, 4) || !prep_aligned(weights_out, 4) ||
            !prep_aligned(weights, w_dtype == DGA_DT_BF16 ? 2 : 4))
            return DGA_E_ALIGN;
        if (m > 0x7FFFFFFFFFFFFFFFll / 512 / heads) return DGA_E_RANGE;   // (rows * 128 elements of 4 bytes stay inside int64)
        const int64_t rows = m * heads;
        unsigned grid;
        if (int rc = grid_of_blocks(rows, 1, grid)) return rc;
        const bool small = rows <= 0xFFFFFFFFll && heads <= 0xFFFFFFFFll;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), q, positions, pos_i64 != 0, cos_sin,
                               table_rows, weights, w_dtype == DGA_DT_BF16, weight_scale, rows, heads, small, static_cast<uint8_t *>(q_fp8),
                               q_scale, weights_out, (flags & DGA_CAST_UE8M0) != 0);
        };
        if (flags & DGA_INDEXER_PREPARE_INTERLEAVED) launch(indexer_prepare_q_kernel<T, true>);
        else launch(indexer_prepare_q_kernel<T, false>);
        return record_hip(hipGetLastError());
    });
}

extern "C" int dga_indexer_prepare_k(const void *k, int k_dtype, int64_t n, const void *positions, int pos_i64, const float *cos_sin,
                                     int64_t table_rows, const void *norm_weight, const void *norm_bias, int w_dtype, float eps, void *k_fp8,
                                     float *kscale, float *mean, float *rstd, void *kv_cache, int64_t num_blocks, int64_t block_stride,
                                     const int64_t *slot_mapping, int flags, void *stream)
{
    using namespace dga;
    if (flags & ~PREP_FLAGS) return DGA_E_RANGE;
    if (n < 0 || table_rows < 0 || (kv_cache && (num_blocks < 1 || block_stride < DGA_PAGED_MQA_LOGITS_BLOCK_BYTES))) return DGA_E_SHAPE;
    if (n == 0) return DGA_OK;
    if (!k || (!k_fp8 && !kv_cache) || !k_fp8 != !kscale || !kv_cache != !slot_mapping || (norm_bias && !norm_weight) ||
        (norm_weight && (!mean || !rstd)))
        return DGA_E_NULL;
    if (int rc = prep_table_check(positions, pos_i64, cos_sin, table_rows)) return rc;
    return dispatch_dtype(k_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (norm_weight && w_dtype != k_dtype && w_dtype != DGA_DT_FP32) return DGA_E_DTYPE;
        if (norm_weight && (!(eps >= 0.f) || std::isinf(eps))) return DGA_E_RANGE;
        if (!prep_aligned(k, 16) || !prep_aligned(k_fp8, 8) || !prep_aligned(kscale, 4) || !prep_aligned(mean, 4) || !prep_aligned(rstd, 4) ||
            !prep_aligned(norm_weight, 16) || !prep_aligned(norm_bias, 16) || !prep_aligned(kv_cache, 16) || !prep_aligned(slot_mapping, 8) ||
            (kv_cache && block_stride % 16 != 0))
            return DGA_E_ALIGN;
        if (n > 0x7FFFFFFFFFFFFFFFll / 512 || (kv_cache && num_blocks > 0x7FFFFFFFFFFFFFFFll / block_stride)) return DGA_E_RANGE;
        unsigned grid;
        if (int rc = grid_of_blocks(n, 1, grid)) return rc;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), k, positions, pos_i64 != 0, cos_sin,
                               table_rows, norm_weight, norm_bias, w_dtype == DGA_DT_FP32, eps, n, static_cast<uint8_t *>(k_fp8), kscale, mean,
                               rstd, static_cast<uint8_t *>(kv_cache), slot_mapping, kv_cache ? num_blocks * PREP_PAGED_KEYS : 0, block_stride,
                               (flags & DGA_CAST_UE8M0) != 0);
        };
        const bool inter = (flags & DGA_INDEXER_PREPARE_INTERLEAVED) != 0;
        if (norm_weight) {
            if (inter) launch(indexer_prepare_k_kernel<T, true, true>);
            else launch(indexer_prepare_k_kernel<T, false, true>);
        } else {
            if (inter) launch(indexer_prepare_k_kernel<T, true, false>);
            else launch(indexer_prepare_k_kernel<T, false, false>);
        }
        return record_hip(hipGetLastError());
    });
}

extern "C" int dga_indexer_prepare_bwd(const float *grad, int64_t rows, int64_t heads, int64_t grad_stride, const void *positions,
                                       int pos_i64, const float *cos_sin, int64_t table_rows, const float *row_div, const float *d_weights,
                                       float weight_scale, void *grad_in, int out_dtype, float *d_weights_raw, int flags, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_INDEXER_PREPARE_INTERLEAVED) return DGA_E_RANGE;
    if (rows < 0 || heads < 1 || rows % heads != 0 || grad_stride < 128 || table_rows < 0) return DGA_E_SHAPE;
    if (rows == 0) return DGA_OK;
    if (!grad || !grad_in || !d_weights != !d_weights_raw || (d_weights && !row_div)) return DGA_E_NULL;
    if (int rc = prep_table_check(positions, pos_i64, cos_sin, table_rows)) return rc;
    return dispatch_dtype(out_dtype, [&](auto tag) -> int {
        using O = decltype(tag);
        if (!prep_aligned(grad, 16) || grad_stride % 4 != 0 || !prep_aligned(grad_in, 16) || !prep_aligned(row_div, 4) ||
            !prep_aligned(d_weights, 4) || !prep_aligned(d_weights_raw, 4))
            return DGA_E_ALIGN;
        if (rows > 0x7FFFFFFFFFFFFFFFll / 4 / grad_stride) return DGA_E_RANGE;
        unsigned grid;
        if (int rc = grid_of_blocks(rows, 1, grid)) return rc;
        const bool small = rows <= 0xFFFFFFFFll && heads <= 0xFFFFFFFFll;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), grad, grad_stride, positions, pos_i64 != 0,
                               cos_sin, table_rows, row_div, d_weights, weight_scale, rows, heads, small, grad_in, d_weights_raw);
        };
        if (flags & DGA_INDEXER_PREPARE_INTERLEAVED) launch(indexer_prepare_bwd_kernel<O, true>);
        else launch(indexer_prepare_bwd_kernel<O, false>);
        return record_hip(hipGetLastError());
    });
}
