// The merge of split sparse MLA attention: (partial_out, partial_lse) of P splits of a token's list -> (out, lse) of the whole list.
//   dga_sparse_mla_merge   partial_out fp32 [P, m, heads, 512], partial_lse fp32 [P, m, heads] (natural log), both contiguous, 1 <= P <= 64
//                          -> out bf16 [m, heads, 512], lse fp32 [m, heads]
// The partials are dga_sparse_mla_fwd_partial's (csrc/dga_sparse_mla.hip: the attention kernel over a contiguous range of the list's tiles,
// out = O (1 / l) left in fp32), or any other producer's of the same meaning: ranks of a context-parallel group, chunks of a longer list.
// Arithmetic, per (token, head), fp32, nothing contracted, p ascending -- with L2E = (float)log2 e and LN2 = (float)ln 2:
//   M = fmax over p of partial_lse[p], from -inf (fmax passes over a NaN);   mu = M, or 0 when M = -inf
//   w_p = v_exp_f32((partial_lse[p] - mu) L2E);   L = ((w_0 + w_1) + w_2) + ...;   N[c] = ((w_0 po_0[c] + w_1 po_1[c]) + w_2 po_2[c]) + ...
//   L == 0 (a NaN is not 0):  out = +0, lse = -inf;   else  out[c] = RNE_bf16(N[c] (1 / L)),  lse = mu + LN2 v_log_f32(L)
// mu = 0 for a head without a valid position keeps -inf - -inf out of the exponent: every w is v_exp_f32(-inf) = 0 and L = 0.  A NaN
// partial_lse gives a NaN w, hence NaN L, out and lse: a head whose only non-empty split is NaN is NaN, not +0.
// With P = 1: w = v_exp_f32(0) = 1, L = 1, N = po, 1 / L = 1 and v_log_f32(1) = 0, so out = RNE_bf16(po) and lse = partial_lse -- the
// attention kernel's own last two operations, which is why partial + merge at one split is dga_sparse_mla_fwd byte for byte.
// A thread owns four columns of one head (a 16-byte load of every split's row, one 8-byte store) and walks p itself; the 128 threads of
// a head read the same partial_lse address.  Every output has one writer, nothing is atomic, nothing of a split >= P is read.
//   dga_sparse_mla_splits   the number of splits worth launching (a pure function of its arguments; see SMLA_MIN_TILES below)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int SMLA_MERGE_DV = DGA_SPARSE_MLA_D_V;              // 512
constexpr int SMLA_MERGE_THREADS = 256;
constexpr int SMLA_MERGE_LANES = SMLA_MERGE_DV / 4;            // threads a head: 128
static_assert(SMLA_MERGE_THREADS % SMLA_MERGE_LANES == 0, "whole heads a workgroup");

// The fewest tiles (of DGA_SPARSE_MLA_TILE positions) a split is given.  A split costs its workgroup's prologue (q to LDS, the first
// tile's gather, which nothing hides) and its share of the merge; a tile of the loop is 1.8 us.  The sweep behind the value is in
// DESIGN.md, "Split-topk sparse MLA decode", and profiles/sparse_mla_split_timing.txt.
constexpr int SMLA_MIN_TILES = DGA_SPARSE_MLA_MIN_TILES;

typedef float smla_merge_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 smla_merge_v4bf __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(SMLA_MERGE_THREADS) sparse_mla_merge_kernel(const float *__restrict__ partial_out,
                                                                              const float *__restrict__ partial_lse, int num_splits,
                                                                              int64_t rows, uint16_t *__restrict__ out, float *__restrict__ lse)
{
    // rows = m heads: what one split's partial_lse holds, and 512 times that its partial_out
    const int64_t at = (int64_t)blockIdx.x * SMLA_MERGE_THREADS + threadIdx.x;
    const int64_t row = at / SMLA_MERGE_LANES;
    const int col = (int)(at % SMLA_MERGE_LANES) * 4;
    if (row >= rows) return;
    const float *ls = partial_lse + row;
    float top = -__builtin_inff();
#pragma unroll 4
    for (int p = 0; p < num_splits; ++p) top = __builtin_fmaxf(top, ls[p * rows]);
    const float mu = top == -__builtin_inff() ? 0.f : top;
    const float *po = partial_out + (row * SMLA_MERGE_DV + col);
    const int64_t pitch = rows * SMLA_MERGE_DV;
    // (the sums start at their first term, not at +0: a -0 of a single split stays -0)
    float total = __builtin_amdgcn_exp2f((ls[0] - mu) * 1.4426950408889634f);
    smla_merge_v4f num = *reinterpret_cast<const smla_merge_v4f *>(po) * total;
#pragma unroll 4
    for (int p = 1; p < num_splits; ++p) {
        const float w = __builtin_amdgcn_exp2f((ls[p * rows] - mu) * 1.4426950408889634f);
        const smla_merge_v4f v = *reinterpret_cast<const smla_merge_v4f *>(po + p * pitch);
        total = total + w;
        num = num + v * w;
    }
    const bool empty = total == 0.f;
    const float inv = empty ? 0.f : 1.0f / total;
    smla_merge_v4bf o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (__bf16)(empty ? 0.f : num[i] * inv);
    *reinterpret_cast<uint2 *>(out + (row * SMLA_MERGE_DV + col)) = __builtin_bit_cast(uint2, o);
    if (col == 0) lse[row] = empty ? -__builtin_inff() : mu + __builtin_amdgcn_logf(total) * 0.693147180559945309f;
}

}  // namespace dga

extern "C" int dga_sparse_mla_merge(const float *partial_out, const float *partial_lse, int num_splits, int64_t m, int heads, void *out, float *lse,
                                    void *stream)
{
    using namespace dga;
    if (m < 0 || heads < 16 || heads > DGA_SPARSE_MLA_MAX_HEADS || heads % 16 || num_splits < 1 || num_splits > DGA_SPARSE_MLA_MAX_SPLITS)
        return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!partial_out || !partial_lse || !out || !lse) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(partial_out) % 16 || reinterpret_cast<uintptr_t>(out) % 16 || reinterpret_cast<uintptr_t>(partial_lse) % 4 ||
        reinterpret_cast<uintptr_t>(lse) % 4)
        return DGA_E_ALIGN;
    // (the grid fits an int32, and P m heads 512 floats an int64)
    if (m > 0x7FFFFFFFll / (heads / 2) || m > 0x7FFFFFFFFFFFFFFFll / 4 / SMLA_MERGE_DV / heads / num_splits) return DGA_E_RANGE;
    const int64_t rows = m * heads;
    const int64_t grid = rows / (SMLA_MERGE_THREADS / SMLA_MERGE_LANES);       // (heads is even)
    hipLaunchKernelGGL(sparse_mla_merge_kernel, dim3(static_cast<unsigned>(grid)), dim3(SMLA_MERGE_THREADS), 0, static_cast<hipStream_t>(stream),
                       partial_out, partial_lse, num_splits, rows, static_cast<uint16_t *>(out), lse);
    return record_hip(hipGetLastError());
}

// max(1, min(cus / (m head_blocks), tiles / MIN_TILES, 64)): as many splits as there are idle CUs for, none shorter than MIN_TILES
// tiles.  cus <= 0 asks the current device.  Arguments outside the attention entries' ranges give 1.
extern "C" int dga_sparse_mla_splits(int64_t m, int heads, int64_t topk, int cus)
{
    using namespace dga;
    if (m < 1 || heads < 1 || topk < 1) return 1;
    if (cus <= 0) cus = static_cast<int>(device_cus());
    const int64_t head_blocks = (static_cast<int64_t>(heads) + 63) / 64;
    const int64_t tiles = (topk - 1) / DGA_SPARSE_MLA_TILE + 1;
    if (m > cus / head_blocks) return 1;                         // (also: m head_blocks cannot overflow below)
    int64_t p = cus / (m * head_blocks);
    if (tiles / SMLA_MIN_TILES < p) p = tiles / SMLA_MIN_TILES;
    if (p > DGA_SPARSE_MLA_MAX_SPLITS) p = DGA_SPARSE_MLA_MAX_SPLITS;
    return p < 1 ? 1 : static_cast<int>(p);
}
