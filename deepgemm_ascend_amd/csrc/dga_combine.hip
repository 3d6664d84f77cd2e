// The combine of an MoE layer and the two sums of its backward, on dga_route_slots' pair -> slot table as it is (dest int64 [tokens, k], a
// dropped choice is -1):
//   dga_combine_rows               out[t] = sum_j w[t, j] * src[dest[t, j]]        (w == NULL: the plain sum -- the backward of the dispatch)
//   dga_combine_rows_weight_grad   dw[t, j] = <src[dest[t, j]], grad[t]>           (the router's gradient)
// A choice whose dest is outside [0, src_rows) is skipped (dw: +0); every element of out and of dw is written.  HBM-bound: each valid
// choice's row is read once, out is written once, grad[t] is read once per 8 choices; 16-byte lanes when the pointers and h allow, else an
// element-wise path with the same result.
//
// The combine's arithmetic is a definition, not an approximation: acc = +0, then for j = 0 .. k - 1 in that order
//   acc = fl32(acc + fl32(w[t, j] * fl32(src[dest[t, j], c]))),        out[t, c] = RNE(acc)
// two roundings per choice, which numpy float32 reproduces bit for bit.  The whole unit is compiled without contraction (the pragma
// below): a fused multiply-add rounds once and gives other bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

#pragma clang fp contract(off)

namespace dga {


constexpr int COMBINE_J = 4;   // choices whose rows are in flight together

// One workgroup per (token, part of the row): a lane owns 8 consecutive channels at a time, chunk c = part * 256 + lane, then every
// 256 * parts further (dga_copy_rows' split of a long row).  The k choices are taken COMBINE_J at a time: their predicated 16-byte loads
// go out together, then the products are added in the order of j.  dest and the weights are the same for the whole workgroup (scalar
// loads), so a dropped choice costs no vector memory traffic.
template <typename T, typename O, bool WEIGHTED>
__global__ void __launch_bounds__(256) combine_rows_kernel(const void *src, const int64_t *dest, const float *weights, void *out,
                                                           int64_t src_rows, int64_t h, int k, int parts, bool vec_in, bool vec_out)
{
    const int64_t t = blockIdx.x / (uint32_t)parts;
    const int part = blockIdx.x - (uint32_t)t * (uint32_t)parts;
    const int64_t *d = dest + t * k;
    const float *w = WEIGHTED ? weights + t * k : nullptr;
    const int64_t chunks = (h + 7) / 8;
    for (int64_t c = part * 256 + threadIdx.x; c < chunks; c += 256 * (int64_t)parts) {
        const int64_t c0 = c * 8;
        const bool whole = c0 + 8 <= h;
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int j0 = 0; j0 < k; j0 += COMBINE_J) {
            bool ok[COMBINE_J];
            float wj[COMBINE_J];
            float v[COMBINE_J][8];
            int64_t row[COMBINE_J];
#pragma unroll
            for (int jj = 0; jj < COMBINE_J; ++jj) {
                row[jj] = j0 + jj < k ? d[j0 + jj] : -1;
                ok[jj] = (uint64_t)row[jj] < (uint64_t)src_rows;
                wj[jj] = (WEIGHTED && j0 + jj < k) ? w[j0 + jj] : 1.f;
            }
            if (vec_in && whole) {
                typename Elem<T>::Raw raw[COMBINE_J];
#pragma unroll
                for (int jj = 0; jj < COMBINE_J; ++jj) {
                    raw[jj] = typename Elem<T>::Raw{};
                    if (ok[jj]) raw[jj] = Elem<T>::load8_raw(src, row[jj] * h + c0);
                }
#pragma unroll
                for (int jj = 0; jj < COMBINE_J; ++jj) Elem<T>::unpack8(raw[jj], v[jj]);
            } else {
#pragma unroll
                for (int jj = 0; jj < COMBINE_J; ++jj) load8_bounded<T>(src, row[jj] * h + c0, v[jj], false, c0, h, ok[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < COMBINE_J; ++jj) {
                if (!ok[jj]) continue;   // (uniform) a dropped choice adds nothing, whatever its weight
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float prod = WEIGHTED ? wj[jj] * v[jj][i] : v[jj][i];   // rounded on its own: no contraction in this unit
                    acc[i] = acc[i] + prod;
                }
            }
        }
        if (vec_out && whole) {
            Store8<O>::run(out, t * h + c0, acc, true);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (c0 + i < h) store1<O>(out, t * h + c0 + i, acc[i]);
        }
    }
}

constexpr int WGRAD_J = 8;   // choices that share one read of grad[t]

// One workgroup per token.  Its lanes walk the row 8 channels at a time; a lane's chunk of grad[t] is read once and meets the same chunk of
// the rows of WGRAD_J choices (9 loads in flight), one fp32 fused multiply-add per product into the lane's partial sum of that choice.  The
// partial sums meet in a fixed order -- the 64 lanes of a wave by butterfly, the 4 waves through LDS, added 0, 1, 2, 3 -- so two runs give the
// same bits: no atomics.  A dropped choice never leaves +0.
template <typename T>
__global__ void __launch_bounds__(256) combine_rows_weight_grad_kernel(const void *src, const void *grad, const int64_t *dest, float *dw,
                                                                       int64_t src_rows, int64_t h, int k, bool vec)
{
    __shared__ float red[4][WGRAD_J];
    const int64_t t = blockIdx.x;
    const int64_t *d = dest + t * k;
    const int64_t chunks = (h + 7) / 8;
    for (int j0 = 0; j0 < k; j0 += WGRAD_J) {
        bool ok[WGRAD_J];
        int64_t row[WGRAD_J];
        float acc[WGRAD_J];
#pragma unroll
        for (int jj = 0; jj < WGRAD_J; ++jj) {
            row[jj] = j0 + jj < k ? d[j0 + jj] : -1;
            ok[jj] = (uint64_t)row[jj] < (uint64_t)src_rows;
            acc[jj] = 0.f;
        }
        for (int64_t c = threadIdx.x; c < chunks; c += 256) {
            const int64_t c0 = c * 8;
            float g[8], v[WGRAD_J][8];
            if (vec && c0 + 8 <= h) {
                typename Elem<T>::Raw graw = Elem<T>::load8_raw(grad, t * h + c0), raw[WGRAD_J];
#pragma unroll
                for (int jj = 0; jj < WGRAD_J; ++jj) {
                    raw[jj] = typename Elem<T>::Raw{};
                    if (ok[jj]) raw[jj] = Elem<T>::load8_raw(src, row[jj] * h + c0);
                }
                Elem<T>::unpack8(graw, g);
#pragma unroll
                for (int jj = 0; jj < WGRAD_J; ++jj) Elem<T>::unpack8(raw[jj], v[jj]);
            } else {
                load8_bounded<T>(grad, t * h + c0, g, false, c0, h);
#pragma unroll
                for (int jj = 0; jj < WGRAD_J; ++jj) load8_bounded<T>(src, row[jj] * h + c0, v[jj], false, c0, h, ok[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < WGRAD_J; ++jj) {
                if (!ok[jj]) continue;   // (uniform)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[jj] = __builtin_fmaf(v[jj][i], g[i], acc[jj]);
            }
        }
#pragma unroll
        for (int jj = 0; jj < WGRAD_J; ++jj) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) acc[jj] = acc[jj] + __shfl_xor(acc[jj], m, 64);
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int jj = 0; jj < WGRAD_J; ++jj) red[threadIdx.x >> 6][jj] = acc[jj];
        }
        __syncthreads();
        if (threadIdx.x < WGRAD_J && j0 + (int)threadIdx.x < k) {
            const int jj = threadIdx.x;
            dw[t * k + j0 + jj] = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
        }
        __syncthreads();   // red is written again by the next WGRAD_J choices
    }
}

// the checks the two entries share, in the fused entries' order as far as they apply: shape, nothing to do, (pointers and dtypes are the
// entry's own), then the sizes a launch cannot take
inline int combine_shape(int64_t src_rows, int64_t h, int64_t tokens, int64_t k)
{
    if (src_rows < 0 || h < 0 || tokens < 0 || k < 1 || (tokens > 0 && k > 0x7FFFFFFFFFFFFFFFll / tokens)) return DGA_E_SHAPE;
    return DGA_OK;
}
inline int combine_range(int64_t src_rows, int64_t h, int64_t tokens, int64_t k)
{
    const int64_t most = src_rows > tokens ? src_rows : tokens;   // element indices of src, out and grad stay inside int64
    if (k > 0x7FFFFFFFll || (most > 0 && h > 0x7FFFFFFFFFFFFFFFll / most)) return DGA_E_RANGE;
    return DGA_OK;
}

}  // namespace dga

extern "C" int dga_combine_rows(const void *src, int src_dtype, int64_t src_rows, int64_t h, const int64_t *dest, const float *weights,
                                int64_t tokens, int64_t k, void *out, int out_dtype, void *stream)
{
    using namespace dga;
    if (int rc = combine_shape(src_rows, h, tokens, k)) return rc;
    if (tokens == 0 || h == 0) return DGA_OK;
    if ((!src && src_rows > 0) || !dest || !out) return DGA_E_NULL;
    if (out_dtype != src_dtype && out_dtype != DGA_DT_FP32) return DGA_E_DTYPE;
    return dispatch_dtype(src_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (int rc = combine_range(src_rows, h, tokens, k)) return rc;
        const int64_t chunks = (h + 7) / 8;
        int64_t parts = (chunks + 511) / 512;   // <= 2 chunks per lane, up to 64 workgroups a row
        if (parts > 64) parts = 64;
        if (tokens > 0x7FFFFFFFll / parts) return DGA_E_RANGE;
        const auto al = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
        const bool vec_in = al(src) && h % 8 == 0, vec_out = al(out) && h % 8 == 0;
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tokens * parts)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dest,
                               weights, out, src_rows, h, static_cast<int>(k), static_cast<int>(parts), vec_in, vec_out);
        };
        if (out_dtype == src_dtype) {
            if (weights) launch(combine_rows_kernel<T, T, true>);
            else launch(combine_rows_kernel<T, T, false>);
        } else {
            if (weights) launch(combine_rows_kernel<T, float, true>);
            else launch(combine_rows_kernel<T, float, false>);
        }
        return record_hip(hipGetLastError());
    });
}

extern "C" int dga_combine_rows_weight_grad(const void *src, const void *grad, int dtype, int64_t src_rows, int64_t h, const int64_t *dest,
                                            int64_t tokens, int64_t k, float *dw, void *stream)
{
    using namespace dga;
    if (int rc = combine_shape(src_rows, h, tokens, k)) return rc;
    if (tokens == 0 || h == 0) return DGA_OK;
    if ((!src && src_rows > 0) || !grad || !dest || !dw) return DGA_E_NULL;
    return dispatch_dtype(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (int rc = combine_range(src_rows, h, tokens, k)) return rc;
        if (tokens > 0x7FFFFFFFll) return DGA_E_RANGE;
        const auto al = [](const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
        const bool vec = al(src) && al(grad) && h % 8 == 0;
        hipLaunchKernelGGL(combine_rows_weight_grad_kernel<T>, dim3(static_cast<unsigned>(tokens)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), src, grad, dest, dw, src_rows, h, static_cast<int>(k), vec);
        return record_hip(hipGetLastError());
    });
}
