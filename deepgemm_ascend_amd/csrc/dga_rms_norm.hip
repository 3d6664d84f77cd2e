// The operator in front of everything an MoE block reads in a pre-norm transformer: n = rms_norm(h + residual) * gamma, quantised in the
// same pass, and its backward.
//   dga_rms_norm_cast_to_fp8_1x128   x (+ residual) [rows, h], weight [h] -> residual_out, rstd [rows], norm_out, (q, sf) per 1x128 block
//   dga_rms_norm_backward            grad_y, z, weight, rstd (+ grad_residual) -> dx [rows, h], dweight fp32 [h]
// Both kernels hold a row in registers in the quantisers' geometry: lane l of the LPR lanes of a row owns the 8 consecutive columns
// (u LPR + l) 8 .. + 7 of pass u = 0 .. U - 1, so 16 consecutive lanes are one 1x128 block (quant_row_block) and a pass of the row is one
// contiguous stream.  (LPR, U) is a function of h alone (norm_geometry): 16 or 32 lanes for a row of one or two blocks, one wave up to
// h = 2048, two waves up to 4096, four beyond, up to 8 passes; the forward keeps the row and the weight as the bytes they were read as
// (Pack8).  The backward keeps four fp32 arrays per lane, so it takes at most two passes and up to 1024 lanes on a row
// (norm_backward_geometry).  Every sum has one order that (h, dtype) fixes: the lane's U 8 terms in
// ascending order as one fma chain, a butterfly over the lanes of a wave (all lanes get the same bits: fp32 addition commutes), then the
// row's waves in ascending order through LDS.  No floating-point atomics anywhere.
// The backward's column sums take two stages: a group of LPR lanes walks norm_chunk_rows(rows) consecutive rows and keeps
// sum_t grad_y x^ of its columns in registers (one fma chain in row order), the chunk's partial goes to the workspace, fp32 [chunks, h];
// stage two adds the chunks of a column in ascending order, four contiguous runs of them first, the runs then in ascending order.
// This unit's own text is compiled without contraction (the pragma below): y is two roundings, and the backward with grad_residual is the
// separate sum of grad_residual and the fp32 dx the entry gives without it.  Every fma below is written as one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <type_traits>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int NORM_THREADS = 256;
// (the backward keeps four arrays of a row's columns per lane and walks many rows: at most two passes, so up to 1024 lanes on a row)
constexpr int norm_backward_threads(int lpr) { return lpr > NORM_THREADS ? lpr : NORM_THREADS; }
constexpr int NORM_MAX_H = DGA_RMS_NORM_MAX_H;
constexpr int NORM_FINISH_SLICES = 4;
constexpr int NORM_FINISH_AHEAD = 8;   // partials a thread of stage two has in flight

// rows of one stage-one chunk of the backward: at least 8, and no more than about 1024 chunks over all the rows -- enough groups to fill
// the part, few enough partials that the workspace stays a few per cent of the traffic.  A function of the row count alone.
inline int64_t norm_chunk_rows(int64_t rows)
{
    const int64_t per = (rows + 1023) / 1024;
    return per < 8 ? 8 : per;
}
inline int64_t norm_chunks(int64_t rows) { return (rows + norm_chunk_rows(rows) - 1) / norm_chunk_rows(rows); }

// 8 fp32 values -> the 16 (fp32: 32) bytes a tensor of type T holds for them, round to nearest even: the inverse of Elem<T>::unpack8 on
// values that are T's own.  A row waits in this form between the statistic and the quantiser: half the registers for the 16-bit types.
template <typename T> struct Pack8;
template <> struct Pack8<float> {
    static __device__ __forceinline__ Elem<float>::Raw run(const float (&v)[8])
    {
        return Elem<float>::Raw{v4f_c{v[0], v[1], v[2], v[3]}, v4f_c{v[4], v[5], v[6], v[7]}};
    }
    static __device__ __forceinline__ void store(void *p, int64_t i, const Elem<float>::Raw &w)
    {
        *(v4f_c *)((float *)p + i) = w.lo;
        *(v4f_c *)((float *)p + i + 4) = w.hi;
    }
};
template <> struct Pack8<Bf16Tag> {
    static __device__ __forceinline__ v4i_c run(const float (&v)[8])
    {
        typedef float v2f __attribute__((ext_vector_type(2)));
        typedef __bf16 v2b __attribute__((ext_vector_type(2)));
        v4i_c w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_bit_cast(int, __builtin_convertvector((v2f{v[2 * j], v[2 * j + 1]}), v2b));
        return w;
    }
    static __device__ __forceinline__ void store(void *p, int64_t i, const v4i_c &w) { *(v4i_c *)((uint16_t *)p + i) = w; }
};
template <> struct Pack8<F16Tag> {
    static __device__ __forceinline__ Elem<F16Tag>::Raw run(const float (&v)[8])
    {
        return Elem<F16Tag>::Raw{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                                 (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
    }
    static __device__ __forceinline__ void store(void *p, int64_t i, const Elem<F16Tag>::Raw &w) { *(Elem<F16Tag>::Raw *)((_Float16 *)p + i) = w; }
};

// load8_bounded that keeps the bytes: one 16-byte (fp32: two) load where the lane's 8 columns are inside and aligned, else element by
// element and packed again (exact: the values are T's own)
template <typename T>
__device__ __forceinline__ typename Elem<T>::Raw load8_raw_bounded(const void *p, int64_t base, bool vec, int64_t c0, int64_t n, bool row_ok = true)
{
    if (row_ok && vec && c0 + 8 <= n) return Elem<T>::load8_raw(p, base);
    float v[8];
    load8_bounded<T>(p, base, v, false, c0, n, row_ok);
    return Pack8<T>::run(v);
}

// a tensor that is of type T or fp32, decided at run time by a uniform flag (weight, dx, grad_residual): one kernel build serves both
template <typename T> __device__ __forceinline__ void load8_either(const void *p, bool f32, int64_t i, float (&v)[8], bool vec, int64_t c0, int64_t n, bool ok = true)
{
    if (f32) load8_bounded<float>(p, i, v, vec, c0, n, ok);
    else load8_bounded<T>(p, i, v, vec, c0, n, ok);
}
template <typename T> __device__ __forceinline__ void store8_either(void *p, bool f32, int64_t i, const float (&v)[8], bool vec, int64_t c0, int64_t n)
{
    if (f32) store8_bounded<float>(p, i, v, vec, c0, n);
    else store8_bounded<T>(p, i, v, vec, c0, n);
}

// The sum of the lane partials p over the LPR lanes of a row, the same bits in every lane of the row: a butterfly inside the wave, then the
// row's waves in ascending order.  part: one float per wave of the workgroup.  Every thread of the workgroup calls it.
template <int LPR> __device__ __forceinline__ float row_sum(float p, float *part)
{
#pragma unroll
    for (int m = 1; m < (LPR < 64 ? LPR : 64); m <<= 1) p = p + __shfl_xor(p, m, 64);
    if constexpr (LPR > 64) {
        constexpr int WPR = LPR / 64;
        const int wave = threadIdx.x >> 6;
        __syncthreads();                       // (the previous row's readers are done with part)
        if ((threadIdx.x & 63) == 0) part[wave] = p;
        __syncthreads();
        const int first = wave / WPR * WPR;
        p = part[first];
#pragma unroll
        for (int v = 1; v < WPR; ++v) p = p + part[first + v];
    }
    return p;
}

// (a + eps)^(-1/2) by the hardware's 1-ULP reciprocal square root, which does not take subnormals: a tiny argument is scaled by 2^100
// first and the result by 2^50, both exact
__device__ __forceinline__ float rsqrt_1ulp(float a)
{
    const bool tiny = a < 0x1p-100f;
    const float r = __builtin_amdgcn_rsqf(tiny ? a * 0x1p100f : a);
    return tiny ? r * 0x1p50f : r;
}

// One group of LPR lanes per row, 256 / LPR rows per workgroup.  Everything is read before anything is written, and a lane writes only the
// columns it read: residual_out may be residual or x.  z and the weight wait as the bytes their tensors hold (W: the weight's type).
template <typename T, typename W, int LPR, int U>
__global__ void __launch_bounds__(NORM_THREADS) rms_norm_cast_kernel(const void *x, const void *residual, const void *weight, int64_t rows, int h,
                                                                    float eps, uint8_t *q, float *sf, void *norm_out, void *residual_out,
                                                                    float *rstd_out, bool vec, bool ue8m0)
{
    __shared__ float part[NORM_THREADS / 64];
    constexpr int RPW = NORM_THREADS / LPR;
    const int l = threadIdx.x % LPR;
    const int64_t row = (int64_t)blockIdx.x * RPW + threadIdx.x / LPR;
    const bool row_ok = row < rows;
    const int64_t base = row * h;
    const int hb_n = (h + 127) >> 7;

    typename Elem<T>::Raw zr[U];
    typename Elem<W>::Raw wr[U];
    if (residual) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c0 = (u * LPR + l) * 8;
            float a[8], r[8];
            load8_bounded<T>(x, base + c0, a, vec, c0, h, row_ok);
            load8_bounded<T>(residual, base + c0, r, vec, c0, h, row_ok);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = a[j] + r[j];
            zr[u] = Pack8<T>::run(a);                       // RNE_T(fl(x + residual)): what is stored, and what is normalised
        }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c0 = (u * LPR + l) * 8;
            zr[u] = load8_raw_bounded<T>(x, base + c0, vec, c0, h, row_ok);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c0 = (u * LPR + l) * 8;
        wr[u] = load8_raw_bounded<W>(weight, c0, vec, c0, h);
    }
    if (residual && row_ok) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c0 = (u * LPR + l) * 8;
            if (vec && c0 + 8 <= h) {
                Pack8<T>::store(residual_out, base + c0, zr[u]);
            } else if (c0 < h) {
                float z[8];
                Elem<T>::unpack8(zr[u], z);
                store8_bounded<T>(residual_out, base + c0, z, false, c0, h);
            }
        }
    }
    float p = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float z[8];
        Elem<T>::unpack8(zr[u], z);
#pragma unroll
        for (int j = 0; j < 8; ++j) p = __builtin_fmaf(z[j], z[j], p);
    }
    p = row_sum<LPR>(p, part);
    const float rstd = rsqrt_1ulp(p / (float)h + eps);
    if (l == 0 && row_ok) rstd_out[row] = rstd;

#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (u * LPR * 8 >= h) break;          // (the whole workgroup: the pass lies beyond the row)
        const int c0 = (u * LPR + l) * 8;
        float z[8], w[8], y[8];
        Elem<T>::unpack8(zr[u], z);
        Elem<W>::unpack8(wr[u], w);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (z[j] * rstd) * w[j];
            y[j] = v != v ? __uint_as_float(0x7FC00000u) : v;   // one NaN, whatever produced it: its code is 0x7F
        }
        const bool mine = row_ok && c0 < h;
        if (norm_out && mine) store8_bounded<T>(norm_out, base + c0, y, vec, c0, h);
        if (q) {
            float s;
            uint32_t w0, w1;
            quant_row_block(y, ue8m0, s, w0, w1);     // (every lane of the wave: a ballot and the 16-lane row maximum inside)
            if (mine) {
                if ((l & 15) == 0) sf[row * hb_n + (c0 >> 7)] = s;
                store_codes8(q + base + c0, w0, w1, vec, c0, h);
            }
        }
    }
}

// One group of LPR lanes per chunk of chunk_rows consecutive rows, 256 / LPR chunks per workgroup (one where LPR >= 256); a group beyond the last chunk walks the
// last one again and writes nothing (its waves still meet the barriers of row_sum).  dx may be grad_residual.
template <typename T, int LPR, int U>
__global__ void __launch_bounds__(norm_backward_threads(LPR)) rms_norm_backward_kernel(const void *grad_y, const void *zin, const void *weight, bool w_f32,
                                                                        const float *rstd_in, const void *grad_residual, int64_t rows, int h,
                                                                        int chunk_rows, int64_t chunks, void *dx, bool dx_f32, float *ws,
                                                                        bool vec)
{
    __shared__ float part[norm_backward_threads(LPR) / 64];
    constexpr int RPW = norm_backward_threads(LPR) / LPR;
    const int l = threadIdx.x % LPR;
    const int64_t slot = (int64_t)blockIdx.x * RPW + threadIdx.x / LPR;
    const bool live = slot < chunks;
    const int64_t chunk = live ? slot : chunks - 1;
    const int64_t first = chunk * chunk_rows;
    const int n = rows - first < chunk_rows ? (int)(rows - first) : chunk_rows;   // the last chunk may be short
    float w[U][8], dw[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c0 = (u * LPR + l) * 8;
        load8_either<T>(weight, w_f32, c0, w[u], vec, c0, h);
#pragma unroll
        for (int j = 0; j < 8; ++j) dw[u][j] = 0.f;
    }
    for (int i = 0; i < chunk_rows; ++i) {   // (every group of the workgroup alike: the barriers of row_sum)
        const bool row_ok = i < n;
        const int64_t row = first + (row_ok ? i : n - 1);
        const int64_t base = row * h;
        float gy[U][8], xh[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c0 = (u * LPR + l) * 8;
            load8_bounded<T>(grad_y, base + c0, gy[u], vec, c0, h);
            load8_bounded<T>(zin, base + c0, xh[u], vec, c0, h);
        }
        const float rstd = rstd_in[row];
        float p = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xh[u][j] = xh[u][j] * rstd;
                p = __builtin_fmaf(gy[u][j] * w[u][j], xh[u][j], p);
            }
        p = row_sum<LPR>(p, part);
        const float c = p / (float)h;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u * LPR * 8 >= h) break;
            const int c0 = (u * LPR + l) * 8;
            float d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                d[j] = rstd * (gy[u][j] * w[u][j] - xh[u][j] * c);
                if (row_ok) dw[u][j] = __builtin_fmaf(gy[u][j], xh[u][j], dw[u][j]);
            }
            const bool mine = live && row_ok && c0 < h;
            if (grad_residual) {
                float a[8];
                load8_either<T>(grad_residual, dx_f32, base + c0, a, vec, c0, h, mine);
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = d[j] + a[j];
            }
            if (mine) store8_either<T>(dx, dx_f32, base + c0, d, vec, c0, h);
        }
    }
    if (ws && live) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c0 = (u * LPR + l) * 8;
            // (the workspace is 16-byte aligned and its rows are h floats: the same condition as the inputs' vector path)
            if (c0 < h) store8_bounded<float>(ws, chunk * h + c0, dw[u], vec, c0, h);
        }
    }
}

// Stage two: thread (slice, x) of a workgroup of 64 columns adds column x's partials over the slice's contiguous run of chunks, in ascending
// order; slice 0 then adds the four runs in ascending order.
__global__ void __launch_bounds__(64 * NORM_FINISH_SLICES) rms_norm_dweight_kernel(const float *ws, float *dweight, int64_t chunks, int h)
{
    __shared__ float lds[NORM_FINISH_SLICES][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    const int64_t c0 = chunks * slice / NORM_FINISH_SLICES, c1 = chunks * (slice + 1) / NORM_FINISH_SLICES;
    float p = 0.f;
    if (x < h) {
        const float *pp = ws + c0 * h + x;
        for (int64_t c = c0; c < c1; c += NORM_FINISH_AHEAD) {
            const int live = (int)(c1 - c < NORM_FINISH_AHEAD ? c1 - c : NORM_FINISH_AHEAD);   // >= 1
            float a[NORM_FINISH_AHEAD];
#pragma unroll
            for (int u = 0; u < NORM_FINISH_AHEAD; ++u) a[u] = pp[(int64_t)(u < live ? u : live - 1) * h];
#pragma unroll
            for (int u = 0; u < NORM_FINISH_AHEAD; ++u) p = u < live ? p + a[u] : p;
            pp += (int64_t)NORM_FINISH_AHEAD * h;
        }
    }
    lds[slice][lane] = p;
    __syncthreads();
    if (slice == 0 && x < h) {
#pragma unroll
        for (int s = 1; s < NORM_FINISH_SLICES; ++s) p = p + lds[s][lane];
        dweight[x] = p;
    }
}

// (LPR, U) for a row of h: f(integral_constant LPR, integral_constant U)
template <typename F> inline int norm_geometry(int64_t h, F &&f)
{
    using std::integral_constant;
    if (h <= 128) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    if (h <= 256) return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    if (h <= 512) return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    if (h <= 1024) return f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
    if (h <= 2048) return f(integral_constant<int, 64>{}, integral_constant<int, 4>{});
    if (h <= 4096) return f(integral_constant<int, 128>{}, integral_constant<int, 4>{});
    if (h <= 8192) return f(integral_constant<int, 256>{}, integral_constant<int, 4>{});
    return f(integral_constant<int, 256>{}, integral_constant<int, 8>{});
}

template <typename F> inline int norm_backward_geometry(int64_t h, F &&f)
{
    using std::integral_constant;
    if (h <= 128) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    if (h <= 256) return f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
    if (h <= 512) return f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    if (h <= 1024) return f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
    if (h <= 2048) return f(integral_constant<int, 128>{}, integral_constant<int, 2>{});
    if (h <= 4096) return f(integral_constant<int, 256>{}, integral_constant<int, 2>{});
    if (h <= 8192) return f(integral_constant<int, 512>{}, integral_constant<int, 2>{});
    return f(integral_constant<int, 1024>{}, integral_constant<int, 2>{});
}

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
inline bool norm_dtypes_ok(int dtype, int other) { return other == dtype || other == DGA_DT_FP32; }

}  // namespace dga

extern "C" int dga_rms_norm_cast_to_fp8_1x128(const void *x, const void *residual, int x_dtype, const void *weight, int w_dtype, int64_t rows,
                                              int64_t h, float eps, void *q, float *sf, void *norm_out, void *residual_out, float *rstd,
                                              int flags, void *stream)
{
    using namespace dga;
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (rows < 0 || h < 0 || h > NORM_MAX_H) return DGA_E_SHAPE;
    if (rows == 0 || h == 0) return DGA_OK;
    if (!x || !weight || !rstd || !q != !sf || (!q && !norm_out) || !residual != !residual_out) return DGA_E_NULL;
    return dispatch_dtype(x_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (!norm_dtypes_ok(x_dtype, w_dtype)) return DGA_E_DTYPE;
        if (!(eps >= 0.f) || std::isinf(eps)) return DGA_E_RANGE;
        // a lane's 8 elements start at element row * h + 8 j: 16-byte aligned in every tensor iff h % 8 == 0 and the tensor is (q: 8-byte)
        const bool vec = h % 8 == 0 && aligned16(x) && aligned16(residual) && aligned16(weight) && aligned16(norm_out) &&
                         aligned16(residual_out) && reinterpret_cast<uintptr_t>(q) % 8 == 0;
        return norm_geometry(h, [&](auto lpr, auto passes) -> int {
            constexpr int LPR = decltype(lpr)::value, U = decltype(passes)::value, RPW = NORM_THREADS / LPR;
            const int64_t grid = (rows + RPW - 1) / RPW;
            if (grid > 0x7FFFFFFFll) return DGA_E_RANGE;
            auto launch = [&](auto wtag) {
                hipLaunchKernelGGL((rms_norm_cast_kernel<T, decltype(wtag), LPR, U>), dim3(static_cast<unsigned>(grid)), dim3(NORM_THREADS), 0,
                                   static_cast<hipStream_t>(stream), x, residual, weight, rows, static_cast<int>(h), eps,
                                   static_cast<uint8_t *>(q), sf, norm_out, residual_out, rstd, vec, (flags & DGA_CAST_UE8M0) != 0);
            };
            if (w_dtype == x_dtype) launch(T{});
            else launch(float{});
            return record_hip(hipGetLastError());
        });
    });
}

extern "C" int64_t dga_rms_norm_backward_workspace_bytes(int64_t rows, int64_t h)
{
    using namespace dga;
    if (rows <= 0 || h <= 0 || h > NORM_MAX_H) return 0;
    return norm_chunks(rows) * h * 4;   // (at most 1024 chunks of at most 16384 floats, or rows / 8 of them)
}

extern "C" int dga_rms_norm_backward(const void *grad_y, const void *z, int dtype, const void *weight, int w_dtype, const float *rstd,
                                     const void *grad_residual, int64_t rows, int64_t h, void *dx, int dx_dtype, float *dweight,
                                     void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace dga;
    if (rows < 0 || h < 0 || h > NORM_MAX_H) return DGA_E_SHAPE;
    if (rows == 0 || h == 0) return DGA_OK;
    if (!grad_y || !z || !weight || !rstd || !dx || (dweight && !workspace)) return DGA_E_NULL;
    return dispatch_dtype(dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        if (!norm_dtypes_ok(dtype, w_dtype) || !norm_dtypes_ok(dtype, dx_dtype)) return DGA_E_DTYPE;
        if (rows > 0x7FFFFFFFll * 8) return DGA_E_RANGE;
        const int64_t chunk_rows = norm_chunk_rows(rows), chunks = norm_chunks(rows);
        if (dweight && (workspace_bytes < chunks * h * 4 || !aligned16(workspace))) return DGA_E_WORKSPACE;
        float *ws = dweight ? static_cast<float *>(workspace) : nullptr;
        const bool vec = h % 8 == 0 && aligned16(grad_y) && aligned16(z) && aligned16(weight) && aligned16(grad_residual) && aligned16(dx);
        const hipStream_t s = static_cast<hipStream_t>(stream);
        int rc = norm_backward_geometry(h, [&](auto lpr, auto passes) -> int {
            constexpr int LPR = decltype(lpr)::value, U = decltype(passes)::value, THREADS = norm_backward_threads(LPR), RPW = THREADS / LPR;
            hipLaunchKernelGGL((rms_norm_backward_kernel<T, LPR, U>), dim3(static_cast<unsigned>((chunks + RPW - 1) / RPW)), dim3(THREADS),
                               0, s, grad_y, z, weight, w_dtype == DGA_DT_FP32, rstd, grad_residual, rows, static_cast<int>(h),
                               static_cast<int>(chunk_rows), chunks, dx, dx_dtype == DGA_DT_FP32, ws, vec);
            return record_hip(hipGetLastError());
        });
        if (rc || !dweight) return rc;
        hipLaunchKernelGGL(rms_norm_dweight_kernel, dim3(static_cast<unsigned>((h + 63) / 64)), dim3(64 * NORM_FINISH_SLICES), 0, s, ws, dweight,
                           chunks, static_cast<int>(h));
        return record_hip(hipGetLastError());
    });
}
