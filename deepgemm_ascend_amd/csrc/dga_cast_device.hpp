// Device helpers shared by the fp8 quantisers (dga_cast.hip, dga_silu_mul_cast.hip): the e4m3fn conversion, the 16-lane
// DPP row max, the block scale and the 8-element quotient recurrence of the 1x128 / 128x128 definition (oracle/:
// quant_1x128), and the 8-element loads of the three input types.  One text, so that every quantiser gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dga {

typedef float v4f_c __attribute__((ext_vector_type(4)));
typedef int v4i_c __attribute__((ext_vector_type(4)));
typedef int v2i_c __attribute__((ext_vector_type(2)));

// two quotients qa = xa / s, qb = xb / s -> two e4m3fn bytes (low 16 bits), any input.  v_cvt_pk_fp8_f32 is OCP e4m3fn on gfx950
// (round to nearest even, subnormals included) but turns overflow into the NaN code and every NaN into 0xFF (probed:
// scripts/ubench/probe_cvt_fp8.hip); the definition saturates (satfinite) and encodes NaN as sign | 0x7F, so quotients are
// clamped first and NaN is patched afterwards.  The sign of a NaN code is the INPUT's: the divide's own choice of a NaN's sign
// is the hardware's business (x NaN; or +-inf / +inf in a block whose amax, and with it s, is infinite -- there a finite x
// gives a zero of x's sign, which the conversion keeps).
__device__ __forceinline__ uint32_t cvt2_e4m3fn(float qa, float qb, float xa, float xb)
{
    const float ca = __builtin_fminf(__builtin_fmaxf(qa, -448.f), 448.f);
    const float cb = __builtin_fminf(__builtin_fmaxf(qb, -448.f), 448.f);
    uint32_t r = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(ca, cb, 0, false) & 0xFFFFu;
    if (qa != qa) r = (r & 0xFF00u) | ((__float_as_uint(xa) >> 24) & 0x80u) | 0x7Fu;
    if (qb != qb) r = (r & 0x00FFu) | ((((__float_as_uint(xb) >> 24) & 0x80u) | 0x7Fu) << 8);
    return r;
}

// |x| as it enters a block maximum: a signalling NaN quieted first (v_max_f32 x, x).  v_max_f32 is IEEE maxNum: it drops a quiet
// NaN operand but answers a signalling one with a NaN -- which the next max then drops together with everything the lane had
// seen so far, and a lane (or a block) that ends on it has no maximum at all.  The definition ignores every NaN.
__device__ __forceinline__ float abs_for_max(float x) { return __builtin_canonicalizef(__builtin_fabsf(x)); }

// max over the 16 lanes of a DPP row (= one 1x128 block), result in every lane: row_mirror, row_half_mirror, then the
// two quad permutes -- four v_max_f32_dpp, no LDS traffic.
template <int CTRL> __device__ __forceinline__ float dpp_max(float x)
{
    const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false);
    return __builtin_fmaxf(x, __builtin_bit_cast(float, y));
}
__device__ __forceinline__ float row16_max(float x)
{
    x = dpp_max<0x140>(x);  // row_mirror: lane i <-> 15 - i
    x = dpp_max<0x141>(x);  // row_half_mirror: i <-> 7 - i inside each half
    x = dpp_max<0x4E>(x);   // quad_perm [2,3,0,1]
    x = dpp_max<0xB1>(x);   // quad_perm [1,0,3,2]
    return x;
}

// DGA_CAST_UE8M0: the block scale rounded UP to a power of two, 2^ceil(log2(amax / 448)) -- upstream DeepGEMM's use_ue8m0
// quantisation; such scales ride in the matrix instruction's E8M0 operands (DGA_POLICY_UE8M0_SCALES).  Exact on the bits: a
// scale with a non-zero mantissa moves to the next exponent.
__device__ __forceinline__ float block_scale(float amax, bool ue8m0)
{
    float s = amax > 0.f ? amax / 448.f : 1.f;
    if (ue8m0) {
        const uint32_t b = __float_as_uint(s);
        if (b & 0x007FFFFFu) s = __uint_as_float((b & 0x7F800000u) + 0x00800000u);
    }
    return s;
}

__device__ __forceinline__ bool has_ff_byte(uint32_t w) { return (((~w) - 0x01010101u) & w & 0x80808080u) != 0; }

// 8 values of one scale block -> 8 codes.  Fast path: the IEEE quotient x / s by the compiler's own fp32 division
// recurrence (rcp, one Newton step, then q, two residual corrections -- the final fma is the correctly rounded
// quotient) with the reciprocal refined once per block instead of once per element, and without the range scaling,
// which is not needed while s is far from the ends of the exponent range.  No clamp either: |x / s| <= 448 (1 + 2^-22)
// rounds to 448.  Anything unusual -- s tiny, huge, infinite, or a NaN among the inputs (the hardware's 0xFF code
// shows it) -- takes the general path: true division, clamp, NaN patch (an infinite amax: scale +inf, finite elements the zero
// of their sign, +-inf and NaN sign | 0x7F).
// Returns whether the fast path met a 0xFF code, i.e. whether a NaN is among the 8 inputs.
__device__ __forceinline__ bool quant8(const float (&v)[8], float s, uint32_t &w0, uint32_t &w1)
{
    const uint32_t sb = __float_as_uint(s);
    const bool s_ok = (sb - 0x20000000u) < 0x3F000000u;  // 2^-63 <= s < 2^63
    const float r0 = __builtin_amdgcn_rcpf(s);
    const float r1 = __builtin_fmaf(__builtin_fmaf(-s, r0, 1.f), r0, r0);
    float q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float q0 = v[j] * r1;
        const float q1 = __builtin_fmaf(__builtin_fmaf(-s, q0, v[j]), r1, q0);
        // s > 0: the quotient has x's sign, also when it is a zero (the residual steps turn -0 into +0)
        q[j] = __builtin_copysignf(__builtin_fmaf(__builtin_fmaf(-s, q1, v[j]), r1, q1), v[j]);
    }
    w0 = ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false) & 0xFFFFu) |
         ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], 0, false) << 16);
    w1 = ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], 0, false) & 0xFFFFu) |
         ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], 0, false) << 16);
    const bool ff = has_ff_byte(w0) || has_ff_byte(w1);
    if (!s_ok || ff) {
        w0 = cvt2_e4m3fn(v[0] / s, v[1] / s, v[0], v[1]) | (cvt2_e4m3fn(v[2] / s, v[3] / s, v[2], v[3]) << 16);
        w1 = cvt2_e4m3fn(v[4] / s, v[5] / s, v[4], v[5]) | (cvt2_e4m3fn(v[6] / s, v[7] / s, v[6], v[7]) << 16);
    }
    return ff;
}

// One 1x128 block held by the 16 lanes of a DPP row, 8 elements per lane: its scale s and the lane's 8 codes.  The maximum is
// taken with plain v_max_f32 first, which a signalling NaN poisons (abs_for_max); quieting every element up front costs the
// two-block kernel 2 % on [32768, 7168] bf16 (profiles/cast_snan_ab.txt).  Any NaN shows as a 0xFF code of the lane that holds
// it, whatever the scale was, so a wave that saw one (a uniform branch, never taken on NaN-free data) takes the maximum again
// with quieted elements and quantises again; its NaN-free rows compute what they had.
__device__ __forceinline__ void quant_row_block(const float (&v)[8], bool ue8m0, float &s, uint32_t &w0, uint32_t &w1)
{
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf(v[j]));
    s = block_scale(row16_max(amax), ue8m0);
    const bool nan = quant8(v, s, w0, w1);
    if (__builtin_amdgcn_ballot_w64(nan) != 0) {
        amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, abs_for_max(v[j]));
        s = block_scale(row16_max(amax), ue8m0);
        quant8(v, s, w0, w1);
    }
}

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return ((const float *)p)[i]; }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8])
    {
        const v4f_c lo = *(const v4f_c *)((const float *)p + i), hi = *(const v4f_c *)((const float *)p + i + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    }
};
struct Bf16Tag {};
struct F16Tag {};
template <> struct Elem<Bf16Tag> {
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ float cv(uint32_t h) { return __uint_as_float(h << 16); }
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return cv(((const uint16_t *)p)[i]); }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8])
    {
        const v4i_c w = *(const v4i_c *)((const uint16_t *)p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float((uint32_t)w[j] << 16);
            v[2 * j + 1] = __uint_as_float((uint32_t)w[j] & 0xFFFF0000u);
        }
    }
};
template <> struct Elem<F16Tag> {
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return (float)((const _Float16 *)p)[i]; }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8])
    {
        typedef _Float16 v8h __attribute__((ext_vector_type(8)));
        const v8h w = *(const v8h *)((const _Float16 *)p + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)w[j];
    }
};

}  // namespace dga
