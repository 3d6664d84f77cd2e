// What the fp8 quantisers share (dga_cast.hip, dga_cast_transposed.hip, dga_cast_transposed_block.hip, dga_adamw_cast.hip, dga_gather_cast_transposed.hip, dga_silu_mul_cast.hip,
// dga_silu_mul_cast_transposed.hip, dga_silu_mul_bwd_cast.hip, dga_silu_mul_bwd_cast_transposed.hip, dga_rms_norm.hip; dga_combine.hip takes the element types' loads and stores).
// Device: the e4m3fn conversion, the 16-lane DPP row max, the block scale and the 8-element quotient recurrence of the 1x128 / 128x128 definition
// (oracle/: quant_1x128); the bounded 8-element loads and stores of the three types (Elem, load8_bounded, Store8, store1, store8_bounded, store_codes8); the fused kernels'
// row locator, refined sigmoid, silu(g) * u and its backward, each with its fp64-rounded block amax; the transposing kernels' row masks and the gathering one's
// table reads.  Host, at the end:
// the dtype dispatcher, the grid of 16-lane blocks and the fused entries' argument checks.  One text, so that every quantiser gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"

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

// An input type: one element, and the lane's 8 consecutive ones as one 16-byte (fp32: two) load.  load8 = unpack8(load8_raw): a kernel that
// issues several predicated loads before it uses any keeps the Raw words until then (the conversion is a use, and a use waits).
template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int kBytes = 4;
    struct Raw { v4f_c lo, hi; };
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return ((const float *)p)[i]; }
    static __device__ __forceinline__ Raw load8_raw(const void *p, int64_t i)
    {
        return Raw{*(const v4f_c *)((const float *)p + i), *(const v4f_c *)((const float *)p + i + 4)};
    }
    static __device__ __forceinline__ void unpack8(const Raw &w, float (&v)[8])
    {
        const v4f_c lo = w.lo, hi = w.hi;
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8]) { unpack8(load8_raw(p, i), v); }
};
struct Bf16Tag {};
struct F16Tag {};
template <> struct Elem<Bf16Tag> {
    static constexpr int kBytes = 2;
    typedef v4i_c Raw;
    static __device__ __forceinline__ float cv(uint32_t h) { return __uint_as_float(h << 16); }
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return cv(((const uint16_t *)p)[i]); }
    static __device__ __forceinline__ Raw load8_raw(const void *p, int64_t i) { return *(const v4i_c *)((const uint16_t *)p + i); }
    static __device__ __forceinline__ void unpack8(const Raw &w, float (&v)[8])
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float((uint32_t)w[j] << 16);
            v[2 * j + 1] = __uint_as_float((uint32_t)w[j] & 0xFFFF0000u);
        }
    }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8]) { unpack8(load8_raw(p, i), v); }
};
template <> struct Elem<F16Tag> {
    static constexpr int kBytes = 2;
    typedef _Float16 Raw __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float load(const void *p, int64_t i) { return (float)((const _Float16 *)p)[i]; }
    static __device__ __forceinline__ Raw load8_raw(const void *p, int64_t i) { return *(const Raw *)((const _Float16 *)p + i); }
    static __device__ __forceinline__ void unpack8(const Raw &w, float (&v)[8])
    {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)w[j];
    }
    static __device__ __forceinline__ void load8(const void *p, int64_t i, float (&v)[8]) { unpack8(load8_raw(p, i), v); }
};

// The lane's 8 elements, columns c0 .. c0 + 7 of a row of n columns, from element index `base` of p.  One 16-byte (fp32: two) load when the
// caller vouches for the alignment (vec) and all 8 are inside the row, else element by element with zeros at and beyond n.  row_ok = false
// (the 128x128 kernel's rows past the last): nothing is read, all 8 are zero.
template <typename T>
__device__ __forceinline__ void load8_bounded(const void *p, int64_t base, float (&v)[8], bool vec, int64_t c0, int64_t n, bool row_ok = true)
{
    if (row_ok && vec && c0 + 8 <= n) {
        Elem<T>::load8(p, base, v);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (row_ok && c0 + j < n) ? Elem<T>::load(p, base + j) : 0.f;
    }
}

// The store counterpart of Elem<T>::load8: 8 fp32 values -> 8 elements of T at element index i, round to nearest even for the 16-bit types
// (v_cvt_pk_bf16_f32, v_cvt_f16_f32), as they are for fp32.  vec: 16-byte stores.
template <typename T> struct Store8;
template <> struct Store8<float> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        float *o = (float *)p + i;
        if (vec) {
            *(v4f_c *)o = v4f_c{v[0], v[1], v[2], v[3]};
            *(v4f_c *)(o + 4) = v4f_c{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = v[j];
        }
    }
};
template <> struct Store8<Bf16Tag> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        typedef float v2f __attribute__((ext_vector_type(2)));
        typedef __bf16 v2b __attribute__((ext_vector_type(2)));
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f{v[2 * j], v[2 * j + 1]}), v2b));
        uint16_t *o = (uint16_t *)p + i;
        if (vec) {
            *(v4i_c *)o = v4i_c{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
        }
    }
};
template <> struct Store8<F16Tag> {
    static __device__ __forceinline__ void run(void *p, int64_t i, const float (&v)[8], bool vec)
    {
        typedef _Float16 v8h __attribute__((ext_vector_type(8)));
        _Float16 *o = (_Float16 *)p + i;
        if (vec) {
            *(v8h *)o = v8h{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3],
                            (_Float16)v[4], (_Float16)v[5], (_Float16)v[6], (_Float16)v[7]};
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (_Float16)v[j];
        }
    }
};

// one fp32 value -> one element of T at element index i, round to nearest even (Store8's conversions, one element at a time)
template <typename T> __device__ __forceinline__ void store1(void *p, int64_t i, float v);
template <> __device__ __forceinline__ void store1<float>(void *p, int64_t i, float v) { ((float *)p)[i] = v; }
template <> __device__ __forceinline__ void store1<Bf16Tag>(void *p, int64_t i, float v)
{
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef __bf16 v2b __attribute__((ext_vector_type(2)));
    ((uint16_t *)p)[i] = (uint16_t)__builtin_bit_cast(uint32_t, __builtin_convertvector((v2f{v, 0.f}), v2b));
}
template <> __device__ __forceinline__ void store1<F16Tag>(void *p, int64_t i, float v) { ((_Float16 *)p)[i] = (_Float16)v; }

// Store8's bounded form, the counterpart of load8_bounded (dga_rms_norm.hip, dga_adamw_cast.hip): columns c0 .. c0 + 7 of a row of n,
// nothing at or beyond n
template <typename T> __device__ __forceinline__ void store8_bounded(void *p, int64_t i, const float (&v)[8], bool vec, int64_t c0, int64_t n)
{
    if (vec && c0 + 8 <= n) {
        Store8<T>::run(p, i, v, true);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < n) store1<T>(p, i + j, v[j]);
    }
}

// The lane's 8 codes (w0: the first four, w1: the rest) to q, the place of columns c0 .. c0 + 7 of a row of n columns.  One 8-byte store when
// the caller vouches for the alignment (vec) and all 8 are inside the row, else byte by byte below n.  (c0, n) = (0, 8): all 8 are inside.
__device__ __forceinline__ void store_codes8(uint8_t *q, uint32_t w0, uint32_t w1, bool vec, int64_t c0, int64_t n)
{
    if (vec && c0 + 8 <= n) {
        *(v2i_c *)q = v2i_c{(int)w0, (int)w1};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c0 + j < n) q[j] = (uint8_t)(((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 0xFF);
    }
}

// a / b for 0 <= a, 0 < b: the 32-bit division when both fit (a quarter of the instructions of the 64-bit one)
__device__ __forceinline__ int64_t udiv(int64_t a, int64_t b, bool small)
{
    return small ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// The fused kernels' geometry: 16-lane block blk of rows of hb_n column blocks -> its row (counted over all groups of mmax rows) and column
// block b.  False: the mask excludes the row (masked_m: row r of group g with r >= masked_m[g]; m_indices: a negative index), and the caller
// returns before it reads anything.  The answer is the row's, so the 16 lanes of a block get the same one and leave together.
__device__ __forceinline__ bool locate_row(int64_t blk, int64_t hb_n, int64_t mmax, const int32_t *masked_m, const int32_t *m_indices,
                                           bool small, int64_t &row, int64_t &b)
{
    row = udiv(blk, hb_n, small);
    b = blk - row * hb_n;
    if (masked_m) {
        const int64_t g = udiv(row, mmax, small);
        return row - g * mmax < masked_m[g];
    }
    return !m_indices || m_indices[row] >= 0;
}

// s = 1 / (1 + e), e = exp(-g) = 2^(g * -log2 e): hardware exponential, hardware reciprocal, one Newton step.  With e = inf the reciprocal
// is 0 and the Newton residual -inf * 0 + 1 is NaN: v_max_f32 drops the NaN (any ordinary residual is far above -1), and the step then
// returns the 0.  A NaN g still comes out NaN (r0 is NaN, and so is -1 * r0 + r0).
constexpr float kNegLog2E = -1.4426950408889634f;
__device__ __forceinline__ float exp_neg(float g) { return __builtin_amdgcn_exp2f(g * kNegLog2E); }
__device__ __forceinline__ float sigmoid_refined(float g, float &e)
{
    e = exp_neg(g);
    const float d = 1.f + e;
    const float r0 = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaxf(__builtin_fmaf(-d, r0, 1.f), -1.f), r0, r0);
}

// silu(g) * u = (g s) u, s the refined sigmoid (sigmoid_refined: 0 for exp(-g) = inf, NaN for a NaN g)
__device__ __forceinline__ float silu_mul(float g, float u)
{
    float e;
    return (g * sigmoid_refined(g, e)) * u;
}

// The lane's largest |h| once more, as the fp32 nearest to the real-number value: the block scale is amax / 448, and an amax that is
// within 2^-19.7 but a ULP or two off the correctly rounded one puts every dequantised value (code x scale) of its block the same
// ULP off.  fp64 exponential and division (error 2^-51, so the one rounding to fp32 is the right one but for 2^-27 of the inputs),
// one element per lane and block.  Where 1 + exp(-g) rounds to 1 in fp32 the value stays h32 = fl32(g * u): the contract for
// gate >= 20.  h32 = |silu_mul(g, u)|.
__device__ __forceinline__ float silu_mul_abs_rounded(float g, float u, float h32)
{
    const bool one = 1.f + exp_neg(g) == 1.f;
    const double gd = g;
    const float hd = (float)(gd / (1.0 + exp(-gd)) * (double)u);
    return one ? h32 : __builtin_fabsf(hd);
}

// dgate = (d u) silu'(g) and dup = d (g s), s the refined sigmoid and e = exp(-g) (sigmoid_refined: s = 0 for e = inf).  t = e s is 1 - s;
// e = inf gives inf * 0 = NaN there, dropped by v_min_f32 in favour of the 1 that 1 - s tends to (e s <= 1 in real numbers, so the min
// changes nothing else).  A NaN g still gives NaN: s is NaN.
__device__ __forceinline__ void silu_mul_bwd(float g, float u, float d, float &dgate, float &dup)
{
    float e;
    const float s = sigmoid_refined(g, e);
    const float t = __builtin_fminf(e * s, 1.f);
    const float gs = g * s;
    dgate = (d * u) * __builtin_fmaf(gs, t, s);
    dup = d * gs;
}

// The lane's largest |dgate| and |dup| once more, as the fp32 nearest to the real-number value (silu_mul_abs_rounded's reasons: the
// block scale is amax / 448).  Where the fp32 factor is exactly 1 the value stays the fp32 product: the contract for gate >= 20.  An
// element whose fp32 value is 0 never is a lane's maximum, so g > -88.8 here and exp(-g) is finite in fp64.
__device__ __forceinline__ float dgate_abs_rounded(float g, float u, float d, float v32)
{
    const float e = exp_neg(g);
    const bool one = 1.f + e == 1.f && __builtin_fmaf(g, e, 1.f) == 1.f;
    const double gd = g, ed = exp(-gd), sd = 1.0 / (1.0 + ed);
    const float vd = (float)((double)d * (double)u * (sd * (1.0 + gd * (ed * sd))));
    return one ? v32 : __builtin_fabsf(vd);
}
__device__ __forceinline__ float dup_abs_rounded(float g, float d, float v32)
{
    const bool one = 1.f + exp_neg(g) == 1.f;
    const double gd = g;
    const float vd = (float)((double)d * (gd / (1.0 + exp(-gd))));
    return one ? v32 : __builtin_fabsf(vd);
}

// ---- the transposing quantisers (dga_cast_transposed.hip, dga_silu_mul_cast_transposed.hip, dga_silu_mul_bwd_cast_transposed.hip): 256 lanes on 128 tokens x 128 channels

// locate_row's predicate for the 8 consecutive rows r0 .. r0 + 7 of t_n > 0 (counted over all groups of mmax rows): ok[p] = the row exists
// and the mask does not exclude it.  No branch between the 8 reads of the mask, so they go out together: a row beyond the last asks about
// the last, and the group and the row in it come from one division, stepped (a step crosses at most one group boundary: mmax >= 1).
__device__ __forceinline__ void rows_valid8(int64_t r0, int64_t t_n, int64_t mmax, const int32_t *masked_m, const int32_t *m_indices,
                                            bool small, bool (&ok)[8])
{
    const int64_t last = t_n - 1, first = r0 < last ? r0 : last;
    if (masked_m) {
        int64_t g = udiv(first, mmax, small), r = first - g * mmax;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            ok[p] = (r < masked_m[g]) & (r0 + p <= last);
            r += r0 + p < last;
            const bool next = r == mmax;
            g += next;
            r = next ? 0 : r;
        }
    } else if (m_indices) {
#pragma unroll
        for (int p = 0; p < 8; ++p) ok[p] = (m_indices[r0 + p < last ? r0 + p : last] >= 0) & (r0 + p <= last);
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) ok[p] = r0 + p <= last;
    }
}

// ---- the 128x128 transposing quantisers (dga_cast_transposed_block.hip, dga_adamw_cast.hip): 256 lanes on one 128x128 tile of one group

// Where a lane stands: workgroup blk of groups x nb_n x kb_n tiles, walked along k, then n, then the groups; 16 lanes share a row, the lane
// holds columns c0 .. c0 + 7 of rows r0 .. r0 + 7, and g0 is the group's first element in [n, k] and in [k, n].
struct BlockTileAt {
    uint32_t g, nb, kb;
    int64_t c0, r0, g0;
};
__device__ __forceinline__ BlockTileAt block_tile_at(uint32_t blk, int t, int64_t n, int64_t k, uint32_t nb_n, uint32_t kb_n)
{
    const int sub = t & 15, rg = t >> 4;
    const uint32_t per_group = nb_n * kb_n;   // (the grid, groups * per_group, fits 31 bits)
    const uint32_t g = blk / per_group, in_g = blk - g * per_group;
    const uint32_t nb = in_g / kb_n, kb = in_g - nb * kb_n;
    const int64_t c0 = (int64_t)kb * 128 + sub * 8;   // the lane's 8 columns
    const int64_t r0 = (int64_t)nb * 128 + rg * 8;    // ... and its 8 rows
    const int64_t g0 = (int64_t)g * n * k;            // the group's first element, in w and q_row (row-major [n, k]) and in qt ([k, n])
    return BlockTileAt{g, nb, kb, c0, r0, g0};
}

// From the lane's 64 values v[pass][column] (zeros at rows where !ok[p] and at columns at and beyond k) to everything the tile writes:
//   tile maximum       in the lane over its 64 values (abs_for_max: no NaN of any kind reaches a maximum), over the wave by six cross-lane
//                      moves, over the 4 waves through red: one scale, written to sft[g, kb, nb] and to sf_row[g, nb, kb]
//   row-wise codes     quant8 on each pass's 8 columns -- cast_128x128_kernel's groups of 8 -- stored directly: a 16-lane group writes 128
//                      contiguous bytes of a row of q_row
//   transposed codes   quant8 on the lane's 8 rows of each of its 8 columns -- cast_128x128_kernel's groups of 8 on w^T --, then
//                      cast_1x128_transposed_kernel's 16 KB tile [128 columns][16 slots of 8 rows], slot r of column c at slot r ^ (c / 8)
//                      (its comment has the bank arithmetic): one 8-byte LDS store per column, one 8-byte load per lane and output row, and a
//                      16-lane group stores 128 contiguous bytes of a row of qt
// Codes of rows at and beyond n and of columns at and beyond k are never stored.  One text for both kernels: the same values give the same
// bytes.
template <bool ROWWISE>
__device__ __forceinline__ void quant_block_tile_transposed(const float (&v)[8][8], const bool (&ok)[8], const BlockTileAt &a, int t,
                                                            uint8_t *qt, float *sft, uint8_t *q_row, float *sf_row, int64_t n, int64_t k,
                                                            uint32_t nb_n, uint32_t kb_n, bool vec_qt, bool vec_row, bool ue8m0)
{
    __shared__ float red[4];
    __shared__ uint64_t tile[128 * 16];
    const int sub = t & 15, rg = t >> 4;
    const uint32_t g = a.g, nb = a.nb, kb = a.kb;
    const int64_t c0 = a.c0, r0 = a.r0, g0 = a.g0;
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, abs_for_max(v[p][j]));
    }
#pragma unroll
    for (int msk = 1; msk < 64; msk <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, msk, 64));
    if ((t & 63) == 0) red[t >> 6] = amax;
    __syncthreads();
    const float s = block_scale(__builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3])), ue8m0);
    if (t == 0) {
        sft[((int64_t)g * kb_n + kb) * nb_n + nb] = s;
        if (ROWWISE) sf_row[((int64_t)g * nb_n + nb) * kb_n + kb] = s;
    }
    if (ROWWISE) {
        // The same scale as a value the compiler cannot see through.  With one visible scale it computes the 64 quotients once for both
        // passes and keeps them beside the 64 inputs (the general path needs those): 212 VGPRs, 2 waves per SIMD, in
        // cast_128x128_transposed_kernel.  Two passes of quant8 as in cast_1x128_transposed_kernel, whose two passes have different
        // scales anyway: 108 (fp32) / 112 VGPRs and 4 waves per SIMD there, 136 .. 142 and 3 waves in the optimizer's kernel.
        float s_row = s;
        asm volatile("" : "+v"(s_row));
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            if (!ok[p]) continue;   // (uniform over the 16 lanes of the row)
            uint32_t w0, w1;
            quant8(v[p], s_row, w0, w1);
            store_codes8(q_row + g0 + (r0 + p) * k + c0, w0, w1, vec_row, c0, k);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float e[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) e[p] = v[p][j];
        uint32_t w0, w1;
        quant8(e, s, w0, w1);
        tile[(sub * 8 + j) * 16 + (rg ^ sub)] = (uint64_t)w0 | ((uint64_t)w1 << 32);
    }
    __syncthreads();
    const int64_t tc = (int64_t)nb * 128 + sub * 8;   // the first of the 8 rows of w this lane stores, of column rg + 16 i
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ch = rg + 16 * i;
        const int64_t c = (int64_t)kb * 128 + ch;
        if (c >= k) break;
        const uint64_t wv = tile[ch * 16 + (sub ^ (ch >> 3))];
        store_codes8(qt + g0 + c * n + tc, (uint32_t)wv, (uint32_t)(wv >> 32), vec_qt, tc, n);
    }
}

// ---- the gathering transposing quantiser (dga_gather_cast_transposed.hip): the rows of src behind a slot -> pair table

// The 8 tokens r0 .. r0 + 7 whose mask answers are ok[] (rows_valid8): token p reads row index[r0 + p] / index_div of src, h elements a
// row.  An index is read only where ok[p] -- the table holds stale values under the mask -- and a value outside [0, pairs) clears ok[p]:
// nothing is dereferenced through it.  No branch between the 8 index reads nor between the 8 scale reads (SCALED: sc[p] =
// row_scale[index], 0 where the row is excluded), so each set goes out together.  at[p] = the element index of column c0 of the row of
// src, meaningful where ok[p].  small: pairs fits 32 bits, and with it every valid index and index_div (udiv).
template <bool SCALED>
__device__ __forceinline__ void gather_rows8(const int64_t *index, const float *row_scale, int64_t r0, int64_t pairs, int64_t index_div,
                                             bool small, int64_t h, int64_t c0, bool (&ok)[8], int64_t (&at)[8], float (&sc)[8])
{
    int64_t ix[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        ix[p] = -1;
        if (ok[p]) ix[p] = index[r0 + p];
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) ok[p] = (uint64_t)ix[p] < (uint64_t)pairs;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        sc[p] = 0.f;
        if (SCALED && ok[p]) sc[p] = row_scale[ix[p]];
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) at[p] = (index_div == 1 ? ix[p] : udiv(ok[p] ? ix[p] : 0, index_div, small)) * h + c0;
}

// ---- host side: what the three units' launchers share

// dtype (DGA_DT_*) -> f(tag), tag an object of the type the kernels are instantiated on (float / Bf16Tag / F16Tag); DGA_E_DTYPE for any other
template <typename F> inline int dispatch_dtype(int dtype, F &&f)
{
    switch (dtype) {
        case DGA_DT_FP32: return f(float{});
        case DGA_DT_BF16: return f(Bf16Tag{});
        case DGA_DT_FP16: return f(F16Tag{});
        default: return DGA_E_DTYPE;
    }
}

// rows * per_row 16-lane blocks -> the grid of 256-thread workgroups (16 blocks each); DGA_E_RANGE beyond 2^31 - 1 workgroups, decided
// without the product: rows * per_row is inside int64 whenever this returns DGA_OK.  per_row > 0.
inline int grid_of_blocks(int64_t rows, int64_t per_row, unsigned &grid)
{
    if (rows > 0x7FFFFFFFll * 16 / per_row) return DGA_E_RANGE;
    grid = static_cast<unsigned>((rows * per_row + 15) / 16);
    return DGA_OK;
}

// What a fused kernel is launched with besides its pointers: rows_total * hb_n blocks of 16 lanes, hb_n = ceil(h / 128)
struct FusedGeometry {
    int64_t blocks, hb_n;
    unsigned grid;
    bool small;   // blocks and mmax fit 32 bits (udiv)
    bool ue8m0;
};

// The body of a fused entry point.  The checks in run_cast's order -- flags, shape (h a multiple of h_multiple), nothing to do, pointers
// (have_ptrs: none of the required ones is null), dtype, groups * rows and the grid -- then launch(tag, geometry).  shape_ok: what else an
// entry asks of its shape, refused with the shape.
template <typename L>
inline int run_fused(int flags, int dtype, int64_t groups, int64_t rows, int64_t h, int64_t h_multiple, const int32_t *masked_m,
                     const int32_t *m_indices, bool have_ptrs, L &&launch, bool shape_ok = true)
{
    if (flags & ~DGA_CAST_UE8M0) return DGA_E_RANGE;
    if (groups < 1 || rows < 0 || h < 0 || h % h_multiple != 0 || (masked_m && m_indices) || (m_indices && groups != 1) || !shape_ok)
        return DGA_E_SHAPE;
    if (rows == 0 || h == 0) return DGA_OK;
    if (!have_ptrs) return DGA_E_NULL;
    return dispatch_dtype(dtype, [&](auto tag) -> int {
        if (groups > 0x7FFFFFFFFFFFFFFFll / rows) return DGA_E_RANGE;
        FusedGeometry g;
        g.hb_n = (h + 127) / 128;
        if (int rc = grid_of_blocks(groups * rows, g.hb_n, g.grid)) return rc;
        g.blocks = groups * rows * g.hb_n;
        g.small = g.blocks <= 0xFFFFFFFFll && rows <= 0xFFFFFFFFll;
        g.ue8m0 = (flags & DGA_CAST_UE8M0) != 0;
        return launch(tag, g);
    });
}

// The transposing entries' row stride: T <= ldqt <= round_up(T, 128) with T = groups * rows, decided without a product or a sum that
// overflows (a T beyond int64 has no ldqt)
inline bool transposed_ldqt_ok(int64_t groups, int64_t rows, int64_t ldqt)
{
    if (groups < 1 || rows < 0 || rows > 0x7FFFFFFFFFFFFFFFll / groups) return false;
    const int64_t t_n = groups * rows;
    return ldqt >= t_n && ldqt - t_n <= (128 - t_n % 128) % 128;
}

}  // namespace dga
