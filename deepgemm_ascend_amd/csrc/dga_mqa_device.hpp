// What the two scoring kernels of the lightning indexer share (dga_mqa_logits.hip: prefill, dga_paged_mqa_logits.hip: decode over the paged
// cache): the device text that fixes the bits of a logit.  One wave, its 64 keys as B fragments bf[nt][s] (key tile nt, k step s: lane l
// holds key 16 nt + (l & 15), codes 32 s + 8 (l >> 4) ..), one token's head tile as A fragments af[s] (lane l: head 16 ht + (l & 15), the
// same codes):
//   mqa_cvt8        8 e4m3 codes -> 8 bf16, exact
//   mqa_head_tile   s = four chained v_mfma_f32_16x16x32_bf16 over d ascending from a zero accumulator, per key tile; relu = s < 0 ? 0 : s
//                   (keeps a NaN); p[nt] = fma(w[reg], relu, p[nt]) over reg ascending -- called for ht ascending, from p = +0, that is P_g
//   mqa_exchange    (P_0 + P_2) + (P_1 + P_3) by the two-step exchange (lane ^ 32, then lane ^ 16) that leaves lane l with key l of the 64
// kscale multiplies the exchange's result once.  One text, so that both kernels give the same bits on the same operands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace dga {

typedef int mqa_v2i __attribute__((ext_vector_type(2)));
typedef int mqa_v4i __attribute__((ext_vector_type(4)));
typedef float mqa_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 mqa_v8bf __attribute__((ext_vector_type(8)));

// 8 e4m3 codes (ascending d) -> 8 bf16, exact
__device__ __forceinline__ mqa_v4i mqa_cvt8(mqa_v2i raw)
{
    mqa_v4i r;
    r[0] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[0], 1.0f, false));
    r[1] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[0], 1.0f, true));
    r[2] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[1], 1.0f, false));
    r[3] = __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(raw[1], 1.0f, true));
    return r;
}

// one head tile of one token against the wave's 64 keys: the dot products, the ReLU and the head tile's four steps of the fma chain
__device__ __forceinline__ void mqa_head_tile(const mqa_v4i (&af)[4], const mqa_v4i (&bf)[4][4], mqa_v4f w, float (&p)[4])
{
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        mqa_v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mqa_v8bf, af[s]), __builtin_bit_cast(mqa_v8bf, bf[nt][s]), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = acc[r] < 0.f ? 0.f : acc[r];          // (keeps a NaN)
            p[nt] = __builtin_fmaf(w[r], s, p[nt]);
        }
    }
}

// (P_0 + P_2) + (P_1 + P_3), lane group g = lane >> 4 keeping key tile g: lane l ends with key l of the wave's 64
__device__ __forceinline__ float mqa_exchange(const float (&p)[4], int g)
{
    const bool up2 = (g & 2) != 0, up1 = (g & 1) != 0;
    float k0 = up2 ? p[2] : p[0], k1 = up2 ? p[3] : p[1];
    k0 = k0 + __shfl_xor(up2 ? p[0] : p[2], 32, 64);
    k1 = k1 + __shfl_xor(up2 ? p[1] : p[3], 32, 64);
    float v = up1 ? k1 : k0;
    v = v + __shfl_xor(up1 ? k0 : k1, 16, 64);
    return v;
}

}  // namespace dga
