// What the router's units share (dga_router.hip: the gate and its backward; dga_router_balance.hip: the balance loss): the layout -- one
// 64-lane wave per token, lane l owning the V consecutive experts l * V .. l * V + V - 1, V = 1, 2, 4, 8 or 16 the power of two with
// 64 V >= e --, the wave reductions on DPP, and a lane's reads and writes of its V elements.  Nothing here multiplies and adds in one
// expression, so the text means the same under either contraction setting; a unit that defines separate roundings sets
// `#pragma clang fp contract(off)` itself, after its includes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dga_cast_device.hpp"

namespace dga {

constexpr int ROUTER_WAVES = 4;          // tokens per workgroup

// ---- wave reductions on DPP alone.  Steps 0 .. 3 exchange inside a row of 16 lanes (quad permutes, then the two mirrors, as row16_max):
// after them every lane holds its row's result.  Steps 4 and 5 hand a row's last lane to the rows after it (row_bcast15 into rows 1 and 3,
// row_bcast31 into rows 2 and 3; a lane outside the mask receives `idle`, the merge's identity), so that lane 63 ends with the wave's result,
// which wave_result then gives to every lane.  The merges are commutative and associative; their order is fixed by the lane pattern.
template <int STEP> __device__ __forceinline__ int lane_xchg(int x, int idle)
{
    if constexpr (STEP == 0) return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
    else if constexpr (STEP == 1) return __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    else if constexpr (STEP == 2) return __builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false);  // row_half_mirror
    else if constexpr (STEP == 3) return __builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false);  // row_mirror
    else if constexpr (STEP == 4) return __builtin_amdgcn_update_dpp(idle, x, 0x142, 0xA, 0xF, false);   // row_bcast15 -> rows 1, 3
    else return __builtin_amdgcn_update_dpp(idle, x, 0x143, 0xC, 0xF, false);                            // row_bcast31 -> rows 2, 3
}
template <int STEP> __device__ __forceinline__ float lane_xchg(float x, float idle)
{
    return __builtin_bit_cast(float, lane_xchg<STEP>(__builtin_bit_cast(int, x), __builtin_bit_cast(int, idle)));
}
__device__ __forceinline__ int wave_result(int x) { return __builtin_amdgcn_readlane(x, 63); }
__device__ __forceinline__ float wave_result(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63)); }

template <int STEP = 0> __device__ __forceinline__ float wave_max(float x)
{
    if constexpr (STEP == 6) return wave_result(x);
    else return wave_max<STEP + 1>(__builtin_fmaxf(x, lane_xchg<STEP>(x, -__builtin_inff())));
}
// (V - 1 additions inside a lane, then these six: two runs give the same bits)
template <int STEP = 0> __device__ __forceinline__ float wave_sum(float x)
{
    if constexpr (STEP == 6) return wave_result(x);
    else return wave_sum<STEP + 1>(x + lane_xchg<STEP>(x, 0.f));
}

// ---- the lane's V consecutive elements of a row of e, experts i0 .. i0 + V - 1, at element index base + i0 of p
template <typename T> struct RouterElem;
template <> struct RouterElem<float> {
    typedef float Raw;
    static __device__ __forceinline__ float up(Raw r) { return r; }
    static __device__ __forceinline__ Raw down(float v) { return v; }
};
template <> struct RouterElem<Bf16Tag> {
    typedef uint16_t Raw;
    static __device__ __forceinline__ float up(Raw r) { return __uint_as_float((uint32_t)r << 16); }
    static __device__ __forceinline__ Raw down(float v)   // round to nearest even (v_cvt_pk_bf16_f32)
    {
        typedef float v2f __attribute__((ext_vector_type(2)));
        typedef __bf16 v2b __attribute__((ext_vector_type(2)));
        return (uint16_t)__builtin_bit_cast(uint32_t, __builtin_convertvector((v2f{v, 0.f}), v2b));
    }
};
template <> struct RouterElem<F16Tag> {
    typedef _Float16 Raw;
    static __device__ __forceinline__ float up(Raw r) { return (float)r; }
    static __device__ __forceinline__ Raw down(float v) { return (_Float16)v; }
};

// vec: the caller vouches that p is aligned to a lane's V elements and that e % V == 0.  Elements at and beyond e read as `pad`.
template <typename T, int V>
__device__ __forceinline__ void load_lane(const void *p, int64_t base, int i0, int e, bool vec, float pad, float (&v)[V])
{
    typedef typename RouterElem<T>::Raw Raw;
    const Raw *q = (const Raw *)p + base + i0;
    if constexpr (V > 1) {
        if (vec) {
            typedef Raw RawV __attribute__((ext_vector_type(V)));
            RawV w;
#pragma unroll
            for (int c = 0; c < V; ++c) w[c] = Raw{};
            if (i0 < e) w = *(const RawV *)q;
#pragma unroll
            for (int c = 0; c < V; ++c) v[c] = i0 < e ? RouterElem<T>::up(w[c]) : pad;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) {
        v[c] = pad;
        if (i0 + c < e) v[c] = RouterElem<T>::up(q[c]);
    }
}
template <typename T, int V>
__device__ __forceinline__ void store_lane(void *p, int64_t base, int i0, int e, bool vec, const float (&v)[V])
{
    typedef typename RouterElem<T>::Raw Raw;
    Raw *q = (Raw *)p + base + i0;
    if constexpr (V > 1) {
        if (vec) {
            typedef Raw RawV __attribute__((ext_vector_type(V)));
            RawV w;
#pragma unroll
            for (int c = 0; c < V; ++c) w[c] = RouterElem<T>::down(v[c]);
            if (i0 < e) *(RawV *)q = w;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c)
        if (i0 + c < e) q[c] = RouterElem<T>::down(v[c]);
}

// V for a row of e <= 1024 experts: the power of two with 64 V >= e -> f(integral_constant<int, V>)
template <typename F> inline int dispatch_lane_width(int64_t e, F &&f)
{
    if (e <= 64) return f(std::integral_constant<int, 1>{});
    if (e <= 128) return f(std::integral_constant<int, 2>{});
    if (e <= 256) return f(std::integral_constant<int, 4>{});
    if (e <= 512) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

// a lane's V elements of `bytes` each go as one vector: the tensor starts on such a vector and every row holds a whole number of them
inline bool router_vec(const void *p, int64_t e, int v, int bytes)
{
    return reinterpret_cast<uintptr_t>(p) % (static_cast<uintptr_t>(v) * bytes) == 0 && e % v == 0;
}

}  // namespace dga
