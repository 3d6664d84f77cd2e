// The gate of an MoE layer between the gate GEMM's logits and dga_route_slots' keys, and the last link of its backward:
//   dga_router_topk            logits [tokens, e] -> scores fp32 [tokens, e], ids int32 [tokens, k], weights fp32 [tokens, k]
//   dga_router_topk_backward   dw [tokens, k] (dga_combine_rows_weight_grad's output), scores, ids -> dlogits [tokens, e]
// One 64-lane wave per token, ROUTER_WAVES tokens per workgroup, the row in registers: lane l owns the V consecutive experts l * V ..
// l * V + V - 1 (V = 1, 2, 4, 8 or 16, the power of two with 64 V >= e), read and written as one vector where the row allows.  Maxima,
// sums, the groups' two largest values and the k rounds of arg-max are wave reductions that carry what they need with the value: six DPP
// steps and one v_readlane each.  No LDS (not even its crossbar), no atomics, nothing the host has to know: one launch, capturable.  HBM traffic: e * (input bytes + 4) + 8 k bytes per token, once.
//
// Two contracts (include/dga_hip.h has them whole): the scores are held to a bound against float64; ids and weights are exact fp32
// functions of the scores this kernel returns -- comparisons, one addition for the bias and for a group's value, the sum of the k chosen
// scores in the order of the choices, one correctly rounded division and one multiplication -- which numpy float32 reproduces bit for bit.
// This unit's own text is compiled without contraction (the pragma below, after the includes): a fused multiply-add rounds once and gives
// other bits.  dga_cast_device.hpp stays under the default; what is taken from it, sigmoid_refined, names its fused operations itself and
// feeds only the scores, which are bounded, not defined.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"
#include "dga_router_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr float kLog2E = 1.4426950408889634f;

// (lane_xchg, wave_result, wave_max and wave_sum: dga_router_device.hpp)
// What the k rounds of arg-max compare, as one unsigned 64-bit key: the high word orders the values as IEEE > does (-0 is +0 first, so the
// two tie; no value is a NaN) and is never 0, the low word is ~index, so of two equal values the lower index is the larger key.  Key 0 is
// "nothing": an expert that cannot (or can no longer) be chosen, and the idle input of a reduction step.
__device__ __forceinline__ uint32_t order_key(float x)
{
    const uint32_t b = __float_as_uint(x + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
template <int STEP = 0> __device__ __forceinline__ void wave_keymax(uint32_t &hi, uint32_t &lo)
{
    if constexpr (STEP < 6) {
        const uint32_t oh = (uint32_t)lane_xchg<STEP>((int)hi, 0), ol = (uint32_t)lane_xchg<STEP>((int)lo, 0);
        const bool other = (((uint64_t)oh << 32) | ol) > (((uint64_t)hi << 32) | lo);
        hi = other ? oh : hi;
        lo = other ? ol : lo;
        wave_keymax<STEP + 1>(hi, lo);
    } else {
        hi = (uint32_t)wave_result((int)hi);
        lo = (uint32_t)wave_result((int)lo);
    }
}
// the two largest values of the multiset (a1 >= a2): every step merges two disjoint sets of lanes
template <int STEP> __device__ __forceinline__ void top2_step(float &a1, float &a2)
{
    const float b1 = lane_xchg<STEP>(a1, -__builtin_inff()), b2 = lane_xchg<STEP>(a2, -__builtin_inff());
    a2 = __builtin_fmaxf(__builtin_fminf(a1, b1), __builtin_fmaxf(a2, b2));
    a1 = __builtin_fmaxf(a1, b1);
}
template <int STEP = 0> __device__ __forceinline__ void wave_top2(float &a1, float &a2)
{
    if constexpr (STEP < 6) {
        top2_step<STEP>(a1, a2);
        wave_top2<STEP + 1>(a1, a2);
    } else {
        a1 = wave_result(a1);
        a2 = wave_result(a2);
    }
}
// a group's value from its two largest sel; (+inf) + (-inf) counts as -inf, like a NaN sel
__device__ __forceinline__ float group_value(float a1, float a2)
{
    const float gv = a1 + a2;
    return gv == gv ? gv : -__builtin_inff();
}

// (load_lane and store_lane: dga_router_device.hpp)

// The widest build's unrolled loops over a lane's 16 elements: left alone the scheduler issues all their comparisons first, and the 16 to 48
// lane masks push the kernel's pointers out of the scalar registers.  A fence after each element keeps a mask's life to its element.
template <int V> __device__ __forceinline__ void lane_mask_fence()
{
    if constexpr (V >= 16) __builtin_amdgcn_sched_barrier(0);
}

// Element `index` of the row (lane index / V, slot index % V), index uniform: every slot of that lane is read with a v_readlane and the
// choice is made among the scalars.  (Choosing the slot first, in the lane, looks like an array indexed at run time to the compiler, which
// then moves the array to LDS.)
template <int V> __device__ __forceinline__ float read_element(const float (&v)[V], int index)
{
    constexpr int LOGV = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : V == 8 ? 3 : 4;
    const int lane = index >> LOGV, slot = index & (V - 1);
    int r = __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[0]), lane);
#pragma unroll
    for (int c = 1; c < V; ++c) {
        const int x = __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c]), lane);
        r = c == slot ? x : r;
    }
    return __builtin_bit_cast(float, r);
}

template <typename T, int V>
__global__ void __launch_bounds__(64 * ROUTER_WAVES) router_topk_kernel(const void *logits, const float *bias, int32_t *ids, float *weights,
                                                                        float *scores, int64_t tokens, int e, int k, int n_groups,
                                                                        int topk_groups, bool sigmoid, bool renormalize, float scale,
                                                                        bool vec_in, bool vec_out)
{
    constexpr int LOGV = V == 1 ? 0 : V == 2 ? 1 : V == 4 ? 2 : V == 8 ? 3 : 4;
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * ROUTER_WAVES + (threadIdx.x >> 6);
    if (t >= tokens) return;   // (the whole wave: every exchange below runs with 64 active lanes)
    const int i0 = lane * V;
    const int64_t base = t * e;
    const float ninf = -__builtin_inff();

    // ---- scores
    float s[V];
    load_lane<T, V>(logits, base, i0, e, vec_in, ninf, s);
    if (sigmoid) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
            float ex;
            s[c] = sigmoid_refined(s[c], ex);
        }
    } else {
        float m = s[0];
#pragma unroll
        for (int c = 1; c < V; ++c) m = __builtin_fmaxf(m, s[c]);
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            s[c] = __builtin_amdgcn_exp2f((s[c] - m) * kLog2E);   // (beyond e: exp2(-inf) = +0, which changes no sum)
            sum = sum + s[c];
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int c = 0; c < V; ++c) s[c] = s[c] / sum;
    }
    store_lane<float, V>(scores, base, i0, e, vec_out, s);

    // ---- what the selection compares: sel = fl32(score + bias), a NaN counts as -inf; avail = the experts that may still be chosen
    float sel[V];
    uint32_t avail = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        float b = 0.f;
        if (bias && i0 + c < e) b = bias[i0 + c];
        const float x = bias ? s[c] + b : s[c];
        sel[c] = x == x ? x : ninf;
        avail |= (i0 + c < e ? 1u : 0u) << c;
    }

    // ---- group-limited routing: a group's value is the sum of its two largest sel; the topk_groups largest groups stay (ties: the lower
    // group), the experts of the others leave avail.
    if (n_groups > 1) {
        const int gs = e / n_groups;
        const int lanes = gs >> LOGV;
        if ((gs & (V - 1)) == 0 && lanes <= 16 && (lanes & (lanes - 1)) == 0) {
            // A group is 1, 2, 4, 8 or 16 whole lanes (DeepSeek-V3: 256 experts in 8 groups, 8 lanes each): the first steps of the reduction
            // stay inside such a set of lanes, so all groups are valued at once and every lane ends with its own group's value.
            float a1 = ninf, a2 = ninf;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                a2 = __builtin_fmaxf(a2, __builtin_fminf(a1, sel[c]));
                a1 = __builtin_fmaxf(a1, sel[c]);
            }
            if (lanes > 1) top2_step<0>(a1, a2);
            if (lanes > 2) top2_step<1>(a1, a2);
            if (lanes > 4) top2_step<2>(a1, a2);
            if (lanes > 8) top2_step<3>(a1, a2);
            const float mine = group_value(a1, a2);
            const int my_group = lane >> (31 - __builtin_clz(lanes));   // (a lane beyond e: a group that does not exist, nothing to lose)
            int rank = 0;
            for (int g = 0; g < n_groups; ++g) {
                const float gv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), g * lanes));
                rank += ((gv > mine) | ((gv == mine) & (g < my_group))) ? 1 : 0;
            }
            if (rank >= topk_groups) avail = 0;
        } else {
            // Any other group size: a group is a range of experts, not of lanes, and the groups are valued one after the other.  Every
            // element keeps its group and the group's value, and counts the groups that go before its own.
            // an element's group, i / gs, without an integer division: (i + 0.5) / gs is at least 2^-11 away from every integer (i, gs <= 1024),
            // the two fp32 roundings move it by less than 2^-13
            const float per_gs = 1.f / (float)gs;
            float gval[V];
            int grp[V], rank[V];
#pragma unroll
            for (int c = 0; c < V; ++c) {
                gval[c] = ninf;
                grp[c] = (int)(((float)(i0 + c) + 0.5f) * per_gs);   // (beyond e: n_groups or more, no group)
                rank[c] = 0;
            }
            for (int g = 0; g < n_groups; ++g) {
                float a1 = ninf, a2 = ninf;
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const float x = grp[c] == g ? sel[c] : ninf;
                    a2 = __builtin_fmaxf(a2, __builtin_fminf(a1, x));
                    a1 = __builtin_fmaxf(a1, x);
                    lane_mask_fence<V>();
                }
                wave_top2(a1, a2);
                const float gv = group_value(a1, a2);
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    gval[c] = grp[c] == g ? gv : gval[c];
                    lane_mask_fence<V>();
                }
            }
            for (int g = 0; g < n_groups; ++g) {
                const float gv = read_element(gval, g * gs);   // the group's first expert holds its value
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    rank[c] += ((gv > gval[c]) | ((gv == gval[c]) & (g < grp[c]))) ? 1 : 0;
                    lane_mask_fence<V>();
                }
            }
#pragma unroll
            for (int c = 0; c < V; ++c)
                if (rank[c] >= topk_groups) avail &= ~(1u << c);
        }
    }

    // ---- k rounds of arg-max over what may still be chosen; lane j keeps choice j.  At least k experts have a key (the entry checks k <= e
    // and topk_groups * (e / n_groups) >= k), so every round finds one: k distinct ids in [0, e), whatever the row holds.
    uint32_t key[V];
#pragma unroll
    for (int c = 0; c < V; ++c) key[c] = ((avail >> c) & 1u) ? order_key(sel[c]) : 0u;
    int my_id = 0;
    float my_r = 0.f, denom = 0.f;
    for (int j = 0; j < k; ++j) {
        uint32_t bk = 0, bl = 0;   // the lane's best candidate, and its score
        float br = 0.f;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const bool take = key[c] > bk;   // (strict: of equal values the lower index stays)
            bk = take ? key[c] : bk;
            bl = take ? ~(uint32_t)(i0 + c) : bl;
            br = take ? s[c] : br;
        }
        wave_keymax(bk, bl);
        const int id = (int)~bl;   // (uniform: the reduction ends in a v_readlane)
#pragma unroll
        for (int c = 0; c < V; ++c) key[c] = i0 + c == id ? 0u : key[c];
        const float r = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, br), id >> LOGV));   // the winner's own
        denom = j == 0 ? r : denom + r;   // ((r_0 + r_1) + ...) + r_{k-1}
        if (lane == j) {
            my_id = id;
            my_r = r;
        }
    }
    if (lane < k) {
        ids[t * k + lane] = my_id;
        weights[t * k + lane] = renormalize ? (my_r / denom) * scale : my_r * scale;
    }
}

// One wave per token: lane j < k holds choice j.  D and w as the forward computed them; the two sums over the choices are wave sums in a
// fixed order; then every lane writes its V elements of the row.
template <typename O, int V>
__global__ void __launch_bounds__(64 * ROUTER_WAVES) router_topk_backward_kernel(const float *dw, const float *scores, const int32_t *ids,
                                                                                 void *dlogits, int64_t tokens, int e, int k, bool sigmoid,
                                                                                 bool renormalize, float scale, bool vec_in, bool vec_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * ROUTER_WAVES + (threadIdx.x >> 6);
    if (t >= tokens) return;
    const int i0 = lane * V;
    const int64_t base = t * e;

    float s[V];
    load_lane<float, V>(scores, base, i0, e, vec_in, 0.f, s);
    int id = -1;
    float d = 0.f, r = 0.f;
    if (lane < k) {
        id = ids[t * k + lane];
        d = dw[t * k + lane];
        if ((uint32_t)id < (uint32_t)e) r = scores[base + id];   // (an id outside [0, e) reads nothing and meets no element below)
    }
    float g = scale * d;
    if (renormalize) {
        float denom = 0.f;
        for (int j = 0; j < k; ++j) {
            const float rj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), j));
            denom = j == 0 ? rj : denom + rj;
        }
        const float w = (r / denom) * scale;
        const float dot = wave_sum(lane < k ? d * w : 0.f);
        g = (g - dot) / denom;
    }
    const float sdot = sigmoid ? 0.f : wave_sum(lane < k ? g * r : 0.f);   // sum_l ds_l s_l
    float ds[V];
    uint32_t hit = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) ds[c] = 0.f;
    for (int j = 0; j < k; ++j) {
        const int idj = __builtin_amdgcn_readlane(id, j);
        const float gj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g), j));
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const bool mine = i0 + c == idj;
            ds[c] = mine ? gj : ds[c];
            hit |= (mine ? 1u : 0u) << c;
        }
    }
    float out[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
        if (sigmoid) out[c] = ((hit >> c) & 1u) ? (ds[c] * s[c]) * (1.f - s[c]) : 0.f;   // +0 off the selection, whatever the score
        else out[c] = s[c] * (ds[c] - sdot);
    }
    store_lane<O, V>(dlogits, base, i0, e, vec_out, out);
}

// the checks the two entries share, in the combine entries' order: shape, then (after nothing-to-do, pointers and dtype, which are the
// entry's own) what a launch cannot take
inline int router_shape(int64_t tokens, int64_t e, int64_t k)
{
    if (tokens < 0 || e < 0 || k < 1 || k > e) return DGA_E_SHAPE;
    return DGA_OK;
}
inline int router_range(int64_t tokens, int64_t e, int64_t k, int score_func, int flags, unsigned &grid)
{
    if (e > DGA_ROUTER_MAX_EXPERTS || k > DGA_ROUTER_MAX_TOPK) return DGA_E_RANGE;
    if ((score_func != DGA_ROUTER_SOFTMAX && score_func != DGA_ROUTER_SIGMOID) || (flags & ~DGA_ROUTER_RENORMALIZE)) return DGA_E_RANGE;
    const int64_t groups = (tokens + ROUTER_WAVES - 1) / ROUTER_WAVES;
    if (groups > 0x7FFFFFFFll) return DGA_E_RANGE;
    grid = static_cast<unsigned>(groups);
    return DGA_OK;
}
}  // namespace dga

extern "C" int dga_router_topk(const void *logits, int logits_dtype, int64_t tokens, int64_t experts, int64_t k, int score_func,
                               const float *bias, int64_t n_groups, int64_t topk_groups, int flags, float scale, int32_t *ids, float *weights,
                               float *scores, void *stream)
{
    using namespace dga;
    if (int rc = router_shape(tokens, experts, k)) return rc;
    if (n_groups < 1 || experts % n_groups != 0 || topk_groups < 1 || topk_groups > n_groups) return DGA_E_SHAPE;
    const int64_t gs = experts / n_groups;   // (topk_groups * gs <= experts: no overflow)
    if (topk_groups * gs < k || (n_groups > 1 && gs < 2)) return DGA_E_SHAPE;
    if (tokens == 0) return DGA_OK;
    if (!logits || !ids || !weights || !scores) return DGA_E_NULL;
    return dispatch_dtype(logits_dtype, [&](auto tag) -> int {
        using T = decltype(tag);
        unsigned grid;
        if (int rc = router_range(tokens, experts, k, score_func, flags, grid)) return rc;
        return dispatch_lane_width(experts, [&](auto width) -> int {
            constexpr int V = decltype(width)::value;
            hipLaunchKernelGGL((router_topk_kernel<T, V>), dim3(grid), dim3(64 * ROUTER_WAVES), 0, static_cast<hipStream_t>(stream), logits,
                               bias, ids, weights, scores, tokens, static_cast<int>(experts), static_cast<int>(k), static_cast<int>(n_groups),
                               static_cast<int>(topk_groups), score_func == DGA_ROUTER_SIGMOID, (flags & DGA_ROUTER_RENORMALIZE) != 0, scale,
                               router_vec(logits, experts, V, Elem<T>::kBytes), router_vec(scores, experts, V, 4));
            return record_hip(hipGetLastError());
        });
    });
}

extern "C" int dga_router_topk_backward(const float *dw, const float *scores, const int32_t *ids, int64_t tokens, int64_t experts, int64_t k,
                                        int score_func, int flags, float scale, void *dlogits, int dlogits_dtype, void *stream)
{
    using namespace dga;
    if (int rc = router_shape(tokens, experts, k)) return rc;
    if (tokens == 0) return DGA_OK;
    if (!dw || !scores || !ids || !dlogits) return DGA_E_NULL;
    return dispatch_dtype(dlogits_dtype, [&](auto tag) -> int {
        using O = decltype(tag);
        unsigned grid;
        if (int rc = router_range(tokens, experts, k, score_func, flags, grid)) return rc;
        return dispatch_lane_width(experts, [&](auto width) -> int {
            constexpr int V = decltype(width)::value;
            hipLaunchKernelGGL((router_topk_backward_kernel<O, V>), dim3(grid), dim3(64 * ROUTER_WAVES), 0, static_cast<hipStream_t>(stream),
                               dw, scores, ids, dlogits, tokens, static_cast<int>(experts), static_cast<int>(k),
                               score_func == DGA_ROUTER_SIGMOID, (flags & DGA_ROUTER_RENORMALIZE) != 0, scale,
                               router_vec(scores, experts, V, 4), router_vec(dlogits, experts, V, Elem<O>::kBytes));
            return record_hip(hipGetLastError());
        });
    });
}
