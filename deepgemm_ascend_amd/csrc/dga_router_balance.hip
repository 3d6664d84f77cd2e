// What a trained router needs beside the gate (dga_router.hip): the load-balancing loss over dga_router_topk's scores and ids, its
// backward into the logits' gradient, and DeepSeek-V3's bias update from the same per-expert counts.
//   dga_router_balance_loss            scores [tokens, e], ids [tokens, k] -> loss [B], counts int32 [B, e], psum [B, e]   (B segments of L tokens)
//   dga_router_balance_loss_backward   dloss [B], counts, scores (+ add_to) -> dlogits [tokens, e]
//   dga_router_bias_update             bias[e] += rate * sign(mean count - count of e), compared as integers
// The loss runs in two launches.  Stage one: a workgroup of ROUTER_WAVES waves takes a chunk of balance_chunk_tokens consecutive tokens of
// one segment; every wave walks its tokens in the router's layout (lane l owns experts l * V .. l * V + V - 1), the running sums and
// counts in registers, a lane counting its own experts from v_readlane of the k ids; the four waves meet in LDS and the chunk's sums go
// to the workspace, fp32 and int32 [B, chunks, e].  Stage two: one workgroup per segment adds the chunks' partials in ascending order --
// `slices` threads per expert, each a contiguous run of chunks, the runs then in ascending order --, writes psum and counts and forms the
// loss with wave_sum.  Every sum has one fixed order that depends on the shape alone: no floating-point atomics, the same bits twice.
// The backward is one wave per token like the router's.  This unit's own text is compiled without contraction (the pragma below): the
// backward with add_to is defined as the separate sum of add_to and the value the entry gives without it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_cast_device.hpp"
#include "dga_router_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int BALANCE_FINISH_THREADS = 1024;
constexpr int BALANCE_AHEAD = 4;        // rows a wave of stage one has in flight
constexpr int BALANCE_FINISH_AHEAD = 32; // partials a thread of stage two has in flight, of each kind
constexpr int BIAS_THREADS = DGA_ROUTER_MAX_EXPERTS;

// tokens of a segment one stage-one workgroup takes: a multiple of ROUTER_WAVES, at least 16, and no more than about 2048 chunks over all
// the tokens -- enough workgroups to fill the part when one segment holds them all, few enough partials for stage two.  A function of
// the shape alone, so the order of every sum is too.
inline int64_t balance_chunk_tokens(int64_t tokens)
{
    const int64_t per = ROUTER_WAVES * ((tokens + 2047) / 2048);
    return per < 16 ? 16 : per;
}
inline int64_t balance_chunks(int64_t tokens, int64_t seq_len)
{
    const int64_t per = balance_chunk_tokens(tokens);
    return (seq_len + per - 1) / per;
}

template <int V>
__global__ void __launch_bounds__(64 * ROUTER_WAVES) balance_partial_kernel(const float *scores, const int32_t *ids, float *ws_p, int32_t *ws_c,
                                                                           int64_t seq_len, int chunk_tokens, uint32_t chunks, int e, int k,
                                                                           bool normalize, bool vec)
{
    __shared__ float lds_p[ROUTER_WAVES][64 * V];
    __shared__ int32_t lds_c[ROUTER_WAVES][64 * V];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int64_t first = (int64_t)chunk * chunk_tokens;                      // (inside the segment)
    const int64_t left = seq_len - first;
    const int n = left < chunk_tokens ? (int)left : chunk_tokens;             // the last chunk of a segment may be short
    const int i0 = lane * V;

    float acc[V];
    int32_t cnt[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
        acc[c] = 0.f;
        cnt[c] = 0;
    }
    // The wave's tokens are w, w + 4, w + 8 ... of the chunk, BALANCE_AHEAD of them in flight at a time: the rows are read first, without a
    // condition (a token beyond the chunk reads the chunk's last one again), and what such a token would add is dropped at the sums.
    for (int i = w; i < n; i += ROUTER_WAVES * BALANCE_AHEAD) {   // (uniform in the wave: every exchange below runs with 64 active lanes)
        float s[BALANCE_AHEAD][V];
        int id[BALANCE_AHEAD];
#pragma unroll
        for (int u = 0; u < BALANCE_AHEAD; ++u) {
            const int iu = i + u * ROUTER_WAVES;
            const int64_t t = (int64_t)b * seq_len + first + (iu < n ? iu : n - 1);
            load_lane<float, V>(scores, t * e, i0, e, vec, 0.f, s[u]);
            id[u] = -1;
            if (lane < k) id[u] = ids[t * k + lane];
        }
#pragma unroll
        for (int u = 0; u < BALANCE_AHEAD; ++u) {
            const bool live = i + u * ROUTER_WAVES < n;
            if (normalize) {
                float sum = s[u][0];
#pragma unroll
                for (int c = 1; c < V; ++c) sum = sum + s[u][c];
                sum = wave_sum(sum);
#pragma unroll
                for (int c = 0; c < V; ++c) s[u][c] = s[u][c] / sum;
            }
#pragma unroll
            for (int c = 0; c < V; ++c) acc[c] = live ? acc[c] + s[u][c] : acc[c];
            for (int j = 0; j < (live ? k : 0); ++j) {   // (an id outside [0, e) meets no expert that is written)
                const int idj = __builtin_amdgcn_readlane(id[u], j);
#pragma unroll
                for (int c = 0; c < V; ++c) cnt[c] += i0 + c == idj ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) {
        lds_p[w][i0 + c] = acc[c];
        lds_c[w][i0 + c] = cnt[c];
    }
    __syncthreads();
    const int64_t out = (int64_t)blockIdx.x * e;                             // [B, chunks, e]
    for (int x = threadIdx.x; x < e; x += 64 * ROUTER_WAVES) {
        float p = lds_p[0][x];
        int32_t c = lds_c[0][x];
#pragma unroll
        for (int v = 1; v < ROUTER_WAVES; ++v) {
            p = p + lds_p[v][x];
            c += lds_c[v][x];
        }
        ws_p[out + x] = p;
        ws_c[out + x] = c;
    }
}

// One workgroup per segment.  et = e rounded up to whole waves; thread (slice, x) adds expert x's partials over the slice's chunks.
__global__ void __launch_bounds__(BALANCE_FINISH_THREADS) balance_finish_kernel(const float *ws_p, const int32_t *ws_c, float *loss,
                                                                                int32_t *counts, float *psum, uint32_t chunks, int e, float coef)
{
    __shared__ float lds_p[BALANCE_FINISH_THREADS];
    __shared__ int32_t lds_c[BALANCE_FINISH_THREADS];
    __shared__ float lds_w[BALANCE_FINISH_THREADS / 64];
    const int et = (e + 63) & ~63, slices = BALANCE_FINISH_THREADS / et;
    const int slice = threadIdx.x / et, x = threadIdx.x - slice * et;
    const int64_t seg = (int64_t)blockIdx.x * chunks;
    float p = 0.f;
    int32_t n = 0;
    if (slice < slices && x < e) {
        const uint32_t c0 = (uint32_t)((uint64_t)chunks * slice / slices), c1 = (uint32_t)((uint64_t)chunks * (slice + 1) / slices);
        const float *pp = ws_p + (seg + c0) * e + x;
        const int32_t *pc = ws_c + (seg + c0) * e + x;
        // the loads of a batch first, without a condition (beyond the run its last partial is read again), then the batch's sums in
        // chunk order, where what lies beyond the run is dropped
        for (uint32_t c = c0; c < c1; c += BALANCE_FINISH_AHEAD) {
            const int live = (int)(c1 - c < (uint32_t)BALANCE_FINISH_AHEAD ? c1 - c : (uint32_t)BALANCE_FINISH_AHEAD);   // >= 1
            float a[BALANCE_FINISH_AHEAD];
            int32_t m[BALANCE_FINISH_AHEAD];
#pragma unroll
            for (int u = 0; u < BALANCE_FINISH_AHEAD; ++u) {
                const int64_t at = (int64_t)(u < live ? u : live - 1) * e;
                a[u] = pp[at];
                m[u] = pc[at];
            }
#pragma unroll
            for (int u = 0; u < BALANCE_FINISH_AHEAD; ++u) {
                p = u < live ? p + a[u] : p;
                n += u < live ? m[u] : 0;
            }
            pp += (int64_t)BALANCE_FINISH_AHEAD * e;
            pc += (int64_t)BALANCE_FINISH_AHEAD * e;
        }
    }
    lds_p[threadIdx.x] = p;
    lds_c[threadIdx.x] = n;
    __syncthreads();
    if (slice == 0) {                              // (whole waves: et is a multiple of 64)
        float term = 0.f;
        if (x < e) {
            for (int s = 1; s < slices; ++s) {
                p = p + lds_p[s * et + x];
                n += lds_c[s * et + x];
            }
            psum[(int64_t)blockIdx.x * e + x] = p;
            counts[(int64_t)blockIdx.x * e + x] = n;
            term = (float)n * p;
        }
        term = wave_sum(term);
        if ((threadIdx.x & 63) == 0) lds_w[threadIdx.x >> 6] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = lds_w[0];
        for (int v = 1; v < et / 64; ++v) total = total + lds_w[v];
        loss[blockIdx.x] = coef * total;
    }
}

// One wave per token; q, ds and aux as include/dga_hip.h defines them, the sums over the experts V - 1 additions inside a lane and a
// wave_sum.  add_to may be dlogits itself: a lane reads its V elements before it writes them.
template <typename O, int V>
__global__ void __launch_bounds__(64 * ROUTER_WAVES) balance_backward_kernel(const float *dloss, const int32_t *counts, const float *scores,
                                                                            const float *add_to, void *dlogits, int64_t tokens,
                                                                            int64_t seq_len, int e, bool sigmoid, bool normalize, float coef,
                                                                            bool vec_in, bool vec_add, bool vec_out)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * ROUTER_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= tokens) return;   // (the whole wave)
    const int i0 = lane * V;
    const int64_t base = t * e, b = t / seq_len;

    float s[V], q[V];
    load_lane<float, V>(scores, base, i0, e, vec_in, 0.f, s);
    const float g = dloss[b] * coef;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        int32_t n = 0;
        if (i0 + c < e) n = counts[b * e + i0 + c];
        q[c] = g * (float)n;
    }
    if (normalize) {
        float sum = s[0];
#pragma unroll
        for (int c = 1; c < V; ++c) sum = sum + s[c];
        sum = wave_sum(sum);
        float dot = q[0] * (s[0] / sum);
#pragma unroll
        for (int c = 1; c < V; ++c) dot = dot + q[c] * (s[c] / sum);
        dot = wave_sum(dot);
#pragma unroll
        for (int c = 0; c < V; ++c) q[c] = (q[c] - dot) / sum;   // ds
    }
    float out[V];
    if (sigmoid) {
#pragma unroll
        for (int c = 0; c < V; ++c) out[c] = (q[c] * s[c]) * (1.f - s[c]);
    } else {
        float sdot = q[0] * s[0];
#pragma unroll
        for (int c = 1; c < V; ++c) sdot = sdot + q[c] * s[c];
        sdot = wave_sum(sdot);
#pragma unroll
        for (int c = 0; c < V; ++c) out[c] = s[c] * (q[c] - sdot);
    }
    if (add_to) {
        float a[V];
        load_lane<float, V>(add_to, base, i0, e, vec_add, 0.f, a);
#pragma unroll
        for (int c = 0; c < V; ++c) out[c] = a[c] + out[c];
    }
    store_lane<O, V>(dlogits, base, i0, e, vec_out, out);
}

// One workgroup, thread x = expert x: n_x over the segments, the total over the experts through LDS (integers: any order), the sign of
// total - e n_x, one product and one addition.
__global__ void __launch_bounds__(BIAS_THREADS) bias_update_kernel(float *bias, const int32_t *counts, int64_t segments, int e, float rate)
{
    __shared__ long long lds_n[BIAS_THREADS];
    const int x = threadIdx.x;
    long long n = 0;
    if (x < e)
        for (int64_t b = 0; b < segments; ++b) n += counts[b * e + x];
    lds_n[x] = n;
    __syncthreads();
    for (int half = BIAS_THREADS / 2; half > 0; half >>= 1) {
        if (x < half) lds_n[x] += lds_n[x + half];
        __syncthreads();
    }
    const long long d = lds_n[0] - (long long)e * n;
    if (x < e) bias[x] = bias[x] + rate * (float)(d > 0 ? 1 : d < 0 ? -1 : 0);
}

inline int balance_shape(int64_t tokens, int64_t e, int64_t k, int64_t seq_len)
{
    if (tokens < 0 || e < 0 || k < 1 || k > e || seq_len < 1 || tokens % seq_len != 0) return DGA_E_SHAPE;
    return DGA_OK;
}

}  // namespace dga

extern "C" size_t dga_router_balance_loss_workspace_bytes(int64_t tokens, int64_t experts, int64_t seq_len)
{
    using namespace dga;
    if (tokens <= 0 || experts <= 0 || experts > DGA_ROUTER_MAX_EXPERTS || seq_len < 1 || tokens % seq_len != 0) return 0;
    const int64_t partials = (tokens / seq_len) * balance_chunks(tokens, seq_len);   // (<= tokens: no overflow below)
    if (partials > 0x7FFFFFFFll) return 0;
    return static_cast<size_t>(partials) * static_cast<size_t>(experts) * 8;
}

extern "C" int dga_router_balance_loss(const float *scores, const int32_t *ids, int64_t tokens, int64_t experts, int64_t k, int64_t seq_len,
                                       int flags, float coef, float *loss, int32_t *counts, float *psum, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    using namespace dga;
    if (int rc = balance_shape(tokens, experts, k, seq_len)) return rc;
    if (tokens == 0) return DGA_OK;
    if (!scores || !ids || !loss || !counts || !psum || !workspace) return DGA_E_NULL;
    if (experts > DGA_ROUTER_MAX_EXPERTS || k > DGA_ROUTER_MAX_TOPK || (flags & ~DGA_ROUTER_BALANCE_NORMALIZE)) return DGA_E_RANGE;
    const int64_t segments = tokens / seq_len, chunks = balance_chunks(tokens, seq_len);
    if (segments * chunks > 0x7FFFFFFFll) return DGA_E_RANGE;
    const size_t half = static_cast<size_t>(segments * chunks) * static_cast<size_t>(experts) * 4;
    if (workspace_bytes < 2 * half || reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return DGA_E_RANGE;
    float *ws_p = static_cast<float *>(workspace);
    int32_t *ws_c = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + half);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = dispatch_lane_width(experts, [&](auto width) -> int {
        constexpr int V = decltype(width)::value;
        hipLaunchKernelGGL((balance_partial_kernel<V>), dim3(static_cast<unsigned>(segments * chunks)), dim3(64 * ROUTER_WAVES), 0, s, scores,
                           ids, ws_p, ws_c, seq_len, static_cast<int>(balance_chunk_tokens(tokens)), static_cast<uint32_t>(chunks),
                           static_cast<int>(experts), static_cast<int>(k), (flags & DGA_ROUTER_BALANCE_NORMALIZE) != 0,
                           router_vec(scores, experts, V, 4));
        return record_hip(hipGetLastError());
    });
    if (rc) return rc;
    hipLaunchKernelGGL(balance_finish_kernel, dim3(static_cast<unsigned>(segments)), dim3(BALANCE_FINISH_THREADS), 0, s, ws_p, ws_c, loss,
                       counts, psum, static_cast<uint32_t>(chunks), static_cast<int>(experts), coef);
    return record_hip(hipGetLastError());
}

extern "C" int dga_router_balance_loss_backward(const float *dloss, const int32_t *counts, const float *scores, int64_t tokens, int64_t experts,
                                                int64_t k, int64_t seq_len, int score_func, int flags, float coef, const float *add_to,
                                                void *dlogits, int dlogits_dtype, void *stream)
{
    using namespace dga;
    if (int rc = balance_shape(tokens, experts, k, seq_len)) return rc;
    if (tokens == 0) return DGA_OK;
    if (!dloss || !counts || !scores || !dlogits) return DGA_E_NULL;
    return dispatch_dtype(dlogits_dtype, [&](auto tag) -> int {
        using O = decltype(tag);
        if (experts > DGA_ROUTER_MAX_EXPERTS || k > DGA_ROUTER_MAX_TOPK) return DGA_E_RANGE;
        if ((score_func != DGA_ROUTER_SOFTMAX && score_func != DGA_ROUTER_SIGMOID) || (flags & ~DGA_ROUTER_BALANCE_NORMALIZE)) return DGA_E_RANGE;
        const int64_t groups = (tokens + ROUTER_WAVES - 1) / ROUTER_WAVES;
        if (groups > 0x7FFFFFFFll) return DGA_E_RANGE;
        return dispatch_lane_width(experts, [&](auto width) -> int {
            constexpr int V = decltype(width)::value;
            hipLaunchKernelGGL((balance_backward_kernel<O, V>), dim3(static_cast<unsigned>(groups)), dim3(64 * ROUTER_WAVES), 0,
                               static_cast<hipStream_t>(stream), dloss, counts, scores, add_to, dlogits, tokens, seq_len,
                               static_cast<int>(experts), score_func == DGA_ROUTER_SIGMOID, (flags & DGA_ROUTER_BALANCE_NORMALIZE) != 0, coef,
                               router_vec(scores, experts, V, 4), router_vec(add_to, experts, V, 4),
                               router_vec(dlogits, experts, V, Elem<O>::kBytes));
            return record_hip(hipGetLastError());
        });
    });
}

extern "C" int dga_router_bias_update(float *bias, const int32_t *counts, int64_t segments, int64_t experts, float rate, void *stream)
{
    using namespace dga;
    if (segments < 0 || experts < 0) return DGA_E_SHAPE;
    if (segments == 0 || experts == 0) return DGA_OK;
    if (!bias || !counts) return DGA_E_NULL;
    if (experts > DGA_ROUTER_MAX_EXPERTS) return DGA_E_RANGE;
    hipLaunchKernelGGL(bias_update_kernel, dim3(1), dim3(BIAS_THREADS), 0, static_cast<hipStream_t>(stream), bias, counts, segments,
                       static_cast<int>(experts), rate);
    return record_hip(hipGetLastError());
}
