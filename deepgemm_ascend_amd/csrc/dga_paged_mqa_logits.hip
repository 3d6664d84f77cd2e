// The decode half of the lightning indexer's scoring (DeepSeek sparse attention): upstream DeepGEMM's fp8_paged_mqa_logits.
//   dga_fp8_paged_mqa_logits   q [B, next_n, H, 128] e4m3, a paged key cache, weights [B next_n, H], context_lens int32 [B],
//                              block_tables int32 [B, max_blocks] -> logits fp32 [B next_n, N]
//     ctx_i       = min(max(context_lens[i], 0), N, 64 max_blocks)
//     hi_r        = max(ctx_i - next_n + j + 1, 0)                                 row r = i next_n + j
//     key n of sequence i = key n % 64 of block block_tables[i, n / 64]
//     logits[r,n] = kscale * sum_h weights[r,h] * relu(sum_d q[i,j,h,d] k[d])      for n < hi_r,   -inf for hi_r <= n < N
// A block (page) of the cache is 8448 bytes: the e4m3 codes of its 64 keys, key-major, then their 64 fp32 scales.  A page of 64 keys is
// one wave's key set in mqa_logits_kernel, and the arithmetic is that kernel's (dga_mqa_device.hpp): on the gathered operands the result
// is fp8_mqa_logits' bit for bit.  What is new is the data movement -- q resident, the keys streamed.
//
// Tile: a workgroup of four waves owns one sequence and a chunk of PMQA_CHUNK = 512 keys = 8 pages; the grid is ceil(N / 512) x B, sequences fastest, fixed
// by the shapes, so a captured graph replays under any lengths.  Nothing is read from another workgroup.  A workgroup whose chunk starts at or
// beyond 64 ceil(ctx_i / 64) stores its -inf (clean_logits) or nothing and reads neither q nor weights nor a table entry nor a key.
// Otherwise the sequence's next_n x H x 128 codes are read once per workgroup, 8 bytes a lane, into an LDS image in A-fragment order --
// fragment (token j, head tile ht, k step s) is 512 contiguous bytes, lane l's 8 codes at byte 8 l, as in mqa_logits_kernel -- followed by
// the next_n x H weights; one barrier.  Wave w then walks pages 8 c + w and 8 c + w + 4 of chunk c.  Per page: one table entry (a scalar
// load: the address is wave-uniform), 16 eight-byte loads a lane in B-fragment order (lane l: key 16 nt + (l & 15), bytes
// 32 s + 8 (l >> 4) ..) and one scale a lane at byte 8192 + 4 l; the fragments are converted once (64 VGPRs) and the wave's next page is
// requested before this one is multiplied.  Per token and head tile: four A fragments from LDS, converted, 16 MFMAs, the fold; then the
// exchange, the scale, and one dword store a lane, 256 contiguous bytes a wave.  The LDS image keeps the codes, not bf16: a wave reads
// 8 KB of it per (page, token) at H = 64 where bf16 would be 16 KB, as much LDS time as the MFMAs take.
// A table entry is read only for pages below ceil(ctx_i / 64); one outside [0, num_blocks) dereferences nothing and its page's columns are
// -inf.  No byte outside a named block's 8448 is read, no row of q / weights at or beyond B next_n, and with clean_logits == 0 no byte of
// logits at or beyond column 64 ceil(ctx_i / 64) is written.  Every written element has one writer; no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"
#include "dga_mqa_device.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int PMQA_THREADS = 256;
constexpr int PMQA_CHUNK = DGA_PAGED_MQA_LOGITS_CHUNK_N;     // keys of a workgroup
constexpr int PMQA_PAGE = DGA_PAGED_MQA_LOGITS_BLOCK_KV;     // keys of a block of the cache = of one wave's step
constexpr int PMQA_D = DGA_MQA_LOGITS_HEAD_DIM;
constexpr int PMQA_SCALES = PMQA_PAGE * PMQA_D;              // byte offset of a block's scales
static_assert(PMQA_PAGE == 64 && PMQA_D == 128 && PMQA_CHUNK % 256 == 0 && PMQA_SCALES + 4 * PMQA_PAGE == DGA_PAGED_MQA_LOGITS_BLOCK_BYTES,
              "the kernel's geometry");

template <int H, int NN>
__global__ void __launch_bounds__(PMQA_THREADS) paged_mqa_logits_kernel(const uint8_t *__restrict__ q, const uint8_t *__restrict__ kv,
                                                                        const float *__restrict__ weights, const int32_t *__restrict__ context_lens,
                                                                        const int32_t *__restrict__ block_tables, float *__restrict__ out,
                                                                        int64_t num_blocks, int64_t block_stride, int64_t max_blocks, int n_n,
                                                                        int batch, int clean)
{
    constexpr int HT = H / 16;        // head tiles
    constexpr int FR = NN * HT * 4;   // A fragments of the sequence: (token, head tile, k step), 512 bytes each
    constexpr int FPW = FR / 4;       // ... staged by one wave
    __shared__ mqa_v2i image[FR * 64];
    __shared__ mqa_v4f wimg[NN * H / 4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, c = lane & 15;
    // sequences fastest: the workgroups of one chunk index are neighbours in the grid, so those that score -- the low chunk indices -- are
    // dispatched first and side by side.  Chunks fastest, the scoring workgroups of a short context recur with the period of the chunk
    // count between runs of idle ones, and the round-robin placement put them all on a quarter of the CUs (measured: B = 64, contexts of
    // 4096 under N = 65536 took 42 us against 12 us under N = 4096).
    const int64_t seq = blockIdx.x % batch;
    const int chunk = blockIdx.x / batch;
    const float ninf = -__builtin_inff();

    // the sequence's length, clamped to [0, min(N, 64 max_blocks)]
    int ctx = context_lens[seq];
    ctx = ctx < 0 ? 0 : (ctx > n_n ? n_n : ctx);
    if (ctx > 64 * max_blocks) ctx = (int)(64 * max_blocks);
    const int pages = (ctx + PMQA_PAGE - 1) / PMQA_PAGE;                   // pages with a key in range: the table entries that are read
    const int p0 = chunk * (PMQA_CHUNK / PMQA_PAGE);                       // (n_n <= DGA_PAGED_MQA_LOGITS_MAX_N: no overflow in 64 (p0 + 8))
    const int pend_all = (n_n + PMQA_PAGE - 1) / PMQA_PAGE;                // pages with a column of the output
    const int pend = p0 + PMQA_CHUNK / PMQA_PAGE < pend_all ? p0 + PMQA_CHUNK / PMQA_PAGE : pend_all;
    const int pact = pend < pages ? pend : pages;                          // the chunk's pages [p0, pact) are scored
    float *orow = out + seq * NN * (int64_t)n_n;

    // pages beyond the context: -inf or nothing (whole waves, no operand read)
    if (clean) {
        const int first = p0 > pact ? p0 : pact;
        for (int p = first + ((wave - first) & 3); p < pend; p += 4) {     // wave w: the pages p >= first with p % 4 == w, as below
            const int col = p * PMQA_PAGE + lane;
            if (col < n_n) {
#pragma unroll
                for (int j = 0; j < NN; ++j) orow[(int64_t)j * n_n + col] = ninf;
            }
        }
    }
    if (p0 >= pact) return;                                                // (the whole workgroup alike)

    const int32_t *table = block_tables + seq * max_blocks;
    mqa_v2i raw[4][4];
    float raw_scale = 0.f;
    bool raw_ok = false;
    auto fetch = [&](int p) {                                              // p < pact <= pages: the entry is one that may be read
        const int64_t blk = __builtin_amdgcn_readfirstlane(table[p]);
        raw_ok = blk >= 0 && blk < num_blocks;
        if (raw_ok) {
            const uint8_t *b = kv + blk * block_stride;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) raw[nt][s] = *(const mqa_v2i *)(b + (16 * nt + c) * PMQA_D + 32 * s + 8 * g);
            }
            raw_scale = *(const float *)(b + PMQA_SCALES + 4 * lane);
        }
    };

    // q and weights of the sequence, once per workgroup; the wave's first page is requested behind them and lands during the staging
    const uint8_t *qs = q + seq * (NN * H * PMQA_D);
    mqa_v2i qr[FPW];
#pragma unroll
    for (int j = 0; j < FPW; ++j) {
        const int f = wave * FPW + j;                                      // = (token * HT + ht) * 4 + s
        qr[j] = *(const mqa_v2i *)(qs + ((f >> 2) * 16 + c) * PMQA_D + 32 * (f & 3) + 8 * g);
    }
    mqa_v4f wq = {0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < NN * H / 4) wq = *(const mqa_v4f *)(weights + seq * (NN * H) + 4 * threadIdx.x);
    int p = p0 + wave;
    if (p < pact) fetch(p);
#pragma unroll
    for (int j = 0; j < FPW; ++j) image[(wave * FPW + j) * 64 + lane] = qr[j];
    if (threadIdx.x < NN * H / 4) wimg[threadIdx.x] = wq;
    __syncthreads();

    for (; p < pact; p += 4) {
        const bool ok = raw_ok;
        const float scale = raw_scale;
        mqa_v4i bf[4][4];
        if (ok) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) bf[nt][s] = mqa_cvt8(raw[nt][s]);
            }
        }
        if (p + 4 < pact) fetch(p + 4);                                    // in flight while this page is multiplied
        const int col = p * PMQA_PAGE + lane;
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            const int hi = ctx - NN + j + 1;                               // (<= 0: an empty row)
            float val = ninf;
            if (ok && p * PMQA_PAGE < hi) {                                // wave-uniform
                float pp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ht = 0; ht < HT; ++ht) {
                    mqa_v4i af[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) af[s] = mqa_cvt8(image[((j * HT + ht) * 4 + s) * 64 + lane]);
                    mqa_head_tile(af, bf, wimg[(j * HT + ht) * 4 + g], pp);
                }
                const float v = mqa_exchange(pp, g);
                if (col < hi) val = v * scale;
            }
            if (col < n_n) orow[(int64_t)j * n_n + col] = val;
        }
    }
}

}  // namespace dga

extern "C" int dga_fp8_paged_mqa_logits(const void *q, const void *kv_cache, const float *weights, const int32_t *context_lens,
                                        const int32_t *block_tables, int64_t batch, int next_n, int heads, int head_dim, int64_t num_blocks,
                                        int64_t block_stride, int64_t max_blocks, int64_t max_model_len, int clean_logits, float *logits,
                                        void *stream)
{
    using namespace dga;
    if (batch < 0 || (next_n != 1 && next_n != 2) || (heads != 32 && heads != 64) || head_dim != PMQA_D || num_blocks < 1 ||
        block_stride < DGA_PAGED_MQA_LOGITS_BLOCK_BYTES || max_blocks < 1 || max_model_len < 1)
        return DGA_E_SHAPE;
    if (batch == 0) return DGA_OK;
    if (!q || !kv_cache || !weights || !context_lens || !block_tables || !logits) return DGA_E_NULL;
    // a lane reads 8 codes and four weights at once; a block's codes and scales sit at multiples of 8 and 4 from its start
    if (reinterpret_cast<uintptr_t>(q) % 8 || reinterpret_cast<uintptr_t>(kv_cache) % 16 || block_stride % 16 ||
        reinterpret_cast<uintptr_t>(weights) % 16 || reinterpret_cast<uintptr_t>(context_lens) % 4 ||
        reinterpret_cast<uintptr_t>(block_tables) % 4 || reinterpret_cast<uintptr_t>(logits) % 4)
        return DGA_E_ALIGN;
    if (max_model_len > DGA_PAGED_MQA_LOGITS_MAX_N || num_blocks > 0x7FFFFFFFFFFFFFFFll / block_stride ||
        max_blocks > 0x7FFFFFFFFFFFFFFFll / 64 || batch > 0x7FFFFFFFFFFFFFFFll / max_blocks ||
        batch > 0x7FFFFFFFFFFFFFFFll / (next_n * max_model_len * 4))
        return DGA_E_RANGE;
    const int64_t chunks = (max_model_len + PMQA_CHUNK - 1) / PMQA_CHUNK;
    if (batch > 0x7FFFFFFFll / chunks) return DGA_E_RANGE;
    const dim3 grid(static_cast<unsigned>(batch * chunks)), block(PMQA_THREADS);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<const uint8_t *>(q), static_cast<const uint8_t *>(kv_cache), weights,
                           context_lens, block_tables, logits, num_blocks, block_stride, max_blocks, static_cast<int>(max_model_len),
                           static_cast<int>(batch), clean_logits != 0 ? 1 : 0);
    };
    if (heads == 64 && next_n == 2) launch(paged_mqa_logits_kernel<64, 2>);
    else if (heads == 64) launch(paged_mqa_logits_kernel<64, 1>);
    else if (next_n == 2) launch(paged_mqa_logits_kernel<32, 2>);
    else launch(paged_mqa_logits_kernel<32, 1>);
    return record_hip(hipGetLastError());
}
