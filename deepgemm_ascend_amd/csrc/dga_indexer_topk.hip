// The selecting half of the lightning indexer (DeepSeek sparse attention): what consumes the logits of dga_fp8_mqa_logits and
// dga_fp8_paged_mqa_logits.
//   dga_indexer_topk   logits fp32 [m, n] (rows `stride` elements apart) -> out int32 [m, k]
//     [lo, hi) of row r   row_starts / row_ends:  lo = min(max(ks[r], 0), n), hi = min(max(ke[r], 0), n)
//                         context_lens, next_n:   lo = 0, hi = max(min(max(lens[r / next_n], 0), n) - next_n + r % next_n + 1, 0)
//                         neither:                lo = 0, hi = n
//     key(x)              bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000), every NaN 0xFFFFFFFF
//     column a precedes b iff key is greater, or equal and a < b;  c = min(hi - lo, k)
//     out[r, 0 .. c)      the first c columns of [lo, hi) in that order, ascending by column, mapped (the column, the column - lo, or
//                         the slot block_tables[r / next_n, col / page] * page + col % page, -1 for a bad or missing entry)
//     out[r, c .. k)      -1
// One workgroup of 16 waves owns one row and waits for nobody: no flags in global memory, no spin loops, no floating-point atomics.  The LDS
// integer atomics only count, and a count does not depend on the order of arrival.
// A row with hi - lo <= k reads no logits.  Any other row is walked in 16-byte groups aligned in memory (whatever the row's base, lo and
// the stride: the first group starts up to three columns in front of lo); a group wholly inside [lo, hi) is one dwordx4 load, the at most
// two ragged ones are dword loads of their in-range columns, so no byte outside [lo, hi) is read.  A radix select on key, most significant
// digit first (11, 11 and 10 bits): a pass histograms the digit of the keys that share the prefix found so far, a suffix scan finds the bin
// holding the want-th largest, and want and the prefix descend into it.  As soon as a bin's population fits the LDS candidate buffer
// (DGA_INDEXER_TOPK_CANDIDATES keys) one more walk gathers its keys there and the remaining digits are histogrammed from LDS; until then
// the passes walk the row again, so a row of n equal values costs three counting walks and is still exact.  An LDS add is the costly step
// of a counting walk (the probe builds put it at half the kernel), so most rows never take one: the top digits of 4096 columns spread
// evenly over the row give a guess at a key with between k and DGA_INDEXER_TOPK_CANDIDATES keys at or above it, one walk gathers the keys at
// or above the guess, and when their number lies in that span all three digits are histogrammed from LDS; when it does not the counting
// walks run as described and nothing depends on the guess.  That leaves the threshold key T
// and the number t of keys equal to T to take.  The last walk goes over [lo, hi) in chunks of 4096 columns, four consecutive columns a lane:
// a lane's flags are key > T, or key == T and its rank among the equal keys so far < t (the rank is one more scan, skipped when every
// equal key is taken); ballots and popcounts give the offsets inside a wave, sixteen wave totals in LDS those across the waves, a running
// base those across the chunks.  The output is therefore in column order and every element has exactly one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"

namespace dga {

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_BINS = 2048;                              // 11 bits a digit (the last digit has 10)
constexpr int TOPK_CAND = DGA_INDEXER_TOPK_CANDIDATES;
constexpr int TOPK_CHUNK = TOPK_THREADS * 4;                 // columns of one step of a walk
static_assert(TOPK_BINS == 2 * TOPK_THREADS && TOPK_WAVES == 16 && DGA_INDEXER_TOPK_MAX_K <= TOPK_CHUNK, "the kernel's geometry");

enum { TOPK_MAP_COLUMN = 0, TOPK_MAP_RELATIVE = 1, TOPK_MAP_SLOT = 2 };

__device__ __forceinline__ uint32_t topk_key(uint32_t b)
{
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__global__ void __launch_bounds__(TOPK_THREADS) indexer_topk_kernel(const uint32_t *__restrict__ logits, int64_t stride, int n, int k,
                                                                    const int32_t *__restrict__ ks, const int32_t *__restrict__ ke,
                                                                    const int32_t *__restrict__ lens, int next_n, int mode,
                                                                    const int32_t *__restrict__ tables, int64_t max_blocks, int page,
                                                                    int num_blocks, int32_t *__restrict__ out)
{
    __shared__ uint32_t hist[TOPK_BINS];
    __shared__ uint32_t cand[TOPK_CAND];
    __shared__ uint32_t wtot[2][TOPK_WAVES];                 // the wave totals of a scan, two buffers used in turn
    __shared__ uint32_t found[3];                            // the bin, what is wanted inside it, its population
    __shared__ uint32_t ncand;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t below = (1ull << lane) - 1;               // the lanes in front of this one
    const int64_t r = blockIdx.x;

    int lo = 0, hi = n;
    const int32_t *table = nullptr;
    if (ks) {
        const int s = ks[r], e = ke[r];
        lo = s < 0 ? 0 : (s > n ? n : s);
        hi = e < 0 ? 0 : (e > n ? n : e);
    } else if (lens) {
        const int64_t seq = r / next_n;
        int ctx = lens[seq];
        ctx = ctx < 0 ? 0 : (ctx > n ? n : ctx);
        hi = ctx - next_n + (int)(r % next_n) + 1;
        if (hi < 0) hi = 0;
        if (mode == TOPK_MAP_SLOT) table = tables + seq * max_blocks;
    }
    const int len = hi > lo ? hi - lo : 0;
    int32_t *orow = out + r * k;

    auto mapped = [&](int col) -> int32_t {
        if (mode == TOPK_MAP_COLUMN) return col;
        if (mode == TOPK_MAP_RELATIVE) return col - lo;
        const int pg = col / page;
        if (pg >= max_blocks) return -1;
        const int32_t blk = table[pg];                       // (read for selected columns only)
        if (blk < 0 || blk >= num_blocks) return -1;
        return blk * page + (col - pg * page);               // (num_blocks * page < 2^31: checked on the host)
    };

    if (len <= k) {                                          // everything in range is selected: no logits read
        for (int i = tid; i < k; i += TOPK_THREADS) orow[i] = i < len ? mapped(lo + i) : -1;
        return;
    }

    // the walk: 16-byte groups aligned in memory, group g = columns first + 4 g ..; first in (lo - 4, lo]
    const uint32_t *row = logits + r * stride;
    const int off = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int first = ((lo + off) & ~3) - off;
    const int chunks = (hi - first + TOPK_CHUNK - 1) / TOPK_CHUNK;
    // the bits of columns col .. col + 3 and which of them are in range (a group beyond hi: none, and no load)
    auto fetch = [&](int col, uint4 &v) -> uint32_t {
        v = uint4{0, 0, 0, 0};
        if (col >= lo && col + 4 <= hi) {
            v = *reinterpret_cast<const uint4 *>(row + col);
            return 15u;
        }
        uint32_t valid = 0;
        if (col + 4 > lo && col < hi) {                                      // a ragged end: at most two groups of a row
            if (col >= lo) v.x = row[col], valid |= 1u;
            if (col + 1 >= lo && col + 1 < hi) v.y = row[col + 1], valid |= 2u;
            if (col + 2 >= lo && col + 2 < hi) v.z = row[col + 2], valid |= 4u;
            if (col + 3 < hi) v.w = row[col + 3], valid |= 8u;
        }
        return valid;
    };
    auto keys_of = [](const uint4 &v, uint32_t key[4]) {
        key[0] = topk_key(v.x), key[1] = topk_key(v.y), key[2] = topk_key(v.z), key[3] = topk_key(v.w);
    };
    // body(col, key, valid) over every group of the row, whole waves alike
    auto walk = [&](auto body) {
        for (int ch = 0; ch < chunks; ++ch) {
            const int col = first + 4 * (ch * TOPK_THREADS + tid);
            uint4 v;
            uint32_t key[4];
            const uint32_t valid = fetch(col, v);
            keys_of(v, key);
            body(col, key, valid);
        }
    };
    // one more of `digit` from every lane with p set (whole waves call this): a wave whose lanes agree adds once
    auto count = [&](bool p, uint32_t digit) {
        const uint64_t act = __ballot(p);
        if (act == 0) return;
        const int leader = __builtin_ctzll(act);
        const uint32_t d0 = __builtin_amdgcn_readlane(digit, leader);
        if (__ballot(p && digit == d0) == act) {
            if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
        } else if (p) {
            atomicAdd(&hist[digit], 1u);
        }
    };

    // the bin b with above(b) < wanted <= above(b) + hist[b], above(b) = the population of the bins beyond b: a suffix scan, two bins a
    // thread; returns b, leaves in `rest` what is wanted inside it and in `inside` its population, and empties the candidate counter
    auto find_bin = [&](uint32_t wanted, uint32_t &rest, uint32_t &inside) -> uint32_t {
        __syncthreads();
        const uint32_t h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
        uint32_t v = h0 + h1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_down(v, d);
            if (lane + d < 64) v += u;
        }
        if (lane == 0) wtot[0][wave] = v;
        if (tid == 0) ncand = 0;
        __syncthreads();
        uint32_t above1 = v - (h0 + h1);
        for (int w = wave + 1; w < TOPK_WAVES; ++w) above1 += wtot[0][w];
        const uint32_t above0 = above1 + h1;
        if (above1 < wanted && wanted <= above1 + h1) found[0] = 2 * tid + 1, found[1] = wanted - above1, found[2] = h1;
        else if (above0 < wanted && wanted <= above0 + h0) found[0] = 2 * tid, found[1] = wanted - above0, found[2] = h0;
        __syncthreads();
        rest = found[1];
        inside = found[2];
        return found[0];
    };
    // the keys with pred(key) into cand, in any order (only counts are taken from them); returns how many there are in the row, of which
    // the first TOPK_CAND to arrive are kept
    auto gather = [&](auto pred) -> uint32_t {
        walk([&](int, const uint32_t key[4], uint32_t valid) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool p = ((valid >> j) & 1) && pred(key[j]);
                const uint64_t act = __ballot(p);
                if (act == 0) continue;
                const int leader = __builtin_ctzll(act);
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&ncand, (uint32_t)__popcll(act));
                base = __builtin_amdgcn_readlane(base, leader);
                const uint32_t at = base + (uint32_t)__popcll(act & below);
                if (p && at < (uint32_t)TOPK_CAND) cand[at] = key[j];
            }
        });
        __syncthreads();
        return ncand;
    };
    auto clear_hist = [&]() {
        hist[2 * tid] = 0, hist[2 * tid + 1] = 0;
        __syncthreads();
    };

    uint32_t prefix = 0, fixed = 0, want = (uint32_t)k, population = 0;     // fixed: the bits of prefix that are decided
    bool in_lds = false;
    uint32_t held = 0;                                                      // keys in cand

    // A shortcut that most rows take.  The top digits of 4096 columns spread evenly over the row are counted, and the lower edge of the bin
    // holding the sample's aim-th largest, aim about 2 k 4096 / len, is a guess `low` at a key with between k and TOPK_CAND keys of the
    // row at or above it; one walk gathers exactly those.  When their number is in that span the k largest of the row are the k largest
    // of the candidates and the whole selection runs inside LDS; when it is not -- equal keys, a misleading sample -- nothing is lost and
    // the counting walks below run.  A row that fits the buffer is gathered whole.
    {
        uint32_t low = 0;
        if (len > TOPK_CAND) {
            clear_hist();
            const int groups = (hi - first + 3) >> 2;
            const int col = first + 4 * (int)(((int64_t)tid * groups) >> 10);
            uint4 v;
            uint32_t key[4];
            const uint32_t valid = fetch(col, v);
            keys_of(v, key);
#pragma unroll
            for (int j = 0; j < 4; ++j) count((valid >> j) & 1, key[j] >> 21);
            uint32_t aim = (uint32_t)((2ll * k * TOPK_CHUNK + len - 1) / len);   // (len > TOPK_CAND: below k, and the sample holds more)
            if (aim < 16) aim = 16;
            uint32_t rest, inside;
            low = find_bin(aim, rest, inside) << 21;
        } else {
            if (tid == 0) ncand = 0;
            __syncthreads();
        }
        const uint32_t total = gather([&](uint32_t key) { return key >= low; });
        if (total >= (uint32_t)k && total <= (uint32_t)TOPK_CAND) held = total, in_lds = true;
    }

#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const uint32_t dmask = pass == 2 ? 0x3FFu : 0x7FFu;
        clear_hist();
        if (in_lds) {
            for (uint32_t base = 0; base < held; base += TOPK_THREADS) {
                const uint32_t i = base + tid;
                const uint32_t key = i < held ? cand[i] : 0;
                count(i < held && ((key ^ prefix) & fixed) == 0, (key >> shift) & dmask);
            }
        } else {
            walk([&](int, const uint32_t key[4], uint32_t valid) {
#pragma unroll
                for (int j = 0; j < 4; ++j) count(((valid >> j) & 1) && ((key[j] ^ prefix) & fixed) == 0, (key[j] >> shift) & dmask);
            });
        }
        prefix |= find_bin(want, want, population) << shift;
        fixed |= dmask << shift;
        // the first bin that fits the candidate buffer is gathered
        if (!in_lds && pass < 2 && population <= (uint32_t)TOPK_CAND) {
            const uint32_t total = gather([&](uint32_t key) { return ((key ^ prefix) & fixed) == 0; });
            held = total < (uint32_t)TOPK_CAND ? total : (uint32_t)TOPK_CAND;
            in_lds = true;
        }
    }
    const uint32_t T = prefix, t = want;
    const bool ranked = population != t;                      // some keys equal to T stay out: the equal ones need their rank

    // exclusive scan of up to four flags a lane over the workgroup, in column order; total: their number
    int turn = 0;
    auto scan4 = [&](uint32_t flags, uint32_t &total) -> uint32_t {
        uint32_t pre = 0, mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t b = __ballot((flags >> j) & 1);
            pre += (uint32_t)__popcll(b & below);
            mine += (uint32_t)__popcll(b);
        }
        uint32_t *w = wtot[turn];
        turn ^= 1;
        if (lane == 0) w[wave] = mine;
        __syncthreads();
        // lanes 0 .. 15 hold the sixteen totals; an inclusive prefix along that DPP row (row_shr 1, 2, 4, 8; a lane without a source adds 0)
        uint32_t v = w[lane & (TOPK_WAVES - 1)];
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
        total = __builtin_amdgcn_readlane(v, TOPK_WAVES - 1);
        if (wave > 0) pre += __builtin_amdgcn_readlane(v, wave - 1);
        return pre;
    };

    uint32_t written = 0, equals = 0;
    walk([&](int col, const uint32_t key[4], uint32_t valid) {
        if (written >= (uint32_t)k) return;                   // (the whole workgroup alike: nothing is left to select)
        uint32_t gt = 0, eq = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((valid >> j) & 1) gt |= (uint32_t)(key[j] > T) << j, eq |= (uint32_t)(key[j] == T) << j;
        }
        uint32_t take = gt | eq;
        if (ranked) {
            uint32_t total;
            uint32_t rank = equals + scan4(eq, total);
            equals += total;
            take = gt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((eq >> j) & 1) {
                    if (rank < t) take |= 1u << j;
                    ++rank;
                }
            }
        }
        uint32_t total;
        uint32_t at = written + scan4(take, total);
        written += total;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((take >> j) & 1) {
                if (at < (uint32_t)k) orow[at] = mapped(col + j);
                ++at;
            }
        }
    });
}

}  // namespace dga

extern "C" int dga_indexer_topk(const float *logits, int64_t m, int64_t n, int64_t stride, int k, const int32_t *row_starts,
                                const int32_t *row_ends, const int32_t *context_lens, int next_n, int relative, const int32_t *block_tables,
                                int64_t max_blocks, int page_size, int64_t num_blocks, int32_t *out, void *stream)
{
    using namespace dga;
    if (m < 0 || n < 1 || stride < n) return DGA_E_SHAPE;
    if (m == 0) return DGA_OK;
    if (!logits || !out || (row_starts == nullptr) != (row_ends == nullptr)) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(logits) % 4 || reinterpret_cast<uintptr_t>(out) % 4 || reinterpret_cast<uintptr_t>(row_starts) % 4 ||
        reinterpret_cast<uintptr_t>(row_ends) % 4 || reinterpret_cast<uintptr_t>(context_lens) % 4 ||
        reinterpret_cast<uintptr_t>(block_tables) % 4)
        return DGA_E_ALIGN;
    if (k < 1 || k > DGA_INDEXER_TOPK_MAX_K || n > DGA_INDEXER_TOPK_MAX_N || m > 0x7FFFFFFFll) return DGA_E_RANGE;
    // the exclusive options: ranges or lengths, relative or slots, slots only beside lengths
    if ((row_starts && context_lens) || (relative && block_tables) || (block_tables && !context_lens)) return DGA_E_RANGE;
    if (context_lens) {
        if (next_n != 1 && next_n != 2) return DGA_E_RANGE;
        if (m % next_n) return DGA_E_SHAPE;
    }
    if (stride > 0x7FFFFFFFFFFFFFFFll / 4 / m) return DGA_E_RANGE;          // (k <= 2048 and m < 2^31: m k fits)
    if (block_tables) {
        if (page_size < 1 || max_blocks < 1 || num_blocks < 1) return DGA_E_RANGE;
        if (num_blocks > 0x7FFFFFFFll / page_size || max_blocks > 0x7FFFFFFFFFFFFFFFll / 4 / m) return DGA_E_RANGE;
    }
    const int mode = block_tables ? TOPK_MAP_SLOT : (relative ? TOPK_MAP_RELATIVE : TOPK_MAP_COLUMN);
    hipLaunchKernelGGL(indexer_topk_kernel, dim3(static_cast<unsigned>(m)), dim3(TOPK_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t *>(logits), stride, static_cast<int>(n), k, row_starts, row_ends, context_lens,
                       context_lens ? next_n : 1, mode, block_tables, max_blocks, block_tables ? page_size : 1,
                       static_cast<int>(block_tables ? num_blocks : 1), out);
    return record_hip(hipGetLastError());
}
