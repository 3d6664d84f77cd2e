// What the lightning indexer selects for: sparse MLA attention (DeepSeek sparse attention, forward) over dga_indexer_topk's indices.
//   dga_sparse_mla_fwd   q bf16 [m, heads, 576], kv bf16 [s, 576] (rows kv_stride elements apart), indices int32 [m, topk] (rows
//                        idx_stride apart), offsets int32 [m] or null -> out bf16 [m, heads, 512], lse fp32 [m, heads]
//     row of position j     r_j = indices[t, j] + (offsets ? offsets[t] : 0), valid iff indices[t, j] >= 0 and 0 <= r_j < s
//     s_j                   sm_scale sum_d q[t, h, d] kv[r_j, d] over the valid positions;  lse = ln sum_j exp(s_j)
//     out[t, h, :]          sum_j exp(s_j - lse) kv[r_j, :512];  no valid position: out = +0, lse = -inf
// One workgroup of four waves owns one token and a block of up to 64 heads; wave w owns heads 16 w .. 16 w + 15 of the block and all 512
// value columns of them (128 fp32 accumulators a lane).  The block's slice of q goes to LDS once (64 rows of 1184 bytes).  The selected
// rows are gathered in tiles of 32 positions by 16-byte loads (eight threads a row) into registers while the tile before is computed on,
// and written to one LDS image of 1184-byte rows after it (invalid positions as zeros; the row, once gathered, serves every head of the
// block as key and as value).  The accumulators and the staged tile leave no room for q in registers beside LDS reads in flight, and with
// one wave a SIMD a read that is not in flight ahead of its MFMA costs its whole latency.  Per tile and wave:
//   S^T = K Q^T   two 16-key subtiles, each 18 chained v_mfma_f32_16x16x32_bf16 over d ascending from +0 (K and Q by ds_read_b128, Q the B operand):
//                 lane l holds head l & 15 of the wave and the keys 4 (l >> 4) + i and 16 + 4 (l >> 4) + i, i = 0 .. 3
//   x = S (sm_scale log2 e), -inf at invalid positions;  m' = max(m, max over the tile) (two lane exchanges);  m* = m' or 0 when m' = -inf;
//   alpha = exp2(m - m*);  p = exp2(x - m*);  l = l alpha + (the lane's eight p, fp32, unrounded, ascending key);  O = O alpha (skipped while
//   no lane of the wave has alpha != 1)
//   O^T += V^T P^T  32 column tiles, one v_mfma_f32_16x16x32_bf16 each: P rounded to bf16 (RNE) in the registers S left it in -- the
//                 product's k index runs over the lane's eight keys, and V's fragment is read to match by two ds_read_b64_tr_b16 of the
//                 blocks [keys 4 g .. 4 g + 3] and [keys 16 + 4 g ..] x [16 columns]
// and at the end l is summed over the four lane groups ((l_0 + l_1) + (l_2 + l_3)), out = O (1 / l) rounded to bf16, lse = ln 2 (m + log2 l).
// m* = 0 for a tile without a valid position while m is still -inf keeps -inf - -inf out of the exponent: alpha = exp2(-inf) = 0 on O = 0.
// A head's state lives in the 4 lanes l & 15 == h of one wave, every output has one writer, nothing is atomic: two runs give the same bits.
// Nothing is dereferenced for an invalid position, no kv row outside the list and no column >= 576 is read.
// Workgroup w of the grid takes the logical block (w % 8) chunk + w / 8, chunk = ceil(blocks / 8): workgroups go to the eight XCDs in
// turn, so consecutive tokens -- which select largely the same rows -- share one XCD's L2 (DGA_SPARSE_MLA_LINEAR_GRID turns it off).
//   dga_sparse_mla_fwd_fp8   the same over a paged fp8 latent cache: rows of DGA_SPARSE_MLA_FP8_ROW_BYTES = 656 bytes -- 512 e4m3fn codes,
//                        4 fp32 scales (one per 128 codes), 64 bf16 rope values -- row r at (r / page_size) block_stride + (r % page_size) 656
// One kernel text, instantiated on the cache (SmlaBf16Rows, SmlaFp8Rows): only the gather differs.  Of an fp8 row a thread loads the 16
// bytes of scales, four 16-byte code chunks (chunks tid % 8 + 8 c, chunk c in scale group c) and one 16-byte rope chunk -- 6 staged uint4
// for 9 -- and dequantises its 64 codes in 32 units of two, one unit behind each MFMA of O^T += V^T P^T, where its four vector
// instructions issue while the MFMA runs: v_cvt_pk_f32_fp8 (exact), two v_mul_f32 by the group's scale, v_cvt_pk_bf16_f32 (RNE).  The staged
// registers grow from 6 to 9 uint4 as the units replace codes by bf16, never beyond the bf16 gather's 9.  What goes to LDS at the top of the
// loop is the row's dequantised image, deq[r, d] = RNE_bf16(fl32(e4m3(code) scale)), in the bf16 gather's format: from the barrier on the
// two kernels run the same instructions on the same bytes, so dga_sparse_mla_fwd_fp8(cache) is dga_sparse_mla_fwd(deq(cache)) bit for bit.
// ("Sparse MLA attention over a paged fp8 latent cache", has the schedules that were measured.)
//   dga_sparse_mla_fwd_partial, dga_sparse_mla_fwd_fp8_partial   split-topk decode: the third axis of the one kernel text, <Cache, PARTIAL>.
// With tiles = ceil(topk / 32) and P <= min(tiles, 64) splits the grid is m head_blocks P workgroups, the splits of one token and head block
// adjacent in the same XCD mapping; split p runs the loop above over the tiles [p tiles / P, (p + 1) tiles / P) only (wave-uniform, in
// SGPRs; the read-ahead stops at the split's end) and stores, in fp32 and not rounded, partial_out[p, t, h, :] = O (1 / l) by 16-byte stores
// of a lane's four columns and partial_lse[p, t, h] = ln 2 (m + log2 l) -- +0 and -inf for a split without a valid position.  Every element
// of [P, m, heads, 512] and [P, m, heads] is written.  dga_sparse_mla_merge (dga_sparse_mla_merge.hip) turns them into out and lse; with
// P = 1 the two launches reproduce the one-pass kernel byte for byte.  The one-pass instantiations <Cache, false> are what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dga_hip.h"
#include "dga_internal.hpp"

#pragma clang fp contract(off)

namespace dga {

constexpr int SMLA_D = DGA_SPARSE_MLA_D_QK;                  // 576
constexpr int SMLA_DV = DGA_SPARSE_MLA_D_V;                  // 512
constexpr int SMLA_THREADS = 256;
constexpr int SMLA_TILE = 32;                                // positions of one gathered tile
constexpr int SMLA_ROW_BYTES = SMLA_D * 2 + 32;              // 1184: 296 dwords = 40 mod 64, both kinds of read are free of bank conflicts
constexpr int SMLA_CHUNKS = SMLA_D / 8;                      // 16-byte chunks of a row: 72
constexpr int SMLA_STAGE = SMLA_CHUNKS / 8;                  // chunks a thread gathers per tile: 9, of one row
constexpr int SMLA_KSTEPS = SMLA_D / 32;                     // 18
constexpr int SMLA_CTILES = SMLA_DV / 16;                    // 32
static_assert(SMLA_KSTEPS % 2 == 0 && SMLA_CTILES % 4 == 0 && SMLA_TILE * 8 == SMLA_THREADS && SMLA_CHUNKS == 8 * SMLA_STAGE && SMLA_D % 32 == 0 && SMLA_DV % 16 == 0, "the kernel's geometry");

typedef float smla_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 smla_v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 smla_v4bf __attribute__((ext_vector_type(4)));
typedef short smla_v4s __attribute__((ext_vector_type(4)));
typedef short smla_v8s __attribute__((ext_vector_type(8)));
typedef uint32_t smla_v4u __attribute__((ext_vector_type(4)));
typedef float smla_v2f __attribute__((ext_vector_type(2)));
typedef __bf16 smla_v2bf __attribute__((ext_vector_type(2)));

constexpr int SMLA_FP8_ROW = DGA_SPARSE_MLA_FP8_ROW_BYTES;   // 656: 512 codes, 4 fp32 scales, 64 bf16
constexpr int SMLA_FP8_SLICES = 8;                           // 16-byte chunks of bf16 a thread makes of its 64 codes per tile
static_assert(SMLA_FP8_ROW == SMLA_DV + 16 + 2 * (SMLA_D - SMLA_DV) && SMLA_FP8_ROW % 16 == 0 && SMLA_FP8_SLICES == SMLA_CTILES / 4 &&
              SMLA_FP8_SLICES + 1 == SMLA_STAGE, "the fp8 row, and eight 16-byte chunks of bf16 from its codes");

// What the kernel gathers from.  A cache says where thread gsub (of the eight a row has) starts in row r, what it loads from there
// (RAW uint4, all in flight together), and where chunk c of the nine it ends up with stands in the 1184-byte LDS row.
// bf16 rows: the nine chunks gsub + 8 c of the row as they are.
struct SmlaBf16Rows {
    static constexpr bool FP8 = false;
    static constexpr int RAW = SMLA_STAGE;
    const uint16_t *kv;
    int64_t kv_stride, s_rows;
    static __device__ __forceinline__ SmlaBf16Rows make(const void *kv, int64_t stride, int64_t s_rows, int, int)
    {
        return SmlaBf16Rows{static_cast<const uint16_t *>(kv), stride, s_rows};
    }
    __device__ __forceinline__ const unsigned char *at(int64_t r, int gsub) const
    {
        return reinterpret_cast<const unsigned char *>(kv + r * kv_stride + gsub * 8);
    }
    static __device__ __forceinline__ void load(const unsigned char *p, int gsub, uint4 (&v)[RAW])
    {
#pragma unroll
        for (int c = 0; c < RAW; ++c) v[c] = *reinterpret_cast<const uint4 *>(p + 128 * c);
    }
    static __device__ __forceinline__ int lds_at(int c, int gsub) { return gsub * 16 + 128 * c; }
};
// fp8 rows: v[0 .. 3] the code chunks gsub + 8 c (bytes 16 gsub + 128 c of the row: chunk c lies in scale group c), v[4] the four
// scales (bytes 512 .. 527), v[5] the rope chunk gsub (bytes 528 + 16 gsub ..).  The codes 8 h .. 8 h + 7 of chunk c, image chunk 2 c + h,
// become 16 bytes of bf16 at byte 32 (gsub + 8 c) + 16 h of the LDS row; the rope chunk goes where the bf16 gather puts its ninth.
struct SmlaFp8Rows {
    static constexpr bool FP8 = true;
    static constexpr int RAW = 6;
    const unsigned char *kv;
    int64_t block_stride, s_rows;
    int page_size, page_shift;                               // page_shift >= 0: page_size = 1 << page_shift
    static __device__ __forceinline__ SmlaFp8Rows make(const void *kv, int64_t stride, int64_t s_rows, int page_size, int page_shift)
    {
        return SmlaFp8Rows{static_cast<const unsigned char *>(kv), stride, s_rows, page_size, page_shift};
    }
    __device__ __forceinline__ const unsigned char *at(int64_t r, int gsub) const
    {
        const uint32_t rr = (uint32_t)r;                     // (0 <= r < s_rows < 2^31)
        const uint32_t blk = page_shift >= 0 ? rr >> page_shift : rr / (uint32_t)page_size;
        const uint32_t in = rr - blk * (uint32_t)page_size;
        return kv + (int64_t)blk * block_stride + (int64_t)in * SMLA_FP8_ROW + gsub * 16;
    }
    static __device__ __forceinline__ void load(const unsigned char *p, int gsub, uint4 (&v)[RAW])
    {
        v[4] = *reinterpret_cast<const uint4 *>(p - gsub * 16 + SMLA_DV);   // (first: the first slice needs them beside chunk 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = *reinterpret_cast<const uint4 *>(p + 128 * c);
        v[5] = *reinterpret_cast<const uint4 *>(p + SMLA_DV + 16);
    }
    static __device__ __forceinline__ int lds_at(int c, int gsub)
    {
        return c < SMLA_FP8_SLICES ? gsub * 32 + 256 * (c >> 1) + 16 * (c & 1) : 2 * SMLA_DV + gsub * 16;
    }
};

// two codes' exact fp32 values times the scale of their group, each product rounded once to bf16 (RNE): one dword of the image
__device__ __forceinline__ uint32_t smla_deq2(smla_v2f v, float s)
{
    const float a = v[0] * s, b = v[1] * s;                  // (two v_mul_f32: packed fp32 arithmetic is a loss beside MFMAs)
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((smla_v2f{a, b}), smla_v2bf));
}
// Unit u of the 32 a thread has per tile: the codes 2 (u & 1), 2 (u & 1) + 1 of dword (u >> 1) & 3 of code chunk u >> 3 -> one dword of the
// bf16 image, four vector instructions: v_cvt_pk_f32_fp8 (one half of the dword), two v_mul_f32 by the group's scale, v_cvt_pk_bf16_f32.
// PIN: the code dword goes in (once, at its even unit; the odd one takes it from `pinned`) and the bf16 dword comes out through empty asm
// statements, which keep the unit where it is written.  Without them the compiler sees the same conversions on both sides of the loop's
// `computes` branch, hoists the fp8 -> fp32 half above the branch -- straight behind the loads it then waits for -- and sinks the bf16
// half below the join, parking 64 fp32 products in AGPRs.
constexpr int SMLA_FP8_UNITS = 4 * SMLA_FP8_SLICES;
template <bool PIN>
__device__ __forceinline__ void smla_fp8_unit(int u, const uint4 (&raw)[SmlaFp8Rows::RAW], uint32_t (&pinned)[SMLA_FP8_UNITS / 2],
                                              uint4 (&staged)[SMLA_STAGE])
{
    const int c = u >> 3, d = (u >> 1) & 3;
    const float s = __uint_as_float(c == 0 ? raw[4].x : c == 1 ? raw[4].y : c == 2 ? raw[4].z : raw[4].w);
    if (!(u & 1)) {
        uint32_t w = d == 0 ? raw[c].x : d == 1 ? raw[c].y : d == 2 ? raw[c].z : raw[c].w;
        if (PIN) asm volatile("" : "+v"(w));
        pinned[u >> 1] = w;
    }
    const uint32_t w = pinned[u >> 1];
    uint32_t o = smla_deq2((u & 1) ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), s);
    if (PIN) asm volatile("" : "+v"(o));
    uint4 &dst = staged[2 * c + (d >> 1)];
    const int at = 2 * (d & 1) + (u & 1);
    if (at == 0) dst.x = o;
    else if (at == 1) dst.y = o;
    else if (at == 2) dst.z = o;
    else dst.w = o;
}
// The units are dealt evenly over the O loop's MFMAs 4 SMLA_FP8_FIRST_GROUP .. 31, one (or more) behind each: the number done before MFMA mf
#ifndef DGA_SMLA_FP8_FIRST_GROUP
#define DGA_SMLA_FP8_FIRST_GROUP 0
#endif
constexpr int SMLA_FP8_FIRST_MFMA = 4 * (DGA_SMLA_FP8_FIRST_GROUP);
static_assert(SMLA_FP8_FIRST_MFMA >= 0 && SMLA_FP8_FIRST_MFMA < SMLA_CTILES, "the units start inside the O loop");
__device__ __forceinline__ constexpr int smla_units_before(int mf)
{
    return mf <= SMLA_FP8_FIRST_MFMA ? 0 : (mf - SMLA_FP8_FIRST_MFMA) * SMLA_FP8_UNITS / (SMLA_CTILES - SMLA_FP8_FIRST_MFMA);
}
// what a thread has loaded -> the nine chunks it writes to LDS, units [first, last) of them; the ninth chunk comes with the last unit
template <typename Cache, bool PIN = false>
__device__ __forceinline__ void smla_stage(int first, int last, const uint4 (&raw)[Cache::RAW], uint32_t (&pinned)[SMLA_FP8_UNITS / 2],
                                           uint4 (&staged)[SMLA_STAGE])
{
    if constexpr (Cache::FP8) {
#pragma unroll
        for (int u = first; u < last; ++u) smla_fp8_unit<PIN>(u, raw, pinned, staged);
        if (last == SMLA_FP8_UNITS && first < last) staged[SMLA_FP8_SLICES] = raw[5];
    } else {
        if (last == SMLA_FP8_UNITS && first < last) {
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) staged[c] = raw[c];
        }
    }
}

template <typename Cache, bool PARTIAL>
__global__ void __launch_bounds__(SMLA_THREADS) sparse_mla_fwd_kernel(const uint16_t *__restrict__ q, const void *__restrict__ kv,
                                                                      int64_t kv_stride, int64_t s_rows, const int32_t *__restrict__ indices,
                                                                      int64_t idx_stride, int topk, const int32_t *__restrict__ offsets,
                                                                      int heads, int head_blocks, int64_t blocks, int64_t chunk, float scale2,
                                                                      uint16_t *__restrict__ out, float *__restrict__ lse, int page_size,
                                                                      int page_shift, float *__restrict__ partial_out,
                                                                      float *__restrict__ partial_lse, int num_splits, int64_t split_rows)
{
    // (kv_stride: elements between bf16 rows, bytes between fp8 blocks; the last two are the fp8 cache's alone -- the bf16 kernel's
    // arguments, and with them its machine code, are what they were before the fp8 cache existed; the last four are the PARTIAL
    // instantiations' alone, appended for the same reason: split_rows = m heads, the rows of one split's partial_lse)
    const Cache cache = Cache::make(kv, kv_stride, s_rows, page_size, page_shift);
    __shared__ __attribute__((aligned(16))) unsigned char tile[SMLA_TILE * SMLA_ROW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char qimg[64 * SMLA_ROW_BYTES];   // the block's q, one row a head
    __shared__ __attribute__((aligned(16))) int32_t live[SMLA_TILE];                      // 1 where the tile's position is valid
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, hl = lane & 15;

    // the logical block of this workgroup (see the head of the file); chunk == 0: the grid is taken as it is
    int64_t block = blockIdx.x;
    if (chunk) block = (block & 7) * chunk + (block >> 3);
    if (block >= blocks) return;                             // (the whole workgroup alike, before any barrier)
    // PARTIAL: the splits of one token and head block are adjacent blocks; what is left of the number is the one-pass kernel's
    int split = 0;
    if constexpr (PARTIAL) {
        split = (int)(block % num_splits);
        block = block / num_splits;
    }
    const int64_t t = block / head_blocks;
    const int h0 = (int)(block % head_blocks) * 64 + wave * 16;
    const bool computes = h0 < heads;                        // (a wave beyond the last head tile only gathers)

    const int32_t *irow = indices + t * idx_stride;
    const int64_t shift = offsets ? (int64_t)offsets[t] : 0;
    const int tiles = (topk + SMLA_TILE - 1) / SMLA_TILE;
    // the tiles [tile_lo, tile_hi) this workgroup walks, wave-uniform: all of them, or split `split` of num_splits <= tiles (never empty);
    // positions from `limit` on are not gathered (PARTIAL: the next split's first tile is not this one's to read ahead)
    const int tile_lo = PARTIAL ? (int)((int64_t)split * tiles / num_splits) : 0;
    const int tile_hi = PARTIAL ? (int)((int64_t)(split + 1) * tiles / num_splits) : tiles;
    const int64_t limit = PARTIAL && tile_hi < tiles ? (int64_t)tile_hi * SMLA_TILE : (int64_t)topk;

    // The gather: eight threads a position (position tid / 8 of the tile), thread tid % 8 of them the 16-byte chunks tid % 8 + 8 c,
    // c = 0 .. 8, of the row -- 128 contiguous bytes of a row per eight lanes and step.  A position's index is read one tile ahead of its
    // row (ask: from a position clamped into the list, so that the load needs no branch and nothing waits for it) and turned into the
    // row's address, null for an invalid position, when the row is asked for (row_of).
    const int gpos = tid >> 3, gsub = tid & 7;
    auto ask = [&](int tl) -> int32_t {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        return irow[pos < topk ? pos : topk - 1];
    };
    auto row_of = [&](int tl, int32_t i) -> const unsigned char * {
        const int64_t pos = (int64_t)tl * SMLA_TILE + gpos;
        const int64_t r = (int64_t)i + shift;
        return (pos < limit && i >= 0 && r >= 0 && r < cache.s_rows) ? cache.at(r, gsub) : nullptr;
    };
    // (an invalid position stages zeros: codes 0 under scales 0 are +0 as well)
    auto fetch = [&](const unsigned char *row, uint4 (&v)[Cache::RAW]) {
#pragma unroll
        for (int c = 0; c < Cache::RAW; ++c) v[c] = uint4{0, 0, 0, 0};
        if (row) Cache::load(row, gsub, v);
    };

    uint4 raw[Cache::RAW], staged[SMLA_STAGE];                // what is in flight, and the nine chunks of the row's image it becomes
    const unsigned char *row = row_of(tile_lo, ask(tile_lo));
    fetch(row, raw);
    int32_t asked = ask(tile_lo + 1);

    // the block's slice of q goes to LDS once, in the tile's row format (the first barrier of the loop stands between this and its use):
    // eight threads a head, 32 heads a pass
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int hb = pass * 32 + gpos, head = (int)(block % head_blocks) * 64 + hb;
        if (head < heads) {
            const uint16_t *qrow = q + ((t * heads + head) * SMLA_D + gsub * 8);
            uint4 v[SMLA_STAGE];
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) v[c] = *reinterpret_cast<const uint4 *>(qrow + 64 * c);
#pragma unroll
            for (int c = 0; c < SMLA_STAGE; ++c) *reinterpret_cast<uint4 *>(qimg + hb * SMLA_ROW_BYTES + gsub * 16 + 128 * c) = v[c];
        }
    }

    uint32_t pinned[SMLA_FP8_UNITS / 2];                      // (an fp8 cache's code dwords between their two units)
    smla_stage<Cache>(0, SMLA_FP8_UNITS, raw, pinned, staged);   // (the first tile's: nothing to hide it behind)

    smla_v4f acc[SMLA_CTILES];
#pragma unroll
    for (int ct = 0; ct < SMLA_CTILES; ++ct) acc[ct] = smla_v4f{0.f, 0.f, 0.f, 0.f};
    float mx = -__builtin_inff(), sum = 0.f;                 // the running maximum (log2 domain) of head hl, the lane's share of l

    // LDS addresses of the lane's reads: K rows hl and 16 + hl at bytes 64 s + 16 g; V blocks by ds_read_b64_tr_b16 (lane 4 q + p of
    // a group gives row q, columns 4 p .. of the block)
    const uint32_t tile_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)tile;
    const uint32_t k_addr = tile_base + hl * SMLA_ROW_BYTES + 16 * g;
    const uint32_t v_addr = tile_base + (4 * g + (hl >> 2)) * SMLA_ROW_BYTES + 8 * (hl & 3);
    const uint32_t q_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)qimg + (wave * 16 + hl) * SMLA_ROW_BYTES + 16 * g;

#pragma unroll 1
    for (int tl = tile_lo; tl < tile_hi; ++tl) {
        // the staged tile goes to LDS
#pragma unroll
        for (int c = 0; c < SMLA_STAGE; ++c)
            *reinterpret_cast<uint4 *>(tile + gpos * SMLA_ROW_BYTES + Cache::lds_at(c, gsub)) = staged[c];
        if (gsub == 0) live[gpos] = row != nullptr;
        __syncthreads();
        // the next tile's rows are asked for now and written after this tile's products; the indices of the one after it behind them
        row = row_of(tl + 1, asked);
        fetch(row, raw);
        asked = ask(tl + 2);

        if (computes) {
            // One wave a SIMD: nobody else hides an LDS read's latency, so the reads run one group ahead of the MFMAs that consume
            // them, in the order written here (the scheduling barriers keep it): two d steps a group for S, four column tiles for O.
            const smla_v4u lv0 = *reinterpret_cast<const smla_v4u *>(&live[4 * g]), lv1 = *reinterpret_cast<const smla_v4u *>(&live[16 + 4 * g]);
            smla_v4f s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
            smla_v4u ka[2][2], kb[2][2], qq[2][2];
            auto read_k = [&](int grp) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int s = 2 * grp + j;
                    ka[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(k_addr + 64 * s);
                    kb[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(k_addr + 16 * SMLA_ROW_BYTES + 64 * s);
                    qq[grp & 1][j] = *reinterpret_cast<const smla_v4u __attribute__((address_space(3))) *>(q_addr + 64 * s);
                }
            };
            smla_v4s vlo[2][4], vhi[2][4];
            auto read_v = [&](int grp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ct = 4 * grp + j;
                    vlo[grp & 1][j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(v_addr + 32 * ct));
                    vhi[grp & 1][j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        reinterpret_cast<smla_v4s __attribute__((address_space(3))) *>(v_addr + 16 * SMLA_ROW_BYTES + 32 * ct));
                }
            };
            read_k(0);
#pragma unroll
            for (int grp = 0; grp < SMLA_KSTEPS / 2; ++grp) {
                if (grp + 1 < SMLA_KSTEPS / 2) read_k(grp + 1);
                else read_v(0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, ka[grp & 1][j]),
                                                                 __builtin_bit_cast(smla_v8bf, qq[grp & 1][j]), s0, 0, 0, 0);
                    s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, kb[grp & 1][j]),
                                                                 __builtin_bit_cast(smla_v8bf, qq[grp & 1][j]), s1, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            float x[8];
            float tmax = -__builtin_inff();
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float sv = i < 4 ? s0[i] : s1[i - 4];
                x[i] = (i < 4 ? lv0[i] : lv1[i - 4]) ? sv * scale2 : -__builtin_inff();
                tmax = __builtin_fmaxf(tmax, x[i]);          // (a NaN score is passed over here and reaches the result through p)
            }
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = __builtin_fmaxf(mx, tmax);
            const float muse = mnew == -__builtin_inff() ? 0.f : mnew;
            const float alpha = __builtin_amdgcn_exp2f(mx - muse);
            mx = mnew;
            float p[8];
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                p[i] = __builtin_amdgcn_exp2f(x[i] - muse);
                psum = psum + p[i];
            }
            sum = sum * alpha + psum;
            if (__ballot(alpha != 1.0f) != 0) {
#pragma unroll
                for (int ct = 0; ct < SMLA_CTILES; ++ct) acc[ct] = acc[ct] * alpha;
            }
            smla_v8bf pf;
#pragma unroll
            for (int i = 0; i < 8; ++i) pf[i] = (__bf16)p[i];
#pragma unroll
            for (int grp = 0; grp < SMLA_CTILES / 4; ++grp) {
                if (grp + 1 < SMLA_CTILES / 4) read_v(grp + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const smla_v8s vf = __builtin_shufflevector(vlo[grp & 1][j], vhi[grp & 1][j], 0, 1, 2, 3, 4, 5, 6, 7);
                    acc[4 * grp + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(smla_v8bf, vf), pf, acc[4 * grp + j], 0, 0, 0);
                    if constexpr (Cache::FP8) {
                        // a unit of the next tile's rows behind each MFMA: its four vector instructions issue while the MFMA runs
                        // (the rows were asked for at the top of the loop, a whole S^T and softmax ago)
                        smla_stage<Cache, true>(smla_units_before(4 * grp + j), smla_units_before(4 * grp + j + 1), raw, pinned, staged);
                        if (j < 3) __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (!Cache::FP8) smla_stage<Cache>(0, SMLA_FP8_UNITS, raw, pinned, staged);   // (bf16 rows: as they came)
        } else {
            smla_stage<Cache>(0, SMLA_FP8_UNITS, raw, pinned, staged);   // (a wave beyond the last head tile: all of it at once)
        }
        __syncthreads();
    }

    if (!computes) return;
    // l over the four lane groups that share a head: (l_0 + l_1) + (l_2 + l_3) in every one of them
    sum = sum + __shfl_xor(sum, 16, 64);
    sum = sum + __shfl_xor(sum, 32, 64);
    const bool empty = sum == 0.f;                           // no valid position (a NaN is not equal to 0 and goes through)
    const float inv = empty ? 0.f : 1.0f / sum;
    if constexpr (PARTIAL) {
        // the split's own result, O (1 / l) before its rounding to bf16: 16-byte stores of the lane's four columns
        const int64_t prow = split * split_rows + t * heads + h0 + hl;
        float *orow = partial_out + (prow * SMLA_DV + 4 * g);
#pragma unroll
        for (int ct = 0; ct < SMLA_CTILES; ++ct) {
            smla_v4f o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = empty ? 0.f : acc[ct][i] * inv;
            *reinterpret_cast<smla_v4f *>(orow + 16 * ct) = o;
        }
        if (g == 0) partial_lse[prow] = empty ? -__builtin_inff() : (mx + __builtin_amdgcn_logf(sum)) * 0.693147180559945309f;
    } else {
        uint16_t *orow = out + ((t * heads + h0 + hl) * SMLA_DV + 4 * g);
#pragma unroll
        for (int ct = 0; ct < SMLA_CTILES; ++ct) {
            smla_v4bf o;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = (__bf16)(empty ? 0.f : acc[ct][i] * inv);
            *reinterpret_cast<uint2 *>(orow + 16 * ct) = __builtin_bit_cast(uint2, o);
        }
        if (g == 0) lse[t * heads + h0 + hl] = empty ? -__builtin_inff() : (mx + __builtin_amdgcn_logf(sum)) * 0.693147180559945309f;
    }
}

// What the four entries hand to the one check and the one launch below: the call without its row source and outputs, the row source, and
// the outputs of either kind.  A new row source is one more maker of SmlaSource with its clauses in the four questions the check asks; a
// new axis of the kernel is one more template parameter of the launch.
struct SmlaCall {
    const void *q;
    const int32_t *indices, *index_offsets;
    int64_t m;
    int heads;
    int64_t topk, idx_stride;
    double sm_scale;
    int flags;
    void *stream;
};

// count units of page_size rows each, `stride` apart: bf16 rows (s of them, one a unit, kv_stride elements apart) or the blocks of the
// paged fp8 cache (block_stride bytes apart).  The range clauses divide by what the shape clause has vouched for.
struct SmlaSource {
    bool fp8;
    const void *rows;
    int64_t count, page_size, stride;
    // (stride / 656 < page_size says block_stride < 656 page_size without the product)
    bool shape() const { return count >= 1 && page_size >= 1 && (fp8 ? stride / SMLA_FP8_ROW >= page_size : stride >= SMLA_D); }
    bool aligned() const { return reinterpret_cast<uintptr_t>(rows) % 16 == 0 && stride % (fp8 ? 16 : 8) == 0; }
    bool rows_in_range() const { return count <= 0x7FFFFFFFll / page_size; }
    bool bytes_in_range() const { return stride <= 0x7FFFFFFFFFFFFFFFll / (fp8 ? 1 : 2) / count; }
};

static int page_shift_of(int page) { return (page & (page - 1)) == 0 ? __builtin_ctz(page) : -1; }

// The checks of all four entries, in the documented order: flags, shape, m == 0, null, alignment, range; *launch is set when a launch is
// to follow (not for m == 0).  out and lse are the one-pass entries' (null and unchecked for the partial ones, whose outputs the launch
// checks afterwards).
static int check_sparse_mla(const SmlaCall &c, const SmlaSource &src, bool outputs, const void *out, const void *lse, bool *launch)
{
    *launch = false;
    if (c.flags & ~DGA_SPARSE_MLA_LINEAR_GRID) return DGA_E_RANGE;
    if (c.m < 0 || c.heads < 16 || c.heads > DGA_SPARSE_MLA_MAX_HEADS || c.heads % 16 || !src.shape() || c.topk < 1 || c.idx_stride < c.topk)
        return DGA_E_SHAPE;
    if (c.m == 0) return DGA_OK;
    if (!c.q || !src.rows || !c.indices || (outputs && (!out || !lse))) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(c.q) % 16 || !src.aligned() || reinterpret_cast<uintptr_t>(out) % 16 ||
        reinterpret_cast<uintptr_t>(c.indices) % 4 || reinterpret_cast<uintptr_t>(c.index_offsets) % 4 || reinterpret_cast<uintptr_t>(lse) % 4)
        return DGA_E_ALIGN;
    const int head_blocks = (c.heads + 63) / 64;
    if (!src.rows_in_range() || c.topk > 0x7FFFFFFFll - DGA_SPARSE_MLA_TILE || c.m > (0x7FFFFFFFll - 8) / head_blocks) return DGA_E_RANGE;
    if (!src.bytes_in_range() || c.idx_stride > 0x7FFFFFFFFFFFFFFFll / 4 / c.m) return DGA_E_RANGE;
    *launch = true;
    return DGA_OK;
}

// The launch all four entries end in: one workgroup per token, block of 64 heads and split, the grid walked XCD by XCD unless it is linear.
// PARTIAL: num_splits and the partial pointers are checked first, behind the common checks; *effective_splits is written on success only.
template <typename Cache, bool PARTIAL>
static int launch_sparse_mla(const SmlaCall &c, const SmlaSource &src, void *out, float *lse, int num_splits, int *effective_splits,
                             float *partial_out, float *partial_lse)
{
    const int head_blocks = (c.heads + 63) / 64;
    int splits = 1;
    if constexpr (PARTIAL) {
        if (num_splits < 1 || num_splits > DGA_SPARSE_MLA_MAX_SPLITS) return DGA_E_RANGE;
        const int64_t tiles = (c.topk + SMLA_TILE - 1) / SMLA_TILE;
        splits = num_splits > tiles ? static_cast<int>(tiles) : num_splits;
        if (c.m > (0x7FFFFFFFll - 8) / head_blocks / splits) return DGA_E_RANGE;
        if (!partial_out || !partial_lse) return DGA_E_NULL;
        if (reinterpret_cast<uintptr_t>(partial_out) % 16 || reinterpret_cast<uintptr_t>(partial_lse) % 4) return DGA_E_ALIGN;
        if (effective_splits) *effective_splits = splits;
    }
    const int64_t blocks = c.m * head_blocks * splits;
    const bool linear = (c.flags & DGA_SPARSE_MLA_LINEAR_GRID) != 0;
    const int64_t chunk = linear ? 0 : (blocks + 7) / 8;
    const int64_t grid = linear ? blocks : chunk * 8;
    const int page = src.fp8 ? static_cast<int>(src.page_size) : 0;
    hipLaunchKernelGGL((sparse_mla_fwd_kernel<Cache, PARTIAL>), dim3(static_cast<unsigned>(grid)), dim3(SMLA_THREADS), 0,
                       static_cast<hipStream_t>(c.stream), static_cast<const uint16_t *>(c.q), src.rows, src.stride, src.count * src.page_size,
                       c.indices, c.idx_stride, static_cast<int>(c.topk), c.index_offsets, c.heads, head_blocks, blocks, chunk,
                       static_cast<float>(c.sm_scale * 1.4426950408889634), static_cast<uint16_t *>(out), lse, page,
                       src.fp8 ? page_shift_of(page) : 0, partial_out, partial_lse, splits, PARTIAL ? c.m * c.heads : static_cast<int64_t>(0));
    return record_hip(hipGetLastError());
}

}  // namespace dga

extern "C" int dga_sparse_mla_fwd(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                  int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, void *out,
                                  float *lse, void *stream)
{
    using namespace dga;
    const SmlaCall c{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream};
    const SmlaSource src{false, kv, s, 1, kv_stride};
    bool launch;
    const int rc = check_sparse_mla(c, src, true, out, lse, &launch);
    return launch ? launch_sparse_mla<SmlaBf16Rows, false>(c, src, out, lse, 1, nullptr, nullptr, nullptr) : rc;
}

extern "C" int dga_sparse_mla_fwd_fp8(const void *q, const void *kv_cache, const int32_t *indices, const int32_t *index_offsets, int64_t m,
                                      int heads, int64_t num_blocks, int64_t page_size, int64_t block_stride, int64_t topk, int64_t idx_stride,
                                      double sm_scale, int flags, void *out, float *lse, void *stream)
{
    using namespace dga;
    const SmlaCall c{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream};
    const SmlaSource src{true, kv_cache, num_blocks, page_size, block_stride};
    bool launch;
    const int rc = check_sparse_mla(c, src, true, out, lse, &launch);
    return launch ? launch_sparse_mla<SmlaFp8Rows, false>(c, src, out, lse, 1, nullptr, nullptr, nullptr) : rc;
}

// Split-topk decode: the same checks, then num_splits and the partial pointers (launch_sparse_mla<Cache, true>)
extern "C" int dga_sparse_mla_fwd_partial(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                                          int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags,
                                          int num_splits, int *effective_splits, float *partial_out, float *partial_lse, void *stream)
{
    using namespace dga;
    const SmlaCall c{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream};
    const SmlaSource src{false, kv, s, 1, kv_stride};
    bool launch;
    const int rc = check_sparse_mla(c, src, false, nullptr, nullptr, &launch);
    return launch ? launch_sparse_mla<SmlaBf16Rows, true>(c, src, nullptr, nullptr, num_splits, effective_splits, partial_out, partial_lse) : rc;
}

extern "C" int dga_sparse_mla_fwd_fp8_partial(const void *q, const void *kv_cache, const int32_t *indices, const int32_t *index_offsets, int64_t m,
                                              int heads, int64_t num_blocks, int64_t page_size, int64_t block_stride, int64_t topk,
                                              int64_t idx_stride, double sm_scale, int flags, int num_splits, int *effective_splits,
                                              float *partial_out, float *partial_lse, void *stream)
{
    using namespace dga;
    const SmlaCall c{q, indices, index_offsets, m, heads, topk, idx_stride, sm_scale, flags, stream};
    const SmlaSource src{true, kv_cache, num_blocks, page_size, block_stride};
    bool launch;
    const int rc = check_sparse_mla(c, src, false, nullptr, nullptr, &launch);
    return launch ? launch_sparse_mla<SmlaFp8Rows, true>(c, src, nullptr, nullptr, num_splits, effective_splits, partial_out, partial_lse) : rc;
}
