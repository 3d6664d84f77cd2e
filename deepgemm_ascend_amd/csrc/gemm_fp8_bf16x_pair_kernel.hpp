// Paired body of the bf16-exact policy's dense persistent kernel (gemm_fp8_bf16x_persistent_kernel.hpp, dispatchPolicyTag 7): one
// workgroup of 8 waves computes two vertically adjacent 128 x 256 raster tiles at once -- a 256 x 256 region, wave tiles of
// 64 x 128 (4 waves along M, 2 along N).
//
// Why.  The 64 x 64 wave tile converts 64 A and 64 B fragment registers per 64 MFMAs (2 conversions per MFMA, 3.3 vector
// instructions per MFMA with the promotion and the bookkeeping); the issue port carries two per MFMA for free
// (profiles/r05_valu_rates.txt).  A 64 x 128 wave tile converts 64 A and 128 B per 128 MFMAs (1.5 per MFMA) and puts 128 MFMAs
// behind each barrier and DMA wait instead of 64.
//
// Same arithmetic in the same order per output element as the one-tile build: four chained v_mfma_f32_16x16x32_bf16 per 128-wide
// scale block on operands converted by v_cvt_scalef32_pk_bf16_fp8, then one fmaf by sfa[m] * sfb, k ascending -- bit-identical.
//
// What differs from the 64 x 64 body, all of it to fit 128 accumulators into 256 registers at two waves per SIMD:
//  - Gap order inside an n-tile is (q outer, m-tile inner): the four m-tiles' chains advance together, so a B fragment (n-tile, q)
//    lives for four MFMAs and B needs 2 x 4 fragment registers, not 2 x 16.  The partial-sum ring is the four m-tiles.
//  - The promotion of tile (nt, mt) sits two gaps behind the end of its chain (its register is rewritten two gaps later still);
//    the last two of a k block are promoted behind the block's last MFMA, so no scale of the previous block is kept.
//  - The next block's A fragments are converted in place during the last n-tile from 8-byte raw reads, three in flight.
//  - The DMA's per-lane offsets do not depend on the tile: rows at or beyond M (or N) are beyond the buffer descriptor's extent
//    and come back as zeros; the row part that depends on the piece is added where the piece is issued.
// LDS: two stages of 256 x 128 A bytes, 256 x 128 B bytes and the scale piece, and three 8 KB head slots (156 KB of 160).  Two
// stages are enough because the pieces of a stage have different lifetimes: A (and the scales) of block j+1 is read into registers
// during the last n-tile of block j, so block j+2's A is fetched into that place during block j; B rows are read all through
// their block, so block j+1's B is fetched during block j into the stage block j-1 has left -- except the first n-tile pair of
// each wave column (the "head", 32 rows), whose first n-tile block j reads during block j-1 and whose second it reads at its
// start: heads live in a ring of three slots of their own and are fetched two blocks ahead, with A.  One barrier per k block.
// Dense rasters, bf16 rows, K a multiple of 128 and of at least two k blocks.  A pair whose lower tile lies partly or wholly beyond
// M is a ragged tile like any other: the waves without rows multiply nothing and keep their share of the DMA and the barriers.
#pragma once
#include "gemm_fp8_kernel.hpp"

namespace dga {

struct PairCfg {
    static constexpr int BM = 256, BN = 256, WM = 4, WN = 2, NT = 512, TM = 4, TN = 8;
    static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, SC_BYTES = 512 * 4;
    static constexpr int STAGE_BYTES = A_BYTES + B_BYTES + SC_BYTES;
    static constexpr int HEAD_ROWS = 32;                 // per wave column: n-tiles 0 and 1
    static constexpr int HEAD_BYTES = WN * HEAD_ROWS * 128, HEAD_BASE = 2 * STAGE_BYTES;   // three head slots behind the stages
    static constexpr int LDS_BYTES = HEAD_BASE + 3 * HEAD_BYTES;
    static constexpr int BODY_ROWS = BN / WN - HEAD_ROWS;  // 96
    static constexpr int NL = 4 + 1 + 1 + 3;             // pieces per k block and thread: A x 4, scales, B head, B body x 3
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
gemm_fp8_bf16x_pair_kernel(const GemmParams p)
{
    typedef PairCfg Cfg;
    constexpr int BM = Cfg::BM, BN = Cfg::BN, WN = Cfg::WN, TM = Cfg::TM, TN = Cfg::TN, NL = Cfg::NL;
    typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, kg = lane >> 4;
    const int KB = p.kb_n;   // >= 2 (host)

    // ---- this workgroup's list of pairs: as the one-tile body's list of tiles, on a raster of (tiles_m + 1) / 2 pair rows
    const int pairs_m = (p.tiles_m + 1) >> 1;
    const int total = pairs_m * p.tiles_n;
    int first = 0, count = total, step = gridDim.x, slot = blockIdx.x;
    if (p.xcd_remap) {
        const int xcd = blockIdx.x & 7, q = total >> 3, r = total & 7;
        first = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        count = q + (xcd < r ? 1 : 0);
        step = ((int)gridDim.x - xcd + 7) >> 3;
        slot = blockIdx.x >> 3;
    }
    struct Tile { int m0, n0; };
    auto seek = [&](int local, Tile &t) -> bool {
        if (local >= count) return false;
        const int t_in = first + local;
        const int gm = max(p.raster_group >> 1, 1);
        const int per = gm * p.tiles_n;
        const int band = t_in / per;
        const int row0 = band * gm;
        const int rows = min(pairs_m - row0, gm);
        const int loc = t_in - band * per;
        t.m0 = (row0 + loc % rows) * BM;
        t.n0 = (loc / rows) * BN;
        return true;
    };

    // ---- LDS-DMA sources.  Thread tid carries chunk (tid & 7) of row (tid >> 3) of a 64-row piece; a wave carries 8 whole rows.
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
    const int lr = lane >> 3, ch = lane & 7;
    const uint32_t a_voff = (uint32_t)(wave * 8 + lr) * (uint32_t)p.lda + ((ch ^ swz_a(wave * 8 + lr)) * 16);
    // B: row R + lr with R a wave-uniform multiple of 8: swz_b(R + lr) = swz_b(lr) ^ swz_b(R)
    const uint32_t b_vrow = (uint32_t)lr * (uint32_t)p.ldb;
    const uint32_t b_vcol = (ch ^ swz_b(lr)) * 16;
    auto desc = [&](const uint8_t *base, int row0, int rows_all, int64_t ld, bool real) {
        return make_rsrc(base + (int64_t)row0 * ld, real ? (int64_t)(rows_all - row0) * ld : 0);   // !real: every lane out of range, zeros land
    };
    auto sc_ptr = [&](const Tile &t) -> const float * {   // slot tid: [0, BM) sfa rows of the pair, then its sfb blocks
        return tid < BM ? p.sfa + (int64_t)min(t.m0 + tid, p.m - 1) * p.sfa_ld
                        : p.sfb + (int64_t)min(t.n0 / 128 + min(tid - BM, 7), p.nb_n - 1) * p.kb_n;
    };

    Tile T{}, Tn{};
    int local = slot;
    if (!seek(local, T)) return;
    // the three fetch timelines: A + scales + B head run two blocks ahead, the B body one block ahead
    v4i a_rsrc = desc(p.a, T.m0, p.m, p.lda, true), bh_rsrc = desc(p.b, T.n0, p.n, p.ldb, true), bb_rsrc = bh_rsrc;
    Tile Tsc = T;   // the pair whose scales are fetched (the address is worked out per piece: two registers fewer all along)
    auto issue_a = [&](int it, int stage, int kb) {   // rows [64 it, +64) of the pair
        dma16(a_voff + (uint32_t)(it * 64) * (uint32_t)p.lda, a_rsrc, (uint32_t)(kb * 128),
              lds0 + stage * Cfg::STAGE_BYTES + it * 8192 + wave * 1024);
    };
    auto issue_sc = [&](int stage, int kb) {
        dma4(sc_ptr(Tsc) + kb, lds0 + stage * Cfg::STAGE_BYTES + Cfg::A_BYTES + Cfg::B_BYTES + wave * 256);
    };
    auto issue_b_rows = [&](int R, v4i rsrc, int kb, uint32_t dst) {   // rows [R, R + 8) of B's 256 by this wave
        const uint32_t voff = b_vrow + (b_vcol ^ (uint32_t)(swz_b(R) * 16)) + (uint32_t)R * (uint32_t)p.ldb;
        dma16(voff, rsrc, (uint32_t)(kb * 128), dst);
    };
    auto issue_head = [&](int hslot, int kb) {
        const int h = wave * 8;   // of 2 x 32 head rows, which lie in that order in a head slot
        issue_b_rows((h >> 5) * (BN / WN) + (h & 31), bh_rsrc, kb, lds0 + Cfg::HEAD_BASE + hslot * Cfg::HEAD_BYTES + h * 128);
    };
    auto issue_body = [&](int it, int stage, int kb) {
        const int h = it * 64 + wave * 8;   // of 2 x 96 body rows (a stage keeps the image of all 256 rows; its head rows stay unused)
        const int R = (h / Cfg::BODY_ROWS) * (BN / WN) + Cfg::HEAD_ROWS + h % Cfg::BODY_ROWS;
        issue_b_rows(R, bb_rsrc, kb, lds0 + stage * Cfg::STAGE_BYTES + Cfg::A_BYTES + R * 128);
    };
    // where a head slot's rows would lie were they rows of a stage: head_at(slot) + b_off0 + b_frag_off(0 or 1) is the fragment
    auto head_at = [&](int hslot) -> const uint8_t * {
        return smem + Cfg::HEAD_BASE + hslot * Cfg::HEAD_BYTES - (Cfg::A_BYTES + wn * Cfg::BODY_ROWS * 128);
    };

    // ---- per-lane fragment read offsets (bytes inside a stage; the layout: gemm_fp8_kernel.hpp)
    const int a_row = wm * 64 + li;
    const int a_off0 = a_row * 128 + ((kg ^ swz_a(a_row)) * 16);
    const int a_off1 = a_row * 128 + (((kg + 4) ^ swz_a(a_row)) * 16);
    const int b_row = wn * (BN / WN) + 8 * (li >> 2) + (li & 3);
    const int b_off0 = Cfg::A_BYTES + b_row * 128 + ((kg ^ swz_b(b_row)) * 16);
    const int b_off1 = Cfg::A_BYTES + b_row * 128 + (((kg + 4) ^ swz_b(b_row)) * 16);
    const int sa_off = Cfg::A_BYTES + Cfg::B_BYTES + a_row * 4;
    const int sb_off = Cfg::A_BYTES + Cfg::B_BYTES + (BM + wn) * 4;
    auto b_frag_off = [](int nt) { return (nt >> 1) * 4096 + (nt & 1) * 512; };

    v4f acc[TM][TN];
    v4f part[TM];
    v4i afx[TM][4];     // bf16 A fragments: [q] = the 8 bf16 of MFMA q of the chain
    v4i bq[2];          // bf16 B fragments of (n-tile, q) and of the one after it
    v4i braw[2];        // raw e4m3 bytes of an n-tile: [0] = bytes [16 kg, +16) (q 0, 1), [1] = bytes [64 + 16 kg, +16) (q 2, 3)
    v2i araw[3];        // raw e4m3 bytes of one A fragment (m-tile, q) of the next block, three in flight
    float s_cur[TM];
    auto cvt = [](int w, bool hi) {
        return hi ? __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))
                  : __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
    };
    auto clear_tile = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    };
    auto load_scales = [&](const uint8_t *st) {
        const float sfb0 = *(const float *)(st + sb_off);
#pragma unroll
        for (int i = 0; i < TM; ++i) s_cur[i] = *(const float *)(st + sa_off + i * 64) * sfb0;
    };
    // the fragments of a pair's block 0 out of the stage it has landed in, converted in one burst (the kernel's first pair, and a
    // pair that follows one in which the wave had no rows)
    auto first_fragments = [&](const uint8_t *st, const uint8_t *hd) {
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const v4i raw = *(const v4i *)(st + (h ? a_off1 : a_off0) + mt * 2048);
#pragma unroll
                for (int c = 0; c < 8; ++c) afx[mt][2 * h + (c >> 2)][c & 3] = cvt(raw[c >> 1], c & 1);
            }
        load_scales(st);
        braw[0] = *(const v4i *)(hd + b_off0);
        braw[1] = *(const v4i *)(hd + b_off1);
#pragma unroll
        for (int c = 0; c < 4; ++c) bq[0][c] = cvt(braw[0][c >> 1], c & 1);
    };
    auto rows_present = [&](const Tile &t) { return t.m0 + wm * 64 < p.m; };   // (wave-uniform)

    // ---- prologue: A, scales and head of blocks 0 and 1 and the body of block 0 on their way and landed
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
        for (int it = 0; it < 4; ++it) issue_a(it, d, d);
        issue_sc(d, d);
        issue_head(d, d);
    }
#pragma unroll
    for (int it = 0; it < 3; ++it) issue_body(it, 0, 0);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    clear_tile();
    bool active = rows_present(T);
    if (active) first_fragments(smem, head_at(0));
    int cur = 0, h_cur = 0, h_nxt = 1, h_fill = 2;   // the stage and the head slot of this block, the head slots of the next two
    bool has_next = false;

    // one k block of the pair.  The refills: A, scales and head of block kb + 2 into this block's stage, the body of block kb + 1
    // into the other one; past the pair's last block they are the next pair's (the descriptors have been switched by then).
    auto k_block = [&](int kb2, int kb1) __attribute__((always_inline)) {
        auto refill = [&](int idx) {
            if (idx < 4) issue_a(idx, cur, kb2);
            else if (idx == 4) issue_sc(cur, kb2);
            else if (idx == 5) issue_head(h_fill, kb2);
            else issue_body(idx - 6, cur ^ 1, kb1);
        };
        wait_vmcnt<0>();                         // this wave's pieces issued a block ago have landed
        __builtin_amdgcn_s_barrier();            // ... everyone's have; and everyone has left what is refilled now
        asm volatile("" ::: "memory");
        if (!active) {
#pragma unroll
            for (int idx = 0; idx < NL; ++idx) refill(idx);
        } else {
            const uint8_t *sc = smem + cur * Cfg::STAGE_BYTES;         // being consumed (B raw reloads of this block)
            const uint8_t *sn = smem + (cur ^ 1) * Cfg::STAGE_BYTES;   // the next block's A and scales have landed there
            const uint8_t *hc = head_at(h_cur), *hn = head_at(h_nxt);  // this block's n-tiles 0 and 1; the next block's: landed
#pragma unroll
            for (int u = 0; u < 16 * TN; ++u) {
                const int nt = u >> 4, r = u & 15, q = r >> 2, mt = r & 3;
                part[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(v8bf, bq[q & 1]), __builtin_bit_cast(v8bf, afx[mt][q]),
                    q == 0 ? v4f{0.f, 0.f, 0.f, 0.f} : part[mt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (u >= 4 && u < 4 + NL) refill(u - 4);
                {   // one conversion of the B fragment that follows: (nt, q + 1), or (nt + 1, 0)
                    const int fq = (q + 1) & 3;
                    bq[(q + 1) & 1][mt] = cvt(braw[fq >> 1][(2 * fq + (mt >> 1)) & 3], mt & 1);
                }
                {   // raw B of the n-tile that follows: its first half once this one's q 0, 1 are converted, its second after q 2, 3
                    const int nn = nt + 1;
                    const uint8_t *src = nn == 1 ? hc : nn < TN ? sc : hn;
                    const int off = b_frag_off(nn < TN ? nn : 0);
                    if (r == 4) braw[0] = *(const v4i *)(src + b_off0 + off);
                    if (r == 12) braw[1] = *(const v4i *)(src + b_off1 + off);
                }
                {   // the next block's A: fragment i = 4 q + mt is read two gaps ahead of the gap that converts it in place
                    const int i = u - 16 * (TN - 1) + 2;
                    if (i >= 0 && i < 16) {
                        const int iq = i >> 2, im = i & 3;
                        araw[i % 3] = *(const v2i *)(sn + ((iq >> 1) ? a_off1 : a_off0) + (iq & 1) * 8 + im * 2048);
                    }
                    if (nt == TN - 1) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) afx[mt][q][c] = cvt(araw[r % 3][c >> 1], c & 1);
                    }
                }
                if (u >= 2 && ((u - 2) & 15) >= 12) {   // the promotion of the tile whose chain ended two gaps ago
                    const int jn = (u - 2) >> 4, jm = ((u - 2) & 15) - 12;
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[jm][jn][c] = __builtin_fmaf(part[jm][c], s_cur[jm], acc[jm][jn][c]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int jm = TM - 2; jm < TM; ++jm)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[jm][TN - 1][c] = __builtin_fmaf(part[jm][c], s_cur[jm], acc[jm][TN - 1][c]);
            load_scales(sn);
        }
        cur ^= 1;
        const int hf = h_cur;
        h_cur = h_nxt; h_nxt = h_fill; h_fill = hf;
    };

    for (;;) {
        has_next = seek(local + step, Tn);
        for (int kb = 0; kb < KB - 2; ++kb) k_block(kb + 2, kb + 1);
        // the last two blocks fetch the next pair's first blocks (no next pair: zeros land, nothing is fetched)
        a_rsrc = desc(p.a, Tn.m0, p.m, p.lda, has_next);
        bh_rsrc = desc(p.b, Tn.n0, p.n, p.ldb, has_next);
        if (has_next) Tsc = Tn;
        k_block(0, KB - 1);
        bb_rsrc = bh_rsrc;
        k_block(1, 0);

        // ---- boundary: the stores, the accumulators
        if (active) {
            uint16_t *C = p.out;
            const int m_row = T.m0 + wm * 64 + li;
            const int n_base = T.n0 + wn * (BN / WN) + 8 * kg;
            const bool vec_ok = ((p.ldc & 7) == 0) && ((((uintptr_t)C) & 15) == 0);
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) {
                const int m = m_row + mt * 16;
                if (m >= p.m) continue;
                uint16_t *crow = C + (int64_t)m * p.ldc;
#pragma unroll
                for (int j = 0; j < TN / 2; ++j) {
                    const int n = n_base + 32 * j;
                    const v4f lo = acc[mt][2 * j], hi = acc[mt][2 * j + 1];
                    const v2bf h0 = __builtin_convertvector(v2f{lo.x, lo.y}, v2bf);
                    const v2bf h1 = __builtin_convertvector(v2f{lo.z, lo.w}, v2bf);
                    const v2bf h2 = __builtin_convertvector(v2f{hi.x, hi.y}, v2bf);
                    const v2bf h3 = __builtin_convertvector(v2f{hi.z, hi.w}, v2bf);
                    const v4i pk = v4i{__builtin_bit_cast(int, h0), __builtin_bit_cast(int, h1),
                                       __builtin_bit_cast(int, h2), __builtin_bit_cast(int, h3)};
                    if (vec_ok && n + 8 <= p.n) {
                        if (p.out_nt == 1) asm volatile("global_store_dwordx4 %0, %1, off nt" :: "v"(crow + n), "v"(pk) : "memory");
                        else if (p.out_nt == 2) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(crow + n), "v"(pk) : "memory");
                        else if (p.out_nt == 3) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" :: "v"(crow + n), "v"(pk) : "memory");
                        else *(v4i *)(crow + n) = pk;
                    } else {
                        const uint16_t *e = (const uint16_t *)&pk;
#pragma unroll
                        for (int q = 0; q < 8; ++q)
                            if (n + q < p.n) crow[n + q] = e[q];
                    }
                }
            }
        }
        if (!has_next) break;
        // ---- the next pair becomes the current one: its block 0 sits in stage `cur` (A, scales, head; the body lands behind the
        //      barrier of its first k block), its block 1 is on its way
        const bool was_active = active;
        T = Tn; local += step;
        active = rows_present(T);
        clear_tile();
        // (a wave that multiplied the previous pair has this block's fragments already: converted in place during that pair's
        //  last k block; one that had no rows there sets them up now)
        if (active && !was_active) first_fragments(smem + cur * Cfg::STAGE_BYTES, head_at(h_cur));
    }
    wait_vmcnt<0>();   // the refills past the last pair (zeros) land in LDS nobody reads: drain them before exit
}

}  // namespace dga
