// Text fragment, not a header: the register state of a wave's 64 x 64 tile in the bf16-exact policy's 128 x 256 persistent family
// (gemm_fp8_bf16x_persistent_kernel.hpp, both bodies, and gemm_fp8_bf16x_streamk_kernel.hpp) -- the per-lane fragment offsets, the
// accumulators, the partial-sum ring, the bf16 and raw fragments, the promotion scales, and the lambdas clear_tile / convert /
// b_frag_off / first_fragments.  Included at function scope, where Cfg, BM, BN, WN, TM, TN, RING, SFB_ROWS, wm, wn, li and kg are
// in scope; gemm_fp8_bf16x_k_block.inc is the loop that runs on this state.
// Why text and not functions: these kernels sit at 239..251 of 256 VGPRs with SGPRs spilled to lanes.  A struct with member
// functions, forceinline function templates over references, even one shared helper in place of a local lambda each moved the
// register assignment of at least one of them (the k-grouped body with every single step).  Included text compiles to the code
// the copies compiled to, instruction for instruction (scripts/isa_compare.py), so one place to edit costs nothing.
// ---- per-lane fragment read offsets (bytes inside a stage; the layout: gemm_fp8_kernel.hpp)
    const int a_row = wm * (BM / Cfg::kWM) + li;
    const int a_off0 = a_row * 128 + ((kg ^ swz_a(a_row)) * 16);
    const int a_off1 = a_row * 128 + (((kg + 4) ^ swz_a(a_row)) * 16);
    const int b_row = wn * (BN / WN) + 8 * (li >> 2) + (li & 3);
    const int b_off0 = Cfg::A_BYTES + b_row * 128 + ((kg ^ swz_b(b_row)) * 16);
    const int b_off1 = Cfg::A_BYTES + b_row * 128 + (((kg + 4) ^ swz_b(b_row)) * 16);
    const int sa_off = Cfg::A_BYTES + Cfg::B_BYTES + (wm * (BM / Cfg::kWM) + li) * 4;
    const int sb_off = Cfg::A_BYTES + Cfg::B_BYTES + (BM + (wn * (BN / WN)) / 128) * 4;
    const int sbr_off = Cfg::A_BYTES + Cfg::B_BYTES + (BM + wn * (BN / WN) + 8 * kg) * 4;   // SFB_ROWS: gemm_fp8_kernel.hpp
    auto sbr_nt = [](int nt) { return (32 * (nt >> 1) + 4 * (nt & 1)) * 4; };

    v4f acc[TM][TN];
    v4f part[RING];
    v4i afx[TM][4], bfx[2][4];      // bf16 fragments: [q] = the 8 bf16 of MFMA q of the chain
    v4i braw[2], araw[2][2];         // raw e4m3 bytes: [0] = bytes [16 kg, +16), [1] = bytes [64 + 16 kg, +16)
    float s_cur[TM], s_old[TM], s_nxt[TM];
    v4f sbv[TN];   // SFB_ROWS: the sfb of the lane's columns per n-tile (gemm_fp8_kernel.hpp); finite from the start: 0 * sbv
    if constexpr (SFB_ROWS == 1)   // (only there: an initialised array nobody reads still moves the other builds' schedule)
#pragma unroll
        for (int i = 0; i < TN; ++i) sbv[i] = v4f{0.f, 0.f, 0.f, 0.f};
    auto clear_tile = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < RING; ++i) part[i] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < TM; ++i) s_old[i] = 0.f;    // the first LAGT tiles "promote the previous block": part (= 0) * 0
    };
    auto convert = [](const v4i (&raw)[2], v4i (&dst)[4], int c) {
        const int w = raw[(c >> 1) >> 2][(c >> 1) & 3];
        dst[c >> 2][c & 3] = (c & 1) ? __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))
                                     : __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
    };
    auto b_frag_off = [](int nt) { return (nt >> 1) * 4096 + (nt & 1) * 512; };
    // the fragments of a tile's block 0 out of the stage it has landed in, converted in one burst (a tile's first block in this
    // wave: the kernel's first tile, and a tile that follows one in which the wave had no rows)
    auto first_fragments = [&](const uint8_t *st) {
        const float sfb0 = *(const float *)(st + sb_off);
#pragma unroll
        for (int mt = 0; mt < TM; ++mt) {
            araw[mt & 1][0] = *(const v4i *)(st + a_off0 + mt * 2048);
            araw[mt & 1][1] = *(const v4i *)(st + a_off1 + mt * 2048);
#pragma unroll
            for (int c = 0; c < 16; ++c) convert(araw[mt & 1], afx[mt], c);
            if constexpr (SFB_ROWS == 1) s_cur[mt] = *(const float *)(st + sa_off + mt * 64);
            else
            s_cur[mt] = *(const float *)(st + sa_off + mt * 64) * sfb0;
            s_nxt[mt] = 0.f;
        }
        braw[0] = *(const v4i *)(st + b_off0);
        braw[1] = *(const v4i *)(st + b_off1);
#pragma unroll
        for (int c = 0; c < 16; ++c) convert(braw, bfx[0], c);
        braw[0] = *(const v4i *)(st + b_off0 + b_frag_off(1));   // B(1) of block 0, raw
        braw[1] = *(const v4i *)(st + b_off1 + b_frag_off(1));
    };
