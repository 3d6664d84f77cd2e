// Text fragment, not a header (see gemm_fp8_bf16x_wave_tile.inc, whose state it runs on): one k block of the bf16-exact policy's
// 128 x 256 persistent family -- the 64 MFMA gaps (n-tile outer, m-tile inner) with the refill pieces, the B conversions and raw
// reloads, the in-place A conversions of the next block, the next block's scales and the lagged promotions, then the rotation of
// s_old / s_cur / s_nxt.  The schedule is the one-tile build's (gemm_fp8_kernel.hpp, MATH = 1, which explains it gap by gap).
// Included inside a k-block lambda, where smem, cur, nxt, refill(idx) and Cfg, TM, TN, TILES, G, NL, LAGT, RING, SFB_ROWS, v8bf are
// in scope.
            const uint8_t *sc = smem + cur * Cfg::STAGE_BYTES;   // being consumed (B raw reloads of this block)
            const uint8_t *sn = smem + nxt * Cfg::STAGE_BYTES;   // landed: the next block's fragments are read ahead from it
#pragma unroll
            for (int u = 0; u < 4 * TILES; ++u) {
                const int t = u >> 2, q = u & 3, nt = t / TM, mt = t % TM, g = u % G;
                part[t % RING] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(v8bf, bfx[nt & 1][q]), __builtin_bit_cast(v8bf, afx[mt][q]),
                    q == 0 ? v4f{0.f, 0.f, 0.f, 0.f} : part[t % RING], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (u >= 4 && u < 4 + NL) refill(u - 4);
#pragma unroll
                for (int c = 0; c < 16 / G; ++c) convert(braw, bfx[(nt + 1) & 1], (16 / G) * g + c);
                {
                    const int nn = nt + 2;
                    const uint8_t *src = nn < TN ? sc : sn;
                    const int off = b_frag_off(nn < TN ? nn : nn - TN);
                    if (g == G / 2 - 1) braw[0] = *(const v4i *)(src + b_off0 + off);
                    if (g == G - 1) braw[1] = *(const v4i *)(src + b_off1 + off);
                }
                if (nt == TN - 1 && q == 0) {
                    araw[mt & 1][0] = *(const v4i *)(sn + a_off0 + mt * 2048);
                    araw[mt & 1][1] = *(const v4i *)(sn + a_off1 + mt * 2048);
                }
                if (nt == TN - 1 && mt >= 1) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) convert(araw[(mt - 1) & 1], afx[mt - 1], 4 * q + c);
                }
                if (t == 0) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) convert(araw[(TM - 1) & 1], afx[TM - 1], 4 * q + c);
                }
                if (u == 4 * TILES - 8) {
                    if constexpr (SFB_ROWS == 1) {
#pragma unroll
                        for (int i = 0; i < TM; ++i) s_nxt[i] = *(const float *)(sn + sa_off + i * 64);
                    } else {
                    const float sfbn = *(const float *)(sn + sb_off);
#pragma unroll
                    for (int i = 0; i < TM; ++i) s_nxt[i] = *(const float *)(sn + sa_off + i * 64) * sfbn;
                    }
                }
                {
                    const int j = t >= LAGT ? t - LAGT : TILES + t - LAGT, jn = j / TM, jm = j % TM;
                    float sv = t >= LAGT ? s_cur[jm] : s_old[jm];
                    if constexpr (SFB_ROWS == 1) {
                        if (mt == 0 && q == 0) sbv[nt] = *(const v4f *)(sc + sbr_off + sbr_nt(nt));
                        sv = sv * sbv[jn][q];   // fl(sfa[m] * sfb[n])
                    }
                    acc[jm][jn][q] = __builtin_fmaf(part[j % RING][q], sv, acc[jm][jn][q]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                s_old[i] = s_cur[i];
                s_cur[i] = s_nxt[i];
            }
