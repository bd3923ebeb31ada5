// Frame-loop fragment: |X|^2 -> colour index and level, the tile byte and the merged-cell count per bin, the frame's extremes.
// Expects in scope: re, im, tl, fr, live, gpar, group_frames, s_tile, tile_pitch, s_mm, edge_g, edge_cb, cmax, cell_sp0, LOG2N, MMS,
// LATE_SIDE, and the constants of sp_frames_epilogue_consts.inc.h.
// SP_ABS2(e): the value bin e of the thread is drawn from; the frame's own |X|^2 unless the including kernel defines it (k_frames_peak:
// the largest |X|^2 of the column's sub-frames).
#ifndef SP_ABS2
#define SP_ABS2(e) (re[e] * re[e] + im[e] * im[e])   // worker.js:92
#define SP_ABS2_DEFAULT
#endif
            // ---- |X|^2 -> colour index, centi-bel level ---------------------------------------------------------------------
            // t = a + b*log2((float)|X|^2) in f32 is within the margin m of the real-valued position of |X|^2 on the index
            // scale (sp_host.cpp); a and the clamp bounds are lowered by m, so floor(t) is exact unless fract(t) >= 1 - 2m.
            // Lanes past that threshold (and centi-bel values at or beyond the ends of the scale, +-inf and NaN among them, whose
            // clamp bounds lie past it by construction) take the exact edge compare.
            // four independent min / max chains: a dependent f64 operation waits several issue slots
            double mn4[4] = {spjs::inf(), spjs::inf(), spjs::inf(), spjs::inf()}, mx4[4] = {0.0, 0.0, 0.0, 0.0};
            uint32_t *trow = (uint32_t *)(s_tile + fr * tile_pitch + tl * 16);
            if (live) {
                constexpr int EB = 2;   // bins per batch
                [[maybe_unused]] uint32_t tile_word = 0;          // four colour bytes per tile dword
                constexpr bool TILE_BYTES = LOG2N >= 10;         // (n <= 512: no gain measured; n = 2048: neutral; n = 8192: -0.6 %)
                [[maybe_unused]] const unsigned trow_addr = (unsigned)(size_t)(__attribute__((address_space(3))) uint32_t *)trow;
                // a batch of bins at a time: independent chains for the VALU, one branch per batch, four colour bytes per tile dword
#pragma unroll
                for (int q = 0; q < 16 / EB; q++) {
                    double abs2[EB];
                    float tg[EB], tc[EB];
                    int gi[EB], cell[EB];
                    unsigned cell4[EB];              // 4 * (colour index + level): the byte offset of the pixel's merged cell
                    float worst = 0.0f;   // largest fractional part of the batch, either scale
                    // written stage by stage: the four chains are independent, and every step of a chain waits on the one before
                    float l2[EB];
#pragma unroll
                    for (int k = 0; k < EB; k++) abs2[k] = SP_ABS2(EB * q + k);
#pragma unroll
                    for (int k = 0; k < EB; k++) l2[k] = (float)abs2[k];
#pragma unroll
                    for (int k = 0; k < EB; k++) l2[k] = __log2f(l2[k]);
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        mn4[k & 3] = min_raw(mn4[k & 3], abs2[k]);
                        mx4[k & 3] = max_raw(mx4[k & 3], abs2[k]);
                    }
                    if constexpr (PK_SCALES) {
                        // one v_pk_fma_f32 per scale for the batch's two bins (4.7 issue cycles instead of 2 x 3.5, one instruction
                        // fewer per bin); each half rounds like v_fma_f32
                        static_assert(EB == 2, "a packed fma takes the batch's two bins");
                        const f32x2 lp = {l2[0], l2[1]};
                        const f32x2 tgp = __builtin_elementwise_fma(g_b2, lp, g_a2), tcp = __builtin_elementwise_fma(c_b2, lp, c_a2);
                        tg[0] = tgp.x; tg[1] = tgp.y;
                        tc[0] = tcp.x; tc[1] = tcp.y;
                    } else {
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            tg[k] = fmaf(g_b, l2[k], g_a_v);
                            tc[k] = fmaf(c_b, l2[k], c_a_v);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        tg[k] = __builtin_amdgcn_fmed3f(tg[k], g_lo, g_hi);
                        tc[k] = __builtin_amdgcn_fmed3f(tc[k], c_lo, c_hi_v);
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        gi[k] = floor_to_int(tg[k]);                                   // colour index
                        cell[k] = floor_to_int(tc[k]);                                 // level (= 999 - centi-bel bin)
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        // (the clamps have turned a NaN into a bound, so the fractional parts are numbers; one threshold, the
                        // smaller of the two, serves both scales)
                        worst = fmaxf(fmaxf(worst, __builtin_amdgcn_fractf(tg[k])), __builtin_amdgcn_fractf(tc[k]));   // one v_max3_f32
                    }
                    if (__builtin_expect(__ballot(!(worst < thr)) != 0ull, 0)) {
                        // Rare (one batch in eleven), and nearly always for ONE lane on ONE bin and ONE scale: each (bin, scale) is
                        // decided on its own - the nearest edge of that scale for every lane (one LDS read, one exact comparison),
                        // only the risky lanes keep the result (edges: sp_host.h Thresholds) - so a typical visit costs a quarter
                        // of deciding everything for the whole batch.
#pragma unroll
                        for (int k = 0; k < EB; k++) {
                            const bool rgk = !(__builtin_amdgcn_fractf(tg[k]) < thr), rck = !(__builtin_amdgcn_fractf(tc[k]) < thr);
                            int lev = cell[k];
                            if (__ballot(rgk) != 0ull) {
                                const int r = min(max((int)rintf(tg[k] + g_m), 1), cmax);
                                const int g = abs2[k] >= edge_g[r] ? r : r - 1;
                                gi[k] = rgk ? g : gi[k];
                            }
                            if (__ballot(rck) != 0ull) {
                                const int r = min(max((int)rintf(tc[k] + c_m), 1), SP_CB_HIST_SIZE);
                                const int l = abs2[k] >= edge_cb[r] ? r : r - 1;
                                // -inf / NaN dB: colour 0; +inf dB: last colour; all three: ToInt32 gives key 0 = bin 0      worker.js:105,111
                                // (the clamp bounds of the level scale are risky by construction, so these lanes always come here)
                                // (their cells lie behind the regular ones: the level is set so that colour index + level names them)
                                const bool dark = !(abs2[k] > 0.0), bright = abs2[k] == spjs::inf();
                                gi[k] = rck && dark ? 0 : gi[k];
                                lev = rck ? (dark ? cell_sp0 : bright ? cell_sp0 + 1 - gi[k] : l) : lev;
                            }
                            cell[k] = lev;
                        }
                    }
                    // the merged cell's byte offset, 4 * (colour index + level), as ONE instruction (left to the compiler it becomes an
                    // add on one side of the branch above and a shift on the other)
#pragma unroll
                    for (int k = 0; k < EB; k++) asm("v_add_lshl_u32 %0, %1, %2, 2" : "=v"(cell4[k]) : "v"(gi[k]), "v"(cell[k]));
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        const int e = EB * q + k;                 // compile-time after unrolling
                        if constexpr (TILE_BYTES) {
                            // one ds_write_b8 per bin (base + immediate): packing four indices into a dword first costs three
                            // v_lshl_or_b32 per dword, and every VALU instruction costs what an f64 operation costs; the LDS pipe has room
                            asm volatile("ds_write_b8 %0, %1 offset:%2" ::"v"(trow_addr), "v"(gi[k]), "n"(e) : "memory");
                        } else {
                            tile_word = (e & 3) == 0 ? (uint32_t)gi[k] : tile_word | ((uint32_t)gi[k] << (8 * (e & 3)));
                            if ((e & 3) == 3) trow[e >> 2] = tile_word;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < EB; k++) {
                        lds_count(kOffCells, cell4[k]);
                    }
                }
                const double mn = min_raw(min_raw(mn4[0], mn4[1]), min_raw(mn4[2], mn4[3]));
                const double mx = max_raw(max_raw(mx4[0], mx4[1]), max_raw(mx4[2], mx4[3]));
                unsigned long long *slot = s_mm + 2 * (((LATE_SIDE ? gpar : 0) * group_frames + fr) * MMS + (tl & (MMS - 1)));
                atomicMin(slot, (unsigned long long)__double_as_longlong(mn));
                atomicMax(slot + 1, (unsigned long long)__double_as_longlong(mx));
            }
#ifdef SP_ABS2_DEFAULT
#undef SP_ABS2
#undef SP_ABS2_DEFAULT
#endif
