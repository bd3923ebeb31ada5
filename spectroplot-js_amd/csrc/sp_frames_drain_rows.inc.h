// Frame-loop fragment: the body of the drain_rows lambda behind the fetch of the image's pointer and shape.
// Expects in scope: x0, part, nparts, f0, fcount, dt, dthreads, nt_rows, img, img_width, img_waterfall, img_fast, s_tile, tile_pitch,
// N, T; SP_X_END: the frame count of the request or item.
        if (img) {
            if (!img_waterfall) {
                // spectrogram: image is n rows x width columns; row y holds bin (n/2 - y) mod n            worker.js:90,117
                // The tile keeps a frame as the epilogue leaves it: 16 bytes per thread, byte e = bin tl + e*T.  A write-out item is
                // one of a thread's four dwords (bins tl + (4*e4 + j)*T, j = 0..3) of 4 consecutive frames: four 16-byte stores in four
                // rows; the items of a row segment (8 frame quads) sit in lanes 4 apart, and a wave's dword reads are conflict-free
                // (tile pitch = 1 dword mod 8).
                const int quads = fcount / 4;                     // a power of two (launch_frames)
                const int lq = 31 - __builtin_clz((unsigned)quads);
                const int items = (N / 4) * quads;
                for (int it0 = dt + part * 2 * dthreads; it0 < items; it0 += nparts * 2 * dthreads) {
                    uint32_t gb[2][4];
                    int i0v[2], xav[2];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int it = it0 + u * dthreads;
                        const int itc = it < items ? it : it0;
                        const int e4 = itc & 3, fq = (itc >> 2) & (quads - 1), tq = (itc >> 2) >> lq;   // tq: thread of the frame
                        i0v[u] = tq + 4 * e4 * T;
                        xav[u] = it < items ? x0 + f0 + fq * 4 : SP_X_END;
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            gb[u][k] = *(const uint32_t *)(s_tile + __umul24((unsigned)(f0 + fq * 4), (unsigned)tile_pitch) + k * tile_pitch + tq * 16 + e4 * 4);
                    }
                    uint32_t px[2][4][4];
                    const auto lut_at = [&](unsigned off4) { return lds_read_u32(kOffLut, off4); };
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            px[u][0][k] = lut_at(byte_times4<0>(gb[u][k]));
                            px[u][1][k] = lut_at(byte_times4<1>(gb[u][k]));
                            px[u][2][k] = lut_at(byte_times4<2>(gb[u][k]));
                            px[u][3][k] = lut_at(byte_times4<3>(gb[u][k]));
                        }
                    if (img_fast) {
                        // rows are 16-byte aligned, the width is a multiple of 4 and the image is below 4 GiB: 32-bit offsets from the
                        // uniform base (24-bit multiplies), no per-store checks
#pragma unroll
                        for (int u = 0; u < 2; u++) {
                            const int xa = xav[u];
                            if (xa >= SP_X_END) continue;
                            const unsigned y0 = (unsigned)(N / 2 - i0v[u]) & (N - 1);
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const unsigned y = (y0 - (unsigned)(j * T)) & (N - 1);
                                const unsigned off = (__umul24(y, (unsigned)img_width) + (unsigned)xa) * 4u;
                                // written once, never read by this kernel: non-temporal where a group's row segments are whole
                                // 128-byte lines, so that the image does not displace the capture's lines in L2 (measured: 2.5 % of the
                                // kernel at n = 1024); shorter segments (large n) are pieces of lines that L2 has to merge with the
                                // neighbouring groups' pieces (non-temporal there doubled the HBM traffic)
                                store16_at(img, off, px[u][j][0], px[u][j][1], px[u][j][2], px[u][j][3], nt_rows);
                            }
                        }
                        continue;
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int xa = xav[u];
                        if (xa >= SP_X_END) continue;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int i = i0v[u] + j * T;
                            const int y = (N / 2 - i) & (N - 1);
                            uint8_t *dst = img + ((size_t)y * (size_t)img_width + (size_t)xa) * 4;
                            if (xa + 3 < SP_X_END && (((size_t)dst & 15) == 0)) {
                                *(uint4 *)dst = make_uint4(px[u][j][0], px[u][j][1], px[u][j][2], px[u][j][3]);
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; k++)
                                    if (xa + k < SP_X_END) ((uint32_t *)dst)[k] = px[u][j][k];
                            }
                        }
                    }
                }
            } else {
                // waterfall: image is width rows x n columns; frame x is row width-1-x, bin i is column (i + n/2 - 1) mod n
                // An item is one dword of the tile - the colour bytes of bins t + (4*e4 + j)*T, j = 0..3, of one frame - read once and
                // stored as four pixels T columns apart; consecutive lanes take consecutive t, so each of a wave's four store
                // instructions covers 64 consecutive pixels of an image row.  (Four consecutive COLUMNS per item - one 16-byte store,
                // but four byte reads from four tile columns - took 6 ... 14 % more of the kernel than the spectrogram layout.)
                const int items = fcount * (N / 4);
                for (int it = dt + part * dthreads; it < items; it += nparts * dthreads) {
                    const int tq = it % T, e4 = (it / T) & 3, f = f0 + it / (4 * T);
                    const int xa = x0 + f;
                    if (xa >= SP_X_END) continue;
                    const uint32_t gb = *(const uint32_t *)(s_tile + f * tile_pitch + tq * 16 + e4 * 4);
                    // columns (i + n/2 - 1) mod n of bins i = tq + (4*e4 + j)*T: c0 + j*T without a wrap inside an item - except for
                    // the one item per frame whose first pixel is the row's last (bin n/2): its other three start the row
                    const int c0 = (tq + 4 * e4 * T + N / 2 - 1) & (N - 1);
                    uint32_t *const row = (uint32_t *)(img + (size_t)(img_width - 1 - xa) * N * 4);
                    uint32_t *const p = row + (c0 == N - 1 ? -1 : c0);
                    const auto lut_at = [&](unsigned off4) { return lds_read_u32(kOffLut, off4); };
                    __builtin_nontemporal_store(lut_at(byte_times4<0>(gb)), row + c0);
                    __builtin_nontemporal_store(lut_at(byte_times4<1>(gb)), p + 1 * T);
                    __builtin_nontemporal_store(lut_at(byte_times4<2>(gb)), p + 2 * T);
                    __builtin_nontemporal_store(lut_at(byte_times4<3>(gb)), p + 3 * T);
                }
            }
        }
