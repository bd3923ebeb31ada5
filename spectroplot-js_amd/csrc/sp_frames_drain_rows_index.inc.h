// Frame-loop fragment (k_frames_index): the body of the drain_rows lambda of an INDEXED image - one colour-index byte per pixel, the
// tile byte itself - behind the fetch of the image's pointer and shape.  No LUT read, a quarter of the RGBA write-out's store bytes.
// Expects in scope what sp_frames_drain_rows.inc.h expects.  nt_rows is not used: the row pieces are never whole 128-byte lines here, and
// measured non-temporal 16-byte pieces write 2.3 ... 4.1 x the image at n = 1024 and are slower at every size tried.
        if (img) {
            if (!img_waterfall) {
                // spectrogram: image is n rows x width columns of BYTES; row y holds bin (n/2 - y) mod n               worker.js:90,117
                // The tile keeps a frame as the epilogue leaves it: 16 bytes per thread, byte e = bin tl + e*T.  A write-out item is one
                // of a thread's four dwords (bins tl + (4*e4 + j)*T, j = 0..3) of `pf` consecutive frames - 16, or the whole group where
                // it has 4 or 8: each quad of frames is transposed byte-wise (8 v_perm_b32), which gives `pf` consecutive pixels in each
                // of four rows: four 16-byte stores (four dword stores per quad where the group has 4 or 8 frames).  Item order (e4,
                // piece & 1, thread, piece >> 1): a wave's dword reads are conflict-free (tile pitch = 1 dword mod 8: 16 frames on are 16
                // banks on), and the two 16-byte pieces a 32-frame group gives a row sit in lanes 4 apart of the same store instruction.
                const int pf = fcount < 16 ? fcount : 16;           // a power of two (launch_frames)
                const int lpf = 31 - __builtin_clz((unsigned)pf);
                const int pieces = fcount >> lpf;                   // per row: a power of two
                const int two = pieces >= 2 ? 1 : 0;
                const int items = (N / 4) * pieces;
                for (int it = dt + part * dthreads; it < items; it += nparts * dthreads) {
                    const int e4 = it & 3;
                    int r = it >> 2;
                    const int plo = r & two;
                    r >>= two;
                    const int tq = r & (T - 1);                     // thread of the frame
                    const int fa = f0 + ((((r / T) << two) | plo) << lpf);
                    const int xa = x0 + fa;
                    if (xa >= SP_X_END) continue;
                    const uint8_t *const src = s_tile + __umul24((unsigned)fa, (unsigned)tile_pitch) + tq * 16 + e4 * 4;
                    const unsigned y0 = (unsigned)(N / 2 - (tq + 4 * e4 * T)) & (N - 1);
                    // v_perm_b32: selector byte s < 4 takes byte s of the second operand, 4 <= s < 8 byte s - 4 of the first
#define SP_TRANSPOSE_QUAD(q, o0, o1, o2, o3)                                                                                          \
    {                                                                                                                                 \
        const uint32_t fa0 = *(const uint32_t *)(src + (4 * (q) + 0) * tile_pitch), fa1 = *(const uint32_t *)(src + (4 * (q) + 1) * tile_pitch); \
        const uint32_t fa2 = *(const uint32_t *)(src + (4 * (q) + 2) * tile_pitch), fa3 = *(const uint32_t *)(src + (4 * (q) + 3) * tile_pitch); \
        const uint32_t lo01 = __builtin_amdgcn_perm(fa1, fa0, 0x05010400u), hi01 = __builtin_amdgcn_perm(fa1, fa0, 0x07030602u);     \
        const uint32_t lo23 = __builtin_amdgcn_perm(fa3, fa2, 0x05010400u), hi23 = __builtin_amdgcn_perm(fa3, fa2, 0x07030602u);     \
        o0 = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);                                                                          \
        o1 = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);                                                                          \
        o2 = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);                                                                          \
        o3 = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);                                                                          \
    }
                    if (img_fast && pf == 16) {
                        // rows and pieces are 16-byte aligned (base, width, the launch's first frame and its end are multiples of 16)
                        // and the image is below 4 GiB: 32-bit offsets from the uniform base, no per-store checks
                        uint32_t o[4][4];                           // o[j][q]: row j's pixels of frames 4q .. 4q+3
#pragma unroll
                        for (int q = 0; q < 4; q++) SP_TRANSPOSE_QUAD(q, o[0][q], o[1][q], o[2][q], o[3][q])
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const unsigned y = (y0 - (unsigned)(j * T)) & (N - 1);
                            store16_at_index(img, __umul24(y, (unsigned)img_width) + (unsigned)xa, o[j][0], o[j][1], o[j][2], o[j][3]);
                        }
                        continue;
                    }
                    // groups of 4 or 8 frames, and every image the fast path does not take: quad by quad, a dword per row where the
                    // fast path's conditions hold or the four pixels exist and lie aligned, else byte by byte
                    for (int q = 0; q < (pf >> 2); q++) {
                        uint32_t o[4];
                        SP_TRANSPOSE_QUAD(q, o[0], o[1], o[2], o[3])
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const unsigned y = (y0 - (unsigned)(j * T)) & (N - 1);
                            uint8_t *const dst = img + (size_t)y * (size_t)img_width + (size_t)(xa + 4 * q);
                            if (img_fast || (xa + 4 * q + 3 < SP_X_END && ((size_t)dst & 3) == 0)) {
                                *(uint32_t *)dst = o[j];
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; k++)
                                    if (xa + 4 * q + k < SP_X_END) dst[k] = (uint8_t)(o[j] >> (8 * k));
                            }
                        }
                    }
#undef SP_TRANSPOSE_QUAD
                }
            } else {
                // waterfall: image is width rows x n columns of bytes; frame x is row width-1-x, bin i is column (i + n/2 - 1) mod n
                // An item is one dword of the tile - the colour bytes of bins t + (4*e4 + j)*T, j = 0..3, of one frame - read once and
                // stored as four bytes T columns apart; consecutive lanes take consecutive t, so each of a wave's four store
                // instructions covers 64 consecutive bytes of an image row.
                // (Unlike the spectrogram items these tile reads are NOT conflict-free: consecutive lanes read dwords 16 bytes apart, four
                // lanes per bank, and every store is a byte store.  The scheme in which a lane owns 16 consecutive columns has not been
                // built; DESIGN.md section 13 records the waterfall gain as within the noise at n = 1024.)
                const int items = fcount * (N / 4);
                for (int it = dt + part * dthreads; it < items; it += nparts * dthreads) {
                    const int tq = it % T, e4 = (it / T) & 3, f = f0 + it / (4 * T);
                    const int xa = x0 + f;
                    if (xa >= SP_X_END) continue;
                    const uint32_t gb = *(const uint32_t *)(s_tile + f * tile_pitch + tq * 16 + e4 * 4);
                    // columns (i + n/2 - 1) mod n of bins i = tq + (4*e4 + j)*T: c0 + j*T without a wrap inside an item - except for
                    // the one item per frame whose first pixel is the row's last (bin n/2): its other three start the row
                    const int c0 = (tq + 4 * e4 * T + N / 2 - 1) & (N - 1);
                    uint8_t *const row = img + (size_t)(img_width - 1 - xa) * N;
                    uint8_t *const p = row + (c0 == N - 1 ? -1 : c0);
                    row[c0] = (uint8_t)gb;
                    p[1 * T] = (uint8_t)(gb >> 8);
                    p[2 * T] = (uint8_t)(gb >> 16);
                    p[3 * T] = (uint8_t)(gb >> 24);
                }
            }
        }
