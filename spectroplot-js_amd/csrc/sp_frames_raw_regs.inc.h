// Frame-loop fragment: the registers of a frame's raw words for the prefetching loaders (issue_raw fills them, decode_pf reads them).
// Expects in scope: PFB, LOG2N, tl, group_frames, FPB.
    constexpr bool PF = PFB != 0;
    const int sidx_pf = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
    const int rounds = (group_frames + FPB - 1) / FPB;
    uint32_t raw_lo[PF ? 16 : 1], raw_hi[PFB == 8 ? 16 : 1];
    int raw_back = 0;
