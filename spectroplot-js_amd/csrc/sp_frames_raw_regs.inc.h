// Frame-loop fragment: the registers of a frame's raw words for the prefetching loaders (issue_raw fills them, decode_pf reads them),
// and how a group's frames map to the workgroup's slots (sp_frames_slot_deal.inc.h deals by it).
// Expects in scope: PFB, LOG2N, T, tl, fs, group_frames, FPB.
    constexpr bool PF = PFB != 0;
    const int sidx_pf = (int)(__brev((unsigned)tl) >> (32 - (LOG2N - 4)));
    const int rounds = (group_frames + FPB - 1) / FPB;
    uint32_t raw_lo[PF ? 16 : 1], raw_hi[PFB == 8 ? 16 : 1];
    int raw_back = 0;
    // n = 1024, 32-frame groups: the first / second waves of the SIMDs each take one half of a group's frames
    const bool HALVES = T == 64 && group_frames == 32;
    [[maybe_unused]] const int fs0 = HALVES ? (fs / (FPB / 2)) * (group_frames / 2) + fs % (FPB / 2) : fs;     // the slot's frame in a group's first round
