// Frame-loop fragment: where the taper lives, how many slots a frame's extremes have, when a group's side outputs are evaluated.
// In front of the block of sp_frames_table_loads / table_stores.inc.h, behind the kernel's early request: s_win's place in the body
// matters to the compiler's order (sp_kernel_frames.h), so sp_frames_setup.inc.h cannot take these.
// Expects in scope: N, smem, lay.
    constexpr bool WIN_LDS = lds_win_in_lds(N);   // taper in LDS for n <= 1024, in registers for the whole launch above
    double *s_win = (double *)(smem + lay.off_win);
    constexpr int MMS = mm_slots(N);
    constexpr bool LATE_SIDE = late_side_outputs(N);
