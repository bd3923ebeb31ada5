// Frame-loop fragment: the epilogue's constants, and the registers they are pinned to.
// Expects in scope: LOG2N, CH, PFB, a, cmax.
    // epilogue constants (sp_host.cpp build_thresholds): t = a + b*log2(|X|^2), already lowered by the margin
    const float g_a = a.g2_a, g_b = a.g2_b, g_m = a.g2_m;
    const float c_a = a.c2_a, c_b = a.c2_b, c_m = a.c2_m, c_lo = a.c2_lo, c_hi = a.c2_hi;
    const float thr = fminf(a.g2_thr, a.c2_thr);
    // A VALU instruction reads ONE scalar register: with both coefficients of a scale in SGPRs the compiler copies one of them into a
    // VGPR again for every batch of bins (24 v_mov per frame).  The addends and the upper clamp bound live in VGPRs instead.
    // (n <= 1024, where registers are left: above, the loop sits at the 256-VGPR limit and three more spill)
    float g_a_v = g_a, c_a_v = c_a, c_hi_v = c_hi;
    constexpr bool COEF_VGPR = LOG2N <= 10 && !CH && !(PFB == 8 && LOG2N < 9);
    if constexpr (COEF_VGPR) asm volatile("" : "+v"(g_a_v), "+v"(c_a_v), "+v"(c_hi_v));
    // ... and, at n = 1024, both scales of a batch's two bins as packed pairs (below that size the loop measures the same with and
    // without, and the launch-bound config 1 pays 1 % for the longer set-up: profiles/r05_experiments.txt)
    constexpr bool PK_SCALES = COEF_VGPR && LOG2N == 10;
    [[maybe_unused]] f32x2 g_b2 = {g_b, g_b}, g_a2 = {g_a, g_a}, c_b2 = {c_b, c_b}, c_a2 = {c_a, c_a};
    if constexpr (PK_SCALES) asm volatile("" : "+v"(g_b2), "+v"(g_a2), "+v"(c_b2), "+v"(c_a2));
    // clamp bounds of the colour value: clipped pixels sit in the middle of the first / last step, far from the risky zone
    const float g_lo = 0.5f, g_hi = (float)cmax + 0.5f;
    const int cell_sp0 = a.cells - 2;   // -inf / NaN dB (colour 0, bin 0), +inf dB is the next one (last colour, bin 0)
