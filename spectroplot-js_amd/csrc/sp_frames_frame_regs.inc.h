// Frame-loop fragment: a frame's registers - 16 points and 16 taper values per thread.
// Expects in scope: WIN_LDS, wbase, win_reg, T.
            double re[16], im[16];
            double win[16];
            bool nonfinite = true;   // wave-uniform
#pragma unroll
            for (int e = 0; e < 16; e++) win[e] = WIN_LDS ? wbase[e * T] : win_reg[WIN_LDS ? 0 : e];
