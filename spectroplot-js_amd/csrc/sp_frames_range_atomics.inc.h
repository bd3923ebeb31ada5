// Histogram-flush fragment: the workgroup's share of the dBfs range goes to the reply, one fire-and-forget atomic per bound.
// Expects in scope: tid (0 or 1), out_mm (not null), s_red.
            typedef __attribute__((address_space(1))) double *GlobalF64;
            if (tid == 0) __builtin_amdgcn_global_atomic_fmin_f64((GlobalF64)&out_mm[0], s_red[0]);
            else __builtin_amdgcn_global_atomic_fmax_f64((GlobalF64)&out_mm[1], s_red[1]);
