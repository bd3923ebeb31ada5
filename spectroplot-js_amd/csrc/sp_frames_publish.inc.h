// Frame-loop fragment (k_frames, k_frames_peak): the request's number, behind the reply clear of sp_frames_reply_clear.inc.h.
// Expects in scope: g, r, tid, a.
            // Workgroup 0's first wave publishes the request's number once its clearing stores have landed: after its first frame (group 0
            // is workgroup 0's, and every slot has a frame in a group's first round), when they long have.
            if (g == 0 && r == 0 && a.first && __builtin_amdgcn_readfirstlane(tid >> 6) == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const LateArgs la = late_args();
                if (tid == 0) __hip_atomic_store(la->flag, la->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
