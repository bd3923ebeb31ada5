"""The launch shape of the portable ("scratch") kernels restated in Python: the workgroups of a launch (scratch_blocks, sp_api.hip),
which variant runs (scratch_wide, sp_launch.h), the radix-2 stages the four-stage variant runs between two barriers (scratch_frame,
sp_kernel_scratch.h) and the columns a workgroup serves (the `x += gridDim.x` loops of the four kernels).
tests/test_scratch_shapes_cpu.py pins workgroups() and wide() against the library's own functions (sp_debug_scratch_launch);
tests/test_scratch_shapes_gpu.py chooses its widths with them.  Test infrastructure, not a test."""
SLABS = {"image": 2, "peak": 3, "traces": 4, "power": 2}     # slabs of n doubles a workgroup owns: re, im (+ hold) (+ tmin, tmax)
MAX_N = 1 << 20                                              # SP_MAX_N
CAP_BYTES = 256 << 20                                        # all slabs of a launch
THREADS = 256                                                # kScratchThreads


def workgroups(n, slabs, frames, cu):
    """Workgroups of one launch over `frames` frames on a part with `cu` CUs."""
    return max(1, min(CAP_BYTES // (8 * slabs * n), frames, 4 * cu))


def wide(n):
    """The four-stage variant: every thread still has a 16-point item."""
    return n >= 16 * THREADS


def stage_groups(levels):
    """The stages per barrier of the four-stage variant's transform, in order: fours, then what is left."""
    return [min(4, levels - s + 1) for s in range(1, levels + 1, 4)]


def columns_of(workgroup, frames, workgroups):
    """The frames (counted from the launch's first) that workgroup `workgroup` of `workgroups` serves, in order."""
    return list(range(workgroup, frames, workgroups))
