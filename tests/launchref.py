"""The launch rule of the frame-loop kernels (frames_launch_rule, sp_kernel_frames.h) and the deal of groups to workgroups
(sp_frames_setup.inc.h) restated in Python, a chooser of image widths that reach a wanted launch shape, and the lattice of cases
tests/test_launch_shapes_gpu.py runs.  tests/test_launch_shapes_cpu.py pins the restatement against the library's own rule
(sp_debug_frames_launch).  Test infrastructure, not a test.

Names: gf = frames per group; a launch's `regime` says how many groups its workgroups run:
    one    fewer groups than workgroups: no workgroup runs a second group, nothing is drained inside the loop
    mixed  some workgroups run 2 groups, the others 1
    many   every workgroup runs at least 3 groups: both parities of the per-group buffers are used again
"""
THREADS = 512                                         # kFrameThreads: one workgroup, 16 points per thread
SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]   # frames_kernel_supports
PEAK_SIZES = [n for n in SIZES if n <= 1024]          # frames_peak_supports
BATCH_SIZES = [n for n in SIZES if n <= 512]          # kBatchMaxLog2N
MAX_LUT = 256                                         # kLdsMaxLut
REGIMES = ("one", "mixed", "many")


def group_frames_for(n, want):
    fpb = THREADS * 16 // n
    unit = fpb
    while unit % 4:
        unit *= 2
    cap = min((65536 if n >= 2048 else 32768) // n, want)
    return max(cap // unit * unit, unit)


def wanted(total, cu):
    want = 32
    while want > 4 and (total + want - 1) // want < 2 * cu:
        want >>= 1
    return want


def batch_gf(n, total, cu):
    """frames_group_frames: frames per group of a launch over `total` frames (a batch: the frames of all its items)."""
    return group_frames_for(n, wanted(total, cu))


def grid_for(groups, cu):
    return (min(groups, cu) + 7) // 8 * 8


def launch(n, lut_len, count, cu, gf_fixed=0):
    """(gf, groups, grid) of frames_launch_rule for `count` frames, or for `count` groups of gf_fixed frames; None where the rule refuses."""
    if n not in SIZES or not 2 <= lut_len <= MAX_LUT:
        return None
    gf = gf_fixed if gf_fixed > 0 else batch_gf(n, count, cu)
    if gf & (gf - 1):
        return None
    groups = count if gf_fixed > 0 else (count + gf - 1) // gf
    return gf, groups, grid_for(groups, cu)


def reachable_gf(n):
    """Every gf a launch over some number of frames can have at this n, ascending (the same set for every CU count)."""
    return sorted({group_frames_for(n, w) for w in (4, 8, 16, 32)})


def gf_pairs(sizes=SIZES):
    return [(n, gf) for n in sizes for gf in reachable_gf(n)]


def frames_interval(n, gf, cu):
    """[lo, hi] of the frame counts whose launch has this gf (hi None: no upper end); None if gf is not reachable."""
    wants = [w for w in (4, 8, 16, 32) if group_frames_for(n, w) == gf]
    if not wants:
        return None
    lo = 1 if wants[0] == 4 else wants[0] * (2 * cu - 1) + 1
    hi = None if wants[-1] == 32 else 2 * wants[-1] * (2 * cu - 1)
    return lo, hi


def rounds(n, gf):
    fpb = THREADS * 16 // n
    return (gf + fpb - 1) // fpb


def halves(n, gf):
    """The n = 1024 frame-to-slot mapping of 32-frame groups (HALVES in the kernels)."""
    return n == 1024 and gf == 32


def deal(groups, grid):
    """Groups per workgroup, in workgroup order: workgroup b takes groups (b & 7) * chunk + (b >> 3) + k * (grid >> 3) below the end of
    its XCD's chunk."""
    per_xcd, chunk = grid >> 3, (groups + 7) >> 3
    out = []
    for b in range(grid):
        xcd, lane = b & 7, b >> 3
        first, end = xcd * chunk + lane, min(groups, (xcd + 1) * chunk)
        out.append(0 if first >= end else (end - first + per_xcd - 1) // per_xcd)
    return out


def deal_minmax(groups, grid):
    d = deal(groups, grid)
    return min(d), max(d)


def regime_of(groups, grid):
    if groups < grid:
        return "one"
    d = set(deal(groups, grid))
    if d == {1, 2}:
        return "mixed"
    if min(d) >= 3:
        return "many"
    return None


def choose_width(n, cu, gf, regime, w4, ragged_group=True):
    """A width W (frames, or columns of a peak request) whose launch on a cu-CU part has this gf and regime, with groups not a multiple
    of 8, W % 4 == 0 exactly if w4, and W % gf != 0 if ragged_group (impossible with w4 at gf = 4); None if the rule allows none."""
    iv = frames_interval(n, gf, cu)
    if iv is None or (ragged_group and w4 and gf == 4):
        return None
    lo, hi = iv
    grid_full = grid_for(cu, cu)
    spans = {"one": (max(2, cu * 5 // 8), grid_full), "mixed": (cu + max(1, cu // 8), 2 * grid_full + 1),
             "many": (3 * cu, 8 * grid_full + 64)}[regime]
    for groups in range(*spans):
        if groups % 8 == 0 or regime_of(groups, grid_for(groups, cu)) != regime:
            continue
        for W in range(groups * gf - (1 if ragged_group else 0), (groups - 1) * gf, -1):
            if (W % 4 == 0) == bool(w4) and W >= lo and (hi is None or W <= hi):
                assert launch(n, 2, W, cu) == (gf, groups, grid_for(groups, cu))
                return W
    return None


def unreachable_by_rule(cu, sizes=SIZES):
    """The (n, gf, regime) combinations no width reaches on a part of 8 CUs or more, from the rule alone.  G = grid_for(cu, cu) is the
    grid of every launch with cu groups or more: cu rounded up to the 8 XCDs.
    * A gf above the smallest is only chosen once it gives 2 * cu groups or more: never fewer groups than workgroups.  Where G = cu
      every XCD chunk then holds 2 * cu / 8 groups or more and no workgroup is left with one group while none has three; where G > cu
      2 * G - 1 groups (2 * cu or more) give every workgroup two but the last one of the last XCD: `mixed` is in reach.
    * A gf below the largest is given up beyond 2 * (2 * cu - 1) groups.  With a group count that is no multiple of 8 the last XCD's
      chunk is short, so three groups for every workgroup take 8 * (3 * G / 8 + 1) - 1 = 3 * G + 7 groups: out of reach while
      4 * cu - 2 < 3 * G + 7, i.e. on 8 CUs, and on 12 or 20, whose grids are rounded up by 4."""
    assert cu >= 8
    grid_full = grid_for(cu, cu)
    out = [(n, gf, r) for n in sizes for gf in reachable_gf(n)[1:] for r in (("one", "mixed") if grid_full == cu else ("one",))]
    if 4 * cu - 2 < 3 * grid_full + 7:
        out += [(n, gf, "many") for n in sizes for gf in reachable_gf(n)[:-1]]
    return sorted(out)


def reachable(cases, cu):
    """The cases of a lattice whose (n, gf, regime) cell some width reaches on a cu-CU part: all of them but on 8 and 20 CUs (of the
    counts the tests run), where the `many` cells of every gf below the largest are out of reach."""
    out_of_reach = set(unreachable_by_rule(cu))
    return [c for c in cases if (c["n"], c["gf"], c["regime"]) not in out_of_reach]


# ------------------------------------------------------------------------------------------------------------------ the lattice
# Loaders: the prefetching loader's sample width, 0 = the generic loaders (through a 16-byte format).
LOADER_FORMATS = {1: ("CU4", "CS4"), 2: ("CU8", "CS8"), 3: ("CS12", "CU12"), 4: ("CS16", "CU16"), 8: ("CF32", "CS32"), 0: ("CF64", "CS64")}
LOADERS = (0, 8, 4, 3, 2, 1)
STRIDES = ("overlap", "exact", "sparse")


def _regimes(n, gf):
    return REGIMES if gf == reachable_gf(n)[0] else ("many",)


def frames_lattice():
    """The k_frames cases, the same cells on every part (the widths follow the CU count): dicts of n, gf, regime, loader, fmt, ch (L/R
    split), wf (waterfall), fast (rgba_fast), slow_by ("width": W % 4 != 0, "pointer": image 4 bytes off 16-byte alignment), stride.
    Every (n, gf, loader) occurs once - at least max(2, gfs of n) cases per (n, loader), so that every (n, loader, L/R) occurs too -
    and the other axes rotate; test_launch_shapes_cpu.py asserts what the rotation covers.  Two more cases render a CU8 capture with an
    odd byte count (the last frame ends past the capture: not in bounds, generic loaders) at 3 or more groups per workgroup."""
    cases = []
    for n in SIZES:
        gfs = reachable_gf(n)
        per_gf = {gf: 0 for gf in gfs}
        for li, loader in enumerate(LOADERS):
            slots = max(2, len(gfs))
            for s in range(slots):
                gf = gfs[(s + li) % len(gfs)]
                i = per_gf[gf]
                per_gf[gf] += 1
                regs = _regimes(n, gf)
                fast = (i // 2) % 2 == 0
                cases.append(dict(n=n, gf=gf, regime=regs[i % len(regs)], loader=loader, fmt=LOADER_FORMATS[loader][s % 2], ch=s % 2 == 1,
                                  wf=((i + 1) // 2) % 2 == 1, fast=fast, slow_by=None if fast else ("width", "pointer")[(i // 4 + i) % 2],
                                  stride=STRIDES[(i + i // 3) % 3], oob=False))
    for n, gf in ((256, 32), (1024, 32)):
        cases.append(dict(n=n, gf=gf, regime="many", loader=0, fmt="CU8", ch=n == 1024, wf=n == 256, fast=n == 256, slow_by=None if n == 256 else "width",
                          stride="overlap", oob=True))
    return cases


def peak_lattice():
    """The k_frames_peak cases: at every n = 64 ... 1024 one case per loader; the (gf, regime) cells of that n - the smallest gf in
    `mixed` and `many`, a larger one in `many` - rotate over them, as do L/R split, layout, M in {2, 3} and rgba_fast."""
    cases = []
    for n in PEAK_SIZES:
        gfs = reachable_gf(n)
        cells = [(gfs[0], "mixed"), (gfs[0], "many")] + [(gf, "many") for gf in gfs[1:]]
        for i, loader in enumerate(LOADERS):
            gf, regime = cells[i % len(cells)]
            fast = i % 3 != 2
            cases.append(dict(n=n, gf=gf, regime=regime, loader=loader, fmt=LOADER_FORMATS[loader][(i + n // 64) % 2], M=2 + (i + n // 64) % 2,
                              ch=(i + (n >= 256)) % 2 == 1, wf=(i // 2 + (n >= 512)) % 2 == 1, fast=fast,
                              slow_by=None if fast else ("width", "pointer")[(i // 3) % 2]))
    return cases


def batch_lattice():
    """One batch per (n = 64 ... 512, reachable gf)."""
    return [dict(n=n, gf=gf, fmt=("CU8", "CS16", "CF32", "CS12", "CS8")[k % 5], ch=k % 2 == 1, wf=k % 3 == 1)
            for k, (n, gf) in enumerate(gf_pairs(BATCH_SIZES))]


def batch_widths(n, gf, cu):
    """Item widths of the batch that reaches (n, gf) on a cu-CU part: 1, gf - 1, gf, gf + 1, an empty item and two large ragged ones
    (the second rendered by the generic loaders), 3 * cu groups or more in all and a total inside gf's interval."""
    lo, hi = frames_interval(n, gf, cu)
    small = [1, gf - 1, gf, gf + 1, 0]
    big = max(3 * cu * gf + 5 * gf + 3, lo + 2 * gf)
    if hi is not None:
        big = min(big, hi - 4 * gf)
    a = big * 2 // 3 | 1
    widths = small + [a, big - a]
    assert batch_gf(n, sum(widths), cu) == gf, (n, gf, cu, widths)
    return widths


def case_id(c):
    return "n%d_gf%d_%s_%s" % (c["n"], c["gf"], c.get("regime", "batch"), c["fmt"]) + ("_lr" if c["ch"] else "") + ("_wf" if c["wf"] else "") \
        + ("" if c.get("fast", True) else "_slow" + c["slow_by"]) + ("_M%d" % c["M"] if "M" in c else "") + ("_oob" if c.get("oob") else "")
