"""Every compiled variant of the frame-loop kernels - family x LOG2N x (I/Q or L/R split) x loader - written from the rule, and the one
request that reaches each of them.  tests/test_variants_cpu.py pins the lattice against the kernels in the built objects and each
request against frames_prefetch_width; tests/test_variants_gpu.py runs one case per cell.  Test infrastructure, not a test.

The rule: k_frames is built for n = 2^6 ... 2^13, k_frames_batch for n <= 512 (frames_batch_variant_built), k_frames_peak, k_frames_traces
and k_frames_power for n = 2^6 ... 2^10, k_frames_index for n = 2^6 ... 2^13 without the L/R split through the generic loaders at
n <= 256 (frames_index_variant_built); each of them for both channel modes and the six loaders.

Every request is shaped for a part of CU CUs (sp_context_debug_set_cu_count): the smallest frames per group of its n and GROUPS groups,
the last one ragged.  launchref.deal gives the eight workgroups of that launch 3, 3, 3, 3, 3, 3, 1 and 0 groups: six of them cross two
group boundaries with the next frame's prefetch in flight, one renders the ragged last group alone.  Frames overlap with a stride of
n / 2 + 3 samples (unaligned starts); the peak family's capture is sparse (M * n samples per column)."""
import launchref
import siggen

CU = 8
GROUPS = 19
LOADERS = (0, 1, 2, 3, 4, 8)                           # the prefetching loader's sample width; 0: the generic loaders
GENERIC_FORMATS = ("CF64", "CS64", "CU64")             # 16-byte samples, in turn over the generic cells
# family: (kernel, its LOG2N)
FAMILIES = {"frames": ("k_frames", range(6, 14)), "batch": ("k_frames_batch", range(6, 10)), "peak": ("k_frames_peak", range(6, 11)),
            "traces": ("k_frames_traces", range(6, 11)), "power": ("k_frames_power", range(6, 11)), "index": ("k_frames_index", range(6, 14))}
OBJECTS = {"frames": "frames_*.o", "batch": "frames_*.o", "peak": "peak_*.o", "traces": "traces_*.o", "power": "power_*.o", "index": "index_*.o"}
COUNTS = {"frames": 96, "batch": 48, "peak": 60, "traces": 60, "power": 60, "index": 93}


def frames_batch_variant_built(n, ch, loader):
    return n <= 512


def frames_index_variant_built(n, ch, loader):
    return not (ch and loader == 0 and n <= 256)


def built(family, n, ch, loader):
    if family == "batch":
        return frames_batch_variant_built(n, ch, loader)
    if family == "index":
        return frames_index_variant_built(n, ch, loader)
    return True


def variants(family):
    """[(log2n, L/R split, loader)] of the family's compiled kernels, by the rule."""
    return [(lg, ch, p) for lg in FAMILIES[family][1] for ch in (False, True) for p in LOADERS if built(family, 1 << lg, ch, p)]


def mangled(family):
    """The start of the family's mangled kernel names (namespace spk2), up to the template arguments."""
    name = FAMILIES[family][0]
    return "_ZN4spk2%d%sI" % (len(name), name)


def lattice():
    """One cell per compiled kernel: dicts of family, n, ch, loader, fmt, wf (waterfall), fast (the 16-byte write-out, where a ragged
    width allows it) and M (peak).  The generic cells take the three 16-byte formats in turn, the others the two formats of their loader."""
    cells, generic = [], 0
    for family in FAMILIES:
        for k, (lg, ch, p) in enumerate(variants(family)):
            if p == 0:
                fmt = GENERIC_FORMATS[generic % 3]
                generic += 1
            else:
                fmt = launchref.LOADER_FORMATS[p][(k // 6 + k) % 2]
            c = dict(family=family, n=1 << lg, ch=ch, loader=p, fmt=fmt, wf=family in ("frames", "batch", "peak", "index") and (k // 2 + lg) % 2 == 1,
                     fast=(k + k // 6) % 2 == 0)
            if family == "peak":
                c["M"] = 2 + (k + lg) % 2
            cells.append(c)
    return cells


def case_id(c):
    return "%s_n%d_%s_p%d_%s" % (c["family"], c["n"], "lr" if c["ch"] else "iq", c["loader"], c["fmt"]) + ("_wf" if c["wf"] else "") \
        + ("_M%d" % c["M"] if "M" in c else "")


def gf_of(n):
    return launchref.reachable_gf(n)[0]


def width_of(c):
    """GROUPS groups of the smallest gf, the last one ragged.  Where the cell asks for the fast write-out the width is the largest such
    multiple of 4 (of 16 for the index image) - there is none at gf = 4, nor below gf = 32 for the index image: those cells write slowly."""
    gf, unit = gf_of(c["n"]), 16 if c["family"] == "index" else 4
    if c["fast"] and c["family"] in ("frames", "peak", "index") and gf > unit:
        return GROUPS * gf - unit
    return GROUPS * gf - 1


def is_fast(c):
    W = width_of(c)
    return W % (16 if c["family"] == "index" else 4) == 0


def batch_widths(n):
    """Three items: gf + 1 frames, one frame, and the rest of the GROUPS groups with a ragged last one."""
    gf = gf_of(n)
    return [gf + 1, 1, (GROUPS - 3) * gf - 1]


def hop(n):
    return n // 2 + 3


def samples_of(c, W):
    """The capture's length in samples for W frames (columns): every frame inside it, the stride exact."""
    n = c["n"]
    if W == 1:
        return n + 5
    if c["family"] == "peak":
        return n + (W - 1) * c["M"] * n + (W - 1) // 2 + 1      # a fractional stride: the last column has one sub-frame only
    return n + (W - 1) * hop(n)


def requests(c):
    """[(W, samples, nbytes)] of the cell's request - the three items of a batch cell."""
    sw = siggen.SAMPLE_WIDTH[c["fmt"]]
    widths = batch_widths(c["n"]) if c["family"] == "batch" else [width_of(c)]
    return [(W, samples_of(c, W), samples_of(c, W) * sw) for W in widths]


# ---------------------------------------------------------------------------------- the loader rule (frames_prefetch_width) restated
def frame_start(samples_f, n, W, x):
    return int(0.5 + (samples_f - n) / (W - 1) * x) if W > 1 else 0


def prefetch_width(fmt, n, nbytes, W):
    """frames_prefetch_width over spgeo::geometry: the sample width where every frame lies inside the capture and the width is 1, 2, 3, 4
    or 8 bytes - with 3-byte samples only if the last frame starts past sample 0 - else 0."""
    sw = siggen.SAMPLE_WIDTH[fmt]
    samples_f = nbytes / sw
    if W == 1:
        in_bounds = n * sw <= nbytes
    else:
        stride = (samples_f - n) / (W - 1)
        in_bounds = stride >= 0.0 and (frame_start(samples_f, n, W, W - 1) + n) * sw <= nbytes
    p = sw if in_bounds and (sw <= 4 or sw == 8) else 0
    if p == 3 and not (W >= 2 and frame_start(samples_f, n, W, W - 1) >= 1):
        return 0
    return p


def batch_launches(c):
    """The launch of each item of a batch cell: 0 prefetching, 1 generic (the single frame of 3-byte samples starts at sample 0)."""
    return [0 if prefetch_width(c["fmt"], c["n"], nb, W) else 1 for W, _, nb in requests(c)]
