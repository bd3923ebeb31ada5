"""The lattice of cases tests/test_index_launch_shapes_gpu.py runs through k_frames_index, built on tests/launchref.py (the launch rule
restated), and what an indexed reply must hold given the oracle's reply with an injective LUT whose R channel is the index.  Test
infrastructure, not a test."""
import launchref

# how the index image is laid so that the write-out is fast (16-byte pieces) or not: by width or by pointer
WRITEOUTS = ("fast", "w4", "fast", "w1", "p1", "p4")


def built(n, loader, ch):
    """Does k_frames_index render this variant?  (The L/R split with the generic loaders at n <= 256 is left to render_extract.)"""
    return n in launchref.SIZES and not (ch and loader == 0 and n <= 256)


def width_ok(W, writeout):
    return {"fast": W % 16 == 0, "p1": W % 16 == 0, "p4": W % 16 == 0, "w4": W % 16 != 0 and W % 4 == 0, "w1": W % 4 != 0}[writeout]


def misalign(writeout):
    return {"p1": 1, "p4": 4}.get(writeout, 0)


def choose_width(n, cu, gf, regime, writeout):
    """A width whose launch on a cu-CU part has this gf and regime, groups not a multiple of 8, and the write-out's width property."""
    lo, hi = launchref.frames_interval(n, gf, cu)
    for groups in range(2, 8 * launchref.grid_for(cu, cu) + 64):
        if groups % 8 == 0 or launchref.regime_of(groups, launchref.grid_for(groups, cu)) != regime:
            continue
        for W in range(groups * gf, (groups - 1) * gf, -1):
            if width_ok(W, writeout) and W >= lo and (hi is None or W <= hi):
                assert launchref.launch(n, 2, W, cu) == (gf, groups, launchref.grid_for(groups, cu))
                return W
    return None


def lattice():
    """One case per (n, loader): the cells (smallest gf, mixed), (smallest gf, many), (each larger gf, many) rotate over the loaders, as
    do L/R split, layout and write-out."""
    cases = []
    for ni, n in enumerate(launchref.SIZES):
        gfs = launchref.reachable_gf(n)
        cells = [(gfs[0], "mixed"), (gfs[0], "many")] + [(gf, "many") for gf in gfs[1:]]
        for i, loader in enumerate(launchref.LOADERS):
            gf, regime = cells[(i + ni) % len(cells)]
            ch = (i + ni) % 2 == 1 and built(n, loader, True)
            cases.append(dict(n=n, gf=gf, regime=regime, loader=loader, fmt=launchref.LOADER_FORMATS[loader][(i + ni) % 2], ch=ch,
                              wf=(i // 2 + ni) % 2 == 1, writeout=WRITEOUTS[(i + 2 * ni) % len(WRITEOUTS)]))
    return cases


def case_id(c):
    return "n%d_gf%d_%s_%s%s%s_%s" % (c["n"], c["gf"], c["regime"], c["fmt"], "_lr" if c["ch"] else "", "_wf" if c["wf"] else "", c["writeout"])


def expected_index(want):
    """The index image of the oracle's reply rendered with a LUT whose R channel is the index."""
    return want["rgba"].reshape(-1, 4)[:, 0].copy()
