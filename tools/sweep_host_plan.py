#!/usr/bin/env python3
"""Compares the host planning arithmetic of two builds of the library, word for word, over a fixed-seed sweep of request shapes:
sp_debug_upload_plan (want_image 0 and 1), sp_debug_batch_plan and sp_peak_subframes.  No device is used.  The first library is the
reference (build it from the parent commit in a `git worktree`), the second the one under test; status codes are compared too.
    tools/sweep_host_plan.py PARENT/lib/libspectroplot_hip.so spectroplot-js_amd/lib/libspectroplot_hip.so [shapes]
Prints the number of shapes compared and the first mismatch; exit status 1 on a mismatch."""
import ctypes as C
import random
import sys

FORMATS = ["CU4", "CS4", "CU8", "CS8", "CU12", "CS12", "CU16", "CS16", "CU32", "CS32", "CU64", "CS64", "CF32", "CF64"]
CAP = 1 << 16


def load(path):
    L = C.CDLL(path, mode=getattr(C, "RTLD_LOCAL", 0))
    L.sp_format_parse.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sp_debug_upload_plan.argtypes = [C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_size_t)]
    L.sp_debug_batch_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_int32,
                                      C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_size_t)]
    L.sp_peak_subframes.argtypes = [C.c_int32, C.c_int32, C.c_size_t, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.buf = (C.c_int64 * CAP)()
    return L


def upload(L, fid, n, nbytes, width, want):
    used = C.c_size_t(0)
    rc = L.sp_debug_upload_plan(fid, n, nbytes, width, want, L.buf, CAP, C.byref(used))
    return (rc, used.value, tuple(L.buf[:min(used.value, CAP)]) if rc == 0 else ())


def peak(L, fid, n, nbytes, width):
    m, last = C.c_int32(-7), C.c_int32(-7)
    rc = L.sp_peak_subframes(fid, n, nbytes, width, C.byref(m), C.byref(last))
    return (rc, m.value, last.value)


def batch(L, fid, n, lut_len, cus, items):
    nb = (C.c_size_t * len(items))(*[i[0] for i in items])
    wd = (C.c_int32 * len(items))(*[i[1] for i in items])
    used = C.c_size_t(0)
    rc = L.sp_debug_batch_plan(fid, n, lut_len, cus, nb, wd, len(items), L.buf, CAP, C.byref(used))
    return (rc, used.value, tuple(L.buf[:min(used.value, CAP)]) if rc == 0 else ())


def shapes(rng, sw_of, total):
    """(format id, n, nbytes, width): the corners by construction, then random fill."""
    out = []
    three = [i for i in range(len(FORMATS)) if sw_of[i] == 3]

    def add(fid, n, samples, width, odd=0):
        out.append((fid, n, max(0, samples) * sw_of[fid] + odd, width))

    for fid in range(len(FORMATS)):
        for n in (2, 64, 256, 1024, 8192):
            for width in (0, 1, 2, 3, 4, 33, 1024, 1056):
                for samples in (0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1):          # shorter than a frame, one frame, two
                    add(fid, n, samples, width)
                if width < 2:
                    continue
                for mult_num, mult_den in ((1, 2), (1, 1), (3, 2), (2, 1), (5, 2), (3, 1), (7, 1)):   # stride = n * num / den exactly ...
                    base = n + (n * mult_num * (width - 1)) // mult_den
                    for d in (-2, -1, 0, 1, 2, width - 1, -(width - 1)):                        # ... and just below / above it
                        add(fid, n, base + d, width)
    # sample counts just under 2^31 - n; last-frame positions on either side of 2147483000 and 2147483647
    for fid in list(range(len(FORMATS))) + three * 3:
        for n in (2, 64, 1024, 4096):
            for width in (1, 2, 3, 64, 1000, 1024, 4096):
                for d in range(-3, 4):
                    add(fid, n, (1 << 31) - n + d, width)
                    add(fid, n, 2147483000 + n + d, width)       # last start = ~~(0.5 + samples - n)
                    add(fid, n, 2147483647 + n + d, width)
                    add(fid, n, 2147483000 + d, width)
                    add(fid, n, 2147483647 + d, width)
    while len(out) < total:
        fid = rng.choice(three) if rng.random() < 0.2 else rng.randrange(len(FORMATS))
        n = 1 << rng.randrange(1, 14)
        width = rng.choice((0, 1, 2)) if rng.random() < 0.05 else int(2 ** rng.uniform(1, 13.5))
        kind = rng.random()
        if kind < 0.35:      # strides around n .. 3n
            stride = n * rng.choice((1.0, 1.0 + 1e-6, 1.5, 2.0 - 1e-6, 2.0, 2.0 + 1e-6, rng.uniform(0.9, 3.2)))
            samples = int(n + stride * max(width - 1, 0)) + rng.randrange(-2, 3)
        elif kind < 0.7:     # sparse: long captures at screen-wide widths
            samples = int(n + n * rng.uniform(2, 400) * max(width - 1, 1)) + rng.randrange(-2, 3)
        elif kind < 0.8:     # dense / overlapping frames, captures shorter than the frames ask for
            samples = int(n * rng.uniform(0, 1.2) * max(width, 1) * rng.random())
        else:                # near the int32 limits
            samples = rng.choice((2147483000, 2147483647, 1 << 31)) + rng.randrange(-2 * n, 2 * n)
        add(fid, n, min(samples, (1 << 32)), width, odd=rng.randrange(sw_of[fid]) if rng.random() < 0.1 else 0)
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    ref, new = load(argv[1]), load(argv[2])
    total = int(argv[3]) if len(argv) > 3 else 24000
    sw_of = []
    for name in FORMATS:
        fid, sw = C.c_int32(0), C.c_int32(0)
        ref.sp_format_parse(name.encode(), C.byref(fid), C.byref(sw))
        assert fid.value == len(sw_of)
        sw_of.append(sw.value)
    rng = random.Random(20261017)
    todo = shapes(rng, sw_of, total)
    compared = {"upload": 0, "peak": 0, "batch": 0}
    for k, (fid, n, nbytes, width) in enumerate(todo):
        calls = [("upload want_image=0", upload, (fid, n, nbytes, width, 0)), ("upload want_image=1", upload, (fid, n, nbytes, width, 1)),
                 ("peak", peak, (fid, n, nbytes, width))]
        # a batch of this shape and up to seven of its neighbours in the list that share its format and n
        mates = [(b, w) for (f2, n2, b, w) in todo[k:k + 40] if f2 == fid and n2 == n][:rng.randrange(1, 9)]
        calls.append(("batch", batch, (fid, n, rng.choice((1, 2, 256, 1024, 4096)), rng.choice((1, 64, 256, 304)), mates)))
        for what, fn, args in calls:
            a, b = fn(ref, *args), fn(new, *args)
            compared[what.split()[0]] += 1
            if a != b:
                print("MISMATCH in %s at shape %d: args %r\n  reference: %r\n  this:      %r" % (what, k, args, a[:2] + (a[2][:40],) if len(a) == 3 and isinstance(a[2], tuple) else a,
                                                                                                 b[:2] + (b[2][:40],) if len(b) == 3 and isinstance(b[2], tuple) else b))
                print("%d shapes compared before the mismatch" % k)
                return 1
    print("%d shapes compared (%d upload plans, %d peak shapes, %d batch plans): every status and every word equal; first mismatch: none"
          % (len(todo), compared["upload"], compared["peak"], compared["batch"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
