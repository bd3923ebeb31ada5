"""Batches without a device: the new entry points are exported and check their arguments, the host's work list (sp_debug_batch_plan)
covers every frame of every item once with launch_frames' rules, and the batch kernels leave k_frames as it was."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from __graft_entry__ import ROOT, build, load_package

SW = [1, 1, 2, 2, 3, 3, 4, 4, 8, 8, 16, 16, 8, 16]      # bytes per complex sample, enum sp_format order
ELEM = [1, 1, 1, 1, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8]        # element size of the typed view


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.lib_path()):
        build()
    return p


class _Reply(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rgba", "gmin", "gmax", "gamp", "c", "cb", "mm")]


class _Item(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("nbytes", C.c_size_t), ("width", C.c_int32), ("reserved", C.c_int32), ("reply", _Reply)]


def test_batch_symbols_and_argument_errors(pkg):
    lib = C.CDLL(pkg.lib_path())
    for name in ("sp_plan_execute_batch", "sp_render_batch", "sp_debug_batch_plan"):
        assert hasattr(lib, name), name
    lib.sp_plan_execute_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.sp_render_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    items = (_Item * 2)()
    for f in (lambda it, c: lib.sp_plan_execute_batch(None, it, c), lambda it, c: lib.sp_render_batch(None, None, it, c)):
        assert f(items, -1) == -1                       # count < 0
        assert f(None, 1) == -1                         # items == NULL with count > 0
    dev = pkg.Library.get().device_count()
    want = -5 if dev == 0 else -1                       # no context: SP_ERR_NO_DEVICE without a device
    assert lib.sp_plan_execute_batch(None, items, 2) == want
    assert lib.sp_render_batch(None, None, items, 2) == want
    with pytest.raises(pkg.SpectroplotError):
        pkg.binding.debug_batch_plan("cu8", 512, 256, 256, [100], [-1])


def _group_frames_for(n, want):
    fpb = 512 * 16 // n
    unit = fpb
    while unit % 4:
        unit *= 2
    cap = min((65536 if n >= 2048 else 32768) // n, want)
    return max(cap // unit * unit, unit)


def _batch_gf(n, total, cu):
    want = 32
    while want > 4 and (total + want - 1) // want < 2 * cu:
        want >>= 1
    return _group_frames_for(n, want)


def _launch(fmt, n, nbytes, w):
    """launch_frames' loader choice for one item: 0 prefetching, 1 generic, 3 nothing to render."""
    if w == 0:
        return 3
    sw = SW[fmt]
    sc = nbytes / sw
    if w == 1:
        stride, ib = 0.0, n * sw <= nbytes
    else:
        stride = (sc - n) / (w - 1)
        ib = False
        if stride >= 0 and np.isfinite(stride) and 0.5 + stride * (w - 1) < 2147483647.0:
            ib = (int(0.5 + stride * (w - 1)) + n) * sw <= nbytes
    pf = ib and (sw <= 4 or sw == 8)
    if pf and sw == 3 and not (w >= 2 and int(0.5 + stride * (w - 1)) >= 1):
        pf = False
    return 0 if pf else 1


def test_batch_work_list_on_random_item_lists(pkg):
    rng = np.random.default_rng(2026)
    checked = 0
    for case in range(3000):
        fmt = int(rng.integers(0, 14))
        n = 1 << int(rng.choice(list(range(1, 14)) + [6, 7, 8, 9] * 4))   # mostly the sizes the batch kernel takes
        cu = int(rng.choice([8, 64, 256]))
        count = int(rng.integers(1, 40))
        widths, nbytes = [], []
        for _ in range(count):
            w = int(rng.choice([0, 1, int(rng.integers(2, 5000))]))
            kind = rng.integers(0, 3)
            if kind == 0:
                samples = int(rng.integers(0, n))                          # shorter than a frame
            elif kind == 1:
                samples = n + max(w - 1, 0) * int(rng.integers(n + 1, 3 * n))   # stride above n
            else:
                samples = int(rng.integers(n, 4 * n + w * n // 2 + 1))
            nb = samples * SW[fmt] // ELEM[fmt] * ELEM[fmt]
            widths.append(w)
            nbytes.append(nb)
        gf, grids, groups, rows = pkg.binding.debug_batch_plan(fmt, n, 256, cu, nbytes, widths)
        if not 64 <= n <= 512:                              # (k_frames_batch is built for n <= 512: larger plans go item by item)
            assert gf == 0 and all(r[0] == 2 for r in rows), (fmt, n)
            continue
        assert gf == _batch_gf(n, sum(widths), cu), (fmt, n, cu)
        per = {0: [], 1: []}
        for k, (lw, first, cnt) in enumerate(rows):
            assert lw == _launch(fmt, n, nbytes[k], widths[k]), (case, k, fmt, n, nbytes[k], widths[k])
            if lw == 3:
                assert cnt == 0
                continue
            assert cnt == -(-widths[k] // gf)                # every frame in exactly one group, the last one possibly partial
            per[lw].append((first, cnt))
        for lw in (0, 1):
            spans = sorted(per[lw])
            at = 0
            for first, cnt in spans:                         # an item's groups are its own and follow the previous item's
                assert first == at
                at += cnt
            assert at == groups[lw]
            assert grids[lw] == (0 if at == 0 else (min(at, cu) + 7) // 8 * 8)
        checked += 1
    assert checked > 1500


def _notes(obj):
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as t:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, os.path.join(t, "fb.bin")])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + os.path.join(t, "fb.bin"),
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + os.path.join(t, "k.co")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(t, "k.co")], text=True)


def _frame_objs():
    objs = sorted(glob.glob(os.path.join(ROOT, "spectroplot-js_amd", "build", "frames_*.o")))
    if len(objs) < 8:
        build()
        objs = sorted(glob.glob(os.path.join(ROOT, "spectroplot-js_amd", "build", "frames_*.o")))
    assert len(objs) == 8
    return objs


def test_batch_kernels_prefetching_iq_variants_use_no_scratch_memory():
    """Every I/Q prefetching variant of k_frames_batch has a private segment of zero bytes and no spilled VGPR, as every k_frames one
    (test_isa_checks.py).  The batch kernel is built for n = 64 ... 512 only; no object holds one for a larger n."""
    seen = 0
    for o in _frame_objs():
        for blk in _notes(o).split(".name:")[1:]:
            m = re.match(r"\s*_ZN4spk214k_frames_batchILi(\d+)ELb([01])ELi(\d+)E", blk)
            if not m:
                continue
            assert int(m.group(1)) <= 9, m.group(0)
            if m.group(2) == "1" or m.group(3) == "0":
                continue
            seen += 1
            priv = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            assert priv == 0 and spill == 0, (m.group(0), priv, spill)
    assert seen == 4 * 5           # four sizes x five prefetch widths


def _k_frames_streams(objs, prefix="_ZN4spk28k_framesI"):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_lds_reads as c
    out = {}
    for o in objs:
        cur = None
        for ln in c.disassemble(o):
            h = re.match(r"^[0-9a-f]+ <(.*)>:", ln)
            if h:
                cur = h.group(1) if h.group(1).startswith(prefix) else None
                if cur:
                    out[cur] = []
                continue
            t = re.sub(r"<[^>]*>", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", ln.split("//")[0])).strip()
            if cur and t and t != "...":
                out[cur].append(t)
    # what follows a kernel's last s_endpgm is alignment padding (zero dwords, which disassemble as v_cndmask_b32), not its code
    for k, v in out.items():
        ends = [i for i, t in enumerate(v) if t.startswith("s_endpgm")]
        out[k] = v[:ends[-1] + 1] if ends else v
    return out


def test_k_frames_instruction_streams_match_the_parent_commit():
    """Every k_frames<L, C, P> of this tree has the instruction stream (addresses stripped) of the commit before the batch kernel was
    added: the batch path must not move the single-request kernels.  This guards that change only: a later commit that changes k_frames
    on purpose replaces the reference below with its own parent (HEAD^ of the commit that last touched sp_kernel_frames.h's loop)."""
    if shutil.which("git") is None or not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("no git history here to build the parent commit from")
    git = lambda *a: subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, text=True)  # noqa: E731
    added = git("log", "--diff-filter=A", "--format=%H", "--", "spectroplot-js_amd/csrc/sp_kernel_frames_batch.h").stdout.split()
    ref = (added[-1] + "^") if added else "HEAD"
    if git("rev-parse", "--verify", "-q", ref).returncode:
        pytest.skip("the parent commit is not in this clone's history")
    mine = _k_frames_streams(_frame_objs())
    with tempfile.TemporaryDirectory() as t:
        wt = os.path.join(t, "parent")
        r = git("worktree", "add", "--detach", wt, ref)
        if r.returncode:
            pytest.skip("git worktree failed: " + r.stderr[-200:])
        try:
            subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(wt, "spectroplot-js_amd")]
                                  + ["build/frames_%d.o" % lg for lg in range(6, 14)])
            theirs = _k_frames_streams(sorted(glob.glob(os.path.join(wt, "spectroplot-js_amd", "build", "frames_*.o"))))
        finally:
            git("worktree", "remove", "--force", wt)
    assert len(theirs) == 96 and set(mine) == set(theirs)
    differ = [k for k in theirs if mine[k] != theirs[k]]
    assert not differ, differ[:5]


def test_k_frames_batch_instruction_streams_match_the_commit_that_added_them():
    """Every k_frames_batch<L, C, P> of this tree (n = 64 ... 512) has the instruction stream (addresses stripped) of the commit that added
    sp_kernel_frames_batch.h: sharing the frame loop's stages with k_frames (the sp_frames_*.inc.h fragments) must not move the batch
    kernel either.  This guards that change only: a later commit that changes k_frames_batch on purpose replaces the reference below with
    its own parent (HEAD^ of the commit that last touched the batch kernel's loop)."""
    if shutil.which("git") is None or not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("no git history here to build the reference commit from")
    git = lambda *a: subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, text=True)  # noqa: E731
    added = git("log", "--diff-filter=A", "--format=%H", "--", "spectroplot-js_amd/csrc/sp_kernel_frames_batch.h").stdout.split()
    ref = added[-1] if added else "HEAD"
    if git("rev-parse", "--verify", "-q", ref).returncode:
        pytest.skip("the reference commit is not in this clone's history")
    prefix = "_ZN4spk214k_frames_batchI"
    mine = _k_frames_streams(_frame_objs(), prefix)
    with tempfile.TemporaryDirectory() as t:
        wt = os.path.join(t, "reference")
        r = git("worktree", "add", "--detach", wt, ref)
        if r.returncode:
            pytest.skip("git worktree failed: " + r.stderr[-200:])
        try:
            subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(wt, "spectroplot-js_amd")]
                                  + ["build/frames_%d.o" % lg for lg in range(6, 14)])
            theirs = _k_frames_streams(sorted(glob.glob(os.path.join(wt, "spectroplot-js_amd", "build", "frames_*.o"))), prefix)
        finally:
            git("worktree", "remove", "--force", wt)
    assert len(theirs) == 48 and set(mine) == set(theirs)
    differ = [k for k in theirs if mine[k] != theirs[k]]
    assert not differ, differ[:5]
