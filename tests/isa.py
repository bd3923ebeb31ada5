"""What the tests that look at the compiled gfx950 code objects share (no GPU needed: hipcc cross-compiles, llvm-objdump disassembles):
the built objects, an object's notes, the instruction streams of its kernels, and the streams of another commit of this repository."""
import functools
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

from __graft_entry__ import ROOT, build

LLVM = "/opt/rocm/lib/llvm/bin"
PKG = os.path.join(ROOT, "spectroplot-js_amd")
FRAME_TARGETS = tuple("build/frames_%d.o" % lg for lg in range(6, 14))     # k_frames and k_frames_batch
PEAK_TARGETS = tuple("build/peak_%d.o" % lg for lg in range(6, 11))        # k_frames_peak
INDEX_TARGETS = tuple("build/index_%d.o" % lg for lg in range(6, 14))      # k_frames_index
TRACES_TARGETS = tuple("build/traces_%d.o" % lg for lg in range(6, 11))    # k_frames_traces
POWER_TARGETS = tuple("build/power_%d.o" % lg for lg in range(6, 11))      # k_frames_power
API_TARGETS = ("build/sp_api.o",)                                          # what held the scratch kernels and every small kernel in the
#                                                                            reference commit; now build/sp_kernels.o does (api_objs)
CONSUMER_UNITS = ("band", "track", "occupancy", "quantile", "burst", "pulse", "blockmean")   # a plane consumer's kernels, a unit each
# ... and the reference commit's, which had the moments in a unit of their own beside the band sums
CONSUMER_TARGETS = tuple("build/sp_%s.o" % u for u in CONSUMER_UNITS + ("moment",))


def _built(pattern, at_least):
    objs = sorted(glob.glob(os.path.join(PKG, "build", pattern)))
    if len(objs) < at_least:
        build()
        objs = sorted(glob.glob(os.path.join(PKG, "build", pattern)))
    return objs


def frame_objs():
    objs = _built("frames_*.o", 8)
    assert len(objs) == 8
    return objs


def peak_objs():
    objs = _built("peak_*.o", 5)
    assert len(objs) == 5
    return objs


def index_objs():
    objs = _built("index_*.o", 8)
    assert len(objs) == 8
    return objs


def traces_objs():
    objs = _built("traces_*.o", 5)
    assert len(objs) == 5
    return objs


def power_objs():
    objs = _built("power_*.o", 5)
    assert len(objs) == 5
    return objs


def api_objs():
    """The object of the scratch kernels and every small kernel (csrc/sp_kernels.hip); sp_api.o and sp_group.o are host code only."""
    objs = _built("sp_kernels.o", 1)
    assert len(objs) == 1
    return objs


def consumer_objs():
    """The objects of the plane consumers' kernels (csrc/sp_band.hip ... sp_blockmean.hip)."""
    api_objs()            # (builds the library where it is not built yet)
    objs = [os.path.join(PKG, "build", "sp_%s.o" % u) for u in CONSUMER_UNITS]
    assert all(os.path.exists(o) for o in objs), objs
    return objs


def product_objs():
    """Every object of the library that can hold device code."""
    objs = [o for o in _built("*.o", 9) if not o.endswith("sp_host.o")]
    assert len(objs) >= 9
    return objs


def checker():
    """tools/check_lds_reads.py as a module (disassemble, check_listing)."""
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import check_lds_reads
    return check_lds_reads


def notes(obj):
    """llvm-readelf --notes of the gfx950 code object inside a host object: one `.name:` block per kernel."""
    with tempfile.TemporaryDirectory() as t:
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, os.path.join(t, "fb.bin")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + os.path.join(t, "fb.bin"),
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + os.path.join(t, "k.co")],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(t, "k.co")], text=True)


def streams(objs, prefix):
    """{kernel name: its instructions, addresses and encodings stripped} for the kernels whose mangled name starts with `prefix`."""
    c = checker()
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


class NoReference(Exception):
    """This checkout cannot build the commit asked for (no git, or the commit is not in its history)."""


def _git(*a):
    return subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, text=True)


def commit_that_added(path):
    """The commit that added `path`, or "HEAD" where the history does not show it."""
    if shutil.which("git") is None or not os.path.isdir(os.path.join(ROOT, ".git")):
        raise NoReference("no git history here to build the reference commit from")
    added = _git("log", "--diff-filter=A", "--format=%H", "--", path).stdout.split()
    return added[-1] if added else "HEAD"


@functools.lru_cache(maxsize=None)
def _commit_streams(sha, targets):
    with tempfile.TemporaryDirectory() as t:
        wt = os.path.join(t, "reference")
        r = _git("worktree", "add", "--detach", wt, sha)
        if r.returncode:
            raise NoReference("git worktree failed: " + r.stderr[-200:])
        try:
            subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(wt, "spectroplot-js_amd")] + list(targets))
            return streams([os.path.join(wt, "spectroplot-js_amd", o) for o in targets], "")
        finally:
            _git("worktree", "remove", "--force", wt)


def commit_streams(ref, targets, prefix):
    """streams() of the objects `targets` (make targets of spectroplot-js_amd/Makefile) as commit `ref` builds them, in a detached
    worktree that is removed again; a commit is built once per test session."""
    if shutil.which("git") is None or not os.path.isdir(os.path.join(ROOT, ".git")):
        raise NoReference("no git history here to build the reference commit from")
    r = _git("rev-parse", "--verify", "-q", ref + "^{commit}")
    if r.returncode:
        raise NoReference("the reference commit is not in this clone's history")
    # (a truncated history names its oldest commit as the one that added every file: that commit need not hold a unit removed since)
    for unit in re.findall(r"build/(sp_\w+)\.o", " ".join(targets)):
        if _git("cat-file", "-e", "%s:spectroplot-js_amd/csrc/%s.hip" % (r.stdout.strip(), unit)).returncode:
            raise NoReference("the commit found for the reference does not hold csrc/%s.hip" % unit)
    return {k: v for k, v in _commit_streams(r.stdout.strip(), tuple(targets)).items() if k.startswith(prefix)}
