"""Checks on the compiled gfx950 code objects (no GPU needed: hipcc cross-compiles, llvm-objdump disassembles).

The re-distributions of the frame loop read LDS with inline-asm ds_read_b64 instructions whose wait comes later, in a separate asm
statement (sp_frame_parts.h); the compiler does not know the destination registers are invalid in between.  tools/check_lds_reads.py
follows the in-order LDS counter through every kernel of the product and fails on any access to a register with an outstanding read."""
import os
import re

import pytest

import isa
from __graft_entry__ import ROOT


def test_checker_sees_a_register_touched_before_its_read_has_returned():
    c = isa.checker()
    ok = """
0000000000001000 <k>:
	ds_write_b64 v10, v[2:3]                                   // 000000001000: D89A0000 0000020A
	ds_read_b64 v[2:3], v11 offset:8                           // 000000001008: D8EC0008 0200000B
	ds_read_b64 v[4:5], v11 offset:16                          // 000000001010: D8EC0010 0400000B
	v_add_f64 v[6:7], v[8:9], v[8:9]                           // 000000001018: D2800006 00021108
	s_waitcnt lgkmcnt(1)                                       // 000000001020: BF8CC17F
	v_mul_f64 v[2:3], v[2:3], v[8:9]                           // 000000001024: D2810002 00021102
	s_waitcnt lgkmcnt(0)                                       // 00000000102C: BF8CC07F
	v_mul_f64 v[4:5], v[4:5], v[8:9]                           // 000000001030: D2810004 00021104
	s_endpgm                                                   // 000000001038: BF810000
""".split("\n")
    assert c.check_listing(ok) == []
    copied_early = [ln.replace("v_add_f64 v[6:7], v[8:9], v[8:9]", "v_mov_b32_e32 v20, v4") for ln in ok]        # a copy before the wait
    assert len(c.check_listing(copied_early)) == 1
    clobbered = [ln.replace("v_add_f64 v[6:7], v[8:9], v[8:9]", "v_add_f64 v[2:3], v[8:9], v[8:9]") for ln in ok]   # a write under the read
    assert len(c.check_listing(clobbered)) == 1
    short_wait = [ln.replace("s_waitcnt lgkmcnt(1)", "s_waitcnt lgkmcnt(2)") for ln in ok]                           # waits for nothing
    assert len(c.check_listing(short_wait)) == 1


def test_no_kernel_of_the_product_touches_a_register_with_an_outstanding_lds_read():
    objs = isa.product_objs()
    c = isa.checker()
    bad, reads = [], 0
    for o in objs:
        lines = c.disassemble(o)
        reads += sum(1 for ln in lines if " ds_read_b64 " in ln.replace("\t", " "))
        bad += c.check_listing(lines, os.path.basename(o))
    assert reads > 5000            # the asm reads are there (16 per component and re-distribution in every variant)
    assert not bad, bad[:10]


def test_the_prefetching_iq_variants_of_the_frame_loop_use_no_scratch_memory():
    """A kernel that touches scratch (spilled VGPRs, or the argument structure dropped to the stack because a lambda was not inlined: it
    happened in an experiment and cost 40 %) launches its waves slower and reads its arguments from memory.  Every variant the BASELINE
    configs run - interleaved I/Q, samples prefetched (PFB != 0) - must have a private segment of zero bytes and no spilled VGPR."""
    seen = 0
    for o in isa.frame_objs():
        for blk in isa.notes(o).split(".name:")[1:]:
            m = re.match(r"\s*_ZN4spk28k_framesILi(\d+)ELb([01])ELi(\d+)E", blk)
            if not m or m.group(2) == "1" or m.group(3) == "0":
                continue
            seen += 1
            priv = int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", blk).group(1))
            spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", blk).group(1))
            assert priv == 0 and spill == 0, (m.group(0), priv, spill)
    assert seen == 8 * 5           # eight sizes x five prefetch widths


def test_the_prologue_waits_for_its_tables_not_for_the_first_frames_samples():
    """n <= 1024, prefetching variants: the first frame's 16 sample loads are issued BEHIND the table loads and the wait in front of the
    LDS table stores counts them (s_waitcnt vmcnt(16)).  Vector-memory operations complete in order: a vmcnt(0) there - the samples
    requested ahead of the tables, or a request the compiler cannot count - makes the table wait a wait for HBM (+1.5 us per launch)."""
    objs = isa.frame_objs()
    c = isa.checker()
    seen = 0
    for o in objs:
        m = re.search(r"frames_(\d+)\.o$", o)
        if int(m.group(1)) > 10:
            continue
        kernel, waits = None, []
        for ln in c.disassemble(o):
            h = re.match(r"[0-9a-f]+ <_ZN4spk28k_framesILi(\d+)ELb([01])ELi(\d+)E", ln)
            if h:
                kernel, waits = h.groups(), []
                continue
            if kernel is None:
                continue
            t = ln.replace("\t", " ")
            w = re.search(r" s_waitcnt .*vmcnt\((\d+)\)", t)
            if w:
                waits.append(int(w.group(1)))
            if " s_barrier" in t:                      # the prologue's barrier: everything before it is the prologue
                if kernel[2] != "0" and kernel[1] == "0":
                    assert waits and waits[-1] == 16 and 0 not in waits, (kernel, waits)
                    seen += 1
                kernel = None
    assert seen >= 5 * 5          # five prefetch widths at n = 64 .. 1024


def test_the_instrumentation_patch_applies_to_the_kernel_sources():
    """tools/experiments/frames_instrumentation.patch (per-wave clocks for tools/stamps.py, cost-attribution switches, the round-5 tile
    prototype) lives outside the product sources and is applied to a copy by tools/build_variant.sh: a kernel change that moves its
    context must refresh it, or the next round finds its measuring tools broken."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("patch") is None:
        pytest.skip("no patch(1) here")
    with tempfile.TemporaryDirectory() as t:
        os.makedirs(os.path.join(t, "spectroplot-js_amd"))
        shutil.copytree(os.path.join(ROOT, "spectroplot-js_amd", "csrc"), os.path.join(t, "spectroplot-js_amd", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(t, "include"))
        with open(os.path.join(ROOT, "tools", "experiments", "frames_instrumentation.patch")) as fh:
            r = subprocess.run(["patch", "-p1", "--dry-run", "-s"], cwd=t, stdin=fh, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-500:]


def _regs(operand):
    """VGPR numbers an operand names: 'v7' -> {7}, 'v[4:7]' -> {4..7}, anything else -> empty."""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def store_hazards(lines, where=""):
    """gfx940 / gfx950: a VMEM store of more than 64 bits reads its data registers late - a VALU instruction that overwrites them needs 2
    wait states behind the store (LLVM's GCNHazardRecognizer inserts them for stores it knows; k_frames issues its write-out stores as
    inline asm, which it cannot see: ADVICE r5).  Returns the stores followed within 2 wait states by a VALU write to their data."""
    ins = []
    for ln in lines:
        t = ln.replace("\t", " ").split("//")[0].strip()
        if not t or t.endswith(":") or re.match(r"[0-9a-f]+ <", t):
            continue
        ins.append(t)
    bad = []
    for i, t in enumerate(ins):
        m = re.match(r"global_store_dwordx[34] (\S+), (v\[\d+:\d+\])", t)
        if not m:
            continue
        data = _regs(m.group(2).rstrip(","))
        states, j = 0, i + 1
        while states < 2 and j < len(ins):
            u = ins[j]
            nop = re.match(r"s_nop (\d+)", u)
            if nop:
                states += int(nop.group(1)) + 1
                j += 1
                continue
            if u.startswith("v_"):
                ops = [o.strip().rstrip(",") for o in u.split(None, 1)[1].split(",")] if " " in u else []
                dests = ops[:2] if ("_swap" in u.split()[0]) else ops[:1]
                written = set().union(*[_regs(o) for o in dests]) if dests else set()
                if written & data:
                    bad.append("%s: `%s` then `%s`" % (where, t, u))
            states += 1
            j += 1
    return bad


def test_store_hazard_checker_sees_a_data_register_overwritten_too_early():
    ok = ["\tglobal_store_dwordx4 v1, v[4:7], s[2:3] nt   // 0000: X", "\tv_mov_b32_e32 v9, v4  // 0008", "\ts_nop 0  // 000c",
          "\tv_mov_b32_e32 v4, v9  // 0010"]
    assert store_hazards(ok) == []
    assert len(store_hazards([ok[0], "\tv_mov_b32_e32 v5, v9 // x"])) == 1
    assert len(store_hazards([ok[0], ok[1], "\tv_add_f64 v[6:7], v[8:9], v[8:9] // x"])) == 1
    assert store_hazards([ok[0], "\ts_nop 1 // x", "\tv_mov_b32_e32 v5, v9 // x"]) == []
    assert len(store_hazards([ok[0], "\tv_permlane32_swap_b32_e32 v20, v7 // x"])) == 1


def test_no_valu_write_lands_on_the_data_of_a_wide_store_within_two_wait_states():
    objs = isa.product_objs()
    c = isa.checker()
    bad, stores = [], 0
    for o in objs:
        lines = c.disassemble(o)
        stores += sum(1 for ln in lines if "global_store_dwordx4" in ln)
        bad += store_hazards(lines, os.path.basename(o))
    assert stores > 500            # the write-out's 16-byte stores are there, in every variant
    assert not bad, bad[:10]


_BATCH_H = "spectroplot-js_amd/csrc/sp_kernel_frames_batch.h"
_PEAK_H = "spectroplot-js_amd/csrc/sp_kernel_frames_peak.h"
_INDEX_H = "spectroplot-js_amd/csrc/sp_kernel_frames_index.h"
_TRACES_H = "spectroplot-js_amd/csrc/sp_kernel_frames_traces.h"
_POWER_H = "spectroplot-js_amd/csrc/sp_kernel_frames_power.h"
_MEAN_H = "spectroplot-js_amd/csrc/sp_kernel_mean.h"
_MOMENT_CORE_H = "spectroplot-js_amd/csrc/sp_moment_core.h"


# family -> (prefix of the mangled names, the file whose first commit is the reference, "^" for that commit's parent, the objects, streams)
STREAM_FAMILIES = {
    "k_frames": ("_ZN4spk28k_framesI", _BATCH_H, "^", isa.FRAME_TARGETS, isa.frame_objs, 96),
    "k_frames_batch": ("_ZN4spk214k_frames_batchI", _BATCH_H, "", isa.FRAME_TARGETS, isa.frame_objs, 48),
    "k_frames_peak": ("_ZN4spk213k_frames_peakI", _PEAK_H, "", isa.PEAK_TARGETS, isa.peak_objs, 60),
    # (no later commit changed one of these three on purpose: each is pinned to the commit that added its header; k_frames_index has the
    # 96 variants of k_frames less the three that frames_index_variant_built drops)
    "k_frames_index": ("_ZN4spk214k_frames_indexI", _INDEX_H, "", isa.INDEX_TARGETS, isa.index_objs, 93),
    "k_frames_traces": ("_ZN4spk215k_frames_tracesI", _TRACES_H, "", isa.TRACES_TARGETS, isa.traces_objs, 60),
    "k_frames_power": ("_ZN4spk214k_frames_powerI", _POWER_H, "", isa.POWER_TARGETS, isa.power_objs, 60),
    # every kernel of sp_kernels.o against sp_api.o, which held them, as the commit that added the mean kernels builds it, the last one
    # before the host side of the scratch launches was folded: 56 k_scratch_radix2, 28 k_scratch_traces, 28 k_scratch_power,
    # 14 k_synth_trinoise and 15 single kernels
    "sp_api": ("", _MEAN_H, "", isa.API_TARGETS, isa.api_objs, 141),
    # every kernel of the plane consumers' units - band sums and moments, track, occupancy, quantile, bursts, pulses, block mean - as the
    # commit that added sp_moment_core.h builds them, the last one that changed any of them: 4 band / moment kernels, k_track_max,
    # k_occupancy_count, 5 quantile, 3 burst, 3 pulse kernels, k_blockmean and k_power_to_index.  Since then the band sums and the
    # moments are one body (STREAM_RENAMED, STREAM_DROPPED) and the pulse kernels take their wave sum from sp_wave_sum.h.
    "consumers": ("", _MOMENT_CORE_H, "", isa.CONSUMER_TARGETS, isa.consumer_objs, 19),
}

_BAND_ARGS = "PKdixNS_8BandListEPdxx"
# {a kernel of this tree: its name in the family's reference build}: k_band_sum<ORDER> is k_band_sum at ORDER 0 and k_moment_sum<ORDER> above
STREAM_RENAMED = {
    "consumers": {
        "_ZN3spk10k_band_sumILi0EEEv" + _BAND_ARGS: "_ZN3spk10k_band_sumE" + _BAND_ARGS,
        "_ZN3spk10k_band_sumILi1EEEv" + _BAND_ARGS: "_ZN3spk12k_moment_sumILi1EEEv" + _BAND_ARGS,
        "_ZN3spk10k_band_sumILi2EEEv" + _BAND_ARGS: "_ZN3spk12k_moment_sumILi2EEEv" + _BAND_ARGS,
    },
}
# the reference build's kernels without a successor: k_moment_sum<0> gave k_band_sum's bits from a third body
STREAM_DROPPED = {"consumers": {"_ZN3spk12k_moment_sumILi0EEEv" + _BAND_ARGS}}


@pytest.mark.parametrize("family", sorted(STREAM_FAMILIES))
def test_kernel_instruction_streams_match_their_reference_commit(family):
    """Every variant <L, C, P> of the six frame-loop kernels has the instruction stream (addresses stripped) of a reference build: k_frames
    of the commit before the batch kernel was added, each other kernel of the commit that added its header (sp_kernel_frames_batch.h,
    _peak.h, _index.h, _traces.h, _power.h); so has every kernel of sp_kernels.o - the scratch kernels in all their formats, the
    synthesiser and the small kernels around the frame loops - of the commit that added sp_kernel_mean.h, which built them into sp_api.o
    beside the host code that launched them (the "sp_api" family keeps that name); and so has every kernel of the plane consumers' units
    ("consumers"), under the names the reference build gave them.  What the frame-loop kernels share since - the sp_frames_*.inc.h fragments of the stages, of the
    prologue, of the loop's shell, the write-out lambdas, the finale and the two whole bodies - must not move any of them.  This guards those changes only: a later commit that
    changes a kernel on purpose replaces that family's reference with its own parent (HEAD^ of the commit that last touched the kernel's
    loop)."""
    prefix, added_file, parent, targets, objs, count = STREAM_FAMILIES[family]
    try:
        added = isa.commit_that_added(added_file)
        theirs = isa.commit_streams(added + parent if added != "HEAD" else "HEAD", targets, prefix)
    except isa.NoReference as e:
        pytest.skip(str(e))
    renamed, dropped = STREAM_RENAMED.get(family, {}), STREAM_DROPPED.get(family, set())
    built = isa.streams(objs(), prefix)
    assert set(renamed) <= set(built) and dropped <= set(theirs)
    mine = {renamed.get(k, k): v for k, v in built.items()}
    assert len(theirs) == count and len(mine) == len(built) == count - len(dropped) and set(mine) == set(theirs) - dropped
    differ = [k for k in mine if mine[k] != theirs[k]]
    assert not differ, differ[:5]


def test_the_host_units_hold_no_device_code():
    """The C ABI (sp_api.hip) and the group render (sp_group.hip) are host code: every kernel they launch lies in another object and is
    reached through a plain launcher (sp_launch.h, spk2::launch_frames*), so a change to them neither rebuilds nor moves a kernel."""
    isa.api_objs()            # (builds the library where it is not built yet)
    for unit in ("sp_api.o", "sp_group.o"):
        obj = os.path.join(isa.PKG, "build", unit)
        assert os.path.exists(obj), obj
        assert isa.streams([obj], "") == {}, unit
