"""bench.py's own contract on an MI355X: a plain run prints the headline alone and --dump-outputs writes the last step's reply; with
--full, one JSON line with the roofline object, and the N > 1 path (ranks sharing the one GPU of the test machine, gloo for the
collectives) with a batch size that does not divide the step count."""
import json
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_once(cmd):
    # own process group: a timeout must also end the ranks torch.distributed.run started
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, start_new_session=True)
    try:
        out, err = p.communicate(timeout=240)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        return None
    return p.returncode, out, err


def run_bench(*argv):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + list(argv)
    # (a run timed out once in ~30 on a box whose image was still paging in, three processes importing torch at once: one more try)
    r = run_once(cmd) or run_once(cmd)
    if r is None:
        pytest.skip("bench.py did not finish within 2 x 240 s (process start-up / rendezvous on this box), nothing was measured")
    rc, out, err = r
    assert rc == 0, err[-2000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line_has_roofline_and_checks():
    d = run_bench("--full", "--steps", "50", "--warmup", "10", "--no-cpu-baseline", "--no-e2e")
    assert d["n_gpus"] == 1 and d["unit"] == "frames/s" and d["dtype"] == "f64" and d["kernel"] == "frames"
    assert d["checks"]["c_hist_sum"] == d["checks"]["expected"] == 16384 * 1024
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0.0 < r["frac"] < 1.0
    # frac = achieved / peak; the one-set figure is achieved_one_set = algorithmic bytes / the timed loop's kernel duration.  Where the
    # rotating leg finds the one-set loop leaning on the Infinity Cache, the headline pair is the rotating sets' (lower), and says so
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(r["achieved_one_set"] - r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved_one_set"]
    assert abs(r["frac_one_set"] - r["achieved_one_set"] / r["peak"]) < 1e-12
    if "rotation" in r["frac_basis"]:
        assert r["frac"] == r["frac_rotating"] <= r["frac_one_set"] * 1.02
    else:
        assert r["frac"] == r["frac_one_set"]
    # the profiled child run's own step time sits beside its kernel average: same process, so kernel <= step holds without a band
    assert r["child_run_ms_per_step"] is None or r["kernel_ms"] <= r["child_run_ms_per_step"] * 1.05
    # `value` is what the command describes: --steps steps right after --warmup steps of the fresh process; the figure
    # behind the clock spin-up sits beside it and is a separate, later timed region of the same process
    assert d["warmup"] == 10 and d["steps"] == 50 and "right after --warmup steps" in d["value_is"] and "--warmup 10" in d["value_is"]
    assert abs(d["value"] - 16384 * 50 / (d["ms_per_step"] * 50e-3)) < 1e-6 * d["value"]
    assert d["value_steady"] > 0.8 * d["value"] and d["ms_per_step_steady"] > 0 and "spin-up" in d["value_steady_note"]
    assert d["cold"]["next_steps"] == 9 and d["cold"]["first_step_ms"] > 0          # the cold figures are part of the 10 warm-up steps
    assert "spinup_steps_untimed" not in d
    # the kernel time is rocprofv3's own figure (a child run of the same command), never an event time with something subtracted;
    # the live event-pair figure of THIS process sits beside it (two runs, and the pair adds its dispatch latency: a band, not an order)
    assert r["kernel_ms_source"].startswith("rocprofv3 --kernel-trace") and abs(r["kernel_ms"] / r["kernel_ms_event_pair"] - 1.0) < 0.2
    # one kernel per step: the step is the kernel (plus launch gaps), not the kernel plus a finish launch - at steady clocks, as the
    # kernel average is; right after 10 warm-up steps the shader clock still ramps and `value` says what that costs (5-15 %)
    assert d["ms_per_step_steady"] < 1.08 * r["kernel_ms"] and d["ms_per_step"] < 1.35 * r["kernel_ms"]
    rot = r["rotating"]
    assert rot["sets"] == 3 and rot["working_set_MiB"] > 256 and 0.8 < rot["ratio"] < 1.3 and "kernel duration" in rot["verdict"]
    t = d["two_in_flight"]
    assert t["outputs_equal"] is True and d["value_two_in_flight"] == t["value_two_in_flight"] > 0.8 * d["value"]
    assert r["traffic"] is None or "profiles/" in r["traffic_source"] or "--pmc" in r["traffic_source"]
    if r["traffic"] is not None:   # counter traffic within 0.9 ... 1.6 x the algorithmic bytes of a launch (config 5 re-reads: 1.25 x)
        assert 0.9 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.6
    v = d["roofline_valu"]
    # (fused f64 instructions: only the divisions of the side outputs' log10 - a few thousand of 12.8 M f64 wave-instructions per launch;
    # a fused butterfly graph would show up as millions)
    assert v is None or (v["bound"] == "f64 VALU issue" and v["fused_f64_insts"] < 2e-3 * v["f64_wave_insts"] and 0.0 < v["frac"] < 1.0)


@pytest.mark.parametrize("merge_every,per_render", [(1, False), (3, False), (3, True)], ids=["every_render", "batches_of_3", "batches_of_3_merged_per_render"])
def test_two_ranks_on_one_gpu_merge_every_render(merge_every, per_render):
    d = run_bench("--full", "--gpus", "2", "--oversubscribe", "--backend", "gloo", "--steps", "20", "--warmup", "5", "--merge-every", str(merge_every),
                  *(["--merge-per-render"] if per_render else []))
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["renders_per_collective"] == merge_every
    assert d["checks"]["c_hist_sum"] == d["checks"]["expected"] == 2 * 16384 * 1024      # the LAST render's merged histogram
    assert d["rgba_gather_ms"] > 0
    seen = d["rccl_ranks_seen"]
    assert seen["world_size"] == 2 and [r["rank"] for r in seen["ranks"]] == [0, 1] and seen["distinct_devices"] == 1   # (both ranks on the box's one GPU)


def test_one_rank_rccl_group_runs_the_collectives():
    """The N > 1 path's collectives through the nccl backend (RCCL) with a one-rank group: all the box has is one GPU."""
    d = run_bench("--full", "--force-dist", "--steps", "40", "--warmup", "5", "--merge-every", "16", "--no-cpu-baseline", "--no-e2e", "--no-rocprof")
    assert d["n_gpus"] == 1 and d["renders_per_collective"] == 16
    assert d["checks"]["c_hist_sum"] == d["checks"]["expected"] == 16384 * 1024
    assert d["rgba_gather_ms"] > 0
    assert d["rccl_ranks_seen"]["world_size"] == 1 and d["rccl_ranks_seen"]["backend"] == "nccl"


@pytest.mark.parametrize("gpus", [1, 2], ids=["one_rank", "two_ranks_on_one_gpu"])
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path, gpus):
    """Without --full: the headline alone, and --dump-outputs writes the last timed step's reply (the merged side outputs for N > 1)."""
    import numpy as np
    dump = str(tmp_path / "out")
    extra = ["--gpus", "2", "--oversubscribe", "--backend", "gloo"] if gpus == 2 else []
    d = run_bench(*extra, "--steps", "20", "--warmup", "5", "--dump-outputs", dump)
    assert d["n_gpus"] == gpus and d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "frames/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and abs(d["value"] - gpus * 16384 * 20 / (d["ms_per_step"] * 20e-3)) < 1e-6 * d["value"]
    assert not {"roofline", "roofline_valu", "checks", "value_steady", "two_in_flight", "cpu_baseline", "e2e", "rgba_gather_ms"} & set(d)
    names = sorted(f[:-4] for f in os.listdir(dump))
    assert names == d["dumped_outputs"] and "rgba_sample" in names and "c_hist" in names
    a = {k: np.load(os.path.join(dump, k + ".npy")) for k in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    assert a["c_hist"].sum() == gpus * 16384 * 1024 and a["gauge_mins"].shape == (16384,)
    assert a["rgba_sample"].shape[1] == 4 and a["rgba_sample"].min() >= 0 and a["rgba_sample"].max() <= 255
    assert a["dBfs_min"][0] <= a["dBfs_max"][0]
