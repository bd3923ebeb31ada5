"""bench.py's host-side pieces that need no GPU: how the rocprofv3 --pmc child runs' CSVs become `roofline.traffic`, and what
--dump-outputs writes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench


def _write(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write('"Correlation_Id","Dispatch_Id","Agent_Id","Kernel_Name","Counter_Name","Counter_Value"\n')
        for i, (kernel, counter, value) in enumerate(rows):
            f.write('%d,%d,"Agent 4","%s","%s",%s\n' % (i, i, kernel, counter, value))


def test_counter_mean_takes_the_second_half_of_the_frame_loops_dispatches(tmp_path):
    k = "void spk2::k_frames<10, false, 8>(spk::FrameArgs, int, HIP_vector_type<double, 2u> const*, int, int)"
    rows = [(k, "FETCH_SIZE", 1000.0 + i) for i in range(10)]                    # warm-up half 1000..1004, counted half 1005..1009
    rows += [("void spk::k_synth_trinoise<12>(spk::SynthArgs)", "FETCH_SIZE", 9e9)]  # another kernel of the run: ignored
    rows += [(k, "WRITE_SIZE", 5.0)] * 10                                           # another counter: ignored
    _write(str(tmp_path / "host" / "123_counter_collection.csv"), rows)
    assert bench.pmc_counter_mean(str(tmp_path), "FETCH_SIZE") == 1007.0
    assert bench.pmc_counter_mean(str(tmp_path), "WRITE_SIZE") == 5.0


def test_counter_mean_refuses_a_run_that_is_too_short_or_empty(tmp_path):
    k = "void spk2::k_frames<10, false, 8>(spk::FrameArgs, int, HIP_vector_type<double, 2u> const*, int, int)"
    _write(str(tmp_path / "a" / "1_counter_collection.csv"), [(k, "FETCH_SIZE", 1.0)] * 7)
    assert bench.pmc_counter_mean(str(tmp_path), "FETCH_SIZE") is None
    assert bench.pmc_counter_mean(str(tmp_path / "nothing_here"), "FETCH_SIZE") is None


def test_dump_outputs_writes_the_reply_as_float_arrays_within_the_limit(tmp_path):
    """--dump-outputs: every array float32 / float64, the RGBA pixels a fixed sample of the image, the whole within 64 MB."""
    import numpy as np
    import torch
    L, W, n = 256, 4096, 1024                                    # 4 M pixels: more than the sample, so it is sampled
    g = torch.Generator().manual_seed(7)
    rgba = torch.randint(0, 256, (4 * W * n,), dtype=torch.uint8, generator=g)
    gauges = torch.randint(0, 256, (3 * W,), dtype=torch.uint8, generator=g)
    record = torch.randint(0, 1 << 20, (L + 1000 + 2,), dtype=torch.int64, generator=g)
    record[L + 1000:].view(torch.float64)[:] = torch.tensor([-87.5, -3.25], dtype=torch.float64)
    names = bench.dump_outputs(str(tmp_path / "a"), rgba, gauges, record, L, W)
    assert names == sorted(["rgba_sample", "rgba_sample_index", "gauge_mins", "gauge_maxs", "gauge_amps", "c_hist", "cB_hist",
                            "dBfs_min", "dBfs_max"])
    d = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in names}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in names) <= 64 * 10**6
    idx = d["rgba_sample_index"].astype(np.int64)
    assert 0.7 * bench.DUMP_RGBA_PIXELS < len(idx) < W * n and np.all(np.diff(idx) > 0)
    assert np.array_equal(d["rgba_sample"], rgba.view(-1, 4).numpy()[idx].astype(np.float32))
    gn = gauges.numpy()
    assert np.array_equal(d["gauge_mins"], gn[:W]) and np.array_equal(d["gauge_maxs"], gn[W:2 * W]) and np.array_equal(d["gauge_amps"], gn[2 * W:])
    assert np.array_equal(d["c_hist"], record[:L].numpy()) and np.array_equal(d["cB_hist"], record[L:L + 1000].numpy())
    assert d["dBfs_min"].tolist() == [-87.5] and d["dBfs_max"].tolist() == [-3.25]
    # the same image size draws the same pixels: two builds' dumps compare element for element
    bench.dump_outputs(str(tmp_path / "b"), rgba, gauges, record, L, W)
    assert np.array_equal(np.load(str(tmp_path / "b" / "rgba_sample_index.npy")), d["rgba_sample_index"])
