"""The occupancy counts through the Node layer: HipWorker.renderOccupancy (asynchronous and synchronous, a threshold per row and one
number), the addon's renderOccupancy / renderOccupancySync and js/cli.js --occupancy-rows / --occupancy-frames with --threshold and
--threshold-over-mean, against arrays written here from tests/occref.py on the hopping capture of tests/test_track_gpu.py; a peak
detector is refused with status -4, bad bands and a threshold of the wrong length with -1, before anything is rendered
(tests/js/check_occupancy.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bandref
import meanref
import occref
import powerref
from __graft_entry__ import ROOT, build
from oracle import pyoracle
from test_track_gpu import hopping

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GAIN, RANGE = 3.0, 45.0
FREQS = [(-0.125, 0.25), (0.0, 0.0), (0.3, 9.0)]
K_ROTATION = (0.5, 1.0, 2.0, 0.0, 4.0, 1e6, 0.25)      # per row, as in tests/test_occupancy_gpu.py
OVER_MEAN = 1.5                                          # cli.js --threshold-over-mean

# (id, format, n, width, stride in samples, L/R split)
CASES = [
    ("cu8_256", "CU8", 256, 40, 256 // 2 + 3, False),
    ("cf32_1024", "CF32", 1024, 64, 1024 // 2 + 3, True),
]


def test_occupancy_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    d = str(tmp_path)
    cases = []
    for cid, fmt, n, width, stride, ch in CASES:
        data = hopping(fmt, n + (width - 1) * stride)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        plane = powerref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, width, ch)["power"]
        powerref.assert_telling(plane[:, 1:] if ch else plane, cid)          # (the split forces bin n/2, row 0, to zero)
        bands = bandref.standard_bands(n)
        from_freqs = [bandref.band_rows(n, lo, hi) for lo, hi in FREQS]
        mean = meanref.expected(plane)
        power = float(np.median(plane))
        sets = {"": np.array([K_ROTATION[y % len(K_ROTATION)] for y in range(n)]) * mean,      # a threshold per row
                ".k": np.float64(OVER_MEAN) * mean,                                              # K * the mean trace
                ".p": np.full(n, power)}                                                         # one power for all rows
        for tag, thr in sets.items():
            rows, frames = occref.expected(plane, thr, bands + from_freqs)
            # the telling condition, on the expected arrays alone
            share = int(rows.astype(np.int64).sum()) / float(n * width)
            assert 0.02 <= share <= 0.98 and len(np.unique(frames[2])) >= 8, (cid, tag, share)
            if tag == "":
                assert (rows == 0).any() and (rows == width).any(), cid
            rows.astype("<u4").tofile(os.path.join(d, cid + tag + ".rows"))
            frames.astype("<u4").tofile(os.path.join(d, cid + tag + ".frames"))
        sets[""].astype("<f8").tofile(os.path.join(d, cid + ".thr"))
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "hann", "gain": GAIN,
                      "range": RANGE, "channelMode": ch, "rows": bands, "freqs": FREQS, "rowsOfFreqs": from_freqs, "overMean": OVER_MEAN,
                      "power": power})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_occupancy.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "occupancy ok: %d cases" % len(CASES) in out.stdout
