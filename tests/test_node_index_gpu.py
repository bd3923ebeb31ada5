"""Indexed image replies through the Node layer: HipWorker.renderIndexed / renderIndexedSync, the addon's renderIndexSync, recolour and
js/cli.js --index against fixtures written here from the oracle (tests/indexref.py) and confirmed against Context.render_index;
malformed messages end in onerror with status -1 / a throw (tests/js/check_index.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import indexref
import peakref
import siggen
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle
from test_launch_shapes_gpu import _lut

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GEN = {"kind": "trinoise", "seed": 3141, "step": 5003, "gshift": 10, "amp": 0.45, "namp": 0.03}
GAIN, RANGE = 6.0, 30.0

# (id, format, n, width, samples, L/R split, waterfall, detector, cli run): the frame loop, and the peak detector at M = 2 (render_extract)
CASES = [
    ("cu8_256", "CU8", 256, 300, 256 + 299 * 100, False, False, None, True),
    ("cs16_256_wf", "CS16", 256, 300, 256 + 299 * 64 + 7, True, True, None, True),
    ("cu8_256_peak", "CU8", 256, 300, 256 + 299 * 2 * 256 + 150, False, False, "peak", True),
]


def test_indexed_replies_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    pkg = load_package()
    ctx = pkg.Context(0)
    d = str(tmp_path)
    lut = _lut()
    lut[0], lut[-1] = (0, 0, 0), (255, 255, 255)                 # (as the caller forces the ends: cli.js renders by name)
    cases = []
    try:
        for cid, fmt, n, width, samples, ch, wf, det, cli in CASES:
            data = siggen.generate(fmt, GEN, samples)
            data.tofile(os.path.join(d, cid + ".bin"))
            win, weight = pyoracle.window("blackmanHarris", n)
            if det == "peak":
                want = peakref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, width, ch, wf)
                assert want["M"] == 2
            else:
                want = pyoracle.render(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, width, ch, wf)
            index = indexref.expected_index(want)
            got = ctx.render_index(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, width, ch, wf, detector=det or "sample")
            assert np.array_equal(got["index"], index), cid                      # the Python result is the fixture
            assert len(np.unique(index)) > 32
            index.tofile(os.path.join(d, cid + ".index"))
            lut.tofile(os.path.join(d, cid + ".lut"))
            for k in ("gauge_mins", "gauge_maxs", "gauge_amps"):
                np.asarray(want[k], np.uint8).tofile(os.path.join(d, cid + "." + k))
            mm = np.array([want["dBfs_min"], want["dBfs_max"]], np.float64).view(np.uint64)
            with open(os.path.join(d, cid + ".json"), "w") as fh:
                json.dump({"c_hist": [int(v) for v in want["c_hist"]], "cB_hist": [int(v) for v in want["cB_hist"]],
                           "dBfs_min": "%016x" % int(mm[0]), "dBfs_max": "%016x" % int(mm[1])}, fh)
            cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "blackmanHarris",
                          "gain": GAIN, "range": RANGE, "channelMode": ch, "waterfall": wf, "detector": det, "cli": cli})
    finally:
        ctx.close()
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_index.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "index ok: %d cases" % len(CASES) in out.stdout
