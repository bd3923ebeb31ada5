"""Per-bin min / max traces through the Node layer: HipWorker.renderTraces, the addon's renderTracesSync and js/cli.js --traces against
fixtures written here from tests/tracesref.py; malformed fields end in onerror / a throw (tests/js/check_traces.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import siggen
import tracesref
from __graft_entry__ import ROOT, build
from oracle import pyoracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GEN = {"kind": "trinoise", "seed": 2718, "step": 5003, "gshift": 10, "amp": 0.45, "namp": 0.03}

# (id, format, n, width, stride in samples, L/R split): k_frames_traces and the portable kernel, overlapping and sparse
CASES = [
    ("cu8_256", "CU8", 256, 44, 3 * 256 + 1, False),
    ("cf32_1024", "CF32", 1024, 36, 700, True),
    ("cs16_2048", "CS16", 2048, 12, 2048 + 5, False),
]


def test_traces_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    d = str(tmp_path)
    cases = []
    for cid, fmt, n, width, stride, ch in CASES:
        data = siggen.generate(fmt, GEN, n + (width - 1) * stride)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        want = tracesref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 45.0, width, ch)
        moved = slice(1, None) if ch else slice(None)           # (the split forces bin n/2, row 0, to zero)
        assert not (want["trace_min"][moved] == 0.0).any() and len(np.unique(want["trace_max"])) >= n // 2
        want["trace_min"].astype("<f8").tofile(os.path.join(d, cid + ".tmin"))
        want["trace_max"].astype("<f8").tofile(os.path.join(d, cid + ".tmax"))
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "hann", "gain": 3.0,
                      "range": 45.0, "channelMode": ch})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_traces.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "traces ok: %d cases" % len(CASES) in out.stdout
