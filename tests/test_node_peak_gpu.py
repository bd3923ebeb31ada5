"""The peak detector through the Node layer: HipWorker.postMessage, renderNamed, renderSliced per slice and js/cli.js --detector peak
against expected replies built from the oracle (tests/peakref.py); unknown detectors end in onerror (tests/js/check_peak.js)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import peakref
import siggen
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GEN = {"kind": "trinoise", "seed": 2718, "step": 5003, "gshift": 10, "amp": 0.45, "namp": 0.03}

# (id, format, n, M, width, extra samples, L/R split, waterfall): frames_peak and the portable kernel, integer and fractional strides
CASES = [
    ("cu8_256", "CU8", 256, 3, 44, 0, False, False),
    ("cf32_1024", "CF32", 1024, 2, 36, 5, False, True),
    ("cs16_2048", "CS16", 2048, 3, 10, 3, True, False),
]


def _named_lut(pkg, cmap):
    _, key, L = pkg.binding.named_resolve("hann", cmap)
    lut = np.zeros((L, 3), np.uint8)
    got = C.c_int32()
    assert pkg.Library.get().L.sp_cmap(key.encode(), lut.ctypes.data_as(C.c_void_p), L, C.byref(got)) == 0
    lut[0] = 0
    lut[-1] = 255
    return lut


def _js_number(v):
    """A double as a string JavaScript's Number() reads back exactly (JSON has no infinities)."""
    v = float(v)
    return "NaN" if v != v else "Infinity" if v == float("inf") else "-Infinity" if v == float("-inf") else repr(v)


def _dump(d, name, want):
    for key, ext in (("rgba", "rgba"), ("gauge_mins", "gmin"), ("gauge_maxs", "gmax"), ("gauge_amps", "gamp")):
        want[key].tofile(os.path.join(d, "%s.%s" % (name, ext)))
    with open(os.path.join(d, name + ".json"), "w") as fh:
        json.dump({"c_hist": [int(v) for v in want["c_hist"]], "cB_hist": [int(v) for v in want["cB_hist"]],
                   "dBfs_min": _js_number(want["dBfs_min"]), "dBfs_max": _js_number(want["dBfs_max"])}, fh, allow_nan=False)


def test_peak_detector_through_hipworker_render_named_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    pkg = load_package()
    d = str(tmp_path)
    lut = _named_lut(pkg, "viridis")
    cases = []
    for cid, fmt, n, M, width, extra, ch, wf in CASES:
        data = siggen.generate(fmt, GEN, n + (width - 1) * M * n + extra)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        want = peakref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 45.0, lut, width, ch, wf)
        assert want["M"] == M and all(c == M for c in want["counts"][:-1])
        _dump(d, cid, want)
        sw = peakref.SW[fmt]
        for k in range(2):                       # the caller's two slices (lib/samples.js:253-258), each its own request
            b0, b1 = pyoracle.slice_bounds(data.size, sw, k, 2)
            ws = peakref.expected(fmt, data[b0:b1], n, win, 1.0 / weight, 3.0, 45.0, lut, width // 2, ch, wf)
            assert ws["M"] >= 2
            _dump(d, "%s.s%d" % (cid, k), ws)
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "M": M, "last": want["counts"][-1],
                      "window": "hann", "cmap": "viridis", "gain": 3.0, "range": 45.0, "channelMode": ch, "waterfall": wf})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_peak.js"), d], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "peak ok: %d cases" % len(CASES) in out.stdout
