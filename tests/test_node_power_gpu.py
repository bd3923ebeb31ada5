"""Power plane replies through the Node layer: HipWorker.renderPower (asynchronous and synchronous, `db` both ways), the addon's
renderPowerSync and js/cli.js --power / --power-db against planes written here from tests/powerref.py; a peak detector is refused with
status -4, an unknown one with -1, before anything is rendered (tests/js/check_power.js)."""
import json
import os
import shutil
import subprocess

import pytest

import powerref
import siggen
from __graft_entry__ import ROOT, build
from oracle import pyoracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GEN = {"kind": "trinoise", "seed": 1618, "step": 5003, "gshift": 10, "amp": 0.45, "namp": 0.03}

# (id, format, n, width, stride in samples, L/R split): k_frames_power and the portable kernel, overlapping and sparse
CASES = [
    ("cu8_256", "CU8", 256, 44, 3 * 256 + 1, False),
    ("cf32_1024", "CF32", 1024, 36, 700, True),
    ("cs16_2048", "CS16", 2048, 12, 2048 + 5, False),
]


def test_power_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    d = str(tmp_path)
    cases = []
    for cid, fmt, n, width, stride, ch in CASES:
        data = siggen.generate(fmt, GEN, n + (width - 1) * stride)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        want = powerref.expected(fmt, data, n, win, 1.0 / weight, 3.0, 45.0, width, ch)
        powerref.assert_telling(want["power"][:, 1:] if ch else want["power"], cid)          # (the split forces bin n/2, row 0, to zero)
        want["power"].astype("<f8").tofile(os.path.join(d, cid + ".power"))
        want["db"].astype("<f8").tofile(os.path.join(d, cid + ".db"))
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "hann", "gain": 3.0,
                      "range": 45.0, "channelMode": ch})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_power.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "power ok: %d cases" % len(CASES) in out.stdout
