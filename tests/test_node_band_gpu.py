"""The exact band-power series through the Node layer: HipWorker.renderBandPower (asynchronous and synchronous, `db` both ways), the
addon's renderBandPower / renderBandPowerSync / bandRows and js/cli.js --bandpower / --bandpower-db with --bands and --band-freqs,
against arrays written here from tests/bandref.py; a peak detector is refused with status -4 and bad bands with -1, before anything is
rendered (tests/js/check_band.js)."""
import json
import os
import shutil
import subprocess

import pytest

import bandref
import meanref
import powerref
import siggen
from __graft_entry__ import ROOT, build
from oracle import pyoracle

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GEN = {"kind": "trinoise", "seed": 2718, "step": 5003, "gshift": 10, "amp": 0.45, "namp": 0.03}
GAIN, RANGE = 3.0, 45.0
FREQS = [(-0.125, 0.25), (0.0, 0.0), (0.3, 9.0)]

# (id, format, n, width, stride in samples, L/R split)
CASES = [
    ("cu8_256", "CU8", 256, 40, 3 * 256 + 1, False),
    ("cf32_1024", "CF32", 1024, 64, 700, True),
]


def test_bandpower_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    d = str(tmp_path)
    cases = []
    for cid, fmt, n, width, stride, ch in CASES:
        data = siggen.generate(fmt, GEN, n + (width - 1) * stride)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        want = powerref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, width, ch)
        powerref.assert_telling(want["power"][:, 1:] if ch else want["power"], cid)          # (the split forces bin n/2, row 0, to zero)
        rows = bandref.standard_bands(n)
        from_freqs = [bandref.band_rows(n, lo, hi) for lo, hi in FREQS]
        series = bandref.expected(want["power"], rows + from_freqs)
        series.astype("<f8").tofile(os.path.join(d, cid + ".bands"))
        meanref.db_of(series.reshape(-1), 1.0 / weight, GAIN).astype("<f8").tofile(os.path.join(d, cid + ".db"))
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "hann", "gain": GAIN,
                      "range": RANGE, "channelMode": ch, "rows": rows, "freqs": FREQS, "rowsOfFreqs": from_freqs})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_band.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "band ok: %d cases" % len(CASES) in out.stdout
