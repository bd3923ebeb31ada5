"""The peak track through the Node layer: HipWorker.renderTrack (asynchronous and synchronous, `db` both ways), the addon's
renderTrack / renderTrackSync, HipWorker.rowFreq and js/cli.js --track-rows / --track-power / --track-db with --bands and --band-freqs,
against arrays written here from tests/trackref.py on the hopping capture of tests/test_track_gpu.py; a peak detector is refused with
status -4 and bad bands with -1, before anything is rendered (tests/js/check_track.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bandref
import meanref
import powerref
import trackref
from __graft_entry__ import ROOT, build
from oracle import pyoracle
from test_track_gpu import hopping

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")
GAIN, RANGE = 3.0, 45.0
FREQS = [(-0.125, 0.25), (0.0, 0.0), (0.3, 9.0)]

# (id, format, n, width, stride in samples, L/R split)
CASES = [
    ("cu8_256", "CU8", 256, 40, 256 // 2 + 3, False),
    ("cf32_1024", "CF32", 1024, 64, 1024 // 2 + 3, True),
]


def test_track_through_hipworker_the_addon_and_cli(tmp_path):
    if not os.path.exists(ADDON):
        build()
    d = str(tmp_path)
    cases = []
    for cid, fmt, n, width, stride, ch in CASES:
        data = hopping(fmt, n + (width - 1) * stride)
        data.tofile(os.path.join(d, cid + ".bin"))
        win, weight = pyoracle.window("hann", n)
        want = powerref.expected(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, width, ch)
        powerref.assert_telling(want["power"][:, 1:] if ch else want["power"], cid)          # (the split forces bin n/2, row 0, to zero)
        bands = bandref.standard_bands(n)
        from_freqs = [bandref.band_rows(n, lo, hi) for lo, hi in FREQS]
        rows, peaks = trackref.expected(want["power"], bands + from_freqs)
        assert len(np.unique(rows[2])) >= 8, cid
        rows.astype("<i4").tofile(os.path.join(d, cid + ".rows"))
        peaks.astype("<f8").tofile(os.path.join(d, cid + ".peaks"))
        meanref.db_of(peaks.reshape(-1), 1.0 / weight, GAIN).astype("<f8").tofile(os.path.join(d, cid + ".db"))
        cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "hann", "gain": GAIN,
                      "range": RANGE, "channelMode": ch, "rows": bands, "freqs": FREQS, "rowsOfFreqs": from_freqs})
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_track.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "track ok: %d cases" % len(CASES) in out.stdout
