"""The persistence spectrum through the Node layer: HipWorker.renderDensity / renderDensitySync, the addon's renderDensitySync and
js/cli.js --density against fixtures written here from the oracle (tests/densityref.py) and confirmed against Context.render_density;
malformed messages end in onerror with status -1 / -4 and never in counts (tests/js/check_density.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import densityref
import peakref
import siggen
from __graft_entry__ import ROOT, build, load_package
from oracle import pyoracle
from test_launch_shapes_gpu import _lut
from test_node_index_gpu import CASES, GAIN, GEN, RANGE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")


def test_density_replies_through_hipworker_the_addon_and_cli(tmp_path):
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
            density = densityref.expected(want, n, len(lut), width, wf)
            got = ctx.render_density(fmt, data, n, win, 1.0 / weight, GAIN, RANGE, lut, width, ch, wf, detector=det or "sample")
            assert np.array_equal(got, density), cid                            # the Python result is the fixture
            assert (density.sum(axis=1) == width).all() and np.array_equal(density.sum(axis=0), want["c_hist"])
            density.astype("<u4").tofile(os.path.join(d, cid + ".density"))
            np.minimum(density, 65535).astype(">u2").tofile(os.path.join(d, cid + ".pgm_body"))   # what cli.js --density writes
            lut.tofile(os.path.join(d, cid + ".lut"))
            cases.append({"id": cid, "file": cid + ".bin", "format": fmt.lower(), "n": n, "width": width, "window": "blackmanHarris",
                          "gain": GAIN, "range": RANGE, "channelMode": ch, "waterfall": wf, "detector": det, "cli": cli})
    finally:
        ctx.close()
    with open(os.path.join(d, "cases.json"), "w") as fh:
        json.dump(cases, fh)
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_density.js"), d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "density ok: %d cases" % len(CASES) in out.stdout
