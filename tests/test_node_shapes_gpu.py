"""The addon's reply shapes and refusals on one context (tests/js/check_addon_shapes.js gpu): per render entry point the well-formed
request - the reply's property names in order with each value's type, length, digest, byteOffset and buffer size - its callback form,
the request with one field broken at a time, a group handle and a destroyed handle, against the table recorded before the addon's reply
kinds were folded into shared readers and writers.  Every case is one request of 512 bytes or a refusal before any rendering."""
import os
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")


def test_addon_reply_shapes_and_refusals_hold_the_recorded_table():
    if not os.path.exists(ADDON):
        build()
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_addon_shapes.js"), "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "addon shapes ok (gpu): 384 cases, 40 exports" in out.stdout
