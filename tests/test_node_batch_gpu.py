"""Batches through the Node layer: renderMany and the addon's renderBatch / renderBatchSync (sp_render_batch), js/cli.js --out-dir."""
import os
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT, build

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")]
ADDON = os.path.join(ROOT, "spectroplot-js_amd", "lib", "spectroplot_hip.node")


def test_render_many_cli_out_dir_and_malformed_items():
    if not os.path.exists(ADDON):
        build()
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "check_batch.js")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch ok" in out.stdout
