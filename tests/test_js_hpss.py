"""The HPSS API of the JavaScript facade (meyda_amd/js/meyda.js) without a GPU: getSignalHpss' arguments, defaults,
result shapes and refusals against a stand-in addon that records its calls (tests/js/hpss_facade.js with
tests/js/hpss_addon.js)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def node(script, *args):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", script), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_facade_hpss_plumbing():
    assert "hpss_facade: 4 checks passed" in node("hpss_facade.js")
