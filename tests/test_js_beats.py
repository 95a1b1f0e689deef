"""The beat API of the JavaScript facade (meyda_amd/js/meyda.js) without a GPU: getSignalBeats' arguments, defaults and
per-signal lists against a stand-in addon that records its calls (tests/js/beats_facade.js with
tests/js/beats_addon.js), and Meyda.beatTables through the built N-API addon against the values tests/beat_ref.py
computes in this test run and passes in as JSON (tests/js/beats_cpu.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import beat_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")

# (maxPeriod, the facade's tightness or None for its default)
TABLES = [(1, None), (2, 100.0), (7, 400.0), (64, 37.5)]


def node(script, *args):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", script), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_facade_beats_plumbing():
    assert "beats_facade: 5 checks passed" in node("beats_facade.js")


def test_facade_tables(tmp_path):
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    cases = {"tables": []}
    for P, tightness in TABLES:
        gauss, penalty = beat_ref.tables(P, 100.0 if tightness is None else tightness)
        cases["tables"].append({"maxPeriod": P, "tightness": tightness, "gaussBits": gauss.view(np.uint32).tolist(),
                                "penalty": [None if np.isneginf(v) else float(v) for v in penalty]})
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    assert "beats_cpu: 2 checks passed" in node("beats_cpu.js", str(tmp_path / "cases.json"))
