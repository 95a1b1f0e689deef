"""The tempo API of the JavaScript facade (meyda_amd/js/meyda.js) without a GPU: getSignalTempo's arguments, defaults
and bpm arithmetic against a stand-in addon that records its calls (tests/js/tempo_facade.js with
tests/js/tempo_addon.js), and Meyda.tempogramWindow and Meyda.tempoPrior through the built N-API addon against the
values tests/tempo_ref.py computes in this test run and passes in as JSON (tests/js/tempo_cpu.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tempo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")

WINDOWS = [2, 3, 64, 384, 1000, 1024]
# (frameRate, numLags, the facade's options, tempo_ref.prior_ref's keywords)
PRIORS = [(172.265625, 384, None, {}),
          (689.0625, 1024, {}, {}),
          (86.1328125, 100, {"startBpm": 90, "stdOctaves": 0.5}, dict(start_bpm=90.0, std_octaves=0.5)),
          (31.25, 8, {"maxBpm": 0}, dict(max_bpm=0.0)),
          (1000.0, 1, {"maxBpm": 10}, dict(max_bpm=10.0))]


def node(script, *args):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", script), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_facade_tempo_plumbing():
    assert "tempo_facade: 5 checks passed" in node("tempo_facade.js")


def test_facade_window_and_prior(tmp_path):
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    cases = {"windows": [{"winLength": w, "bits": tempo_ref.window_ref(w).view(np.uint32).tolist()} for w in WINDOWS], "priors": []}
    for rate, L, options, kw in PRIORS:
        case = {"frameRate": rate, "numLags": L, "values": tempo_ref.prior_ref(rate, L, **kw).tolist()}
        if options is not None:
            case["options"] = options
        cases["priors"].append(case)
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    assert "tempo_cpu: 3 checks passed" in node("tempo_cpu.js", str(tmp_path / "cases.json"))
