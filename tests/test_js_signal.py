"""The JavaScript facade's hopSize API (getBatchSignal, getBatchWav with a hop, Meyda.signalFrames) under Node:
its argument plumbing against a stand-in addon that records calls (no GPU), and its results on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


def run_node(script):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_facade_hop_size_host_side():
    out = run_node("facade_signal.js")
    assert "facade_signal: 6 checks passed" in out
    assert "ok Meyda.signalFrames agrees with the formula through the real addon" in out


@pytest.mark.gpu
def test_facade_hop_size_on_gpu():
    out = run_node("facade_signal_gpu.js")
    assert "facade_signal_gpu: 3 checks passed" in out
