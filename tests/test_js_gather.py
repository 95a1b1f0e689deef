"""getBatchSignals / getBatchGather through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on
the GPU: three signals in one call equal the per-signal getBatchSignal results and the C ABI call's rows
(mgx_extract_gather_host through ctypes), frameOffsets is right, the async forms agree, and options.devices
throws (tests/js/gather_gpu.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_signals_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    x = np.random.default_rng(41).uniform(-1, 1, 9 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "gather_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "gather_gpu: 4 checks passed" in r.stdout
    cuts = [0, 5 * n + 77, 5 * n + 77 + n - 1, 5 * n + 77 + n - 1 + n + hop]  # (as tests/js/gather_gpu.js cuts them)
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)
    try:
        ref, fo = plan.extract_signals([x[cuts[s]:cuts[s + 1]] for s in range(3)], hop, ["melBands", "mfcc"])
    finally:
        plan.close()
    assert fo.tolist() == [0, 17, 17, 19]

    def same(name, width, b, what):
        a = np.fromfile(tmp_path / name, np.float32).reshape(-1, width)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what

    same("signals_mel.f32", nm, ref["melBands"], "getBatchSignals melBands")
    same("signals_mfcc.f32", 13, ref["mfcc"], "getBatchSignals mfcc")
