"""bufferSize 4096 through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on the GPU:
`new Meyda(ctx, null, 4096)`, get() of a few features and getBatchSignal at hop 1024 return the values of the
C ABI call (through ctypes), bit for bit (tests/js/n4096_gpu.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_at_4096_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop = 4096, 1024
    x = np.random.default_rng(4096).uniform(-1, 1, 9 * hop + n + 77).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "n4096_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "n4096_gpu: 3 checks passed" in r.stdout
    plan = capi.Plan(buffer_size=n, scalar_f64=True)  # (the facade's plans use float64 scalars)
    try:
        ref = plan.extract_signal(x, hop, ["rms", "spectralCentroid", "mfcc", "amplitudeSpectrum"])
        one = plan.extract(x[2 * hop:2 * hop + n][None, :], ["rms", "spectralCentroid", "mfcc", "amplitudeSpectrum"])
    finally:
        plan.close()
    F = capi.signal_frames(x.size, n, hop)
    assert F == 10 and ref["rms"].shape == (F,)

    def same(a, b, what):
        a = a.reshape(b.shape)
        u = np.uint64 if b.dtype.itemsize == 8 else np.uint32
        assert a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u)), what

    assert (tmp_path / "scalar_bytes.txt").read_text() == "8"
    same(np.fromfile(tmp_path / "signal_rms.bin", np.float64), ref["rms"], "getBatchSignal rms")
    same(np.fromfile(tmp_path / "signal_centroid.bin", np.float64), ref["spectralCentroid"], "getBatchSignal spectralCentroid")
    same(np.fromfile(tmp_path / "signal_mfcc.f32", np.float32), ref["mfcc"], "getBatchSignal mfcc")
    same(np.fromfile(tmp_path / "signal_amp.f32", np.float32), ref["amplitudeSpectrum"], "getBatchSignal amplitudeSpectrum")
    same(np.fromfile(tmp_path / "get_amp_2.f32", np.float32), one["amplitudeSpectrum"], "get amplitudeSpectrum")
    same(np.fromfile(tmp_path / "get_mfcc_2.f32", np.float32), one["mfcc"], "get mfcc")
    same(np.fromfile(tmp_path / "get_scalars_2.f64", np.float64), np.array([one["rms"][0], one["spectralCentroid"][0]]), "get scalars")
