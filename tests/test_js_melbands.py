"""'melBands' through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on the GPU: get(),
getBatchSignal and getBatchWav at a hop on one signal with 40 bands return the rows of the C ABI call
(mgx_extract_host_ex through ctypes), and options.devices throws (tests/js/melbands_gpu.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import wavgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_mel_bands_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    codes = wavgen.random_codes(np.random.default_rng(40), 20 * n + 77, 1, "s16")
    x = wavgen.decode(codes[:, 0], "s16")  # the signal is what the file decodes to
    x.tofile(tmp_path / "signal.f32")
    (tmp_path / "signal.wav").write_bytes(wavgen.wav_bytes(codes, "s16"))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "melbands_gpu.js"), str(tmp_path / "signal.f32"),
                        str(tmp_path / "signal.wav"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "melbands_gpu: 6 checks passed" in r.stdout
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)
    try:
        ref = plan.extract_signal(x, hop, ["melBands", "mfcc"])
        dense = plan.extract_signal(x, n, ["melBands"])
    finally:
        plan.close()

    def rows(name, width):
        return np.fromfile(tmp_path / name, np.float32).reshape(-1, width)

    def same(a, b, what):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what

    same(rows("signal_mel.f32", nm), ref["melBands"], "getBatchSignal melBands")
    same(rows("signal_mfcc.f32", 13), ref["mfcc"], "getBatchSignal mfcc")
    same(rows("get_mel_3.f32", nm), ref["melBands"][3:4], "get(['melBands'])")
    same(rows("wav_mel.f32", nm), ref["melBands"], "getBatchWav at a hop")
    same(rows("wav_dense_mel.f32", nm), dense["melBands"], "getBatchWav without a hop")
