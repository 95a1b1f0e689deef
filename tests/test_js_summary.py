"""getSignalSummaries / getSignalSummariesAsync through the JavaScript facade (meyda_amd/js/meyda.js) and the
N-API addon on the GPU: three signals pooled per signal equal Plan.summarize_signals (mgx_summarize_host through
ctypes) bit for bit, and the async form equals the synchronous one (tests/js/summary_gpu.js)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_summaries_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    x = np.random.default_rng(43).uniform(-1, 1, 9 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "summary_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "summary_gpu: 2 checks passed" in r.stdout
    cuts = [0, 5 * n + 77, 5 * n + 77 + n - 1, 5 * n + 77 + n - 1 + n + hop]  # (as tests/js/summary_gpu.js cuts them)
    feats = ["rms", "spectralRolloff", "mfcc", "melBands", "loudness", "powerSpectrum"]
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        ref, fo = plan.summarize_signals([x[cuts[s]:cuts[s + 1]] for s in range(3)], hop, feats)
    finally:
        plan.close()
    assert fo.tolist() == [0, 17, 17, 19]
    assert set(ref) == {"rms", "spectralRolloff", "mfcc", "melBands", "loudness.specific", "loudness.total", "powerSpectrum"}
    for k, v in ref.items():
        for j, st in enumerate(capi.STATS):
            a = np.fromfile(tmp_path / ("%s.%s.f64" % (k, st)), np.float64).reshape(3, -1)
            b = np.ascontiguousarray(v[:, j, :])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (k, st)
