"""getSignalSummaries / getSignalSummariesAsync with {flux: [...]} through the JavaScript facade
(meyda_amd/js/meyda.js) and the N-API addon on the GPU: the `flux` of three signals equals Plan.summarize_signals
with flux (mgx_summarize_flux_host through ctypes) bit for bit -- this test writes the binding's values to files,
tests/js/flux_gpu.js reads and compares them --, the async form equals the synchronous one, and the result without
the option is the existing call's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_flux_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    x = np.random.default_rng(53).uniform(-1, 1, 9 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 5 * n + 77, 5 * n + 77 + n - 1, 5 * n + 77 + n - 1 + n + hop]  # (as tests/js/flux_gpu.js cuts them)
    # (as tests/js/flux_gpu.js asks for them)
    flux = [dict(feature="melBands", per_frame=True), dict(feature="amplitudeSpectrum", mode="l2", lag=2, per_frame=True),
            dict(feature="mfcc", mode="l1", lag=8), dict(feature="loudness", mode="rectified", lag=1)]
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        base, fo, res = plan.summarize_signals([x[cuts[s]:cuts[s + 1]] for s in range(3)], hop, ["rms", "mfcc"], flux=flux)
    finally:
        plan.close()
    assert list(fo) == [0, 17, 17, 19] and len(res) == 4
    for i, r in enumerate(res):
        v = r["summary"]
        assert v.shape == (3, 4) and np.isnan(v[1]).all() and np.isfinite(v[[0, 2]]).all(), i
        assert v[2, 3] > 0  # the last signal has two buffers: its second row's flux is not zero
        for j, st in enumerate(capi.STATS):
            np.ascontiguousarray(v[:, j]).tofile(tmp_path / ("flux.%d.%s.f64" % (i, st)))
        if r["per_frame"] is not None:
            assert r["per_frame"].shape == (19,) and r["per_frame"].dtype == np.float32
            r["per_frame"].tofile(tmp_path / ("flux.%d.perFrame.f32" % i))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "flux_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "flux_gpu: 5 checks passed" in r.stdout
