"""getSignalSummaries / getSignalSummariesAsync with {deltaWidth, deltaOrder} through the JavaScript facade
(meyda_amd/js/meyda.js) and the N-API addon on the GPU: `delta` and `delta2` of three signals equal
Plan.summarize_signals with deltas (mgx_summarize_deltas_host through ctypes) bit for bit -- this test writes the
binding's values to files, tests/js/delta_gpu.js reads and compares them --, the async form equals the synchronous
one, and the result without the option is the existing call's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_delta_summaries_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    x = np.random.default_rng(47).uniform(-1, 1, 9 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 5 * n + 77, 5 * n + 77 + n - 1, 5 * n + 77 + n - 1 + n + hop]  # (as tests/js/delta_gpu.js cuts them)
    feats = ["rms", "spectralRolloff", "mfcc", "melBands", "loudness"]
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        base, rows, d1, d2 = plan.summarize_signals([x[cuts[s]:cuts[s + 1]] for s in range(3)], hop, feats, deltas=(2, 2))
    finally:
        plan.close()
    assert rows == {} and set(base) == set(d1) == set(d2) == {"rms", "spectralRolloff", "mfcc", "melBands", "loudness.specific",
                                                               "loudness.total"}
    for order, summ in (("base", base), ("delta", d1), ("delta2", d2)):
        for k, v in summ.items():
            assert v.shape[:2] == (3, 4) and np.isnan(v[1]).all() and np.isfinite(v[[0, 2]]).all(), (order, k)
            for j, st in enumerate(capi.STATS):
                np.ascontiguousarray(v[:, j, :]).tofile(tmp_path / ("%s.%s.%s.f64" % (order, k, st)))
    # the last signal has two buffers: its deltas are not all zero (the files hold something to compare)
    assert (d1["mfcc"][2, 3] > 0).any() and (d2["mfcc"][0, 1] > 0).all()
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "delta_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "delta_gpu: 4 checks passed" in r.stdout
