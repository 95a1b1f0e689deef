"""getSignalHpss / getSignalHpssAsync through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on the
GPU: the two parts, the chroma of the harmonic part, the flux of the percussive part and the summaries of three
signals equal Plan.hpss_signals (mgx_hpss_host through ctypes) on the same signals bit for bit -- this test writes the
binding's values to files, tests/js/hpss_gpu.js reads and compares them --, and the async form equals the synchronous
one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_hpss_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop = 1024, 128
    x = np.random.default_rng(67).uniform(-1, 1, 17 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 9 * n + 77, 9 * n + 77 + n - 1, x.size]  # (as tests/js/hpss_gpu.js cuts them)
    signals = [x[cuts[s]:cuts[s + 1]] for s in range(3)]
    plan = capi.Plan(buffer_size=n, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        # (as tests/js/hpss_gpu.js asks for them)
        res = plan.hpss_signals(signals, hop, kernel_size=(17, 31), margin=(2.0, 1.5), harmonic=True, percussive=True,
                                chroma=dict(summary=True), flux=dict(mode="rectified", lag=2, summary=True))
        hard = plan.hpss_signals(signals, hop, power=float("inf"), percussive=True)
    finally:
        plan.close()
    fo = res["frame_offsets"]
    F = int(fo[3])
    assert list(fo[:3]) == [0, 65, 65] and F > 100 and res["harmonic"].shape == (F, n // 2) and res["chroma"].shape == (F, 12)
    assert np.isnan(res["flux_summary"][1]).all() and np.isfinite(res["flux_summary"][[0, 2]]).all()
    assert (res["harmonic"] != 0).any() and (res["percussive"] != 0).any() and (hard["percussive"] == 0).any()
    for k in ("harmonic", "percussive", "chroma", "flux"):
        res[k].tofile(tmp_path / ("hpss.%s.f32" % k))
    hard["percussive"].tofile(tmp_path / "hard.percussive.f32")
    for j, st in enumerate(capi.STATS):
        np.ascontiguousarray(res["chroma_summary"][:, j, :]).tofile(tmp_path / ("hpss.chroma.%s.f64" % st))
        np.ascontiguousarray(res["flux_summary"][:, j]).tofile(tmp_path / ("hpss.flux.%s.f64" % st))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "hpss_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "hpss_gpu: 4 checks passed" in r.stdout
