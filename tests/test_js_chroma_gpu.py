"""getSignalChroma / getSignalChromaAsync through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on
the GPU: the chroma rows and the summaries of three signals equal Plan.chroma_signals (mgx_chroma_host through
ctypes) on the same signals bit for bit -- this test writes the binding's values to files, tests/js/chroma_gpu.js
reads and compares them --, and the async form equals the synchronous one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_chroma_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop = 1024, 256
    x = np.random.default_rng(61).uniform(-1, 1, 9 * n).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 5 * n + 77, 5 * n + 77 + n - 1, x.size]  # (as tests/js/chroma_gpu.js cuts them)
    signals = [x[cuts[s]:cuts[s + 1]] for s in range(3)]
    plan = capi.Plan(buffer_size=n, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        res = plan.chroma_signals(signals, hop, summary=True)
        # (as tests/js/chroma_gpu.js asks for them)
        r13 = plan.chroma_signals(signals, hop, norm="none", num_chroma=13, octave_width=0.0, base_c=False)
    finally:
        plan.close()
    fo = res["frame_offsets"]
    assert list(fo) == [0, 17, 17, 25] and res["chroma"].shape == (25, 12) and r13["chroma"].shape == (25, 13)
    assert res["summary"].shape == (3, 4, 12) and np.isnan(res["summary"][1]).all() and np.isfinite(res["summary"][[0, 2]]).all()
    res["chroma"].tofile(tmp_path / "chroma.rows.f32")
    r13["chroma"].tofile(tmp_path / "chroma13.rows.f32")
    for j, st in enumerate(capi.STATS):
        np.ascontiguousarray(res["summary"][:, j, :]).tofile(tmp_path / ("chroma.%s.f64" % st))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "chroma_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "chroma_gpu: 4 checks passed" in r.stdout
