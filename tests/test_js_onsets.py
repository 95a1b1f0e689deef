"""getSignalOnsets / getSignalOnsetsAsync through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on
the GPU: the onsets of three signals equal Plan.onsets (mgx_onsets_host through ctypes) on the same signals -- this
test writes the binding's values to files, tests/js/onsets_gpu.js reads and compares them --, and the async form
equals the synchronous one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_onsets_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop, nm = 1024, 256, 40
    rng = np.random.default_rng(59)
    # noise whose level jumps every few thousand samples: bursts with clear onsets
    level = np.repeat(10.0 ** rng.uniform(-3, 0, 70), n)
    x = (rng.uniform(-1, 1, level.size) * level).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 40 * n + 77, 40 * n + 77 + n - 1, x.size]  # (as tests/js/onsets_gpu.js cuts them)
    lens = [cuts[s + 1] - cuts[s] for s in range(3)]
    starts, fo = capi.signals_frame_starts(lens, n, hop)
    # (as tests/js/onsets_gpu.js asks for them)
    params = dict(pre_max=3, post_max=3, pre_avg=8, post_avg=8, delta=0.5, wait=4)
    plan = capi.Plan(buffer_size=n, num_mel_bands=nm, scalar_f64=True)  # (the facade's plans: scalarF64)
    try:
        res = plan.onsets(x, starts, fo, feature="melBands", mode="rectified", lag=1, envelope=True, **params)
    finally:
        plan.close()
    offs, peaks = res["peak_offsets"], res["peaks"]
    assert offs[0] == 0 and offs[1] == offs[2] and offs[1] > 2 and offs[3] > offs[2] + 2 and peaks.size == offs[3]
    offs.astype(np.float64).tofile(tmp_path / "onsets.offsets.f64")
    peaks.astype(np.float64).tofile(tmp_path / "onsets.peaks.f64")
    res["envelope"].tofile(tmp_path / "onsets.envelope.f32")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "onsets_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "onsets_gpu: 4 checks passed" in r.stdout
