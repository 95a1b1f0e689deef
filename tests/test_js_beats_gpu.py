"""getSignalBeats / getSignalBeatsAsync through the JavaScript facade (meyda_amd/js/meyda.js) and the N-API addon on
the GPU: the lags, the beat lists and the envelope of three signals equal Plan.beats_signals (mgx_beats_host through
ctypes) on the same signals -- this test writes the binding's values to files, tests/js/beats_gpu.js reads and
compares them --, and the async form equals the synchronous one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")


@pytest.mark.gpu
def test_facade_beats_on_gpu(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    from meyda_amd import capi
    n, hop = 256, 64
    rng = np.random.default_rng(67)
    x = rng.uniform(-0.05, 0.05, 1000 * hop + 3 * n).astype(np.float32)
    for at in range(0, x.size - n, 24 * hop):  # a click every 24 buffers
        x[at:at + 32] += rng.uniform(-1, 1, 32).astype(np.float32)
    x.tofile(tmp_path / "signal.f32")
    cuts = [0, 600 * hop + n + 7, 600 * hop + n + 7 + n - 1, x.size]  # (as tests/js/beats_gpu.js cuts them)
    signals = [x[cuts[s]:cuts[s + 1]] for s in range(3)]
    plan = capi.Plan(buffer_size=n, scalar_f64=True, num_mel_bands=40)  # (the facade's plans: scalarF64)
    try:
        kw = dict(win_length=64, num_lags=48, start_bpm=1722.65625, max_bpm=0.0)
        res = plan.beats_signals(signals, hop, envelope=True, **kw)
        loose = plan.beats_signals(signals, hop, trim=False, **kw)
    finally:
        plan.close()
    fo, off = res["frame_offsets"], res["peak_offsets"]
    assert list(fo[:3]) == [0, 601, 601] and res["lag"].shape == (3,) and off.shape == (4,)
    assert res["lag"][1] == 0 and off[1] == off[2] and (res["lag"][[0, 2]] > 0).all() and off[1] > 5 and off[3] - off[2] > 5
    res["lag"].tofile(tmp_path / "beats.lag.u32")
    off.tofile(tmp_path / "beats.offsets.u64")
    res["beats"].tofile(tmp_path / "beats.rows.u64")
    res["envelope"].tofile(tmp_path / "beats.envelope.f32")
    loose["beats"].tofile(tmp_path / "loose.rows.u64")
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "beats_gpu.js"), str(tmp_path / "signal.f32"), str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "beats_gpu: 4 checks passed" in r.stdout
