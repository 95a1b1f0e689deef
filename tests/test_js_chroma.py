"""Meyda.chromaFilterBank through the JavaScript facade (meyda_amd/js/meyda.js) and the built N-API addon, without a
GPU: the bank equals, within one unit of the last place per entry, the values tests/chroma_ref.py computes in this
test run and passes in as JSON (tests/js/chroma_cpu.js), and the facade's and the addon's refusals."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import chroma_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")

# (bufferSize, sampleRate, the facade's options, chroma_ref.weights' keywords)
CASES = [(256, 44100, None, {}),
         (1024, 44100, {}, {}),
         (1024, 16000, {"numChroma": 12, "baseC": False}, dict(num_chroma=12, base_c=False)),
         (1024, 44100, {"numChroma": 13, "octaveWidth": 0}, dict(num_chroma=13, octave_width=0.0)),
         (256, 16000, {"numChroma": 36}, dict(num_chroma=36)),
         (256, 44100, {"numChroma": 1, "baseC": False, "octaveWidth": 0}, dict(num_chroma=1, base_c=False, octave_width=0.0)),
         (4096, 44100, {"a440": 432, "centerOctave": 4, "octaveWidth": 1.5}, dict(a440=432.0, center_octave=4.0, octave_width=1.5)),
         (4096, 16000, {"numChroma": 24, "baseC": True}, dict(num_chroma=24, base_c=True))]


def test_facade_chroma_filter_bank(tmp_path):
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    cases = []
    for n, sr, options, kw in CASES:
        w = chroma_ref.weights(n, float(sr), **kw)
        case = {"bufferSize": n, "sampleRate": sr, "bits": w.view(np.uint32).ravel().tolist()}
        if options is not None:
            case["options"] = options
        cases.append(case)
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "chroma_cpu.js"), str(tmp_path / "cases.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "chroma_cpu: 3 checks passed" in r.stdout
