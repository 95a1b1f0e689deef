"""melBands -- the log mel band energies (mfcc.js:53-65), feature 19 of the C ABI and an auxiliary output
(mgx_aux_outputs of the mgx_extract_*_ex calls) -- as far as it can be checked without a device: the
feature registry, the bindings' name lists, the facade's featureInfo and the argument checks that run
before any device call."""
import ctypes
import os
import shutil
import subprocess

import pytest

from meyda_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_feature_registry():
    L = capi.lib()
    assert L.mgx_feature_index(b"melBands") == 19
    assert L.mgx_feature_name(19) == b"melBands"
    assert L.mgx_feature_info(19) == 1  # MGX_TYPE_ARRAY
    assert L.mgx_feature_name(20) is None and L.mgx_feature_info(20) == -1
    # indices 0..18 did not move
    assert L.mgx_feature_index(b"mfcc") == 14 and L.mgx_feature_index(b"buffer") == 18
    assert L.mgx_abi_version() == 2


def test_binding_name_lists():
    assert capi.FEATURE_NAMES[19] == "melBands" and len(capi.FEATURE_NAMES) == 20
    assert "melBands" not in capi.ALL_FEATURES
    for sym in ("mgx_extract_device_ex", "mgx_extract_host_ex", "mgx_extract_host_pcm_ex"):
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    assert ctypes.sizeof(capi.AuxOutputs) == 16


def test_ex_calls_refuse_null_plan_or_outputs():
    L = capi.lib()
    o = capi.Outputs()
    a = capi.AuxOutputs()
    a.struct_size = ctypes.sizeof(capi.AuxOutputs)
    assert L.mgx_extract_device_ex(None, None, 0, 1, ctypes.byref(o), ctypes.byref(a), None) == -1
    assert b"NULL" in L.mgx_last_error()
    assert L.mgx_extract_host_ex(None, None, 0, 1, ctypes.byref(o), ctypes.byref(a)) == -1
    assert L.mgx_extract_host_pcm_ex(None, None, 0, 0, 0, 1, 0, 1, ctypes.byref(o), ctypes.byref(a)) == -1


def test_host_outputs_carry_the_aux_struct():
    """"melBands" by name gives an (F, num_mel_bands) float32 array and an AuxOutputs riding on the Outputs;
    without it the Outputs is as it was (no aux: the existing entry points are called)."""
    class P:  # (what Plan._host_outputs reads, without a device)
        n = 512
        scalar_dtype = "float32"
        desc = capi.make_desc(buffer_size=512, num_mel_bands=40)
    out, o = capi.Plan._host_outputs(P, 7, ["mfcc", "melBands"])
    assert out["melBands"].shape == (7, 40) and out["melBands"].dtype.name == "float32"
    assert o.aux.struct_size == 16 and o.aux.reserved == 0 and o.aux.mel_bands == out["melBands"].ctypes.data
    out, o = capi.Plan._host_outputs(P, 7, ["mfcc"])
    assert capi._aux(o) is None


def test_facade_feature_info():
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    js = ("const fi = require(%r); if (JSON.stringify(fi.melBands) !== JSON.stringify({type: 'array'})) process.exit(1);"
          "if (fi.mfcc.type !== 'array' || Object.keys(fi).length !== 19) process.exit(2); console.log('ok');"
          % os.path.join(ROOT, "meyda_amd", "js", "feature-info.js"))
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
