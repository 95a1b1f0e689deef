"""The code around the FFT passes (frame start, zcr ballots, amplitude range test, per-frame reductions, the mel
scan's DPP steps and stores, the frame loop's bounds) on the inputs that take each of its branches: 67 frames
(a ragged last batch of 4 and a ragged last group of 16) of seeded noise with a silent frame, a frame of
denormals, a NaN sample, an Inf sample, a frame of +-2^60 (the non-tame butterflies and the f64 amplitude path)
and a frame alternating +-0, every output requested, against the CPU oracle (tests/tolerance.py bars, zcr
exact) and byte for byte between two runs."""
import numpy as np
import pytest

import tolerance
from test_gpu_edge import FEATS, compare

pytestmark = pytest.mark.gpu

EVERY = FEATS + ["powerSpectrum", "complexSpectrum", "melBands"]
F = 67


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def frames(n):
    rng = np.random.default_rng(1000 + n)
    x = rng.uniform(-1, 1, (F, n)).astype(np.float32)
    x[3] = 0.0                                                           # silence
    x[9] = (x[9] * np.float32(1e-39)).astype(np.float32)                 # denormal samples
    x[14, n // 3] = np.nan                                               # one NaN sample
    x[22, 7] = np.inf                                                    # one Inf sample (test_gpu_edge's position)
    x[37] = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0).astype(np.float32) * np.float32(2.0 ** 60)
    x[65] = np.where(np.arange(n) % 2 == 0, 0.0, -0.0).astype(np.float32)  # +0, -0, +0, ...: no sign change counts
    return x


@pytest.fixture(scope="module", params=[256, 1024])
def case(request, capi, oracle_mod):
    n = request.param
    x = frames(n)
    ref = oracle_mod.extract(x, want_complex=True)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    return n, x, ref, plan.extract(x, EVERY), plan.extract(x, EVERY)


def test_against_oracle(case):
    n, x, ref, out, _ = case
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])  # exact, the NaN frame and the signed zeros included
    compare(out, ref, n)
    fin = np.isfinite(ref["amp"]).all(1) & np.isfinite(ref["complex_re"]).all(1) & np.isfinite(ref["complex_im"]).all(1)
    assert fin.sum() == F - 2  # every frame but the NaN and the Inf one
    for part, key in (("complexSpectrum.real", "complex_re"), ("complexSpectrum.imag", "complex_im")):
        bad, _ = tolerance.check_spectra(out[part][fin], ref[key][fin])
        assert not bad, (part, bad)
    # powerSpectrum.js: the float32 square of the amplitude
    a = out["amplitudeSpectrum"]
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.array_equal(out["powerSpectrum"], a * a, equal_nan=True)
    assert np.isfinite(a[37]).all()  # the 2^60 frame: huge, not overflowing


def test_two_runs_byte_identical(case):
    _, _, _, a, b = case
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
