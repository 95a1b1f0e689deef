"""The host paths walk the output arrays by a table of fields (meyda_amd/csrc/out_fields.h). What a table can
get wrong is one field: its bytes per frame, its place in the layout after a field that is absent, its words in
the one-frame wait, its copy back. So every field is requested alone (the complex spectrum as its pair) through
mgx_extract_host_ex, on each host path -- 1 frame (the wait on the output words; for a spectrum the completion
word), 2 frames (the one-launch path with its completion word), 513 frames (one past small_max: the staged
path) -- in both scalar widths, and sparse subsets with a middle field of the layout absent and present, also on
an MGX_FLAG_RESIDENT plan around a request the resident workgroup does not serve.

Every comparison is byte equality with the same field of one all-fields call on the same frames (that call is
held to the oracle by test_gpu_parity.py and test_gpu_melbands.py), and every array that was not requested must
keep the bytes the test put there.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NMEL, NCOEF = 512, 26, 13
FMAX = 513
FILL = 0xA5
MEL = 19  # the field after mgx_outputs' 19 (mgx_aux_outputs.mel_bands)
# one request per field, the complex spectrum as its pair
SINGLES = [(i,) for i in range(17)] + [(17, 18), (MEL,)]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(0x6F7574).uniform(-1, 1, (FMAX, N)).astype(np.float32)


def widths(capi, f64):
    """(elements per frame, dtype) of the 20 fields, in field order."""
    sd = np.float64 if f64 else np.float32
    return ([(1, sd)] * capi.NUM_SCALARS + [(capi.NUM_BARK, np.float32), (NCOEF, np.float32), (N // 2, np.float32),
                                            (N // 2, np.float32), (N, np.float32), (N, np.float32), (NMEL, np.float32)])


def run(capi, plan, f64, x, want):
    """The fields `want` of the frames x through mgx_extract_host_ex: all 20 arrays, preset to FILL."""
    F = x.shape[0]
    arrays = []
    for per, dt in widths(capi, f64):
        a = np.empty((F, per), dt)
        a.view(np.uint8)[...] = FILL
        arrays.append(a)
    o = capi.Outputs()
    aux = capi.AuxOutputs(ctypes.sizeof(capi.AuxOutputs), 0, None)
    names = ["loudness_specific", "mfcc", "amplitude_spectrum", "power_spectrum", "complex_real", "complex_imag"]
    for i in want:
        if i < capi.NUM_SCALARS:
            o.scalars[i] = arrays[i].ctypes.data
        elif i < MEL:
            setattr(o, names[i - capi.NUM_SCALARS], arrays[i].ctypes.data)
        else:
            aux.mel_bands = arrays[i].ctypes.data
    capi.check(capi.lib().mgx_extract_host_ex(plan._h, x.ctypes.data, F * N, N, ctypes.byref(o), ctypes.byref(aux)))
    return arrays


def check(got, ref, want, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        if i in want:
            assert np.array_equal(g.view(np.uint8), r.view(np.uint8)), (what, "field", i, g, r)
        else:
            assert (g.view(np.uint8) == FILL).all(), (what, "field", i, "was not requested")


def make_plan(capi, f64, **kw):
    return capi.Plan(buffer_size=N, num_mel_bands=NMEL, num_mfcc_coeffs=NCOEF, scalar_f64=f64, **kw)


@pytest.mark.parametrize("F", [1, 2, FMAX])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_each_field_alone(capi, frames, f64, F):
    x = frames[:F]
    plan = make_plan(capi, f64)
    try:
        ref = run(capi, plan, f64, x, range(20))
        check(ref, ref, range(20), "all fields")
        for want in SINGLES:
            check(run(capi, plan, f64, x, want), ref, want, (F, want))
    finally:
        plan.close()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_sparse_subsets_and_the_resident_plan(capi, frames, f64):
    """rms, mfcc, mel_bands of one frame: with mfcc, the middle field of the three, absent and present; and on an
    MGX_FLAG_RESIDENT plan without mel_bands (the resident workgroup), with it (a launch, which ends the resident
    one), without it again (a resident workgroup under the same key)."""
    x = frames[:1]
    plain = make_plan(capi, f64)
    res = make_plan(capi, f64, resident=True)
    try:
        ref = run(capi, plain, f64, x, range(20))
        for want in [(0, MEL), (0, 14, MEL)]:
            check(run(capi, plain, f64, x, want), ref, want, ("plain", want))
        for want in [(0, 14), (0, 14, MEL), (0, 14)]:
            check(run(capi, res, f64, x, want), ref, want, ("resident", want))
    finally:
        res.close()
        plain.close()
