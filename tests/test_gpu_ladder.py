"""The magnitude ladder (tests/ladder.py) through every family of the frame kernel, against the CPU oracle.

kernels.hip chooses between code paths by the magnitude of what a frame holds (the f64 energy redo, the tame
or two-form butterflies, the rsq amplitude or slot_amp, the paired log or log2f, the segmented band sums or
nonfinite_frame_sums, ref_ln or the library log, the float32 stores of f64 scalars), each choice a ballot over
one frame. The ladder crosses every one of those thresholds: five base frames at every scale 2^k a float32
holds, 1,385 frames, in a seeded permutation so that the 4 frames of a wave's batch and the 16 of a group
belong to different regimes, plus 18 noise frames with one huge sample each. tests/test_ladder_host.py holds
the conditions that keep these tests from going vacuous; tests/test_oracle_golden.py pins the oracle to the
reference on the ladder itself.

Frames with a denormal float32 power (ladder.mel_excluded, from the oracle alone) are left out of the mfcc and
melBands value comparisons only: the reference's own mel sums have a few significant bits there
(tests/test_gpu_edge.py edge_frames). precision="fast" is not run through the ladder: its float32 amplitude
overflows above |X| = 2^64 and underflows below 2^-63, by design. tests/test_gpu_fast.py holds that mode to its
own contract (the exact transform within the float32 FFT bound, the features of the spectrum it returned) at
every buffer size and on every route, and states its magnitude range.
"""
import numpy as np
import pytest

import ladder
import tolerance
from test_gpu_edge import FEATS, SCALARS, SUBSETS, compare
from test_gpu_melbands import bins_of, device_run, restate
from test_gpu_parity import _mfcc_reference_checks
from test_gpu_signal import env_plan

pytestmark = pytest.mark.gpu

EVERY = FEATS + ["powerSpectrum", "complexSpectrum", "melBands"]
NOTIME = [f for f in FEATS if f not in ("rms", "energy", "zcr")]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


_REF, _RUN = {}, {}


def reference(oracle_mod, n, **kw):
    """The oracle on ladder.host_frames(n) (ladder order, then the outliers): computed once, never modified."""
    key = (n,) + tuple(sorted(kw.items()))
    if key not in _REF:
        ref = oracle_mod.extract(ladder.host_frames(n), **kw)
        for v in ref.values():
            v.setflags(write=False)
        ref["mel_ok"] = ~ladder.mel_excluded(ref["amp"])
        _REF[key] = ref
    return _REF[key]


def run(plan, n, feats, device=False):
    """The plan over the permuted ladder and the outliers; the rows back in ladder order."""
    x = ladder.gpu_frames(n)
    out = device_run(plan, x, feats) if device else plan.extract(x, feats)
    return {k: ladder.unpermute(v, n) for k, v in out.items()}


def default_run(capi, n):
    """Two runs of the default plan (float64 scalars) with every output requested, shared by the tests below."""
    if n not in _RUN:
        plan = capi.Plan(buffer_size=n, scalar_f64=True)
        try:
            _RUN[n] = (run(plan, n, EVERY), run(plan, n, EVERY))
        finally:
            plan.close()
    return _RUN[n]


def assert_same_up_to_nan_sign(got, ref, what):
    """Bit for bit, except that a NaN may differ in its sign (tests/test_gpu_parity.py
    test_scalar_windows_equal_per_batch_form)."""
    for k, v in got.items():
        if k not in ref:
            continue
        a, b = np.asarray(v), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        same = (a.view(np.uint8) == b.view(np.uint8)).reshape(a.shape + (-1,)).all(-1) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (what, k, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def against_oracle(oracle_mod, out, ref, n, sr=44100.0, num_mel=26):
    """test_gpu_edge.compare with its stated policy on every frame but those whose reference spectrum holds a
    float32 denormal (0 < a < 2^-126), DESIGN.md §6's exception. Down there the spectrum lives on the grid of
    2^-149: the reference rounds every butterfly output of its log2(N) stages to it, half a step each, and the
    kernel, which forms the same butterflies in another order, lands up to a few steps beside it (3 measured;
    nothing is flushed, the denormals are kept). A step is not small against such a bin, so no feature that
    weighs the bins (centroid, spread, loudness, ...) can meet a relative bar against the reference's value.
    On these frames, therefore: every bin within the unchanged norm-wise bar RTOL ||ref||_inf or, where that
    is finer than the grid itself, within log2(N) steps of 2^-149; and every feature against the oracle's
    features of the spectrum the GPU returned (oracle_features_from_amp), by the unchanged bars."""
    amp = ref["amp"].astype(np.float64)
    L = amp.shape[1]
    den = denormal_frames(ref)
    # DESIGN.md §6's two bins: where an infinity enters the reference's FFT before its last stage, its bins 0
    # and N/4 are NaN (0 x Inf) and the kernel's +-Inf, which compare() allows for. When the overflow is in
    # those bins alone (a loud DC on finite samples), what reads them differs the same way: loudness.total
    # Inf for NaN, perceptualSharpness 0 for NaN. The frames whose reference has a NaN in bin 0 or N/4 are
    # therefore held, by compare()'s own rules, to the oracle's features of the spectrum the GPU returned.
    two = np.isnan(amp[:, 0]) | np.isnan(amp[:, L // 2])
    assert two.sum() >= 1 and not (two & den).any()
    rest = ~den & ~two
    compare({k: v[rest] for k, v in out.items()}, {k: v[rest] for k, v in ref.items()}, n, sr=sr,
            mel_ok=ref["mel_ok"][rest])
    x = ladder.host_frames(n)
    own = dict(oracle_mod.features_from_amp(x[two], out["amplitudeSpectrum"][two], sample_rate=sr, num_mel=num_mel),
               amp=ref["amp"][two])
    compare({k: v[two] for k, v in out.items()}, own, n, sr=sr, mel_ok=ref["mel_ok"][two])
    assert 150 <= den.sum() <= 250, den.sum()  # (ladder.regimes: "denormal |X|")
    a = out["amplitudeSpectrum"][den]
    assert np.isfinite(a).all() and (a >= 0).all()
    bad = grid_bar(a, ref["amp"][den], n)
    assert not len(bad), np.nonzero(den)[0][bad][:10].tolist()
    own = oracle_mod.features_from_amp(x[den], a, sample_rate=sr, num_mel=num_mel)
    got_s = np.stack([out[k][den].astype(np.float64) for k in SCALARS], 1)
    fails = tolerance.check_scalars(got_s, own["scalars"], a, n, sr=sr)
    assert not fails, fails[:10]
    ok = ref["mel_ok"][den]
    assert not tolerance.check_vectors(out["mfcc"][den][ok], own["mfcc"][ok])
    assert not tolerance.check_vectors(out["loudness.specific"][den], own["loudness_specific"])


def denormal_frames(ref):
    """Frames whose reference amplitude spectrum holds a float32 denormal."""
    amp = ref["amp"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ((amp > 0) & (amp < 2.0 ** -126)).any(1)


def grid_bar(got, ref, n):
    """Rows of `got` further from `ref` than the norm-wise bar RTOL ||ref||_inf or, where that is finer than
    the float32 grid down there, than log2(N) steps of 2^-149."""
    g, r = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(g - r).max(1)
    bar = np.maximum(tolerance.RTOL * np.abs(r).max(1), np.log2(n) * 2.0 ** -149)
    return np.nonzero(~(err <= bar))[0]


# ------------------------------------------------------------------ a. the default plan against the oracle
@pytest.mark.parametrize("n", ladder.SIZES)
def test_default_plan_against_oracle(capi, oracle_mod, n):
    ref = reference(oracle_mod, n, want_complex=True)
    out, _ = default_run(capi, n)
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    against_oracle(oracle_mod, out, ref, n)
    # powerSpectrum.js: the float32 square of the amplitude
    a = out["amplitudeSpectrum"]
    with np.errstate(all="ignore"):
        p = a * a
    same = (out["powerSpectrum"].view(np.uint32) == p.view(np.uint32)) | (np.isnan(p) & np.isnan(out["powerSpectrum"]))
    assert same.all(), np.argwhere(~same)[:5].tolist()
    fin = np.isfinite(ref["amp"]).all(1) & np.isfinite(ref["complex_re"]).all(1) & np.isfinite(ref["complex_im"]).all(1)
    assert fin.sum() >= len(fin) - 40  # (the overflowing rungs only)
    den = denormal_frames(ref)
    for part, key in (("complexSpectrum.real", "complex_re"), ("complexSpectrum.imag", "complex_im")):
        bad, _ = tolerance.check_spectra(out[part][fin & ~den], ref[key][fin & ~den])
        assert not bad, (part, bad[:10])
        bad = grid_bar(out[part][den], ref[key][den], n)  # (the denormal spectra: against_oracle)
        assert not len(bad), (part, np.nonzero(den)[0][bad][:10].tolist())


@pytest.mark.parametrize("n", ladder.SIZES)
def test_default_plan_mel_bands_are_the_restatement(capi, oracle_mod, n):
    ok = reference(oracle_mod, n, want_complex=True)["mel_ok"]
    out, _ = default_run(capi, n)
    exp = restate(out["powerSpectrum"][ok], bins_of(capi, n, 26))
    mel = out["melBands"][ok]
    assert np.array_equal(tolerance._cls(mel), tolerance._cls(exp)), np.argwhere(tolerance._cls(mel) != tolerance._cls(exp))[:5].tolist()
    bad = tolerance.check_vectors(mel, exp)
    assert not bad, (n, np.nonzero(ok)[0][bad[:5]].tolist(), mel[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("n", ladder.SIZES)
def test_default_plan_two_runs_byte_identical(capi, n):
    a, b = default_run(capi, n)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------ b. float32 scalars
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_float32_scalars_are_the_rounded_float64_ones(capi, n):
    """The kernel stores (float)v: numpy's conversion is the reference for it. Overflow goes to Inf, float32
    denormal results are kept, a NaN is a NaN."""
    f64, _ = default_run(capi, n)
    plan = capi.Plan(buffer_size=n)
    try:
        f32 = run(plan, n, FEATS)
    finally:
        plan.close()
    for k in SCALARS:
        assert f32[k].dtype == np.float32 and f64[k].dtype == np.float64
        with np.errstate(all="ignore"):
            exp = f64[k].astype(np.float32)
        same = (f32[k].view(np.uint32) == exp.view(np.uint32)) | (np.isnan(f32[k]) & np.isnan(exp))
        bad = np.nonzero(~same)[0]
        assert not len(bad), (n, k, len(bad), bad[:5].tolist(), f32[k][bad[:5]], f64[k][bad[:5]])


# ------------------------------------------------------------------ c. the subset kernels
@pytest.mark.parametrize("n", [1024, 4096])
def test_subset_kernels_equal_the_full_request(capi, n):
    """SUB (test_gpu_edge.SUBSETS), LIGHT (a spectrum, the mfcc or the mel rows alone: light_nonfinite decides
    from the amplitudes' bits) and NOTIME (no rms / energy / zcr)."""
    full, _ = default_run(capi, n)
    sets = dict(SUBSETS, mfcc=["mfcc"], amp=["amplitudeSpectrum"], mel=["melBands"], notime=NOTIME)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        for name, feats in sets.items():
            assert_same_up_to_nan_sign(run(plan, n, feats), full, (n, name))
    finally:
        plan.close()


# ------------------------------------------------------------------ d. the reference-order MFCC
@pytest.mark.parametrize("bands", [26, 40])
@pytest.mark.parametrize("n", [512, 1024, 2048])
def test_reference_order_mfcc(capi, oracle_mod, n, bands):
    ref = reference(oracle_mod, n, num_mel=bands)
    ok = ref["mel_ok"]
    plan = capi.Plan(buffer_size=n, num_mel_bands=bands, mfcc_reference=True)
    try:
        out = run(plan, n, ["mfcc", "amplitudeSpectrum"])
    finally:
        plan.close()
    frac, nexact = _mfcc_reference_checks(out["mfcc"][ok], out["amplitudeSpectrum"][ok], ref["mfcc"][ok], ref["amp"][ok])
    print("N=%d bands=%d: reference-order MFCC bit-exact on %.4f of the coefficients, %d of %d frames with a "
          "bit-exact spectrum" % (n, bands, frac, nexact, int(ok.sum())))


# ------------------------------------------------------------------ e. other families
def test_hamming_40_bands_16k(capi, oracle_mod):
    n, sr = 1024, 16000.0
    ref = reference(oracle_mod, n, window="hamming", num_mel=40, sample_rate=sr)
    plan = capi.Plan(buffer_size=n, window="hamming", num_mel_bands=40, sample_rate=sr, scalar_f64=True)
    try:
        out = run(plan, n, FEATS)
    finally:
        plan.close()
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    against_oracle(oracle_mod, out, ref, n, sr=sr, num_mel=40)


def test_dct_sequential(capi, oracle_mod):
    n = 1024
    ref = reference(oracle_mod, n, want_complex=True)
    plan = capi.Plan(buffer_size=n, dct_sequential=True, scalar_f64=True)
    try:
        out = run(plan, n, FEATS)
    finally:
        plan.close()
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    against_oracle(oracle_mod, out, ref, n)


def test_literal_mode(capi, oracle_mod):
    n = 1024
    ref = reference(oracle_mod, n, literal=True)
    plan = capi.Plan(buffer_size=n, mode="literal", scalar_f64=True)
    try:
        out = run(plan, n, ["amplitudeSpectrum", "loudness"])
    finally:
        plan.close()
    a, r = out["amplitudeSpectrum"], ref["amp"]
    assert np.isfinite(r).all()  # |w x| of finite samples
    assert np.array_equal(a.view(np.uint32), r.view(np.uint32)), np.argwhere(a.view(np.uint32) != r.view(np.uint32))[:5].tolist()
    bad = tolerance.check_vectors(out["loudness.specific"], ref["loudness_specific"])
    assert not bad, bad[:10]


# ------------------------------------------------------------------ f. the scalar-window form
@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_scalar_window_form(capi, oracle_mod, n):
    """A grid capped at 4 workgroups: 1,403 frames are 88 batches >= 8 x 4, so the scalars run once per window of
    a wave's batches (plan.cpp scal_defer; kernels.hip scalar_pass). Against the uncapped plan's per-batch form
    up to a NaN's sign, and against the oracle directly."""
    ref = reference(oracle_mod, n, want_complex=True)
    capped = env_plan(capi, {"MGX_GRID_CAP": 4}, buffer_size=n, scalar_f64=True)
    plain = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = run(capped, n, FEATS, device=True)
        base = run(plain, n, FEATS, device=True)
    finally:
        capped.close()
        plain.close()
    assert sorted(got) == sorted(base)
    assert_same_up_to_nan_sign(got, base, (n, "MGX_GRID_CAP=4"))
    assert np.array_equal(got["zcr"], ref["scalars"][:, 2])
    against_oracle(oracle_mod, got, ref, n)


# ------------------------------------------------------------------ g. one frame per call
@pytest.mark.parametrize("n,kw", [(256, {}), (1024, {}), (2048, {}), (512, {"resident": True})],
                         ids=["256-kernarg", "1024-kernarg", "2048-small-batch", "512-resident"])
def test_one_frame_calls_equal_the_batch_rows(capi, n, kw):
    """One-frame host calls (N <= 1024: the frame inside the kernel arguments; 2048: the small-batch path; a
    resident plan: the workgroup that stays on the device) on both sides of every threshold."""
    full, _ = default_run(capi, n)
    x = ladder.ladder(n)
    plan = capi.Plan(buffer_size=n, scalar_f64=True, **kw)
    try:
        for b in ladder.ONE_FRAME_BASES:
            for k in ladder.ONE_FRAME_K:
                i = ladder.frame_index(k, b)
                one = plan.extract(x[i:i + 1], FEATS)
                assert_same_up_to_nan_sign(one, {key: v[i:i + 1] for key, v in full.items()}, (n, "base", b, "k", k))
    finally:
        plan.close()
