"""precision="fast" (MGX_PRECISION_FAST: float32 butterflies, a float32 twiddle table, at N = 512 .. 2048 that
table staged in LDS, a float32 amplitude) held to its contract at every buffer size and on every route. The
contract (tests/fast_ref.py states its first item without the kernel; tests/test_fast_host.py holds the
conditions that keep these tests from going vacuous):

1. amplitudeSpectrum and complexSpectrum are within (7 log2 N + 2) 2^-24 of the exact transform of the windowed
   frame in relative 2-norm, per frame: the bound of a float32 radix-2 FFT, about ten times what honest float32
   arithmetic gives and orders of magnitude below a wrong twiddle.
2. amplitudeSpectrum is within the project's norm-wise bar of the CPU oracle's (tolerance.check_spectra).
3. powerSpectrum is the float32 square of amplitudeSpectrum, bit for bit.
4. Every feature behind the spectrum is the oracle's feature of the spectrum the GPU returned
   (oracle.features_from_amp), under the unchanged policy of tests/tolerance.py; melBands is the restatement
   (tests/test_gpu_melbands.py restate) of the returned powerSpectrum. The mode's features do NOT promise the
   oracle's own values off broadband input: a small bin carries the spectrum's error, absolute in the frame's
   norm, into a logarithm. tools/fast_precision_report.py measures by how much (profiles/fast_precision.txt).
5. rms, energy and zcr never see the FFT: the faithful plan's bits.

The mode's magnitude range. Every operation of the fast path is a float32 one, so a frame scaled by 2^k gives
the k = 0 spectra scaled by 2^k bit for bit while no intermediate leaves float32's normal range (test 4: k = -40
.. 40 on frames whose bins span 2^10). The amplitude is sqrtf(re^2 + im^2) with the squares in float32: a bin
with |X| >= 2^64 overflows to Inf, one below 2^-63 has a denormal square (a few significant bits) and one below
2^-75 is returned as 0 -- where the faithful precision, which squares in double, returns every amplitude a
float32 holds. |X| is at most sqrt(N) / 2 of the largest sample, so samples within about [2^-50, 2^57] keep every
bin that is within 2^-10 of the frame's largest inside the range.
"""
import numpy as np
import pytest

import fast_ref
import tolerance
from test_gpu_edge import FEATS, SCALARS, compare
from test_gpu_gather import gather_vs_dense
from test_gpu_ladder import assert_same_up_to_nan_sign
from test_gpu_melbands import bins_of, device_run, restate, same_bits, same_dict
from test_gpu_signal import SPECTRA, dense_frames, env_plan, signal

pytestmark = pytest.mark.gpu

SIZES = fast_ref.SIZES
EVERY = FEATS + ["powerSpectrum", "complexSpectrum", "melBands"]
NONFINITE = {9: "nan", 22: "+inf", 41: "-inf"}  # frame: the sample it gets (three different batches of 4)


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


_RUN, _REF = {}, {}


def fast_plan(capi, n, **kw):
    return capi.Plan(buffer_size=n, precision="fast", **dict({"scalar_f64": True}, **kw))


def fast_run(capi, n):
    """The dense device launch of the fast plan (26 bands, float64 scalars) over fast_ref.frames(n) with every
    output requested: run once, shared, never modified."""
    if n not in _RUN:
        plan = fast_plan(capi, n)
        try:
            out = device_run(plan, fast_ref.frames(n), EVERY)
        finally:
            plan.close()
        for v in out.values():
            v.setflags(write=False)
        _RUN[n] = out
    return _RUN[n]


def reference(oracle_mod, n):
    """The oracle on fast_ref.frames(n): computed once, never modified."""
    if n not in _REF:
        ref = oracle_mod.extract(fast_ref.frames(n), want_complex=True)
        for v in ref.values():
            v.setflags(write=False)
        _REF[n] = ref
    return _REF[n]


def plan_window(capi, n, **kw):
    return capi.host_tables(buffer_size=n, **kw)["window"]


def assert_exact(out, ex, what):
    """Item 1 on the amplitude and the complex spectrum; returns the two worst ratios to the bar."""
    bad_a, worst_a = fast_ref.check_exact(out["amplitudeSpectrum"], ex)
    bad_c, worst_c = fast_ref.check_exact(fast_ref.complex_of(out), ex)
    print("%s: worst ||got - exact||_2 / (bar ||exact||_2): amplitude %.4f, complex %.4f (bar %.3g)"
          % (what, worst_a, worst_c, fast_ref.spectrum_bar(ex.shape[1])))
    assert not bad_a, (what, "amplitudeSpectrum", bad_a[:10], worst_a)
    assert not bad_c, (what, "complexSpectrum", bad_c[:10], worst_c)
    return worst_a, worst_c


def assert_power_is_the_square(out, what):
    a = out["amplitudeSpectrum"]
    with np.errstate(all="ignore"):
        p = a * a
    same = (out["powerSpectrum"].view(np.uint32) == p.view(np.uint32)) | (np.isnan(p) & np.isnan(out["powerSpectrum"]))
    assert same.all(), (what, np.argwhere(~same)[:5].tolist())


def assert_features_of_own_spectrum(oracle_mod, capi, out, x, n, rows=None, sr=44100.0, bands=26, **kw):
    """Item 4: the features against the oracle's features of the returned spectrum (test_gpu_edge.compare), and
    melBands against the restatement of the returned power spectrum."""
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    amp = out["amplitudeSpectrum"][rows]
    own = dict(oracle_mod.features_from_amp(x[rows], amp, sample_rate=sr, num_mel=bands), amp=amp)
    compare({k: v[rows] for k, v in out.items()}, own, n, sr=sr)
    exp = restate(out["powerSpectrum"][rows], bins_of(capi, n, bands, sample_rate=sr, **kw))
    mel = out["melBands"][rows]
    assert np.array_equal(tolerance._cls(mel), tolerance._cls(exp)), (n, np.argwhere(tolerance._cls(mel) != tolerance._cls(exp))[:5].tolist())
    bad = tolerance.check_vectors(mel, exp)
    assert not bad, (n, bands, rows[bad[:5]].tolist(), mel[bad[0]], exp[bad[0]])


# ------------------------------------------------------------------ 1. the spectra
@pytest.mark.parametrize("n", SIZES)
def test_spectra(capi, oracle_mod, n):
    x = fast_ref.frames(n)
    w = plan_window(capi, n)
    out, ref = fast_run(capi, n), reference(oracle_mod, n)
    assert out["amplitudeSpectrum"].shape == (fast_ref.F, n // 2) and out["complexSpectrum.real"].shape == (fast_ref.F, n)
    assert_exact(out, fast_ref.exact(x, w), "N=%d" % n)
    bad, exact = tolerance.check_spectra(out["amplitudeSpectrum"], ref["amp"])
    g, r = out["amplitudeSpectrum"].astype(np.float64), ref["amp"].astype(np.float64)
    live = np.abs(r).max(1) > 0
    print("N=%d: against the oracle, worst ||d||_inf / ||ref||_inf %.3g (bar %g), bit-exact fraction %.4f"
          % (n, (np.abs(g - r).max(1)[live] / np.abs(r).max(1)[live]).max(), tolerance.RTOL, exact))
    assert not bad, bad
    assert_power_is_the_square(out, n)
    sil = np.nonzero(fast_ref.silent_rows(x, w))[0]
    assert len(sil) == 3  # the silent frame and, under hanning, the two impulses at the frame's ends
    for k in ("amplitudeSpectrum", "powerSpectrum", "complexSpectrum.real", "complexSpectrum.imag"):
        assert not out[k][sil].any(), (n, k)


# ------------------------------------------------------------------ 2. the features
@pytest.mark.parametrize("bands", [26, 40])
@pytest.mark.parametrize("n", SIZES)
def test_features(capi, oracle_mod, n, bands):
    x = fast_ref.frames(n)
    if bands == 26:
        out = fast_run(capi, n)
    else:
        plan = fast_plan(capi, n, num_mel_bands=bands)
        try:
            out = device_run(plan, x, EVERY)
        finally:
            plan.close()
        same_dict({k: v for k, v in out.items() if k not in ("mfcc", "melBands")},
                  {k: v for k, v in fast_run(capi, n).items() if k not in ("mfcc", "melBands")}, (n, "40 bands beside 26"))
    assert_features_of_own_spectrum(oracle_mod, capi, out, x, n, bands=bands)
    # item 5: the faithful plan's bits
    plan = capi.Plan(buffer_size=n, scalar_f64=True, num_mel_bands=bands)
    f32 = fast_plan(capi, n, num_mel_bands=bands, scalar_f64=False)
    try:
        faithful = device_run(plan, x, EVERY)
        single = device_run(f32, x, FEATS)
    finally:
        plan.close()
        f32.close()
    ref = reference(oracle_mod, n)
    for k in ("rms", "energy", "zcr"):
        assert out[k].dtype == np.float64 and np.array_equal(out[k].view(np.uint64), faithful[k].view(np.uint64)), (n, k)
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    # float32 scalars: the float64 ones through numpy's conversion
    for k in SCALARS:
        assert single[k].dtype == np.float32
        with np.errstate(all="ignore"):
            exp = out[k].astype(np.float32)
        same = (single[k].view(np.uint32) == exp.view(np.uint32)) | (np.isnan(single[k]) & np.isnan(exp))
        bad = np.nonzero(~same)[0]
        assert not len(bad), (n, k, bad[:5].tolist(), single[k][bad[:5]], out[k][bad[:5]])
    for k in ("amplitudeSpectrum", "mfcc", "loudness.specific"):
        same_bits(single[k], out[k], (n, k, "float32 scalars"))


@pytest.mark.parametrize("n", [512, 2048])
def test_hamming_40_bands_16k(capi, oracle_mod, n):
    sr, bands = 16000.0, 40
    x = fast_ref.frames(n)
    kw = dict(window="hamming", sample_rate=sr, num_mel_bands=bands)
    plan = fast_plan(capi, n, **kw)
    try:
        out = device_run(plan, x, EVERY)
    finally:
        plan.close()
    ex = fast_ref.exact(x, plan_window(capi, n, window="hamming"))
    assert_exact(out, ex, "N=%d hamming" % n)
    ref = oracle_mod.extract(x, sample_rate=sr, window="hamming", num_mel=bands)
    bad, _ = tolerance.check_spectra(out["amplitudeSpectrum"], ref["amp"])
    assert not bad, bad
    assert_power_is_the_square(out, n)
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    assert_features_of_own_spectrum(oracle_mod, capi, out, x, n, sr=sr, bands=bands, window="hamming")


# ------------------------------------------------------------------ 3. non-finite samples and isolation
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_samples_stay_in_their_frames(capi, oracle_mod, n):
    x = fast_ref.frames(n).copy()
    x[9, n // 3] = np.nan
    x[22, 7] = np.inf
    x[41, n - 1] = -np.inf
    rows = sorted(NONFINITE)
    plan = fast_plan(capi, n)
    try:
        out = device_run(plan, x, EVERY)
    finally:
        plan.close()
    assert np.isnan(out["amplitudeSpectrum"][9]).all()
    assert not np.isfinite(out["amplitudeSpectrum"][[22, 41]]).any()
    assert np.array_equal(out["zcr"][rows], oracle_mod.extract(x[rows])["scalars"][:, 2])
    assert_power_is_the_square(out, n)
    assert_features_of_own_spectrum(oracle_mod, capi, out, x, n, rows=rows)
    rest = np.setdiff1d(np.arange(fast_ref.F), rows)
    same_dict({k: v[rest] for k, v in out.items()}, {k: v[rest] for k, v in fast_run(capi, n).items()}, (n, "the other frames"))


# ------------------------------------------------------------------ 4. scale equivariance
@pytest.mark.parametrize("n", SIZES)
def test_spectra_scale_with_the_frame(capi, n):
    """x 2^k gives the spectra x 2^k, bit for bit, for k = -40, -20, 20, 40: float32 throughout and nothing leaves
    the normal range (the header; tests/test_fast_host.py test_scale_frames_have_no_small_bins is the condition)."""
    x0 = fast_ref.spread_frames(n)
    e = np.abs(fast_ref.exact(x0, plan_window(capi, n)))
    assert (e.min(1) >= 2.0 ** -10 * e.max(1)).all() and (e > 0).all()
    ks = [0, -40, -20, 20, 40]
    x = np.concatenate([np.ldexp(x0, k).astype(np.float32) for k in ks])
    plan = fast_plan(capi, n)
    try:
        out = device_run(plan, x, ["amplitudeSpectrum", "complexSpectrum"])
    finally:
        plan.close()
    m = len(x0)
    for i, k in enumerate(ks[1:], 1):
        for key, v in out.items():
            assert np.isfinite(v).all()
            same_bits(v[i * m:(i + 1) * m], np.ldexp(v[:m], k), (n, k, key))


# ------------------------------------------------------------------ 5. the routes
@pytest.mark.parametrize("n", SIZES)
def test_routes_equal_the_dense_launch(capi, n):
    """The signal launch, the gather launch and the host path against the dense device launch of the same plan,
    bit for bit; a one-frame call is that row of the batch; asking for melBands changes nothing else."""
    F = fast_ref.F
    fr = fast_ref.frames(n)
    sig = np.concatenate([fr.reshape(-1), signal(2 * n, n)])
    base = fast_run(capi, n)
    plan = fast_plan(capi, n)
    try:
        for hop in (63, n // 4, n + 1):
            x = sig[:(F - 1) * hop + n + 5]
            d = dense_frames(x, n, hop)
            assert d.shape[0] == F
            dense = device_run(plan, d, EVERY)
            same_dict(device_run(plan, x, EVERY, hop), dense, (n, "signal launch", hop))
            if hop == n // 4:
                gather_vs_dense(plan, x, np.arange(F, dtype=np.uint64) * hop, EVERY, (n, "gather at f hop"))
                st = np.random.default_rng(n).integers(0, x.size - n + 1, F).astype(np.uint64)
                st[5], st[6], st[40], st[66] = st[4], st[4], x.size - n, 0
                gather_vs_dense(plan, x, st, EVERY, (n, "gather, shuffled and repeated starts"))
        for count in (1, 3, 5, F):
            same_dict(plan.extract(fr[:count], EVERY), {k: v[:count] for k, v in base.items()}, (n, "host path", count))
        for i in (9, 40, 66):
            same_dict(plan.extract(fr[i:i + 1], EVERY), {k: v[i:i + 1] for k, v in base.items()}, (n, "one-frame call", i))
            one = plan.extract(fr[i:i + 1], ["spectralCentroid", "mfcc"])  # (no spectrum: the call waits on its output words)
            same_dict(one, {k: base[k][i:i + 1] for k in one}, (n, "one-frame call without a spectrum", i))
        without = device_run(plan, fr, FEATS + SPECTRA[1:])
        same_dict(without, {k: base[k] for k in without}, (n, "without melBands"))
    finally:
        plan.close()


# ------------------------------------------------------------------ 6. the large-launch regime
def many_frames(n, F):
    """fast_ref.frames(n) over and over (67 is odd: a frame's lane, batch and group change with every repeat)."""
    reps = -(-F // fast_ref.F)
    return np.tile(fast_ref.frames(n), (reps, 1))[:F], np.tile(np.arange(fast_ref.F), reps)[:F]


def against_chunks(capi, n, env, small_env, F, chunk):
    x, idx = many_frames(n, F)
    big = env_plan(capi, env, buffer_size=n, precision="fast", scalar_f64=True)
    small = env_plan(capi, small_env, buffer_size=n, precision="fast", scalar_f64=True)
    try:
        got = device_run(big, x, EVERY)
        parts = [device_run(small, x[i:i + chunk], EVERY) for i in range(0, F, chunk)]
    finally:
        big.close()
        small.close()
    ref = {k: np.concatenate([p[k] for p in parts]) for k in got}
    assert sorted(got) == sorted(ref)
    assert_same_up_to_nan_sign(got, ref, (n, env))
    ex = fast_ref.exact(fast_ref.frames(n), plan_window(capi, n))[idx]
    assert_exact(got, ex, "N=%d %s" % (n, env))
    assert_power_is_the_square(got, (n, env))


@pytest.mark.parametrize("n", [256, 1024, 2048])
def test_large_launch_regime(capi, n):
    """A grid capped at 8 workgroups: 3,001 frames are 12+ groups per workgroup and 8+ batches per wave (the scalar
    windows, the many-group shares, at N = 2048 the tail pool), against chunks of 512 on an uncapped plan."""
    against_chunks(capi, n, {"MGX_GRID_CAP": 8}, {}, 3001, 512)


def test_tail_pool_at_4096(capi):
    """N = 4096 with half the groups taken by ticket (MGX_POOL_PCT, tests/test_gpu_melbands.py
    test_tail_pool_stolen_batches), against launches of 997 without the pool."""
    against_chunks(capi, 4096, {"MGX_POOL_PCT": 50}, {"MGX_POOL_PCT": 0}, 1001, 997)


# ------------------------------------------------------------------ 7. the literal mode at N = 256
def test_literal_mode_n256(capi, oracle_mod):
    """The one size at which mode="literal" (|w x| for a spectrum, no transform) had neither a fixture nor an oracle
    test."""
    n, F = 256, 37
    x = oracle_mod.synth_frames(fast_ref.SEED, 0, F, n)
    ref = oracle_mod.extract(x, literal=True)
    plan = capi.Plan(buffer_size=n, mode="literal", scalar_f64=True)
    try:
        out = plan.extract(x, ["amplitudeSpectrum", "loudness", "rms", "zcr"])
    finally:
        plan.close()
    same_bits(out["amplitudeSpectrum"], ref["amp"], "literal amplitudes")
    assert not tolerance.check_vectors(out["loudness.specific"], ref["loudness_specific"])
    assert np.allclose(out["loudness.total"], ref["scalars"][:, 10], rtol=1e-6, atol=0)
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
