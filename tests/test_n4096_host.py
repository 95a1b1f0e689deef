"""bufferSize 4096 without a GPU: what mgx_plan_create accepts and refuses ahead of the device, the oracle
pinned to the reference at this size (tests/golden/N4096/, the checks tests/test_oracle_golden.py makes for
512..2048), the library's host tables against the oracle's, and the frame arithmetic of the signal paths.
"""
import numpy as np
import pytest

import golden_n4096
import tolerance

N = 4096
E_UNSUPPORTED, E_NO_DEVICE = -3, -6


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    return capi


def create_error(capi, **kw):
    """The MgxError of a plan creation that must fail, or None (with the plan closed) when it succeeds."""
    try:
        plan = capi.Plan(**kw)
    except capi.MgxError as e:
        return e
    plan.close()
    return None


# ------------------------------------------------------------------ mgx_plan_create, ahead of the device
def test_4096_passes_the_range_check(capi):
    """Without a device the 4096 plan gets as far as the device check (MGX_E_NO_DEVICE), not the range
    check's MGX_E_UNSUPPORTED; with one it is created."""
    e = create_error(capi, buffer_size=N)
    if capi.device_count() == 0:
        assert e is not None and e.status == E_NO_DEVICE, e
    else:
        assert e is None, e


def test_8192_is_refused_with_the_new_range(capi):
    e = create_error(capi, buffer_size=8192)
    assert e is not None and e.status == E_UNSUPPORTED and "256..4096" in str(e), e


def test_128_is_still_refused(capi):
    e = create_error(capi, buffer_size=128)
    assert e is not None and e.status == E_UNSUPPORTED, e


@pytest.mark.parametrize("kw,flag", [(dict(mfcc_reference=True), "MGX_FLAG_MFCC_REFERENCE"),
                                     (dict(resident=True), "MGX_FLAG_RESIDENT")], ids=["mfcc_reference", "resident"])
def test_flags_without_a_4096_form_are_refused(capi, kw, flag):
    """Refused by name and size, ahead of the device as the range check is -- never dropped silently."""
    e = create_error(capi, buffer_size=N, **kw)
    assert e is not None and e.status == E_UNSUPPORTED, e
    assert flag in str(e) and "4096" in str(e), e
    # (the fast precision and the literal mode ignore MGX_FLAG_MFCC_REFERENCE at the other sizes: refused here too)
    if "mfcc_reference" in kw:
        for more in (dict(precision="fast"), dict(mode="literal")):
            e = create_error(capi, buffer_size=N, **kw, **more)
            assert e is not None and e.status == E_UNSUPPORTED and flag in str(e), (more, e)


def test_the_flags_keep_their_sizes_below(capi):
    """2048 with either flag still passes every check ahead of the device."""
    for kw in (dict(mfcc_reference=True), dict(resident=True)):
        e = create_error(capi, buffer_size=2048, **kw)
        assert e is None or e.status == E_NO_DEVICE, (kw, e)


# ------------------------------------------------------------------ the oracle against the reference
@pytest.fixture(scope="module")
def golden():
    return golden_n4096.load()


@pytest.fixture(scope="module")
def oracle_out(golden, oracle_mod):
    return oracle_mod.extract(golden["input"], want_complex=True)


def test_fixture_families(golden):
    lab = golden["labels"]
    assert golden["F"] == len(lab) == golden["input"].shape[0] and golden["input"].shape[1] == N
    assert len([l for l in lab if l.startswith("noise:")]) == 8
    for s in ("sound1", "sound2", "sound3"):
        assert len([l for l in lab if l.startswith(s + ":")]) >= 4
    assert {"edge:zeros", "edge:square", "edge:tiny", "edge:loud", "edge:signedZeros"} <= set(lab)
    assert golden["hamming_frames"][:4] == [0, 1, 2, 3] and golden["literal_frames"] == [0, 1, 2, 3]


def test_tables_bit_exact(golden, oracle_mod):
    t = oracle_mod.tables(N)
    for k in ("hann", "hamming", "bark", "bblimits", "mel_bins", "mel_values", "mel_freq", "dct", "twiddle_seeds"):
        assert np.array_equal(t[k].view(np.uint8), golden[k].view(np.uint8)), k
    t40 = oracle_mod.tables(N, num_mel=40)
    assert np.array_equal(t40["mel_bins"], golden["mel40_bins"])
    assert np.array_equal(t40["dct"].view(np.uint32), golden["dct40"].view(np.uint32))


def test_amplitude_bit_exact(golden, oracle_out):
    assert np.array_equal(oracle_out["amp"].view(np.uint32), golden["amp"].view(np.uint32))


def test_complex_spectrum_bit_exact(golden, oracle_out):
    c = golden["complex_frames"]
    assert np.array_equal(oracle_out["complex_re"][:c].view(np.uint32), golden["complex_re"].view(np.uint32))
    assert np.array_equal(oracle_out["complex_im"][:c].view(np.uint32), golden["complex_im"].view(np.uint32))


def test_scalars(golden, oracle_out):
    got, ref = oracle_out["scalars"], golden["scalars"]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True)
    rel = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
    assert rel.max() <= 1e-12
    assert not tolerance.check_scalars(got, ref, golden["amp"], N)


def test_vectors_bit_exact(golden, oracle_out):
    assert np.array_equal(oracle_out["loudness_specific"].view(np.uint32), golden["loudness_specific"].view(np.uint32))
    assert np.array_equal(oracle_out["mfcc"].view(np.uint32), golden["mfcc"].view(np.uint32))


def test_mfcc40_bit_exact(golden, oracle_mod):
    o = oracle_mod.extract(golden["input"], num_mel=40)
    assert np.array_equal(o["mfcc"].view(np.uint32), golden["mfcc40"].view(np.uint32))


def test_hamming_window(golden, oracle_mod):
    o = oracle_mod.extract(golden["input"][golden["hamming_frames"]], window="hamming")
    assert np.array_equal(o["amp"].view(np.uint32), golden["hamming_amp"].view(np.uint32))
    assert np.array_equal(o["mfcc"].view(np.uint32), golden["hamming_mfcc"].view(np.uint32))
    assert not tolerance.check_scalars(o["scalars"], golden["hamming_scalars"], golden["hamming_amp"], N)


def test_literal_snapshot_mode(golden, oracle_mod):
    o = oracle_mod.extract(golden["input"][golden["literal_frames"]], literal=True)
    assert np.array_equal(o["amp"].view(np.uint32), golden["literal_amp"].view(np.uint32))
    assert np.array_equal(o["loudness_specific"].view(np.uint32), golden["literal_loudness_specific"].view(np.uint32))
    assert np.array_equal(o["scalars"][:, 10], golden["literal_loudness_total"])


def test_synth_matches_golden_noise(golden, oracle_mod):
    noise = [i for i, l in enumerate(golden["labels"]) if l.startswith("noise:")]
    x = oracle_mod.synth_frames(0x6D657964, 0, len(noise), N)
    assert np.array_equal(x.view(np.uint32), golden["input"][noise].view(np.uint32))


# ------------------------------------------------------------------ the library's host tables
@pytest.mark.parametrize("sr", [44100.0, 8000.0, 96000.0])
@pytest.mark.parametrize("nmel", [1, 26, 40, 64])
def test_host_tables_against_the_oracle(capi, oracle_mod, nmel, sr):
    t = capi.host_tables(buffer_size=N, num_mel_bands=nmel, sample_rate=sr)
    o = oracle_mod.tables(N, sample_rate=sr, num_mel=nmel)
    for mine, theirs in (("hanning", "hann"), ("hamming", "hamming"), ("bark_scale", "bark"), ("bark_limits", "bblimits"),
                         ("mel_bins", "mel_bins"), ("dct", "dct")):
        assert np.array_equal(np.ascontiguousarray(t[mine]).view(np.uint8), np.ascontiguousarray(o[theirs]).view(np.uint8)), mine
    assert np.array_equal(t["window"].view(np.uint32), t["hanning"].view(np.uint32))
    ham = capi.host_tables(buffer_size=N, window="hamming")
    assert np.array_equal(ham["window"].view(np.uint32), ham["hamming"].view(np.uint32))
    assert t["bark_limits"][0] == 0 and t["bark_limits"][-1] <= N // 2 and np.all(np.diff(t["bark_limits"]) >= 0)


# ------------------------------------------------------------------ frame arithmetic
def test_signal_frames_at_4096(capi):
    assert capi.signal_frames(N - 1, N, 1024) == 0
    assert capi.signal_frames(N, N, 1024) == 1
    assert capi.signal_frames(N + 1023, N, 1024) == 1
    assert capi.signal_frames(N + 1024, N, 1024) == 2
    assert capi.signal_frames(10 * N, N, N) == 10
    assert capi.signal_frames(32775 + N, N, 1) == 32776  # the host path's first chunk seam plus 8
    for S, hop in ((123457, 300), (1 << 20, 1024), (5 * N + 7, N + 1)):
        assert capi.signal_frames(S, N, hop) == (S - N) // hop + 1


def test_signals_frame_starts_at_4096(capi):
    lengths = [N - 1, N, 3 * N + 5, 0, 2 * N]
    hop = 1024
    starts, fo = capi.signals_frame_starts(lengths, N, hop)
    exp_counts = [0 if l < N else (l - N) // hop + 1 for l in lengths]
    assert fo.tolist() == np.concatenate([[0], np.cumsum(exp_counts)]).tolist()
    exp, base = [], 0
    for l, c in zip(lengths, exp_counts):
        exp += [base + k * hop for k in range(c)]
        base += l
    assert starts.tolist() == exp
    assert all(s + N <= sum(lengths) for s in exp)
