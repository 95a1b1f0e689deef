"""bufferSize 4096 on the GPU: the fused kernel's N = 4096 instances (32 slots per lane, three passes, two
workgroups per CU) and every path that leads to them, against the CPU oracle (tests/tolerance.py bars, zcr
exact, the amplitude spectrum bit for bit on noise), against the reference's own outputs
(tests/golden/N4096/) and against each other byte for byte. The shapes are the smallest that reach each
mechanism: 37 frames (three workgroups, a partial batch), the schedule's corner counts, a grid capped at 8
workgroups for the many-group shares, the scalar windows and the tail pool.
"""
import numpy as np
import pytest

import golden_n4096
import tolerance
import wavgen
from test_gpu_edge import compare
from test_gpu_melbands import (SENTINEL, bins_of, check_against_small_launches, device_frames, device_run, restate,
                               same_bits, same_dict)
from test_gpu_signal import SPECTRA, dense_frames, env_plan, signal

pytestmark = pytest.mark.gpu

N = 4096
SEED = 0x6D657964
FEATS = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope",
         "spectralRolloff", "spectralSpread", "spectralSkewness", "spectralKurtosis", "loudness",
         "perceptualSpread", "perceptualSharpness", "mfcc", "amplitudeSpectrum", "powerSpectrum", "complexSpectrum"]
SCALARS = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope",
           "spectralRolloff", "spectralSpread", "spectralSkewness", "spectralKurtosis",
           "loudness.total", "perceptualSpread", "perceptualSharpness"]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


@pytest.fixture(scope="module")
def frames37(oracle_mod):
    x = oracle_mod.synth_frames(SEED, 0, 37, N)
    x.setflags(write=False)
    return x


def against_oracle(out, ref, sr=44100.0, exact_amp=True):
    """check_scalars, check_vectors, check_spectra (amplitude, power, complex) and zcr exact."""
    gs = np.stack([out[k].astype(np.float64) for k in SCALARS], 1)
    fails = tolerance.check_scalars(gs, ref["scalars"], ref["amp"], N, sr=sr)
    assert not fails, fails[:10]
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    bad, exact = tolerance.check_spectra(out["amplitudeSpectrum"], ref["amp"])
    print("amplitude spectrum: bit-exact fraction %.6f" % exact)
    assert not bad, bad
    if exact_amp:
        assert exact == 1.0, exact
    power = (ref["amp"] * ref["amp"]).astype(np.float32)  # powerSpectrum.js on the Float32Array
    assert not tolerance.check_spectra(out["powerSpectrum"], power)[0]
    if "complex_re" in ref:
        assert not tolerance.check_spectra(out["complexSpectrum.real"], ref["complex_re"])[0]
        assert not tolerance.check_spectra(out["complexSpectrum.imag"], ref["complex_im"])[0]
    assert not tolerance.check_vectors(out["mfcc"], ref["mfcc"])
    assert not tolerance.check_vectors(out["loudness.specific"], ref["loudness_specific"])


# ------------------------------------------------------------------ 1. parity with the oracle
VARIANTS = [dict(), dict(sample_rate=8000.0), dict(sample_rate=96000.0), dict(window="hamming"), dict(scalar_f64=False),
            dict(num_mel_bands=1), dict(num_mel_bands=40), dict(num_mel_bands=64), dict(dct_sequential=True)]


@pytest.mark.parametrize("kw", VARIANTS, ids=["default", "sr8000", "sr96000", "hamming", "scalar_f32", "mel1", "mel40",
                                              "mel64", "dct_sequential"])
def test_parity_with_the_oracle(capi, oracle_mod, frames37, kw):
    kw = dict({"scalar_f64": True}, **kw)
    ref = oracle_mod.extract(frames37, sample_rate=kw.get("sample_rate", 44100.0), window=kw.get("window", "hanning"),
                             num_mel=kw.get("num_mel_bands", 26), want_complex=True)
    plan = capi.Plan(buffer_size=N, **kw)
    try:
        out = device_run(plan, frames37, FEATS)
    finally:
        plan.close()
    assert out["rms"].dtype == (np.float64 if kw["scalar_f64"] else np.float32)
    if not kw["scalar_f64"]:  # float32 scalar arrays: the oracle's doubles stored to float32 (rolloff is held exact)
        ref = dict(ref, scalars=ref["scalars"].astype(np.float32).astype(np.float64))
    against_oracle(out, ref, sr=kw.get("sample_rate", 44100.0))


def test_against_the_reference_fixtures(capi):
    """The GPU against tests/golden/N4096/ directly (the reference under node), as tests/test_gpu_parity.py does
    at the other sizes: every frame within policy, zcr exact, the noise frames' spectrum bit for bit."""
    g = golden_n4096.load()
    plan = capi.Plan(buffer_size=N, scalar_f64=True)
    ham = capi.Plan(buffer_size=N, scalar_f64=True, window="hamming")
    try:
        out = plan.extract(g["input"], FEATS)
        hout = ham.extract(g["input"][g["hamming_frames"]], FEATS)
    finally:
        plan.close()
        ham.close()
    for o, amp, scal, mfcc in ((out, g["amp"], g["scalars"], g["mfcc"]),
                               (hout, g["hamming_amp"], g["hamming_scalars"], g["hamming_mfcc"])):
        bad, exact = tolerance.check_spectra(o["amplitudeSpectrum"], amp)
        assert not bad, [g["labels"][i] for i in bad]
        # (no bar on the fraction here: 22 of the 30 frames are tonal or edge frames, whose near-cancelled bins
        # may sit an ulp of the frame's norm away; the noise frames are held bit for bit below)
        print("golden frames: amplitude bit-exact fraction %.6f" % exact)
        gs = np.stack([o[k].astype(np.float64) for k in SCALARS], 1)
        fails = tolerance.check_scalars(gs, scal, amp, N)
        assert not fails, fails[:10]
        assert not tolerance.check_vectors(o["mfcc"], mfcc)
        assert np.array_equal(o["zcr"], scal[:, 2])
    assert not tolerance.check_vectors(out["loudness.specific"], g["loudness_specific"])
    assert not tolerance.check_spectra(out["powerSpectrum"], g["power"])[0]
    c = g["complex_frames"]
    assert not tolerance.check_spectra(out["complexSpectrum.real"][:c], g["complex_re"])[0]
    assert not tolerance.check_spectra(out["complexSpectrum.imag"][:c], g["complex_im"])[0]
    noise = [i for i, l in enumerate(g["labels"]) if l.startswith("noise:")]
    assert np.array_equal(out["amplitudeSpectrum"][noise].view(np.uint32), g["amp"][noise].view(np.uint32))


# ------------------------------------------------------------------ 2. fast precision and literal mode
def test_fast_precision_noise_only(capi, oracle_mod):
    x = oracle_mod.synth_frames(SEED, 5000, 37, N)
    ref = oracle_mod.extract(x)
    plan = capi.Plan(buffer_size=N, precision="fast", scalar_f64=True)
    try:
        out = plan.extract(x, ["amplitudeSpectrum", "spectralCentroid", "spectralSpread", "rms"])
    finally:
        plan.close()
    bad, _ = tolerance.check_spectra(out["amplitudeSpectrum"], ref["amp"])
    assert not bad
    assert np.allclose(out["spectralCentroid"], ref["scalars"][:, 3], rtol=1e-5)
    assert np.allclose(out["spectralSpread"], ref["scalars"][:, 7], rtol=1e-5)


def test_literal_mode_against_the_oracles_literal_path(capi, oracle_mod, frames37):
    ref = oracle_mod.extract(frames37, literal=True)
    g = golden_n4096.load()
    plan = capi.Plan(buffer_size=N, mode="literal", scalar_f64=True)
    try:
        out = plan.extract(frames37, ["amplitudeSpectrum", "loudness", "rms", "zcr"])
        gout = plan.extract(g["input"][g["literal_frames"]], ["amplitudeSpectrum", "loudness"])
    finally:
        plan.close()
    assert np.array_equal(out["amplitudeSpectrum"].view(np.uint32), ref["amp"].view(np.uint32))
    assert not tolerance.check_vectors(out["loudness.specific"], ref["loudness_specific"])
    assert np.allclose(out["loudness.total"], ref["scalars"][:, 10], rtol=1e-6)
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    assert np.array_equal(gout["amplitudeSpectrum"].view(np.uint32), g["literal_amp"].view(np.uint32))
    assert not tolerance.check_vectors(gout["loudness.specific"], g["literal_loudness_specific"])


# ------------------------------------------------------------------ 3. edge frames
def edge_frames(oracle_mod):
    x = oracle_mod.synth_frames(SEED, 77, 10, N).copy()
    x[0] = 0.0                                   # silence
    x[1, N // 3] = np.nan
    x[2, 7] = np.inf
    x[3, N - 1] = -np.inf
    x[4] = (x[4] * np.float32(1e-40)).astype(np.float32)   # denormal samples
    x[5] = 3.0e38                                # the non-tame passes, the non-finite sums
    x[6, ::2] = 3.0e38
    x[6, 1::2] = -3.0e38
    x[7] = np.where(np.arange(N) < N // 2, 1.0, -1.0)      # a full-scale square wave
    return x.astype(np.float32)                  # x[8], x[9]: plain noise


def test_edge_frames(capi, oracle_mod):
    x = edge_frames(oracle_mod)
    ref = oracle_mod.extract(x)
    plan = capi.Plan(buffer_size=N, scalar_f64=True)
    try:
        out = plan.extract(x, FEATS[:15])
    finally:
        plan.close()
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])
    compare(out, ref, N)  # classes match the oracle, values within policy (tests/test_gpu_edge.py)


# ------------------------------------------------------------------ 4. frame counts at the schedule's corners
def rows_with_sentinel(capi, plan, frames_t, F, feats):
    """Every output of `feats` for the first F rows of frames_t, in (F + 1)-row arrays prefilled with a sentinel."""
    import torch
    out, o = plan.alloc_outputs(F + 1, feats)
    for t in out.values():
        (t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)).fill_(SENTINEL)
    plan.extract_device(frames_t.data_ptr(), F, o, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def test_small_frame_counts(capi):
    feats = FEATS + ["melBands"]
    frames = device_frames(capi, N, 67)
    plan = capi.Plan(buffer_size=N, num_mel_bands=33)
    try:
        ones = [rows_with_sentinel(capi, plan, frames[i:i + 1], 1, feats) for i in range(67)]
        for F in (1, 3, 4, 5, 16, 17, 67):
            got = rows_with_sentinel(capi, plan, frames, F, feats)
            for k, v in got.items():
                assert (bits(v[F]) == SENTINEL).all(), (F, k, "row F was written")
                assert not (bits(v[:F]) == SENTINEL).any(), (F, k, "a row below F was left unwritten")
                ref = np.concatenate([ones[i][k][:1] for i in range(F)])
                assert np.array_equal(bits(v[:F]), bits(ref)), (F, k, np.argwhere(bits(v[:F]) != bits(ref))[:4].tolist())
    finally:
        plan.close()


# ------------------------------------------------------------------ 5. large-launch regime
@pytest.mark.parametrize("pct", [15, 0], ids=["pool", "no_pool"])
def test_large_launch_regime(capi, pct):
    """A grid capped at 8 workgroups: 3,001 frames are 12+ groups per workgroup and 8+ batches per wave (the ranked
    shares, the scalar windows, and with MGX_POOL_PCT=15 the tail pool's stolen batches), against launches of 97."""
    import torch
    F = 3001
    feats = capi.ALL_FEATURES + ["melBands"]
    plan = env_plan(capi, {"MGX_GRID_CAP": 8, "MGX_POOL_PCT": pct}, buffer_size=N, num_mel_bands=33)
    small = env_plan(capi, {"MGX_POOL_PCT": 0}, buffer_size=N, num_mel_bands=33)
    try:
        frames = device_frames(capi, N, F)
        got = plan.extract_torch(frames, feats)
        torch.cuda.synchronize()
        for i in range(0, F, 97):
            ref = small.extract_torch(frames[i:i + 97], feats)
            torch.cuda.synchronize()
            for k in ref:
                a, b = got[k][i:i + 97].contiguous().view(torch.int32), ref[k].view(torch.int32)
                assert torch.equal(a, b), (pct, k, i)
        check_against_small_launches(capi, plan, small, frames, F, 97, (N, pct), extra=capi.ALL_FEATURES)
    finally:
        plan.close()
        small.close()


# ------------------------------------------------------------------ 6. the paths agree byte for byte
def test_paths_agree(capi):
    import torch
    F = 67
    feats = FEATS + ["melBands"]
    plan = capi.Plan(buffer_size=N, scalar_f64=True)
    try:
        for hop in (N, 1024, 300):
            x = signal((F - 1) * hop + N + 5, 100 + hop)
            d = dense_frames(x, N, hop)
            dense = device_run(plan, d, feats)
            same_dict(device_run(plan, x, feats, hop), dense, ("device signal", hop))
            same_dict(plan.extract_signal(x, hop, feats), dense, ("host signal small path", hop))
        # (the last signal, hop 300) the gather with unsorted, repeated and odd starts
        rng = np.random.default_rng(9)
        starts = np.concatenate([rng.integers(0, x.size - N + 1, 61), [x.size - N, 0, 0, 1, 4097, x.size - N]]).astype(np.uint64)
        gd = {k: v.cpu().numpy() for k, v in plan.extract_gather_torch(torch.from_numpy(x).cuda(), starts, feats).items()}
        ref = device_run(plan, np.stack([x[int(s):int(s) + N] for s in starts]), feats)
        same_dict(gd, ref, "device gather")
        same_dict(plan.extract_gather(x, starts, feats), ref, "host gather small path")
    finally:
        plan.close()


def test_host_batches(capi, oracle_mod):
    """1 (the one-frame launch), 64, 512 (the one-launch path's last) and 513 (the staged path's first) frames."""
    import torch
    feats = ["mfcc", "rms", "zcr", "spectralRolloff", "loudness", "amplitudeSpectrum", "melBands"]
    x = oracle_mod.synth_frames(SEED, 9000, 513, N)
    plan = capi.Plan(buffer_size=N)
    try:
        ref = {k: v.cpu().numpy() for k, v in plan.extract_torch(torch.from_numpy(x).cuda(), feats).items()}
        for F in (1, 64, 512, 513):
            same_dict(plan.extract(x[:F], feats), {k: v[:F] for k, v in ref.items()}, ("host batch", F))
    finally:
        plan.close()


def test_wav_path(capi):
    hop = 1000
    codes = wavgen.random_codes(np.random.default_rng(5), 12 * N + 37, 2, "s16")
    wav, chan = wavgen.wav_bytes(codes, "s16"), wavgen.decode(codes[:, 1], "s16")
    plan = capi.Plan(buffer_size=N)
    try:
        for h in (hop, None):
            got = plan.extract_wav(wav, ["melBands", "rms", "mfcc"], channel=1, hop=h)
            ref = plan.extract_signal(chan, h or N, ["melBands", "rms", "mfcc"])
            assert got["rms"].shape == (capi.signal_frames(chan.size, N, h or N),)
            same_dict(got, ref, h)
    finally:
        plan.close()


def test_host_chunked_path_across_the_seam(capi):
    """32,776 buffers of a signal at hop 1: a staging chunk holds 32,768 buffers at N = 4096 (a slot keeps the
    bytes it has at N = 2048), so the second chunk starts at buffer 32,768."""
    hop, chunk, nmel = 1, 32768, 7
    F = chunk + 8
    x = signal(F - 1 + N, 32768)
    feats = ["melBands", "mfcc", "rms"]
    plan = capi.Plan(buffer_size=N, num_mel_bands=nmel)
    try:
        got = plan.extract_signal(x, hop, feats)
        ref = device_run(plan, x, feats, hop)
        around = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(x, N)[chunk - 8:chunk + 8])
        dense = plan.extract(around, feats)
    finally:
        plan.close()
    assert got["melBands"].shape == (F, nmel)
    seam = slice(chunk - 8, chunk + 8)
    same_dict({k: v[seam] for k, v in got.items()}, dense, "seam, dense")
    same_dict(got, ref, "all")


# ------------------------------------------------------------------ 7. melBands
@pytest.mark.parametrize("nmel", [1, 26, 64])
def test_mel_bands_against_the_restatement(capi, frames37, nmel):
    plan = capi.Plan(buffer_size=N, num_mel_bands=nmel)
    try:
        out = device_run(plan, frames37, ["melBands", "powerSpectrum"])
        without = device_run(plan, frames37, FEATS)
        with_mel = device_run(plan, frames37, ["melBands"] + FEATS)
    finally:
        plan.close()
    ref = restate(out["powerSpectrum"], bins_of(capi, N, nmel))
    bad = tolerance.check_vectors(out["melBands"], ref)
    assert not bad, (nmel, bad[:5], out["melBands"][bad[0]], ref[bad[0]])
    same_bits(with_mel.pop("melBands"), out["melBands"], "melBands beside every other output")
    same_dict(with_mel, without, "asking for melBands changes no other output")


# ------------------------------------------------------------------ 8. groups
def test_two_rank_loopback_group(capi):
    import torch
    F, ranks = 70, 2
    feats = capi.ALL_FEATURES + SPECTRA
    g = capi.Group(buffer_size=N, loopback=ranks, scalar_f64=True)
    plan = capi.Plan(buffer_size=N, scalar_f64=True)
    try:
        counts = [capi.shard_range(F, ranks, r)[1] for r in range(ranks)]
        starts = [capi.shard_range(F, ranks, r)[0] for r in range(ranks)]
        xs = [device_frames(capi, N, c, first=s) for s, c in zip(starts, counts)]
        got, o = plan.alloc_outputs(F, feats)
        for v in got.values():
            v.fill_(float("nan"))
        stream = torch.cuda.current_stream().cuda_stream
        g.extract_device([t.data_ptr() for t in xs], counts, o, capi.output_mask(o), num_chunks=1, streams=[stream] * ranks)
        torch.cuda.synchronize()
        want = plan.extract_torch(device_frames(capi, N, F), feats)
        torch.cuda.synchronize()
        for k in want:
            v = torch.int64 if want[k].element_size() == 8 else torch.int32
            assert torch.equal(got[k].view(v), want[k].view(v)), k
    finally:
        g.close()
        plan.close()


# ------------------------------------------------------------------ 9. graph replay
def test_graph_replay(capi):
    """A launch of 4,099 frames captured after an uncaptured warm-up on the stream, replayed three times: the same
    bytes each time (the tail pool's counter resets itself on the device)."""
    import torch
    F = 4099
    feats = ["mfcc", "rms", "spectralRolloff", "amplitudeSpectrum"]
    frames = device_frames(capi, N, F)
    plan = capi.Plan(buffer_size=N)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            warm, wo = plan.alloc_outputs(64, feats)
            plan.extract_device(frames.data_ptr(), 64, wo, s.cuda_stream)  # the stream's scratch set, uncaptured
            ref, ro = plan.alloc_outputs(F, feats)
            plan.extract_device(frames.data_ptr(), F, ro, s.cuda_stream)
        torch.cuda.synchronize()
        out, o = plan.alloc_outputs(F, feats)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.extract_device(frames.data_ptr(), F, o, s.cuda_stream)
        torch.cuda.synchronize()
        for rep in range(3):
            for t in out.values():
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for k in ref:
                assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), (rep, k)
        g.reset()
    finally:
        plan.close()
