"""Overlapping buffers of one contiguous signal (mgx_extract_signal_*, include/meyda_gpu.h): a signal of S
samples cut every `hop` samples gives F = (S - N) / hop + 1 buffers, buffer f at samples [f hop, f hop + N),
read in place by the kernel (KernelArgs::frame_stride). The defining property: every output equals, bit for
bit and NaN for NaN, what the existing dense entry points give on the same F buffers materialised with
numpy's sliding_window_view -- the buffer indices, the schedule, the scalar windows and the tail pool are
functions of F alone, so only the load address differs.
"""
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import tolerance
import wavgen

pytestmark = pytest.mark.gpu

SPECTRA = ["amplitudeSpectrum", "powerSpectrum", "complexSpectrum"]
GOLDEN_SCALARS = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope",
                  "spectralRolloff", "spectralSpread", "spectralSkewness", "spectralKurtosis",
                  "loudness.total", "perceptualSpread", "perceptualSharpness"]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def env_plan(capi, env, **kw):
    """A plan created with `env` set (the knobs mgx_plan_create reads), the environment restored."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return capi.Plan(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def signal(S, seed):
    return np.random.default_rng(seed).uniform(-1, 1, S).astype(np.float32)


def dense_frames(x, n, hop):
    return np.ascontiguousarray(sliding_window_view(x, n)[::hop])


def on_device(x, pad=4096):
    """The signal as a slice from element 1 of a larger allocation (a base pointer aligned to 4 bytes
    only), NaN before and after it: a read past the last buffer would reach the last buffers' outputs."""
    import torch
    big = torch.full((1 + x.size + pad,), float("nan"), dtype=torch.float32, device="cuda")
    big[1:1 + x.size] = torch.from_numpy(x).cuda()
    return big[1:1 + x.size]


def bits_t(t):
    import torch
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_device(got, ref, what):
    import torch
    assert sorted(got) == sorted(ref), what
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not torch.equal(bits_t(got[k]), bits_t(ref[k])):
            bad = (bits_t(got[k]) != bits_t(ref[k])).nonzero()
            raise AssertionError((what, k, int(bad.shape[0]), bad[:4].tolist()))


def same_host(got, ref, what):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        u = np.uint64 if got[k].dtype.itemsize == 8 else np.uint32
        if not np.array_equal(got[k].view(u), ref[k].view(u)):
            bad = np.argwhere(got[k].view(u) != ref[k].view(u))
            raise AssertionError((what, k, len(bad), bad[:4].tolist()))


def signal_vs_dense(capi, plan, x, hop, feats, what, F=None):
    """The device signal launch against the dense launch over the same buffers; returns the signal's outputs."""
    import torch
    n = plan.n
    d = dense_frames(x, n, hop)
    if F is not None:
        assert d.shape[0] == F, (what, d.shape, F)
    assert capi.signal_frames(x.size, n, hop) == d.shape[0], what
    ref = plan.extract_torch(torch.from_numpy(d).cuda(), feats)
    got = plan.extract_signal_torch(on_device(x), hop, feats)
    torch.cuda.synchronize()
    same_device(got, ref, what)
    return got


# ------------------------------------------------------------------ 1. the schedule's corners
@pytest.mark.parametrize("n", [256, 512, 1024, 2048])
def test_device_signal_equals_dense_at_the_schedules_corners(capi, n):
    """Partial wave batch, one batch, a batch plus one, a group of 16 plus one, several workgroups and (N =
    2048) the tail pool, at hops below, at and above N, with and without a dropped tail of hop - 1 samples."""
    feats = capi.ALL_FEATURES + SPECTRA
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        for hop in (1, 63, n // 4, n - 1, n, n + 1):
            for F in (1, 3, 4, 5, 17, 67, 203):
                for r in sorted({0, hop - 1}):
                    S = (F - 1) * hop + n + r
                    signal_vs_dense(capi, plan, signal(S, 1000 * n + 7 * F + hop), hop, feats, (n, hop, F, r), F=F)
    finally:
        plan.close()


# ------------------------------------------------------------------ 2. the large-launch regime
@pytest.mark.parametrize("n,hop", [(512, 128), (1024, 256), (2048, 512), (256, 1)])
def test_device_signal_large_launch_regime(capi, n, hop):
    """A grid capped at 8 workgroups (MGX_GRID_CAP, read at plan creation): 3,001 buffers are then 12+ groups
    per workgroup and 8+ batches per wave -- the scalar windows, the many-group shares, the pool at N = 2048."""
    F = 3001
    plan = env_plan(capi, {"MGX_GRID_CAP": 8}, buffer_size=n, scalar_f64=True)
    try:
        x = signal((F - 1) * hop + n + (hop - 1), 77 + n)
        signal_vs_dense(capi, plan, x, hop, capi.ALL_FEATURES + SPECTRA, (n, hop), F=F)
    finally:
        plan.close()


# ------------------------------------------------------------------ 3. every kernel family
FAMILIES = [
    ("fast", 1024, dict(precision="fast"), None),
    ("literal", 1024, dict(mode="literal"), None),
    ("mfcc_reference", 1024, dict(mfcc_reference=True), None),
    ("mfcc_reference_512", 512, dict(mfcc_reference=True), None),
    ("dct_sequential", 1024, dict(dct_sequential=True), None),
    ("hamming", 1024, dict(window="hamming"), None),
    ("mel40", 1024, dict(num_mel_bands=40), None),
    ("float32_scalars", 1024, dict(scalar_f64=False), None),
    ("sub_time", 1024, dict(), ["rms", "zcr"]),
    ("sub_centroid_mfcc", 1024, dict(), ["spectralCentroid", "mfcc"]),
]


@pytest.mark.parametrize("name,n,kw,feats", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_device_signal_every_kernel_family(capi, name, n, kw, feats):
    hop, F = 300, 67
    kw = dict({"scalar_f64": True}, **kw)
    plan = capi.Plan(buffer_size=n, **kw)
    try:
        x = signal((F - 1) * hop + n + 11, 4242)
        signal_vs_dense(capi, plan, x, hop, feats or capi.ALL_FEATURES + SPECTRA, name, F=F)
    finally:
        plan.close()


# ------------------------------------------------------------------ 4. both load kinds
@pytest.mark.parametrize("nt_min_mb", [0, 1 << 20], ids=["nt", "plain"])
@pytest.mark.parametrize("hop", [256, 1024])
def test_device_signal_both_load_kinds(capi, nt_min_mb, hop):
    n, F = 1024, 203
    plan = env_plan(capi, {"MGX_NT_MIN_MB": nt_min_mb}, buffer_size=n, scalar_f64=True)
    try:
        x = signal((F - 1) * hop + n + 3, 9)
        signal_vs_dense(capi, plan, x, hop, capi.ALL_FEATURES + SPECTRA, (nt_min_mb, hop), F=F)
    finally:
        plan.close()


# ------------------------------------------------------------------ 5. against the oracle
def test_device_signal_against_the_oracle(capi, oracle_mod):
    import torch
    n, hop, F = 512, 128, 67
    x = signal((F - 1) * hop + n + 100, 31337)
    d = dense_frames(x, n, hop)
    assert d.shape[0] == F
    ref = oracle_mod.extract(d)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = plan.extract_signal_torch(on_device(x), hop, capi.ALL_FEATURES + ["amplitudeSpectrum", "powerSpectrum"])
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in got.items()}
    finally:
        plan.close()
    bad, _ = tolerance.check_spectra(out["amplitudeSpectrum"], ref["amp"])
    assert not bad
    scal = np.stack([out[k].astype(np.float64) for k in GOLDEN_SCALARS], 1)
    fails = tolerance.check_scalars(scal, ref["scalars"], ref["amp"], n)
    assert not fails, fails[:10]
    assert not tolerance.check_vectors(out["mfcc"], ref["mfcc"])
    assert not tolerance.check_vectors(out["loudness.specific"], ref["loudness_specific"])
    assert np.array_equal(out["zcr"], ref["scalars"][:, 2])


# ------------------------------------------------------------------ 6. the host path
@pytest.mark.parametrize("n,hop,F", [(1024, 256, 1), (1024, 256, 2), (512, 128, 512), (512, 128, 513), (512, 517, 600),
                                     (512, 517, 40)])
def test_host_signal_equals_dense(capi, n, hop, F):
    """One buffer (the inline-frame launch), two, the one-launch path's last size and the chunked path's
    first, and a hop above N on both (gathered densely / the chunk's span in the slot)."""
    feats = capi.ALL_FEATURES + SPECTRA
    x = signal((F - 1) * hop + n + min(hop - 1, 50), 5 * F + hop)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        d = dense_frames(x, n, hop)
        assert d.shape[0] == F
        same_host(plan.extract_signal(x, hop, feats), plan.extract(d, feats), (n, hop, F))
    finally:
        plan.close()


def test_host_signal_chunk_seam(capi):
    """70,000 buffers of a 70,255-sample signal at hop 1: the second staging chunk starts at buffer 65,536,
    re-sending the N - 1 samples it shares with the first."""
    n, hop, F = 256, 1, 70000
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum"]
    x = signal(F - 1 + n, 65536)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = plan.extract_signal(x, hop, feats)
        ref = plan.extract(dense_frames(x, n, hop), feats)
    finally:
        plan.close()
    seam = slice(65536 - 8, 65536 + 8)
    same_host({k: v[seam] for k, v in got.items()}, {k: v[seam] for k, v in ref.items()}, "seam")
    same_host(got, ref, "all")


# ------------------------------------------------------------------ 7. the PCM path
def stereo_wav(fmt, sample_frames, seed):
    codes = wavgen.random_codes(np.random.default_rng(seed), sample_frames, 2, fmt)
    return wavgen.wav_bytes(codes, fmt), wavgen.decode(codes[:, 1], fmt)


@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
@pytest.mark.parametrize("hop", [128, 512, 700])
def test_wav_at_a_hop_equals_the_decoded_channel(capi, fmt, hop):
    n = 512
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum"]
    wav, chan = stereo_wav(fmt, 40 * n + 37, 17 + hop)  # (a partial tail)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = plan.extract_wav(wav, feats, channel=1, hop=hop)
        ref = plan.extract_signal(chan, hop, feats)
    finally:
        plan.close()
    assert got["rms"].shape[0] == capi.signal_frames(chan.size, n, hop) > 0
    same_host(got, ref, (fmt, hop))


def test_wav_at_a_hop_chunk_seam(capi):
    n, hop = 256, 1
    feats = ["rms", "zcr", "spectralCentroid", "mfcc", "loudness"]
    wav, chan = stereo_wav("s16", 70300, 3)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = plan.extract_wav(wav, feats, channel=1, hop=hop)
        ref = plan.extract_signal(chan, hop, feats)
    finally:
        plan.close()
    assert got["rms"].shape[0] == 70300 - n + 1
    seam = slice(65536 - 8, 65536 + 8)
    same_host({k: v[seam] for k, v in got.items()}, {k: v[seam] for k, v in ref.items()}, "seam")
    same_host(got, ref, "all")


def test_pcm_short_buffer_refused_with_a_hop(capi):
    n = 512
    plan = capi.Plan(buffer_size=n)
    try:
        pcm = np.zeros(4 * n * 2, np.int16)  # 4 N stereo sample frames
        with pytest.raises(capi.MgxError) as e:
            plan.extract_pcm(pcm, 4 * n + 1, "s16", 2, channel=1, features=["rms"], hop=128)
        assert e.value.status == -1
        with pytest.raises(capi.MgxError) as e:
            plan.extract_pcm(pcm, 4 * n, "s16", 2, channel=1, features=["rms"], hop=0)
        assert e.value.status == -1
    finally:
        plan.close()


# ------------------------------------------------------------------ 8. stream order
def test_two_signal_launches_on_two_streams(capi):
    import torch
    n = 1024
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum"]
    x = signal(203 * 256 + n, 88)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        xs = on_device(x)
        ref = {h: plan.extract_torch(torch.from_numpy(dense_frames(x, n, h)).cuda(), feats) for h in (256, 777)}
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a = plan.extract_signal_torch(xs, 256, feats, stream=s1.cuda_stream)
        b = plan.extract_signal_torch(xs, 777, feats, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        same_device(a, ref[256], "hop 256")
        same_device(b, ref[777], "hop 777")
    finally:
        plan.close()
