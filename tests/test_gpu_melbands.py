"""melBands: the log mel band energies (loggedMelBands of mfcc.js:53-65, the Float32Array the reference's DCT
reads) as a per-frame output of the mgx_extract_*_ex calls (mgx_aux_outputs.mel_bands).

The expected values are a numpy / math restatement of mfcc.js:40-65 written here: the weights of :45-50 in
double from the plan's own bin edges, per band a float32 accumulator that takes the double products
w * p[j] over j = 0 .. N/2 - 1 in ascending order, then float32(math.log(float(sum))). It is fed with the
power spectrum the SAME GPU call returned, so a spectrum bin that differs from the oracle's can neither hide
nor cause a failure (the spectrum's own parity is tests/test_gpu_parity.py's business).
"""
import ctypes
import math
import os

import numpy as np
import pytest

import tolerance
import wavgen
from test_gpu_signal import FAMILIES, SPECTRA, dense_frames, env_plan, on_device, signal

pytestmark = pytest.mark.gpu

SEED = 0x6D657964
SIZES = [256, 512, 1024, 2048]
BANDS = [1, 7, 16, 17, 26, 33, 40, 64]
SENTINEL = 0x7FC0BEEF  # (as int32) a NaN no computation produces


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def synth(oracle_mod, n, count, first=0):
    return oracle_mod.synth_frames(SEED, first, count, n)


# ---------------------------------------------------------------------------- the restatement
def mel_weights(bins, L):
    """filterBank of mfcc.js:40-50, columns 0 .. L - 1 (the bins :56 reads), in double."""
    nf = len(bins) - 2
    w = np.zeros((nf, L), np.float64)
    for j in range(nf):
        b0, b1, b2 = int(bins[j]), int(bins[j + 1]), int(bins[j + 2])
        for i in range(b0, min(b1, L)):
            w[j, i] = (i - b0) / (b1 - b0)
        for i in range(b1, min(b2, L)):
            w[j, i] = (b2 - i) / (b2 - b1)
    return w


def js_log(v):
    """float32(Math.log(v)) of a float32 band sum (never negative)."""
    v = float(v)
    if v != v:
        return np.float32(np.nan)
    if v == 0.0:
        return np.float32(-np.inf)
    if v == math.inf:
        return np.float32(np.inf)
    return np.float32(math.log(v))


def restate(power, bins):
    """loggedMelBands of mfcc.js:53-65 for every row of `power` (F x N/2 float32)."""
    F, L = power.shape
    w = mel_weights(bins, L)
    acc = np.zeros((F, w.shape[0]), np.float32)
    p = power.astype(np.float64)
    with np.errstate(all="ignore"):
        for j in range(L):  # every bin, in ascending order: a zero weight times an infinite power is NaN
            acc = (acc.astype(np.float64) + w[None, :, j] * p[:, j, None]).astype(np.float32)
    return np.array([[js_log(v) for v in row] for row in acc], np.float32)


def bins_of(capi, n, nmel, **kw):
    return capi.host_tables(buffer_size=n, num_mel_bands=nmel, **kw)["mel_bins"]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(u32(got), u32(ref)):
        bad = np.argwhere(u32(got) != u32(ref))
        raise AssertionError((what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])]))


def same_dict(got, ref, what):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k)


def device_run(plan, x, feats, hop=None):
    """Host arrays of a device launch over the rows of x (dense), or over the signal x at `hop`. Every output
    is prefilled with NaN: one that the plan's mode never writes (literal mode has no complex spectrum)
    then compares equal between two calls instead of showing two allocations' stale bytes."""
    import torch
    if hop is None:
        xs = torch.from_numpy(np.array(x, np.float32)).cuda()
        F = xs.shape[0]
    else:
        xs = on_device(x)
        F = capi_mod().signal_frames(x.size, plan.n, hop)
    out, o = plan.alloc_outputs(F, feats)
    for t in out.values():
        t.fill_(float("nan"))
    s = torch.cuda.current_stream().cuda_stream
    if hop is None:
        plan.extract_device(xs.data_ptr(), F, o, s)
    else:
        plan.extract_signal_device(xs.data_ptr(), x.size, hop, o, s)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def capi_mod():
    from meyda_amd import capi
    return capi


# ------------------------------------------------------------------ 1. reference order, bit for bit
@pytest.mark.parametrize("nmel", BANDS)
@pytest.mark.parametrize("n", SIZES)
def test_reference_order_is_the_restatement_bit_for_bit(capi, oracle_mod, n, nmel):
    F = 37
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel, mfcc_reference=True)
    try:
        out = device_run(plan, synth(oracle_mod, n, F), ["melBands", "powerSpectrum"])
    finally:
        plan.close()
    assert out["melBands"].shape == (F, nmel) and out["melBands"].dtype == np.float32
    same_bits(out["melBands"], restate(out["powerSpectrum"], bins_of(capi, n, nmel)), (n, nmel))


# ------------------------------------------------------------------ 2. the default plan, the vector policy
@pytest.mark.parametrize("nmel", BANDS)
@pytest.mark.parametrize("n", SIZES)
def test_default_plan_within_the_vector_policy(capi, oracle_mod, n, nmel):
    F = 37
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel)
    try:
        out = device_run(plan, synth(oracle_mod, n, F), ["melBands", "powerSpectrum"])
    finally:
        plan.close()
    ref = restate(out["powerSpectrum"], bins_of(capi, n, nmel))
    bad = tolerance.check_vectors(out["melBands"], ref)
    assert not bad, (n, nmel, bad[:5], out["melBands"][bad[0]], ref[bad[0]])


# ------------------------------------------------------------------ 3. the MFCC is the DCT of what was stored
@pytest.mark.parametrize("nc", [13, 20])
@pytest.mark.parametrize("nmel", [7, 26, 40])
@pytest.mark.parametrize("kw", [dict(), dict(dct_sequential=True), dict(mfcc_reference=True)],
                         ids=["default", "dct_sequential", "mfcc_reference"])
def test_mfcc_is_the_dct_of_the_stored_rows(capi, oracle_mod, kw, nmel, nc):
    n, F = 1024, 37
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel, num_mfcc_coeffs=nc, **kw)
    try:
        out = device_run(plan, synth(oracle_mod, n, F), ["melBands", "mfcc"])
    finally:
        plan.close()
    dct = capi.host_tables(buffer_size=n, num_mel_bands=nmel, num_mfcc_coeffs=nc)["dct"].astype(np.float64)
    mel = out["melBands"].astype(np.float64)
    fin = np.isfinite(mel).all(1)
    assert fin.sum() == F
    exp = np.empty((F, nc), np.float32)
    for c in range(nc):
        v = np.zeros(F, np.float64)
        for b in range(nmel):  # mfcc.js:88-91: sequential, ascending, in double (the products are exact)
            v = v + dct[c + b * nc] * mel[:, b]
        exp[:, c] = (v / nc).astype(np.float32)
    same_bits(out["mfcc"][fin], exp[fin], (kw, nmel, nc))


# ------------------------------------------------------------------ 4. asking for it changes nothing else
@pytest.mark.parametrize("name,n,kw,feats", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_request_changes_nothing_else_and_nothing_changes_it(capi, name, n, kw, feats):
    hop, F = 300, 67
    plan = capi.Plan(buffer_size=n, **dict({"scalar_f64": True}, **kw))
    try:
        x = signal((F - 1) * hop + n + 11, 4242)
        alone = device_run(plan, x, ["melBands"], hop)["melBands"]
        assert alone.shape == (F, plan.desc.num_mel_bands)
        for base in (["mfcc"], capi.ALL_FEATURES + SPECTRA) + ((feats,) if feats else ()):
            without = device_run(plan, x, base, hop)
            with_mel = device_run(plan, x, ["melBands"] + base, hop)
            same_bits(with_mel.pop("melBands"), alone, (name, base[:2]))
            same_dict(with_mel, without, (name, base[:2]))
    finally:
        plan.close()


# ------------------------------------------------------------------ 5. frame counts at the schedule's corners
def mel_rows(capi, plan, frames_t, F, extra=()):
    """melBands of the first F rows of the device tensor frames_t, into an (F + 1)-row array prefilled with a
    sentinel; returns the host array (F + 1 rows)."""
    import torch
    nm = plan.desc.num_mel_bands
    mel = torch.full((F + 1, nm), SENTINEL, dtype=torch.int32, device="cuda")
    _, o = plan.alloc_outputs(F, list(extra))
    capi._set_mel_bands(o, mel.data_ptr())
    o.keep = _  # (the other outputs' tensors live as long as the launch)
    plan.extract_device(frames_t.data_ptr(), F, o, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return mel.cpu().numpy()


def check_against_small_launches(capi, plan, small, frames_t, F, step, what, extra=()):
    got = mel_rows(capi, plan, frames_t, F, extra)
    assert (got[F] == SENTINEL).all(), (what, "row F was written")
    assert not (got[:F] == SENTINEL).any(), (what, "a row below F was left unwritten", np.argwhere(got[:F] == SENTINEL)[:4].tolist())
    parts = [mel_rows(capi, small, frames_t[i:i + step], min(step, F - i))[:min(step, F - i)] for i in range(0, F, step)]
    ref = np.concatenate(parts)
    assert np.array_equal(got[:F], ref), (what, np.argwhere(got[:F] != ref)[:4].tolist())


def device_frames(capi, n, F, first=0):
    import torch
    t = torch.empty(F, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(t, SEED, first_frame=first)
    return t


@pytest.mark.parametrize("nmel", [7, 33])
@pytest.mark.parametrize("n", SIZES)
def test_small_frame_counts(capi, n, nmel):
    """1, 3 (a partial batch), 4, 5, a group of 16, 17, several workgroups -- each against one-frame launches --
    on the default and the reference-order plan."""
    frames = device_frames(capi, n, 67)
    for kw in (dict(), dict(mfcc_reference=True)):
        plan = capi.Plan(buffer_size=n, num_mel_bands=nmel, **kw)
        try:
            for F in (1, 3, 4, 5, 16, 17, 67):
                check_against_small_launches(capi, plan, plan, frames, F, 1, (n, nmel, kw, F), extra=["mfcc"] if F == 5 else ())
        finally:
            plan.close()


@pytest.mark.parametrize("n,nmel", [(256, 7), (512, 33), (1024, 7), (2048, 33)])
def test_large_launch_regime(capi, n, nmel):
    """A grid capped at 8 workgroups: 3,001 frames are 12+ groups per workgroup and 8+ batches per wave (the
    scalar windows beside the mel rows, the many-group shares, the pool at N = 2048)."""
    F = 3001
    plan = env_plan(capi, {"MGX_GRID_CAP": 8}, buffer_size=n, num_mel_bands=nmel)
    small = capi.Plan(buffer_size=n, num_mel_bands=nmel)
    try:
        check_against_small_launches(capi, plan, small, device_frames(capi, n, F), F, 97, (n, nmel),
                                     extra=capi.ALL_FEATURES)
    finally:
        plan.close()
        small.close()


@pytest.mark.parametrize("pct,F", [(15, 65538), (15, 4099), (50, 1001)])
def test_tail_pool_stolen_batches(capi, pct, F):
    """N = 2048 with the tail pool engaged (MGX_POOL_PCT): the batches taken by ticket store their rows too."""
    n, nmel = 2048, 33
    plan = env_plan(capi, {"MGX_POOL_PCT": pct}, buffer_size=n, num_mel_bands=nmel)
    small = env_plan(capi, {"MGX_POOL_PCT": 0}, buffer_size=n, num_mel_bands=nmel)
    try:
        check_against_small_launches(capi, plan, small, device_frames(capi, n, F), F, 997, (pct, F), extra=["mfcc", "rms"])
    finally:
        plan.close()
        small.close()


@pytest.mark.parametrize("nmel", [7, 33])
def test_reference_order_waves_ending_on_an_odd_batch(capi, nmel):
    """40,963 frames at N = 1024: waves of 3 batches each -- with up to 31 bands a pair of batches whose chains
    run together (the first batch's rows stored with the pair, at its earlier frame base), then a last batch
    finished alone after the loop -- against launches of 997 frames."""
    n, F = 1024, 40963
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel, mfcc_reference=True)
    try:
        check_against_small_launches(capi, plan, plan, device_frames(capi, n, F, first=3), F, 997, nmel, extra=["mfcc"])
    finally:
        plan.close()


# ------------------------------------------------------------------ 6. the paths agree byte for byte
@pytest.mark.parametrize("kw", [dict(), dict(mfcc_reference=True)], ids=["default", "mfcc_reference"])
def test_paths_agree(capi, kw):
    n, nmel, F = 512, 33, 67
    feats = ["melBands", "mfcc"]
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel, **kw)
    try:
        for hop in (n, n // 4, 300):
            x = signal((F - 1) * hop + n + 5, 100 + hop)
            d = dense_frames(x, n, hop)
            dense = device_run(plan, d, feats)
            same_dict(device_run(plan, x, feats, hop), dense, ("device signal", hop))
            same_dict(plan.extract(d, feats), dense, ("host small path", hop))  # 67 frames: one launch over pinned memory
            same_dict(plan.extract_signal(x, hop, feats), dense, ("host signal small path", hop))
            one = plan.extract(d[:1], ["melBands"])  # one frame: in the kernel arguments, the output words polled
            same_bits(one["melBands"], dense["melBands"][:1], ("host one frame", hop))
            one = plan.extract(d[5:6], feats + ["amplitudeSpectrum"])  # one frame, the completion word
            same_bits(one["melBands"], dense["melBands"][5:6], ("host one frame with a spectrum", hop))
    finally:
        plan.close()


def test_host_chunked_path_across_the_seam(capi):
    """70,000 buffers of a 70,255-sample signal at hop 1: the second staging chunk starts at buffer 65,536."""
    n, hop, F, nmel = 256, 1, 70000, 7
    x = signal(F - 1 + n, 65536)
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel)
    try:
        got = plan.extract_signal(x, hop, ["melBands", "mfcc"])
        ref = device_run(plan, x, ["melBands", "mfcc"], hop)
        dense = plan.extract(dense_frames(x, n, hop)[65536 - 8:65536 + 8], ["melBands"])
    finally:
        plan.close()
    assert got["melBands"].shape == (F, nmel)
    seam = slice(65536 - 8, 65536 + 8)
    same_bits(got["melBands"][seam], ref["melBands"][seam], "seam")
    same_bits(got["melBands"][seam], dense["melBands"], "seam, dense")
    same_dict(got, ref, "all")


@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_wav_path(capi, fmt):
    n, hop, nmel = 512, 200, 33
    codes = wavgen.random_codes(np.random.default_rng(5), 40 * n + 37, 2, fmt)
    wav, chan = wavgen.wav_bytes(codes, fmt), wavgen.decode(codes[:, 1], fmt)
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel)
    try:
        for h in (hop, None):
            got = plan.extract_wav(wav, ["melBands", "rms"], channel=1, hop=h)
            ref = plan.extract_signal(chan, h or n, ["melBands", "rms"])
            assert got["melBands"].shape == (capi.signal_frames(chan.size, n, h or n), nmel)
            same_dict(got, ref, (fmt, h))
    finally:
        plan.close()


def test_resident_plan_one_buffer_call(capi, oracle_mod):
    """A resident plan's one-buffer call that asks for melBands is served by a launch; the calls without it
    before and after are the resident workgroup's, and every value is the ordinary plan's."""
    n = 1024
    x = synth(oracle_mod, n, 3)
    res = capi.Plan(buffer_size=n, resident=True)
    plain = capi.Plan(buffer_size=n)
    try:
        for i in (0, 1, 2):
            ref = plain.extract(x[i:i + 1], ["melBands", "mfcc", "rms"])
            before = res.extract(x[i:i + 1], ["mfcc", "rms"])
            got = res.extract(x[i:i + 1], ["melBands", "mfcc", "rms"])
            after = res.extract(x[i:i + 1], ["mfcc", "rms"])
            same_dict(got, ref, ("resident", i))
            for o in (before, after):
                same_dict(o, {k: ref[k] for k in o}, ("resident without melBands", i))
    finally:
        res.close()
        plain.close()


# ------------------------------------------------------------------ 7. edge values
def edge_frames(oracle_mod, n):
    x = synth(oracle_mod, n, 6).copy()
    x[1] = 0.0           # silence
    x[2, n // 3] = np.nan
    x[3, n // 5] = np.inf
    x[4, 7] = -np.inf
    return x


@pytest.mark.parametrize("kw", [dict(), dict(mfcc_reference=True), dict(mfcc_reference=True, num_mel_bands=40)],
                         ids=["default", "mfcc_reference", "mfcc_reference_40"])
@pytest.mark.parametrize("n", [512, 1024])
def test_edge_values(capi, oracle_mod, n, kw):
    plan = capi.Plan(buffer_size=n, **kw)
    try:
        out = device_run(plan, edge_frames(oracle_mod, n), ["melBands", "powerSpectrum", "mfcc"])
    finally:
        plan.close()
    mel = out["melBands"]
    assert np.isneginf(mel[1]).all(), mel[1]
    ref = restate(out["powerSpectrum"], bins_of(capi, n, plan.desc.num_mel_bands))
    assert np.array_equal(tolerance._cls(mel), tolerance._cls(ref)), (mel[2:5, :4], ref[2:5, :4])
    assert not tolerance.check_vectors(mel, ref)
    if kw.get("mfcc_reference"):  # (a NaN's payload is not the reference's business: its class was checked above)
        num = ~np.isnan(ref)
        same_bits(mel[num], ref[num], "edge frames, reference order")


@pytest.mark.parametrize("kw", [dict(mode="literal"), dict(precision="fast"), dict(window="hamming")],
                         ids=["literal", "fast", "hamming"])
def test_literal_mode_and_fast_precision(capi, oracle_mod, kw):
    n, F = 1024, 37
    plan = capi.Plan(buffer_size=n, **kw)
    try:
        out = device_run(plan, synth(oracle_mod, n, F), ["melBands", "powerSpectrum"])
    finally:
        plan.close()
    ref = restate(out["powerSpectrum"], bins_of(capi, n, 26))
    assert not tolerance.check_vectors(out["melBands"], ref)


# ------------------------------------------------------------------ 8. arguments
def test_arguments(capi, oracle_mod):
    import torch
    n, F = 512, 5
    L = capi.lib()
    plan = capi.Plan(buffer_size=n)
    try:
        x = torch.from_numpy(synth(oracle_mod, n, F)).cuda()
        mel = torch.full((F, 26), SENTINEL, dtype=torch.int32, device="cuda")
        o = capi.Outputs()
        a = capi.AuxOutputs()
        a.mel_bands = mel.data_ptr()
        for size in (0, 8, ctypes.sizeof(capi.AuxOutputs) + 8):
            a.struct_size = size
            rc = L.mgx_extract_device_ex(plan._h, x.data_ptr(), F * n, n, ctypes.byref(o), ctypes.byref(a), None)
            assert rc == -1 and b"mgx_aux_outputs.struct_size" in L.mgx_last_error(), (size, rc, L.mgx_last_error())
            hm = np.zeros((F, 26), np.float32)
            b = capi.AuxOutputs(size, 0, hm.ctypes.data)
            xh = x.cpu().numpy()
            assert L.mgx_extract_host_ex(plan._h, xh.ctypes.data, F * n, n, ctypes.byref(o), ctypes.byref(b)) == -1
            assert b"struct_size" in L.mgx_last_error()
            assert L.mgx_extract_host_pcm_ex(plan._h, xh.ctypes.data, xh.nbytes, F * n, 0, 1, 0, n, ctypes.byref(o),
                                             ctypes.byref(b)) == -1
            assert not hm.any()
        torch.cuda.synchronize()
        assert (mel == SENTINEL).all()
        # every pointer NULL: MGX_OK, nothing to write
        a.struct_size = ctypes.sizeof(capi.AuxOutputs)
        a.mel_bands = None
        assert L.mgx_extract_device_ex(plan._h, x.data_ptr(), F * n, n, ctypes.byref(o), ctypes.byref(a), None) == 0
        assert L.mgx_extract_device_ex(plan._h, x.data_ptr(), F * n, n, ctypes.byref(o), None, None) == 0
        torch.cuda.synchronize()
        assert (mel == SENTINEL).all()
    finally:
        plan.close()


def test_graph_replay(capi):
    """An _ex launch captured into a graph and replayed three times gives the same bytes each time."""
    import torch
    n, F, nmel = 1024, 4099, 33
    frames = device_frames(capi, n, F)
    plan = capi.Plan(buffer_size=n, num_mel_bands=nmel)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            warm, wo = plan.alloc_outputs(64, ["melBands", "mfcc"])
            plan.extract_device(frames.data_ptr(), 64, wo, s.cuda_stream)  # the stream's scratch set, uncaptured
            ref, ro = plan.alloc_outputs(F, ["melBands", "mfcc"])
            plan.extract_device(frames.data_ptr(), F, ro, s.cuda_stream)
        torch.cuda.synchronize()
        out, o = plan.alloc_outputs(F, ["melBands", "mfcc"])
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
