"""Chroma on the host path (mgx_chroma_host, include/meyda_gpu.h): the chroma rows of a corpus of clips computed
behind each chunk's extraction from amplitude rows that stay on the device, and their pooling per clip. Equality of
bits against the device operator (chroma_torch) on the amplitude rows mgx_extract_gather_host returns, and against
the numpy statement (tests/chroma_ref.py); the summaries against numpy on the chroma rows within the summaries' own
documented bounds (tests/test_gpu_summary.py check). One corpus exceeds a 65,536-buffer host chunk."""
import numpy as np
import pytest

import chroma_ref
from test_gpu_summary import check, corpus, reference, same_bits

pytestmark = pytest.mark.gpu

N, HOP = 256, 64
COUNTS = [0, 1, 300, 77, 1029]  # a clip shorter than N (no buffers), one of exactly N, three longer


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def operator(capi, amp, w, norm):
    import torch
    out = capi.chroma_torch(torch.from_numpy(amp).cuda(), w, norm)
    torch.cuda.synchronize()
    return out.cpu().numpy()


class Corpus:
    def __init__(self, capi):
        self.samples, lens = corpus(N, HOP, COUNTS, 77)
        assert lens[0] == N - 1 and lens[1] == N
        self.starts, self.fo = capi.signals_frame_starts(lens, N, HOP)
        assert np.diff(self.fo.astype(np.int64)).tolist() == COUNTS
        self.plan = capi.Plan(buffer_size=N)
        self.args = (self.samples, self.starts, self.fo)
        self.amp = self.plan.extract_gather(self.samples, self.starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]
        self.both = {norm: self.plan.chroma(*self.args, norm=norm, per_frame=True, summary=True) for norm in ("max", "none")}


@pytest.fixture(scope="module")
def c(capi):
    c = Corpus(capi)
    yield c
    c.plan.close()


def test_per_frame_is_the_operator_on_the_amplitude_rows(c, capi):
    for norm, r in c.both.items():
        w = r["weights"]
        assert w.shape == (12, N // 2) and np.array_equal(w, capi.chroma_weights(N, 44100.0))
        got = r["chroma"]
        assert got.shape == (sum(COUNTS), 12) and got.dtype == np.float32 and np.isfinite(got).all()
        same_bits({"chroma": got}, {"chroma": operator(capi, c.amp, w, norm)}, ("operator", norm))
        same_bits({"chroma": got}, {"chroma": chroma_ref.chroma(c.amp, w, norm)}, ("oracle", norm))
    assert (c.both["max"]["chroma"].max(axis=1) == 1.0).all() and (c.both["none"]["chroma"] > 0).all()


def test_summary_is_the_summaries_on_the_chroma_rows(c):
    for norm, r in c.both.items():
        got = {"chroma": r["summary"]}
        rows = {"chroma": r["chroma"]}
        assert r["summary"].shape == (len(COUNTS), 4, 12) and r["summary"].dtype == np.float64
        check(got, reference(rows, c.fo), rows, c.fo, norm)
        assert np.isnan(r["summary"][0]).all()  # the clip without buffers
        one = r["chroma"][0].astype(np.float64)  # the clip of one buffer: its own row, variance 0
        assert np.array_equal(r["summary"][1, 0], one) and (r["summary"][1, 1] == 0).all()
        assert np.array_equal(r["summary"][1, 2], one) and np.array_equal(r["summary"][1, 3], one)


def test_each_output_alone_and_no_signals(c, capi):
    whole = c.both["max"]
    rows = c.plan.chroma(*c.args, summary=False)
    assert set(rows) == {"weights", "chroma"}
    same_bits({"c": rows["chroma"]}, {"c": whole["chroma"]}, "per_frame alone")
    summ = c.plan.chroma(*c.args, per_frame=False, summary=True)
    assert set(summ) == {"weights", "summary"}
    same_bits({"s": summ["summary"]}, {"s": whole["summary"]}, "summary alone")
    # no table: the rows alone; a caller's own bank (signed, 5 rows that are no pitch classes)
    bare = c.plan.chroma(c.samples, c.starts)
    same_bits({"c": bare["chroma"]}, {"c": whole["chroma"]}, "no table")
    w = np.random.default_rng(5).standard_normal((5, N // 2)).astype(np.float32)
    own = c.plan.chroma(*c.args, weights=w, norm="max", summary=True)
    same_bits({"c": own["chroma"]}, {"c": chroma_ref.chroma(c.amp, w, "max")}, "a signed bank")
    assert own["summary"].shape == (len(COUNTS), 4, 5)
    # a repeated call gives the same bits
    again = c.plan.chroma(*c.args, summary=True)
    same_bits({k: again[k] for k in ("chroma", "summary")}, {k: whole[k] for k in ("chroma", "summary")}, "repeated")


def test_no_buffers_and_refusals(c, capi):
    none = c.plan.chroma(c.samples[:N - 1], np.zeros(0, np.uint64), np.array([0, 0, 0], np.uint64), summary=True)
    assert none["chroma"].shape == (0, 12) and none["summary"].shape == (2, 4, 12) and np.isnan(none["summary"]).all()
    bad = [dict(frame_offsets=np.array([0, 5, 3], np.uint64)), dict(frame_offsets=np.array([0, sum(COUNTS) + 1], np.uint64)),
           dict(starts=np.array([c.samples.size - N + 1], np.uint64), frame_offsets=np.array([0, 1], np.uint64))]
    for kw in bad:
        with pytest.raises(capi.MgxError) as e:
            c.plan.chroma(c.samples, kw.get("starts", c.starts), kw["frame_offsets"], summary=True)
        assert e.value.status == -1, str(e.value)
    with pytest.raises(capi.MgxError):
        c.plan.chroma(c.samples, c.starts, None, per_frame=False, summary=True)  # summary without signals
    with pytest.raises(capi.MgxError):
        c.plan.chroma(c.samples, c.starts, c.fo, per_frame=False, summary=False)  # nothing asked for


def test_a_chunk_ends_inside_a_signal_and_the_array_grows(capi):
    """N = 256 at hop 16 over one signal of 70,001 buffers, after a call with a small corpus on the same plan (the
    plan's array grows): the first 65,536-buffer chunk ends inside the signal."""
    hop, count = 16, 70001
    samples, lens = corpus(N, hop, [count], 91)
    starts, fo = capi.signals_frame_starts(lens, N, hop)
    assert starts.size == count > 65536
    plan = capi.Plan(buffer_size=N)
    try:
        small = plan.chroma(samples[:N + 40 * hop], starts[:41])
        r = plan.chroma(samples, starts, fo, summary=True)
        amp = plan.extract_gather(samples, starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]
    finally:
        plan.close()
    w = r["weights"]
    got = r["chroma"]
    same_bits({"c": got}, {"c": operator(capi, amp, w, "max")}, "the whole column against the operator")
    same_bits({"c": small["chroma"]}, {"c": got[:41]}, "the first call's rows")
    lo, hi = 65536 - 300, 65536 + 300
    same_bits({"c": got[lo:hi]}, {"c": chroma_ref.chroma(amp[lo:hi], w, "max")}, "the rows around the chunk's end")
    rows = {"chroma": got}
    check({"chroma": r["summary"]}, reference(rows, fo), rows, fo, "one long signal")


def test_a_resident_plan_goes_back_to_its_workgroup(capi):
    n = 1024
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (4, n)).astype(np.float32)
    sig = rng.uniform(-1, 1, 30 * n).astype(np.float32)
    starts, fo = capi.signals_frame_starts([sig.size], n, 256)
    feats = ["rms", "spectralCentroid", "mfcc"]
    ref = capi.Plan(buffer_size=n)
    res = capi.Plan(buffer_size=n, resident=True)
    try:
        a = res.extract(x[:1], feats)  # the resident workgroup is waiting from here on
        got = res.chroma(sig, starts, fo, summary=True)
        b = res.extract(x[1:2], feats)  # ... and serves again after the chroma call ended it
        want = ref.chroma(sig, starts, fo, summary=True)
        same_bits({k: got[k] for k in ("chroma", "summary")}, {k: want[k] for k in ("chroma", "summary")}, "resident plan")
        same_bits(a, ref.extract(x[:1], feats), "before")
        same_bits(b, ref.extract(x[1:2], feats), "after")
    finally:
        res.close()
        ref.close()
