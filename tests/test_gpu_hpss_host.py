"""HPSS on the host path (mgx_hpss_host, include/meyda_gpu.h): the amplitude rows of a corpus of clips kept on the
device for the length of the call, split there, the chroma of the harmonic part and the flux of the percussive part.
Equality of bits against the composition of the device operators (hpss_torch, chroma_torch, flux_torch) on the
amplitude rows mgx_extract_gather_host returns; the summaries, for which there is no operator on device arrays,
against numpy on those rows within the summaries' own documented bounds (tests/test_gpu_summary.py check). The
corpus spans three 65,536-buffer host chunks, and a clip crosses each chunk end."""
import numpy as np
import pytest

from test_gpu_summary import check, corpus, reference, same_bits

pytestmark = pytest.mark.gpu

N, HOP = 256, 16
COUNTS = [0, 1, 70001, 300, 61500]  # a clip shorter than N (no buffers), one of exactly N, three longer
KERNEL, MARGIN = (31, 17), (2.0, 1.5)


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


class Corpus:
    def __init__(self, capi):
        import torch
        self.samples, lens = corpus(N, HOP, COUNTS, 123)
        assert lens[0] == N - 1 and lens[1] == N
        self.starts, self.fo = capi.signals_frame_starts(lens, N, HOP)
        assert np.diff(self.fo.astype(np.int64)).tolist() == COUNTS and self.starts.size > 2 * 65536
        assert self.fo[2] < 65536 < self.fo[3] and self.fo[4] < 2 * 65536 < self.fo[5]  # a clip across each chunk end
        self.plan = capi.Plan(buffer_size=N)
        self.args = (self.samples, self.starts, self.fo)
        self.opts = dict(kernel_size=KERNEL, mode="soft2", margin=MARGIN)
        amp = self.plan.extract_gather(self.samples, self.starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]
        self.weights = capi.chroma_weights(N, 44100.0)
        # the composition of the device operators on those rows
        h, p = capi.hpss_torch(torch.from_numpy(amp).cuda(), self.fo, **self.opts)
        c = capi.chroma_torch(h, self.weights, "max")
        f = capi.flux_torch(p, self.fo, "rectified", 2)
        torch.cuda.synchronize()
        self.want = {"harmonic": h.cpu().numpy(), "percussive": p.cpu().numpy(), "chroma": c.cpu().numpy(), "flux": f.cpu().numpy()}
        self.asks = dict(harmonic=True, percussive=True, chroma=dict(summary=True), flux=dict(mode="rectified", lag=2, summary=True))
        self.all = self.plan.hpss(*self.args, **self.opts, **self.asks)


@pytest.fixture(scope="module")
def c(capi):
    c = Corpus(capi)
    yield c
    c.plan.close()


ROWS = ("harmonic", "percussive", "chroma", "flux")


def test_rows_are_the_composition_of_the_device_operators(c):
    got = c.all
    assert set(got) == {"harmonic", "percussive", "chroma", "chroma_summary", "weights", "flux", "flux_summary"}
    F = sum(COUNTS)
    assert got["harmonic"].shape == got["percussive"].shape == (F, N // 2) and got["chroma"].shape == (F, 12) and got["flux"].shape == (F,)
    assert np.array_equal(got["weights"], c.weights)
    same_bits({k: got[k] for k in ROWS}, c.want, "composition")
    assert np.isfinite(got["harmonic"]).all() and (got["harmonic"] != 0).any() and (got["percussive"] != 0).any()
    # the separation is a partition under unit margins only; here the margins leave a residual, never a surplus
    assert (got["flux"] >= 0).all() and (got["flux"] > 0).any()


def test_summaries_are_the_summaries_of_the_rows(c):
    got = c.all
    assert got["chroma_summary"].shape == (len(COUNTS), 4, 12) and got["flux_summary"].shape == (len(COUNTS), 4)
    rows = {"chroma": got["chroma"]}
    check({"chroma": got["chroma_summary"]}, reference(rows, c.fo), rows, c.fo, "chroma of the harmonic rows")
    rows = {"flux": got["flux"]}
    check({"flux": got["flux_summary"].reshape(len(COUNTS), 4, 1)}, reference(rows, c.fo), rows, c.fo, "flux of the percussive rows")
    assert np.isnan(got["chroma_summary"][0]).all() and np.isnan(got["flux_summary"][0]).all()  # the clip without buffers
    assert (got["flux_summary"][1] == 0).all()  # the clip of one buffer: flux 0, variance 0


def test_the_same_through_hpss_signals(c):
    bounds = np.concatenate([[0], np.cumsum([n for n in corpus(N, HOP, COUNTS, 123)[1]])])
    signals = [c.samples[bounds[i]:bounds[i + 1]] for i in range(len(COUNTS))]
    got = c.plan.hpss_signals(signals, HOP, **c.opts, **c.asks)
    assert np.array_equal(got.pop("frame_offsets"), c.fo)
    same_bits(got, c.all, "hpss_signals")


def test_each_output_alone_a_repeat_and_no_table(c, capi):
    import torch
    whole = c.all
    for name in ("harmonic", "percussive"):
        one = c.plan.hpss(*c.args, **c.opts, **{name: True})
        assert set(one) == {name}
        same_bits(one, {name: whole[name]}, name + " alone")
    one = c.plan.hpss(*c.args, **c.opts, chroma=dict(per_frame=False, summary=True))
    assert set(one) == {"weights", "chroma_summary"}
    same_bits({"s": one["chroma_summary"]}, {"s": whole["chroma_summary"]}, "chroma summary alone")
    one = c.plan.hpss(*c.args, **c.opts, flux=dict(mode="rectified", lag=2))
    assert set(one) == {"flux"}
    same_bits(one, {"flux": whole["flux"]}, "flux alone")
    again = c.plan.hpss(*c.args, **c.opts, **c.asks)
    same_bits(again, whole, "repeated")
    # no table: one signal, every buffer -- the operator without a table on the same rows
    k = 3000
    bare = c.plan.hpss(c.samples, c.starts[:k], None, **c.opts, harmonic=True, flux=dict(lag=1))
    amp = c.plan.extract_gather(c.samples, c.starts[:k], ["amplitudeSpectrum"])["amplitudeSpectrum"]
    h, p = capi.hpss_torch(torch.from_numpy(amp).cuda(), None, **c.opts)
    f = capi.flux_torch(p, None, "rectified", 1)
    torch.cuda.synchronize()
    same_bits(bare, {"harmonic": h.cpu().numpy(), "flux": f.cpu().numpy()}, "no table")


def test_no_buffers_and_refusals(c, capi):
    none = c.plan.hpss(c.samples[:N - 1], np.zeros(0, np.uint64), np.array([0, 0, 0], np.uint64), harmonic=True,
                       chroma=dict(summary=True), flux=dict(summary=True))
    assert none["harmonic"].shape == (0, N // 2) and none["chroma"].shape == (0, 12)
    assert np.isnan(none["chroma_summary"]).all() and np.isnan(none["flux_summary"]).all()
    bad = [dict(frame_offsets=np.array([0, 5, 3], np.uint64)), dict(frame_offsets=np.array([0, sum(COUNTS) + 1], np.uint64)),
           dict(starts=np.array([c.samples.size - N + 1], np.uint64), frame_offsets=np.array([0, 1], np.uint64))]
    for kw in bad:
        with pytest.raises(capi.MgxError) as e:
            c.plan.hpss(c.samples, kw.get("starts", c.starts), kw["frame_offsets"], harmonic=True)
        assert e.value.status == -1, str(e.value)
    with pytest.raises(capi.MgxError):
        c.plan.hpss(*c.args)  # nothing asked for
    with pytest.raises(capi.MgxError):
        c.plan.hpss(*c.args, kernel_size=8, harmonic=True)
    with pytest.raises(capi.MgxError):
        c.plan.hpss(c.samples, c.starts, None, flux=dict(summary=True))  # a summary without signals
