"""Tempo on the host path (mgx_tempo_host, include/meyda_gpu.h): the flux of a field over a corpus of clips, its
tempogram pooled per clip and the picked lag, computed over the column the host flux path keeps on the device.
Equality of bits throughout: against mgx_tempo_device on the per_frame column of mgx_summarize_flux_host, and, for
the column and the summary the request names, against the flux call itself. N = 256 at hop 64; the buffers exceed one
65,536-buffer host chunk, whose end lies inside the last clip, as does the end of a pass of tempogram rows."""
import numpy as np
import pytest

import tempo_ref
from test_gpu_summary import corpus, same_bits

pytestmark = pytest.mark.gpu

N, HOP = 256, 64
COUNTS = [20000, 30011, 5, 0, 1, 20003]
REQ = dict(feature="melBands", mode="rectified", lag=1)
RATE = 44100.0 / HOP
# (689 rows a second and 48 lags: 861 bpm and above, so the prior is centred there and has no upper limit)
TEMPO = dict(win_length=64, num_lags=48, start_bpm=1200.0, max_bpm=0.0)


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


class Corpus:
    def __init__(self, capi):
        self.samples, lens = corpus(N, HOP, COUNTS, 37)
        self.starts, self.fo = capi.signals_frame_starts(lens, N, HOP)
        assert self.fo[5] < 65536 < self.fo[6] == len(self.starts)
        self.plan = capi.Plan(buffer_size=N, num_mel_bands=40)
        self.args = (self.samples, self.starts, self.fo)
        # the flux call's own column and summary, and the tempo call with both
        _, _, fres = self.plan.summarize_gather(*self.args, [], (), flux=[dict(REQ, per_frame=True, summary=True)])
        self.flux = fres[0]
        self.tempo = self.plan.tempo(*self.args, RATE, mean=True, envelope=True, envelope_summary=True, **REQ, **TEMPO)


@pytest.fixture(scope="module")
def c(capi):
    c = Corpus(capi)
    yield c
    c.plan.close()


def test_host_call_is_the_device_call_on_the_flux_column(c, capi):
    import torch
    col = c.flux["per_frame"]
    assert col.dtype == np.float32 and np.isfinite(col).all() and (col > 0).any()
    dev = capi.tempo_torch(torch.from_numpy(col).cuda(), torch.from_numpy(c.tempo["window"]).cuda(),
                           torch.from_numpy(c.tempo["prior"]).cuda(), c.fo, num_lags=TEMPO["num_lags"])
    torch.cuda.synchronize()
    same_bits({"summary": c.tempo["summary"]}, {"summary": dev["summary"].cpu().numpy()}, "summary")
    assert np.array_equal(c.tempo["lag"], dev["lag"].cpu().numpy().astype(np.uint32))
    assert c.tempo["lag"].dtype == np.uint32 and c.tempo["summary"].shape == (6, 4, 48)
    # ... which is the statement's pick of the returned mean; an empty clip has no tempo
    assert np.array_equal(c.tempo["lag"], tempo_ref.pick_ref(c.tempo["summary"][:, 0, :], c.tempo["prior"]))
    assert c.tempo["lag"][3] == 0 and np.isnan(c.tempo["summary"][3]).all() and np.isnan(c.tempo["bpm"][3])
    live = c.tempo["lag"] > 0
    assert live[[0, 1, 5]].all() and np.array_equal(c.tempo["bpm"][live], 60.0 * RATE / c.tempo["lag"][live])
    # the first rows of the first clip against the statement itself
    rows = tempo_ref.tempogram_ref(col[:2000], c.tempo["window"], 48, tempo_ref.NORM_LAG0, [0, 20000])
    got = capi.tempogram_torch(torch.from_numpy(col).cuda(), torch.from_numpy(c.tempo["window"]).cuda(), c.fo, 48)
    assert np.array_equal(got[:1900].cpu().numpy().view(np.uint32), rows[:1900].view(np.uint32))


def test_request_outputs_are_the_flux_call_s(c):
    same_bits({"per_frame": c.tempo["envelope"]}, {"per_frame": c.flux["per_frame"]}, "per_frame")
    same_bits({"summary": c.tempo["envelope_summary"]}, {"summary": c.flux["summary"]}, "summary")


def test_outputs_are_optional_and_a_repeat_is_equal(c, capi):
    import ctypes
    bare = c.plan.tempo(*c.args, RATE, **REQ, **TEMPO)
    assert set(bare) == {"lag", "bpm", "window", "prior"} and np.array_equal(bare["lag"], c.tempo["lag"])
    again = c.plan.tempo(*c.args, RATE, mean=True, **REQ, **TEMPO)
    same_bits({"summary": again["summary"]}, {"summary": c.tempo["summary"]}, "repeated")
    # the summary alone: no prior, no lag
    reqs, _ = c.plan._flux_requests(c.starts.size, 6, [dict(REQ, per_frame=False, summary=False)], None, None)
    tp = capi.tempo_params(64, 48)
    summ = np.empty((6, 4, 48), np.float64)
    capi.check(capi.lib().mgx_tempo_host(c.plan._h, c.samples.ctypes.data, c.samples.size, c.starts.ctypes.data, c.starts.size,
                                         c.fo.ctypes.data, 6, reqs, ctypes.byref(tp), c.tempo["window"].ctypes.data, None,
                                         summ.ctypes.data, None))
    same_bits({"summary": summ}, {"summary": c.tempo["summary"]}, "summary alone")


def test_signals_and_no_buffers(c, capi):
    sig = [c.samples[:N + 999 * HOP], c.samples[:N - 1], c.samples[5000:5000 + N + 499 * HOP]]
    res = c.plan.tempo_signals(sig, HOP, mean=True, **REQ, **TEMPO)
    assert list(res["frame_offsets"]) == [0, 1000, 1000, 1500] and res["lag"][1] == 0 and np.isnan(res["summary"][1]).all()
    assert np.array_equal(res["prior"], capi.tempo_prior(c.plan.desc.sample_rate / HOP, 48, 1200.0, 1.0, 0.0))
    # no buffer at all: NaN in all four and no tempo, nothing for the device to do
    none = c.plan.tempo_signals([c.samples[:10], c.samples[:20]], HOP, mean=True, **REQ, **TEMPO)
    assert np.isnan(none["summary"]).all() and (none["lag"] == 0).all() and none["summary"].shape == (2, 4, 48)
