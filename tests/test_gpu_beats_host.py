"""Beats on the host path (mgx_beats_host, include/meyda_gpu.h): the flux of a field over a corpus of clips, the lag the
tempo prior picks per clip and the beats tracked at that lag, over the column and the lags that stay on the device.
Equality throughout: against mgx_beats_device on the per_frame column of mgx_summarize_flux_host and the lags of
mgx_tempo_host, against the numpy statement on that column, and, for the column and the summary the request names,
against the flux call itself bit for bit. N = 256 at hop 64; the buffers exceed one 65,536-buffer host chunk, whose end
lies inside the last clip."""
import numpy as np
import pytest

import beat_ref
from test_gpu_summary import corpus, same_bits

pytestmark = pytest.mark.gpu

N, HOP = 256, 64
COUNTS = [20000, 30011, 5, 0, 1, 20003]
REQ = dict(feature="melBands", mode="rectified", lag=1)
RATE = 44100.0 / HOP
# (689 rows a second and 48 lags: the prior is centred on 1,200 bpm and has no upper limit; the lags stay below 48)
TEMPO = dict(win_length=64, num_lags=48, start_bpm=1200.0, max_bpm=0.0)
P = 47


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


class Corpus:
    def __init__(self, capi):
        self.samples, lens = corpus(N, HOP, COUNTS, 41)
        # a burst every 30 buffers in the first clip and every 21 in the last: an envelope with some shape
        at = np.arange(self.samples.size)
        self.samples[:lens[0]] *= np.where(at[:lens[0]] % (30 * HOP) < 2 * HOP, 4.0, 1.0).astype(np.float32)
        self.samples[-lens[5]:] *= np.where(at[:lens[5]] % (21 * HOP) < 2 * HOP, 4.0, 1.0).astype(np.float32)
        self.starts, self.fo = capi.signals_frame_starts(lens, N, HOP)
        assert self.fo[5] < 65536 < self.fo[6] == len(self.starts)
        self.plan = capi.Plan(buffer_size=N, num_mel_bands=40)
        self.args = (self.samples, self.starts, self.fo)
        _, _, fres = self.plan.summarize_gather(*self.args, [], (), flux=[dict(REQ, per_frame=True, summary=True)])
        self.flux = fres[0]
        self.tempo = self.plan.tempo(*self.args, RATE, **REQ, **TEMPO)
        self.tables = capi.beat_tables(P)
        self.beats = self.plan.beats(*self.args, RATE, envelope=True, envelope_summary=True, tables=self.tables, **REQ, **TEMPO)


@pytest.fixture(scope="module")
def c(capi):
    c = Corpus(capi)
    yield c
    c.plan.close()


def test_host_call_is_the_device_call_on_the_column_and_the_lags(c, capi):
    import torch
    col, lag = c.flux["per_frame"], c.tempo["lag"]
    assert np.array_equal(c.beats["lag"], lag) and lag.dtype == np.uint32 and (lag < 48).all()
    assert (lag[[0, 1, 5]] > 0).all() and lag[3] == 0
    dev = capi.beats_torch(torch.from_numpy(col).cuda(), lag, c.tables[0], c.tables[1], c.fo, max_period=P)
    torch.cuda.synchronize()
    off = dev["peak_offsets"].cpu().numpy().astype(np.uint64)
    assert np.array_equal(c.beats["peak_offsets"], off) and c.beats["peak_offsets"].dtype == np.uint64
    total = int(off[-1])
    assert c.beats["beats"].shape == (total,) and total > 2000
    assert np.array_equal(c.beats["beats"], dev["peaks"].cpu().numpy()[:total].astype(np.uint64))
    # ... which is the statement's answer on that column
    ref = beat_ref.beats_ref(col, lag, c.fo, P, *c.tables)
    assert np.array_equal(ref["peak_offsets"], off) and np.array_equal(ref["peaks"], c.beats["beats"])
    # beats are lo(p) .. 2 p rows apart: a long clip has many, and at most n / lo(p) + 1; none in a clip of one row or none
    for s in (0, 1, 5):
        n, k = int(c.fo[s + 1] - c.fo[s]), int(off[s + 1] - off[s])
        rows = c.beats["beats"][int(off[s]):int(off[s + 1])].astype(np.int64)
        assert 100 < k <= n // beat_ref.lo(int(lag[s])) + 1, (s, k)
        assert (np.diff(rows) >= beat_ref.lo(int(lag[s]))).all() and (np.diff(rows) <= 2 * int(lag[s])).all()
        assert rows[0] >= c.fo[s] and rows[-1] < c.fo[s + 1]
    assert off[4] == off[3] and off[5] == off[4]
    assert np.array_equal(c.beats["bpm"][[0, 5]], 60.0 * RATE / lag[[0, 5]])


def test_request_outputs_are_the_flux_call_s(c):
    same_bits({"per_frame": c.beats["envelope"]}, {"per_frame": c.flux["per_frame"]}, "per_frame")
    same_bits({"summary": c.beats["envelope_summary"]}, {"summary": c.flux["summary"]}, "summary")


def test_capacity_and_repeat(c):
    total = int(c.beats["peak_offsets"][-1])
    few = c.plan.beats(*c.args, RATE, tables=c.tables, capacity=100, **REQ, **TEMPO)
    assert set(few) == {"lag", "bpm", "peak_offsets", "beats", "window", "prior"}
    assert np.array_equal(few["peak_offsets"], c.beats["peak_offsets"]) and np.array_equal(few["beats"], c.beats["beats"][:100])
    counts = c.plan.beats(*c.args, RATE, tables=c.tables, capacity=0, **REQ, **TEMPO)
    assert counts["beats"] is None and int(counts["peak_offsets"][-1]) == total
    # the tables made by the call itself, and no trim
    again = c.plan.beats(*c.args, RATE, **REQ, **TEMPO)
    assert np.array_equal(again["beats"], c.beats["beats"])
    loose = c.plan.beats(*c.args, RATE, trim=False, **REQ, **TEMPO)
    assert set(c.beats["beats"]) <= set(loose["beats"])


def test_signals_and_no_buffers(c, capi):
    sig = [c.samples[:N + 999 * HOP], c.samples[:N - 1], c.samples[5000:5000 + N + 499 * HOP]]
    res = c.plan.beats_signals(sig, HOP, **REQ, **TEMPO)
    assert list(res["frame_offsets"]) == [0, 1000, 1000, 1500] and res["lag"][1] == 0
    off = res["peak_offsets"]
    assert off[1] > 20 and off[2] == off[1] and off[3] > off[2] and res["beats"].size == off[3]
    assert (res["beats"][:off[1]] < 1000).all() and (res["beats"][off[2]:] >= 1000).all()
    none = c.plan.beats_signals([c.samples[:10], c.samples[:20]], HOP, **REQ, **TEMPO)
    assert (none["lag"] == 0).all() and (none["peak_offsets"] == 0).all() and none["beats"].size == 0
    with pytest.raises(capi.MgxError):
        c.plan.beats(*c.args, RATE, max_period=46, **REQ, **TEMPO)
