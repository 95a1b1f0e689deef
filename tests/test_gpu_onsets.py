"""Onsets on the host path (mgx_onsets_host, include/meyda_gpu.h): the flux of a field over a corpus of clips and its
peaks within each clip, picked on the device over the column the host flux path keeps there. Equality throughout:
against the numpy picker (tests/peaks_ref.py) on the per_frame column of mgx_summarize_flux_host, against
mgx_peaks_device on the column of mgx_summarize_flux_device, and, for the column and the summary the request names,
against the flux call itself. The buffers exceed one 65,536-buffer host chunk, whose end lies inside the last clip."""
import numpy as np
import pytest

import peaks_ref
from test_gpu_summary import corpus, same_bits

pytestmark = pytest.mark.gpu

N, HOP = 256, 64
COUNTS = [20000, 30011, 5, 1, 20003]
PARAMS = dict(pre_max=3, post_max=3, pre_avg=10, post_avg=10, delta=0.05, wait=4)
REQ = dict(feature="melBands", mode="rectified", lag=1)


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


class Corpus:
    def __init__(self, capi):
        self.samples, lens = corpus(N, HOP, COUNTS, 31)
        self.starts, self.fo = capi.signals_frame_starts(lens, N, HOP)
        assert self.fo[4] < 65536 < self.fo[5] == len(self.starts)
        self.plan = capi.Plan(buffer_size=N, num_mel_bands=40)
        self.args = (self.samples, self.starts, self.fo)
        # the flux call's own column and summary, and the onsets with both
        _, _, fres = self.plan.summarize_gather(*self.args, [], (), flux=[dict(REQ, per_frame=True, summary=True)])
        self.flux = fres[0]
        self.onsets = self.plan.onsets(*self.args, envelope=True, summary=True, **REQ, **PARAMS)


@pytest.fixture(scope="module")
def c(capi):
    c = Corpus(capi)
    yield c
    c.plan.close()


def test_host_call_is_the_picker_on_the_flux_column(c):
    col = c.flux["per_frame"]
    assert col.dtype == np.float32 and np.isfinite(col).all() and (col > 0).any()
    _, wo, wp = peaks_ref.peaks(col, c.fo, **PARAMS)
    assert wp.size > 1000 and (np.diff(wo.astype(np.int64)) > 0).sum() >= 3
    assert np.array_equal(c.onsets["peak_offsets"], wo)
    assert np.array_equal(c.onsets["peaks"], wp)
    # the chunk's end lies between two peaks of the last clip
    assert (wp < 65536).any() and (wp > 65536).any() and wo[4] < np.searchsorted(wp, 65536) < wo[5]


def test_request_outputs_are_the_flux_call_s(c):
    same_bits({"per_frame": c.onsets["envelope"]}, {"per_frame": c.flux["per_frame"]}, "per_frame")
    same_bits({"summary": c.onsets["summary"]}, {"summary": c.flux["summary"]}, "summary")


def test_without_the_request_s_arrays_and_with_a_capacity(c):
    bare = c.plan.onsets(*c.args, **REQ, **PARAMS)
    assert set(bare) == {"peak_offsets", "peaks"}
    assert np.array_equal(bare["peak_offsets"], c.onsets["peak_offsets"]) and np.array_equal(bare["peaks"], c.onsets["peaks"])
    few = c.plan.onsets(*c.args, capacity=100, **REQ, **PARAMS)
    assert np.array_equal(few["peak_offsets"], c.onsets["peak_offsets"]) and np.array_equal(few["peaks"], c.onsets["peaks"][:100])
    counts = c.plan.onsets(*c.args, capacity=0, **REQ, **PARAMS)
    assert counts["peaks"] is None and np.array_equal(counts["peak_offsets"], c.onsets["peak_offsets"])


def test_device_calls_and_the_next_launch_s_table(c, capi):
    import torch
    xs = torch.from_numpy(c.samples).cuda()
    st = torch.from_numpy(c.starts.view(np.int64)).cuda()
    _, _, fres = c.plan.summarize_gather_torch(xs, st, c.fo, [], (), flux=[dict(REQ, per_frame=True, summary=False)])
    col = fres[0]["per_frame"]
    mask, offs, peaks, pst = capi.peaks_torch(col, c.fo, starts=st, **PARAMS)
    torch.cuda.synchronize()
    same_bits({"c": col.cpu().numpy()}, {"c": c.flux["per_frame"]}, "the device call's column")
    total = int(offs[-1])
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), c.onsets["peak_offsets"])
    assert np.array_equal(peaks[:total].cpu().numpy().view(np.uint64), c.onsets["peaks"])
    assert int(mask.sum()) == total
    # the peaks' starts are the next gather launch's table: its rows are the peak buffers' rows
    assert np.array_equal(pst[:total].cpu().numpy().view(np.uint64), c.starts[c.onsets["peaks"].astype(np.int64)])
    pick = slice(0, total, max(total // 300, 1))
    rows = c.plan.extract_gather_torch(xs, pst[:total][pick].contiguous(), ["melBands", "rms"])
    whole = c.plan.extract_gather_torch(xs, st, ["melBands", "rms"])
    torch.cuda.synchronize()
    at = torch.from_numpy(c.onsets["peaks"].astype(np.int64)[pick]).cuda()
    for k in rows:
        same_bits({k: rows[k].cpu().numpy()}, {k: whole[k][at].cpu().numpy()}, ("peak buffers", k))
