"""Flux through the summaries (mgx_summarize_flux_device / _host, include/meyda_gpu.h). The rows come from
Plan.extract_gather on the same plan; the per-frame flux is the numpy definition's on those rows (tests/flux_ref.py;
bit for bit in the RECTIFIED and L1 modes, within the root's last bit in L2 as in test_gpu_flux.py), and its summary
is numpy's on that column under the summaries' own bounds (test_gpu_summary.py check). Everything else is equality
of bits: the host call against the device call wherever the chunks end, and everything the call wrote before
against the calls without flux."""
import numpy as np
import pytest

import flux_ref
from test_gpu_flux import check_l2, same
from test_gpu_summary import COUNTS, check, corpus, reference, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def host_of(d):
    return None if d is None else {k: v.cpu().numpy() for k, v in d.items()}


def flux_host_of(fres):
    return [{k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()} for r in fres]


def device(plan, samples, starts, fo, feats, per_frame=(), deltas=None, flux=None):
    import torch
    r = plan.summarize_gather_torch(torch.from_numpy(samples).cuda(), starts, fo, feats, per_frame, deltas=deltas, flux=flux)
    torch.cuda.synchronize()
    return tuple(flux_host_of(v) if isinstance(v, list) else host_of(v) for v in r)


def same_flux(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        for k in ("summary", "per_frame"):
            assert (x[k] is None) == (y[k] is None), (what, i, k)
            if x[k] is not None:
                same_bits({k: x[k]}, {k: y[k]}, (what, i))


REQS = [dict(feature="melBands", mode="rectified", lag=1, per_frame=True),
        dict(feature="amplitudeSpectrum", mode="l2", lag=2, per_frame=True),
        dict(feature="amplitudeSpectrum", mode="l1", lag=8, per_frame=True),
        dict(feature="loudness", mode="rectified", lag=3, per_frame=True)]
ROWS_OF = {"melBands": "melBands", "amplitudeSpectrum": "amplitudeSpectrum", "loudness": "loudness.specific", "mfcc": "mfcc",
           "powerSpectrum": "powerSpectrum"}


class Corner:
    def __init__(self, capi):
        self.n, self.hop = 256, 64
        self.samples, lens = corpus(self.n, self.hop, COUNTS, 2025)
        self.starts, self.fo = capi.signals_frame_starts(lens, self.n, self.hop)
        self.plan = capi.Plan(buffer_size=self.n, num_mel_bands=40)
        self.rows = self.plan.extract_gather(self.samples, self.starts, ["melBands", "amplitudeSpectrum", "loudness", "mfcc"])
        self.args = (self.samples, self.starts, self.fo)
        _, _, self.flux = device(self.plan, *self.args, [], (), flux=REQS)


@pytest.fixture(scope="module")
def corner(capi):
    c = Corner(capi)
    yield c
    c.plan.close()


def test_per_frame_flux_is_the_definition_s_on_the_rows(corner):
    c = corner
    # (at N = 256 the lowest of 40 mel filters span no bin: their bands are -Infinity in every buffer)
    assert np.isneginf(c.rows["melBands"]).all(axis=0).any()
    for q, r in zip(REQS, c.flux):
        x = c.rows[ROWS_OF[q["feature"]]]
        got = r["per_frame"]
        assert got.dtype == np.float32 and got.shape == (len(c.starts),) and np.isfinite(got).all(), q
        if q["mode"] == "l2":
            check_l2(got, x, c.fo, q["lag"], q, fill=0.0)
        else:
            same(got, flux_ref.flux(x, c.fo, q["mode"], q["lag"]), q)
        first = [int(a) for a, b in zip(c.fo[:-1], c.fo[1:]) if b > a]
        assert (got[first] == 0).all() and (got > 0).any()


def test_summary_is_the_summaries_on_the_flux_column(corner):
    c = corner
    for q, r in zip(REQS, c.flux):
        col = {"flux": r["per_frame"]}
        got = {"flux": r["summary"].reshape(len(COUNTS), 4, 1)}
        check(got, reference(col, c.fo), col, c.fo, q)
        s = COUNTS.index(1)  # a one-buffer signal: its flux is 0
        assert (got["flux"][s] == 0).all()


def test_same_bits_everywhere(corner):
    c = corner
    _, _, host = c.plan.summarize_gather(*c.args, [], (), flux=REQS)
    same_flux(host, c.flux, "host call")
    _, _, again = device(c.plan, *c.args, [], (), flux=REQS)
    same_flux(again, c.flux, "device call repeated")
    # without per_frame the column lives in the workspace: the same summary
    only = [dict(q, per_frame=False) for q in REQS]
    for what, got in (("device", device(c.plan, *c.args, [], (), flux=only)[2]), ("host", c.plan.summarize_gather(*c.args, [], (), flux=only)[2])):
        for g, w in zip(got, c.flux):
            assert g["per_frame"] is None
            same_bits({"s": g["summary"]}, {"s": w["summary"]}, (what, "summary alone"))
    # per_frame alone
    cols = [dict(q, summary=False) for q in REQS[:2]]
    for what, got in (("device", device(c.plan, *c.args, ["rms"], (), flux=cols)[2]), ("host", c.plan.summarize_gather(*c.args, ["rms"], (), flux=cols)[2])):
        for g, w in zip(got, c.flux):
            assert g["summary"] is None
            same_bits({"c": g["per_frame"]}, {"c": w["per_frame"]}, (what, "per_frame alone"))


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_everything_else_is_written_as_before(corner, host):
    c = corner
    pooled, per_frame, deltas = ["rms", "mfcc", "loudness"], ["zcr", "melBands", "amplitudeSpectrum"], (2, 2)
    call = (lambda **kw: c.plan.summarize_gather(*c.args, pooled, per_frame, **kw)) if host else \
        (lambda **kw: device(c.plan, *c.args, pooled, per_frame, **kw))
    # a field requested per frame (amplitudeSpectrum), one pooled and delta'd (loudness), one nothing else keeps
    reqs = REQS + [dict(feature="powerSpectrum", mode="l1", lag=1)]
    reqs = reqs[1:]
    want = call(deltas=deltas)
    got = call(deltas=deltas, flux=reqs)
    assert len(got) == 5 and len(want) == 4
    for g, w, what in zip(got, want, ("base", "rows", "delta", "delta2")):
        same_bits(g, w, (what, "beside flux"))
    same_flux(got[4][:3], c.flux[1:], "flux beside deltas")
    # deltas = NULL
    want = call()
    got = call(flux=reqs)
    assert len(got) == 3
    same_bits(got[0], want[0], "base, deltas = NULL")
    same_bits(got[1], want[1], "rows, deltas = NULL")
    same_flux(got[2][:3], c.flux[1:], "flux, deltas = NULL")
    # no request: the deltas call
    want = call(deltas=deltas)
    got = call(deltas=deltas, flux=[])
    assert got[4] == []
    for g, w, what in zip(got, want, ("base", "rows", "delta", "delta2")):
        same_bits(g, w, (what, "num_flux = 0"))


def test_no_buffers_and_no_signals(corner):
    c = corner
    none = np.empty(0, np.uint64)
    q = [dict(feature="mfcc", per_frame=True)]
    for host in (False, True):
        call = c.plan.summarize_gather if host else (lambda *a, **kw: device(c.plan, *a, **kw))
        summ, _, fl = call(c.samples, none, np.array([0, 0, 0], np.uint64), ["rms"], (), flux=q)
        assert np.isnan(summ["rms"]).all() and fl[0]["summary"].shape == (2, 4) and np.isnan(fl[0]["summary"]).all()
        assert fl[0]["per_frame"].shape == (0,)
        # no signal: the gather call; no row belongs to a signal, and no flux is written
        _, rows, fl = call(c.samples, c.starts, np.array([0], np.uint64), [], ["mfcc"], flux=[dict(q[0], summary=False)])
        same_bits(rows, {"mfcc": c.rows["mfcc"]}, "no signal")
        assert (fl[0]["per_frame"] == 0).all()


def test_rows_of_no_signal_keep_their_sentinels(capi, corner):
    """A table that leaves rows before its first and after its last signal: neither call writes them in per_frame
    (the host call's plan-owned column holds whatever an earlier call left there), and the two agree bit for bit."""
    import ctypes

    import torch
    c = corner
    F = len(c.starts)
    fo = np.array([3, 10, 10, F - 4], np.uint64)
    S = len(fo) - 1
    sentinel = 777.0
    _, so = c.plan._summary_outputs(S, [], lambda shape: np.empty(shape))
    _, none = c.plan._host_outputs(0, [])
    # an earlier host call over every row leaves values in the plan's column
    c.plan.summarize_gather(*c.args, [], (), flux=[dict(feature="amplitudeSpectrum", mode="l1", lag=1, per_frame=True)])

    def request(per_frame_ptr, summary_ptr):
        r = (capi.FluxRequest * 1)()
        r[0].struct_size, r[0].field, r[0].mode, r[0].lag = 32, capi.FLUX_FEATURES["amplitudeSpectrum"], 1, 1
        r[0].per_frame, r[0].summary = per_frame_ptr, summary_ptr
        return r
    hcol, hsum = np.full(F, sentinel, np.float32), np.full((S, 4), sentinel)
    capi.check(capi.lib().mgx_summarize_flux_host(c.plan._h, c.samples.ctypes.data, c.samples.size, c.starts.ctypes.data, F,
                                                  fo.ctypes.data, S, ctypes.byref(none), None, ctypes.byref(so), None,
                                                  request(hcol.ctypes.data, hsum.ctypes.data), 1))
    dcol = torch.full((F,), sentinel, dtype=torch.float32, device="cuda")
    dsum = torch.full((S, 4), sentinel, dtype=torch.float64, device="cuda")
    xs = torch.from_numpy(c.samples).cuda()
    st = torch.from_numpy(c.starts.view(np.int64)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    r = request(dcol.data_ptr(), dsum.data_ptr())
    nbytes = c.plan.summarize_flux_workspace_bytes(none, so, None, r, 1, F, S)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    c.plan.summarize_flux_device(xs.data_ptr(), xs.shape[0], st.data_ptr(), F, tb.data_ptr(), S, none, so, None, r, 1, ws.data_ptr(),
                                 nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dcol, dsum = dcol.cpu().numpy(), dsum.cpu().numpy()
    want = flux_ref.flux(c.rows["amplitudeSpectrum"], fo, "l1", 1, fill=sentinel)
    same(dcol, want, "device call")
    same(hcol, want, "host call")
    assert (hcol[:3] == sentinel).all() and (hcol[F - 4:] == sentinel).all() and hcol[3] == 0 and hcol[10] == 0 and (hcol[4:10] > 0).all()
    same_bits({"s": hsum}, {"s": dsum}, "summaries, host against device")
    assert np.isnan(hsum[1]).all() and np.isfinite(hsum[[0, 2]]).all()


def test_unsupported_field(capi, corner):
    c = corner
    _, so = c.plan._summary_outputs(2, [], lambda shape: np.empty(shape))
    _, none = c.plan._host_outputs(0, [])
    r = (capi.FluxRequest * 1)()
    r[0].struct_size, r[0].mode, r[0].lag, r[0].summary = 32, 0, 1, 256
    for field in (0, 12, 17, 18):
        r[0].field = field
        with pytest.raises(capi.MgxError) as e:
            c.plan.summarize_flux_workspace_bytes(none, so, None, r, 1, 8, 2)
        assert e.value.status == -3


@pytest.fixture(scope="module")
def straddle(capi):
    n, hop, counts = 256, 8, [40000, 30011, 5, 70001]
    samples, lens = corpus(n, hop, counts, 77)
    starts, fo = capi.signals_frame_starts(lens, n, hop)
    # the host path's 65,536-buffer chunks end inside the second and fourth signals
    for end, s in ((65536, 1), (131072, 3)):
        assert fo[s] < end < fo[s + 1]
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    yield plan, samples, starts, fo
    plan.close()


def test_host_chunks_straddle_signals(straddle):
    plan, samples, starts, fo = straddle
    reqs = [dict(feature="mfcc", mode="rectified", lag=1, per_frame=True), dict(feature="mfcc", mode="l1", lag=8, per_frame=True),
            dict(feature="amplitudeSpectrum", mode="l2", lag=1, per_frame=True),
            dict(feature="amplitudeSpectrum", mode="rectified", lag=8, per_frame=True)]
    dev = device(plan, samples, starts, fo, ["rms"], (), deltas=(2, 1), flux=reqs)
    host = plan.summarize_gather(samples, starts, fo, ["rms"], (), deltas=(2, 1), flux=reqs)
    same_bits(host[0], dev[0], "base, host against device")
    same_bits(host[2], dev[2], "delta, host against device")
    same_flux(host[4], dev[4], "flux, host against device")
    amp = dev[4][3]["per_frame"]
    assert np.isfinite(amp).all() and (amp[[65535, 65536, 65537, 65543, 131072, 131079]] > 0).all()
    # the rows around a chunk's end against the definition, on the rows themselves
    rows = plan.extract_gather(samples, starts[65536 - 16:65536 + 16], ["amplitudeSpectrum"])["amplitudeSpectrum"]
    want = flux_ref.flux(rows, None, "rectified", 8)
    same(amp[65536 - 8:65536 + 16], want[8:], "across the chunk's end")
    # the mfcc columns of this scalar_f64 plan (its array fields stay float32) against the definition on the rows of
    # extract_gather, so that no error shared by the routes passes
    mfcc = plan.extract_gather(samples, starts, ["mfcc"])["mfcc"]
    assert mfcc.dtype == np.float32
    for i, q in enumerate(reqs[:2]):
        same(dev[4][i]["per_frame"], flux_ref.flux(mfcc, fo, q["mode"], q["lag"]), ("mfcc against the definition", q))
