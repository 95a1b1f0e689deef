"""Deltas through the summaries (mgx_summarize_deltas_device / _host, include/meyda_gpu.h): the statistics of the
delta and second-order rows of every signal. The rows come from Plan.extract_gather on the same plan and their
deltas from mgx_delta_device (pinned to the definition in test_gpu_delta.py); the expected values are numpy's on
those, under the summaries' own bounds (test_gpu_summary.py check). Everything else is equality of bits: the host
call, a repeated call and a capped grid against the device call, and the base summaries and per-frame rows against
mgx_summarize_device."""
import ctypes

import numpy as np
import pytest

from test_gpu_signal import env_plan
from test_gpu_summary import COUNTS, check, corpus, reference, same_bits

pytestmark = pytest.mark.gpu

W = 2


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def keys(feats):
    return [k for f in feats for k in (["loudness.specific", "loudness.total"] if f == "loudness" else [f])]


def call(capi, plan, samples, starts, fo, base, per_frame=(), d1=None, d2=None, width=W, host=False, no_deltas=False):
    """mgx_summarize_deltas_device (or _host) with separate feature lists for the base summaries, the delta and the
    second-order summaries (None: that pointer of mgx_delta_summaries is NULL; no_deltas: the struct itself is).
    Returns (summaries, rows, delta summaries, second-order summaries) as numpy."""
    import torch
    S, F = len(fo) - 1, len(starts)
    if host:
        alloc = lambda shape: np.empty(shape, np.float64)
        rows, o = plan._host_outputs(F, per_frame)
    else:
        alloc = lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        rows, o = plan.alloc_outputs(F, per_frame)
    summ, so = plan._summary_outputs(S, base, alloc)
    ds = capi.DeltaSummaries()
    ds.struct_size = ctypes.sizeof(capi.DeltaSummaries)
    ds.width = width
    got = [None, None]
    keep = []
    for k, feats in enumerate((d1, d2)):
        if feats is not None:
            got[k], s = plan._summary_outputs(S, feats, alloc)
            keep.append(s)
            setattr(ds, ("delta", "delta2")[k], ctypes.pointer(s))
    dref = None if no_deltas else ds
    if host:
        capi.check(capi.lib().mgx_summarize_deltas_host(plan._h, samples.ctypes.data, samples.size, starts.ctypes.data, F,
                                                        fo.ctypes.data, S, ctypes.byref(o), capi._aux_ref(o), ctypes.byref(so),
                                                        None if dref is None else ctypes.byref(dref)))
        return summ, rows, got[0], got[1]
    xs = torch.from_numpy(samples).cuda()
    st = torch.from_numpy(starts.view(np.int64)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    nbytes = plan.summarize_deltas_workspace_bytes(o, so, dref, F, S)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    plan.summarize_deltas_device(xs.data_ptr(), xs.shape[0], st.data_ptr(), F, tb.data_ptr(), S, o, so, dref, ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host_of = lambda d: None if d is None else {k: v.cpu().numpy() for k, v in d.items()}
    return host_of(summ), host_of(rows), host_of(got[0]), host_of(got[1])


def delta_rows(capi, rows, fo, width=W):
    """mgx_delta_device on every per-frame array: ({name: delta rows}, {name: second-order rows}) as numpy."""
    import torch
    out = ({}, {})
    tb = torch.from_numpy(np.asarray(fo, np.uint64).view(np.int64)).cuda()
    for k, v in rows.items():
        d = capi.delta_torch(torch.from_numpy(v).cuda(), tb, width, 2)
        torch.cuda.synchronize()
        out[0][k], out[1][k] = d[0].cpu().numpy(), d[1].cpu().numpy()
    return out


class Corner:
    """The corner-count corpus of one plan kind: the rows, their deltas, and the device call's results, once."""

    def __init__(self, capi, f64):
        self.n, self.hop = 256, 64
        self.feats = capi.ALL_FEATURES + ["melBands"]  # every scalar, loudness, mfcc, melBands
        self.samples, lens = corpus(self.n, self.hop, COUNTS, 2024)
        self.starts, self.fo = capi.signals_frame_starts(lens, self.n, self.hop)
        self.kw = dict(buffer_size=self.n, num_mel_bands=40, scalar_f64=f64)
        self.plan = capi.Plan(**self.kw)
        self.rows = self.plan.extract_gather(self.samples, self.starts, self.feats)
        self.drows = delta_rows(capi, self.rows, self.fo)
        self.args = (self.samples, self.starts, self.fo)
        self.base, _, self.d1, self.d2 = call(capi, self.plan, *self.args, self.feats, (), self.feats, self.feats)


@pytest.fixture(scope="module", params=[False, True], ids=["scalar_f32", "scalar_f64"])
def corner(request, capi):
    c = Corner(capi, request.param)
    yield c
    c.plan.close()


def test_against_numpy_on_the_delta_rows(corner):
    c = corner
    assert set(c.d1) == set(c.d2) == set(c.rows) and c.d2["melBands"].shape == (len(COUNTS), 4, 40)
    sd = c.rows["rms"].dtype
    assert sd == (np.float64 if c.kw["scalar_f64"] else np.float32) and c.drows[0]["rms"].dtype == sd
    for got, rows, what in ((c.d1, c.drows[0], "delta"), (c.d2, c.drows[1], "delta2")):
        check(got, reference(rows, c.fo), rows, c.fo, what)
    # a one-buffer signal: mean = min = max = 0 and variance exactly 0, wherever its row is finite
    s = COUNTS.index(1)
    for k, v in c.rows.items():
        fin = np.isfinite(v[int(c.fo[s])].reshape(-1))
        # (at N = 256 the lowest of 40 mel filters span no bin: their bands are -Infinity in every buffer, and with
        # them every MFCC; test_finite_mfcc below has the plan whose MFCCs are finite)
        assert fin.any() or k == "mfcc", k
        assert (c.d1[k][s][:, fin] == 0).all() and (c.d2[k][s][:, fin] == 0).all(), k


def test_same_bits_everywhere(capi, corner):
    c = corner
    _, _, h1, h2 = call(capi, c.plan, *c.args, c.feats, (), c.feats, c.feats, host=True)
    same_bits(h1, c.d1, "host call, delta")
    same_bits(h2, c.d2, "host call, delta2")
    _, _, a1, a2 = call(capi, c.plan, *c.args, c.feats, (), c.feats, c.feats)
    same_bits(a1, c.d1, "device call repeated, delta")
    same_bits(a2, c.d2, "device call repeated, delta2")
    capped = env_plan(capi, {"MGX_GRID_CAP": 8}, **c.kw)
    try:
        _, _, g1, g2 = call(capi, capped, *c.args, c.feats, (), c.feats, c.feats)
    finally:
        capped.close()
    same_bits(g1, c.d1, "MGX_GRID_CAP=8, delta")
    same_bits(g2, c.d2, "MGX_GRID_CAP=8, delta2")
    # the binding's own entry points
    xs = __import__("torch").from_numpy(c.samples).cuda()
    _, _, t1, t2 = c.plan.summarize_gather_torch(xs, c.starts, c.fo, c.feats, deltas=(W, 2))
    same_bits({k: v.cpu().numpy() for k, v in t1.items()}, c.d1, "summarize_gather_torch")
    same_bits({k: v.cpu().numpy() for k, v in t2.items()}, c.d2, "summarize_gather_torch")
    _, _, s1, s2 = c.plan.summarize_gather(c.samples, c.starts, c.fo, c.feats, deltas=(W, 2))
    same_bits(s1, c.d1, "summarize_gather")
    same_bits(s2, c.d2, "summarize_gather")


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_base_summaries_and_rows_are_the_summary_call_s(capi, corner, host):
    c = corner
    import torch
    pooled, per_frame = ["rms", "mfcc", "melBands", "loudness"], ["mfcc", "zcr", "amplitudeSpectrum"]
    dfeats = ["mfcc", "spectralRolloff", "melBands"]  # requested per frame and pooled; neither; pooled only
    if host:
        want_s, want_r = c.plan.summarize_gather(*c.args, pooled, per_frame)
    else:
        s, r = c.plan.summarize_gather_torch(torch.from_numpy(c.samples).cuda(), c.starts, c.fo, pooled, per_frame)
        torch.cuda.synchronize()
        want_s, want_r = ({k: v.cpu().numpy() for k, v in d.items()} for d in (s, r))
    summ, rows, d1, d2 = call(capi, c.plan, *c.args, pooled, per_frame, dfeats, dfeats, host=host)
    same_bits(summ, want_s, "base summaries beside deltas")
    same_bits(rows, want_r, "rows beside deltas")
    same_bits(d1, {k: c.d1[k] for k in keys(dfeats)}, "delta")
    same_bits(d2, {k: c.d2[k] for k in keys(dfeats)}, "delta2")
    summ, rows, d1, d2 = call(capi, c.plan, *c.args, pooled, per_frame, host=host, no_deltas=True)
    same_bits(summ, want_s, "base summaries, deltas = NULL")
    same_bits(rows, want_r, "rows, deltas = NULL")
    assert d1 is None and d2 is None


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_second_order_alone_and_no_base_field(capi, corner, host):
    c = corner
    # a field named only in delta2, another only in delta
    summ, _, d1, d2 = call(capi, c.plan, *c.args, ["zcr"], (), ["rms"], ["mfcc", "energy"], host=host)
    same_bits(summ, {"zcr": c.base["zcr"]}, "base")
    same_bits(d1, {"rms": c.d1["rms"]}, "delta")
    same_bits(d2, {k: c.d2[k] for k in ("mfcc", "energy")}, "delta2 alone")
    # delta NULL altogether
    _, _, d1, d2 = call(capi, c.plan, *c.args, ["zcr"], (), None, ["melBands"], host=host)
    assert d1 is None
    same_bits(d2, {"melBands": c.d2["melBands"]}, "delta = NULL")
    # `summary` with no field at all, with and without per-frame rows
    summ, rows, d1, d2 = call(capi, c.plan, *c.args, [], ["mfcc"], ["mfcc", "loudness"], ["mfcc"], host=host)
    assert summ == {}
    same_bits(rows, {"mfcc": c.rows["mfcc"]}, "rows")
    same_bits(d1, {k: c.d1[k] for k in ("mfcc", "loudness.specific", "loudness.total")}, "no base field, delta")
    same_bits(d2, {"mfcc": c.d2["mfcc"]}, "no base field, delta2")
    # order 1 at another width: against numpy on the operator's rows
    _, _, d1, d2 = call(capi, c.plan, *c.args, [], (), ["mfcc"], None, width=8, host=host)
    assert d2 is None
    rows8 = delta_rows(capi, {"mfcc": c.rows["mfcc"]}, c.fo, 8)[0]
    check(d1, reference(rows8, c.fo), rows8, c.fo, "W = 8")


@pytest.mark.parametrize("f64", [False, True], ids=["scalar_f32", "scalar_f64"])
def test_finite_mfcc(capi, f64):
    """N = 1024 with the reference's 26 mel bands: every filter spans a bin, so every MFCC and mel band is finite and
    the bounds bite on them."""
    n, hop, feats = 1024, 256, ["mfcc", "melBands", "spectralCentroid"]
    samples, lens = corpus(n, hop, [1, 5, 260], 1024)
    starts, fo = capi.signals_frame_starts(lens, n, hop)
    plan = capi.Plan(buffer_size=n, scalar_f64=f64)
    try:
        rows = plan.extract_gather(samples, starts, feats)
        dev = call(capi, plan, samples, starts, fo, feats, (), feats, feats)
        host = call(capi, plan, samples, starts, fo, feats, (), feats, feats, host=True)
    finally:
        plan.close()
    assert all(np.isfinite(v).all() for v in rows.values())
    drows = delta_rows(capi, rows, fo)
    for got, r, what in ((dev[2], drows[0], "delta"), (dev[3], drows[1], "delta2")):
        check(got, reference(r, fo), r, fo, what)
        assert all(np.isfinite(v).all() for v in got.values())
        assert all((v[0] == 0).all() for v in got.values())  # the one-buffer signal
    for d, h, what in zip(dev, host, ("base", "rows", "delta", "delta2")):
        same_bits(h, d, (what, "host against device"))


def test_no_buffers_and_no_signals(capi, corner):
    c = corner
    none = np.empty(0, np.uint64)
    for host in (False, True):
        summ, _, d1, d2 = call(capi, c.plan, c.samples, none, np.array([0, 0, 0], np.uint64), ["rms"], (), ["mfcc"], ["mfcc"], host=host)
        assert np.isnan(summ["rms"]).all() and np.isnan(d1["mfcc"]).all() and np.isnan(d2["mfcc"]).all()
        assert d1["mfcc"].shape == (2, 4, 13)
        # no signal: the gather call
        _, rows, _, _ = call(capi, c.plan, c.samples, c.starts, np.array([0], np.uint64), ["rms"], ["mfcc"], ["mfcc"], ["mfcc"], host=host)
        same_bits(rows, {"mfcc": c.rows["mfcc"]}, "no signal")


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


@pytest.mark.parametrize("width", [2, 8])
def test_host_chunks_straddle_signals(capi, straddle, width):
    plan, samples, starts, fo = straddle
    feats = ["rms", "mfcc"]
    dev = call(capi, plan, samples, starts, fo, feats, (), feats, feats, width=width)
    host = call(capi, plan, samples, starts, fo, feats, (), feats, feats, width=width, host=True)
    for d, h, what in zip(dev, host, ("base", "rows", "delta", "delta2")):
        same_bits(h, d, (what, "host against device"))
    assert np.isfinite(dev[2]["rms"]).all() and np.isfinite(dev[3]["rms"]).all()


def test_non_finite_values_stay_in_their_signal(capi):
    """Two silent buffers in the middle signal of three: their melBands are -Infinity, so the delta rows around them
    are -Infinity before and +Infinity after (no NaN: no sum subtracts two infinities of one sign), and the
    second-order rows hold a NaN (the delta rows 11 and 13 are both +Infinity). By the summaries' rules the delta
    summary of that signal is then NaN in mean and variance with min -Infinity and max +Infinity, and the
    second-order summary NaN in all four; the neighbours' are finite."""
    n, hop = 256, 64
    samples, lens = corpus(n, hop, [40, 40, 40], 5)
    z0 = lens[0] + 10 * hop
    samples[z0:z0 + n + hop] = 0.0  # buffers 10 and 11 of the middle signal are silent
    starts, fo = capi.signals_frame_starts(lens, n, hop)
    plan = capi.Plan(buffer_size=n, num_mel_bands=40, scalar_f64=True)
    try:
        rows = plan.extract_gather(samples, starts, ["melBands"])
        _, _, d1, d2 = call(capi, plan, samples, starts, fo, [], (), ["melBands"], ["melBands"])
        _, _, h1, h2 = call(capi, plan, samples, starts, fo, [], (), ["melBands"], ["melBands"], host=True)
    finally:
        plan.close()
    # (at N = 256 the lowest of 40 mel filters span no bin: those bands are -Infinity in every buffer)
    live = np.isfinite(rows["melBands"][:40]).all(axis=0)
    assert live.sum() >= 30 and np.isneginf(rows["melBands"][50:52][:, live]).all()
    drows = delta_rows(capi, rows, fo)
    assert not np.isnan(drows[0]["melBands"][40:80][:, live]).any() and np.isnan(drows[1]["melBands"][52, live]).all()
    for got, r, what in ((d1, drows[0], "delta"), (d2, drows[1], "delta2")):
        check(got, reference(r, fo), r, fo, what)
        for s in (0, 2):
            assert np.isfinite(got["melBands"][s][:, live]).all(), (what, s)
    mid = d1["melBands"][1][:, live]
    assert np.isnan(mid[0]).all() and np.isnan(mid[1]).all() and np.isneginf(mid[2]).all() and np.isposinf(mid[3]).all()
    assert np.isnan(d2["melBands"][1][:, live]).all()
    same_bits(h1, d1, "host against device, delta")
    same_bits(h2, d2, "host against device, delta2")
