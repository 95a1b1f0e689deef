"""Tempogram -> per-clip pooling -> pick on the device (mgx_tempo_device, include/meyda_gpu.h). The tempogram rows
equal the numpy statement (tests/tempo_ref.py) bit for bit; the pooled rows are within the summaries' own stated
bounds of numpy on those rows (tests/test_gpu_summary.py); the lag equals the statement's pick applied to the returned
mean row, exactly; and the route without a tempogram output, which passes the rows through the workspace 65,536 at a
time, gives the bits of the route with one."""
import numpy as np
import pytest

import tempo_ref
from test_gpu_summary import check, reference, same_bits

pytestmark = pytest.mark.gpu

RATE = 44100.0 / 256  # rows a second at hop 256: 172.27
W = L = 384
# click trains over noise: (rows, period); the lag the definition finds on the CPU is the period, or at 43 rows
# (240 bpm) its double, which the prior around 120 bpm prefers. An empty clip and one shorter than the window.
CLIPS = [(1500, 86), (900, 60), (0, 0), (1100, 103), (1000, 43), (50, 20)]
EXPECTED = [86, 60, 0, 103, 86]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def clicks(rows, period, seed, level=0.1):
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal(rows)) * level).astype(np.float32)
    if period:
        x[period // 2::period] += 1.0
    return x


def device(capi, x, h, p, fo, **kw):
    """capi.tempo_torch on host arrays, as numpy."""
    import torch
    res = capi.tempo_torch(torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda(), None if p is None else torch.from_numpy(p).cuda(),
                           fo, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


class Trains:
    def __init__(self, capi):
        self.x = np.concatenate([np.zeros(3, np.float32)] + [clicks(r, per, 100 + i) for i, (r, per) in enumerate(CLIPS)] +
                                [np.ones(2, np.float32)])
        self.fo = (3 + np.concatenate([[0], np.cumsum([r for r, _ in CLIPS])])).astype(np.uint64)
        self.h = capi.tempogram_window(W)
        self.p = capi.tempo_prior(RATE, L)
        self.rows = tempo_ref.tempogram_ref(self.x, self.h, L, tempo_ref.NORM_LAG0, self.fo)
        self.kept = device(capi, self.x, self.h, self.p, self.fo, tempogram=True)
        self.passed = device(capi, self.x, self.h, self.p, self.fo)


@pytest.fixture(scope="module")
def t(capi):
    return Trains(capi)


def test_rows_are_the_statement_s(t):
    same_bits({"t": t.kept["tempogram"]}, {"t": t.rows}, "tempogram")  # (rows of no clip: zero on both sides)


def test_click_trains(t):
    lag = t.kept["lag"]
    assert lag.dtype == np.int32 and list(lag[:5]) == EXPECTED, lag
    bpm = 60.0 * RATE / 86
    assert abs(bpm - 120.19) < 0.005


def test_lag_is_the_pick_of_the_returned_mean(t):
    mean = t.kept["summary"][:, 0, :]
    assert np.array_equal(t.kept["lag"].astype(np.uint32), tempo_ref.pick_ref(mean, t.p))
    assert [tempo_ref.pick_loop(m, t.p) for m in mean] == list(t.kept["lag"])


def test_summary_is_within_the_summaries_bounds(t):
    rows = {"t": t.rows}
    check({"t": t.kept["summary"]}, reference(rows, t.fo), rows, t.fo, "tempogram rows")
    assert np.isnan(t.kept["summary"][2]).all() and t.kept["lag"][2] == 0  # the empty clip: NaN in all four, no tempo
    assert (t.kept["summary"][[0, 1, 3, 4, 5], 0, 0] == 1.0).all()  # lag 0 of every normalised row is exactly 1


def test_both_routes_give_the_same_bits(t):
    assert set(t.passed) == {"summary", "lag"}
    same_bits(t.passed, {k: t.kept[k] for k in t.passed}, "with and without the tempogram output")


def test_outputs_are_optional(t, capi):
    only = device(capi, t.x, t.h, None, t.fo)
    same_bits(only, {"summary": t.kept["summary"]}, "summary alone")
    only = device(capi, t.x, t.h, t.p, t.fo, summary=False)
    same_bits(only, {"lag": t.kept["lag"]}, "lag alone")
    only = device(capi, t.x, t.h, None, t.fo, summary=False, tempogram=True)
    same_bits(only, {"tempogram": t.kept["tempogram"]}, "tempogram alone")
    with pytest.raises(capi.MgxError):
        device(capi, t.x, t.h, None, t.fo, summary=False)


def test_one_signal_without_a_table(t, capi):
    x = t.x[3:1503]
    one = device(capi, x, t.h, t.p, None, tempogram=True)
    assert one["lag"].shape == (1,) and one["summary"].shape == (1, 4, L) and one["lag"][0] == 86
    tab = device(capi, x, t.h, t.p, np.array([0, 1500], np.uint64), tempogram=True)
    same_bits(one, tab, "no table is one signal")


def test_across_the_pass_of_rows(capi):
    """F = 70,000 at W = L = 8: the route through the workspace takes two passes, and a clip and a block of the
    summaries lie across their border."""
    F, w = 70000, 8
    rng = np.random.default_rng(5)
    x = (np.abs(rng.standard_normal(F)) * 2.0 ** rng.integers(-8, 9, F)).astype(np.float32)
    x[3::5] += 50.0
    fo = np.array([0, 20000, 20000, 65000, 65537, 69990], np.uint64)
    assert (65536 - 20000) % 256 != 0 and fo[3] < capi.TEMPO_CHUNK_ROWS < fo[4]
    h, p = capi.tempogram_window(w), capi.tempo_prior(10.0, w)
    kept = device(capi, x, h, p, fo, tempogram=True)
    passed = device(capi, x, h, p, fo)
    same_bits(passed, {k: kept[k] for k in passed}, "two passes")
    rows = tempo_ref.tempogram_ref(x, h, w, tempo_ref.NORM_LAG0, fo)
    same_bits({"t": kept["tempogram"]}, {"t": rows}, "tempogram")
    check({"t": kept["summary"]}, reference({"t": rows}, fo), {"t": rows}, fo, "70,000 rows")
    assert np.array_equal(kept["lag"].astype(np.uint32), tempo_ref.pick_ref(kept["summary"][:, 0, :], p))
    assert kept["lag"][1] == 0 and (kept["lag"][[0, 2, 3, 4]] > 0).all()
    # the unnormalised rows and a float64 envelope take the same two routes
    x64 = x.astype(np.float64) * (1 + 2.0 ** -40)
    a, b = device(capi, x64, h, p, fo, norm="none", tempogram=True), device(capi, x64, h, p, fo, norm="none")
    same_bits(b, {k: a[k] for k in b}, "two passes, float64, norm none")
    same_bits({"t": a["tempogram"]}, {"t": tempo_ref.tempogram_ref(x64, h, w, tempo_ref.NORM_NONE, fo)}, "float64 tempogram")


def test_repeat_and_graph_replay(t, capi):
    import torch
    x, h, p = (torch.from_numpy(v).cuda() for v in (t.x, t.h, t.p))
    fo = torch.from_numpy(t.fo.view(np.int64)).cuda()
    ws = torch.empty(capi.tempo_workspace_bytes(t.x.size, len(t.fo) - 1, capi.tempo_params(W, L), False), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = capi.tempo_torch(x, h, p, fo, stream=s.cuda_stream, workspace=ws)
    torch.cuda.synchronize()
    for _ in range(2):
        res["summary"].fill_(7.0)
        res["lag"].fill_(7)
        ws.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same_bits({k: v.cpu().numpy() for k, v in res.items()}, t.passed, "graph replay")
