"""The beat tracker on the device (mgx_beats_device, include/meyda_gpu.h) against the numpy statement
(tests/beat_ref.py): the local and the cumulative score bit for bit on the rows a signal owns, the fill elsewhere, and
mask, peak_offsets, peaks and peak_starts equal. The tables on both sides are the library's (tests/test_beats_host.py
compares those with the statement's)."""
import numpy as np
import pytest

import beat_ref
from test_gpu_summary import same_bits
from test_gpu_tempo import RATE, clicks

pytestmark = pytest.mark.gpu

# click trains over noise, (rows, period), seeds 100 + i as in tests/test_gpu_tempo.py; an empty clip, clips of two rows
# and of one
CLIPS = [(1500, 86), (900, 60), (0, 0), (1000, 43), (50, 20), (300, 7), (130, 5), (65, 3), (40, 2), (9, 1), (2, 1), (1, 1)]
P = 128
FILL = -7.25  # the scores' fill: rows of no signal keep it


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


@pytest.fixture(scope="module")
def big(capi):
    """The tables of the largest period, made once."""
    return capi.beat_tables(beat_ref.MAX_PERIOD)


def device(capi, x, period, tables, fo, max_period, **kw):
    """capi.beats_torch on host arrays, as numpy."""
    import torch
    res = capi.beats_torch(torch.from_numpy(x).cuda(), np.asarray(period, np.uint32), tables[0], tables[1], fo, max_period=max_period,
                           scores=True, score_fill=FILL, mask_fill=9, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def agree(got, ref, what):
    """Scores bit for bit (fill included), mask, counts and rows equal."""
    same_bits({k: got[k] for k in ("local_score", "cum_score")}, {k: ref[k] for k in ("local_score", "cum_score")}, what)
    assert np.array_equal(got["mask"], ref["mask"]), what
    assert np.array_equal(got["peak_offsets"].astype(np.uint64), ref["peak_offsets"]), (what, got["peak_offsets"], ref["peak_offsets"])
    total = int(ref["peak_offsets"][-1])
    cap = min(total, got["peaks"].size)
    assert np.array_equal(got["peaks"][:cap].astype(np.uint64), ref["peaks"][:cap]), what


def reference(x, period, tables, fo, max_period, trim=1):
    return beat_ref.beats_ref(x, period, fo, max_period, tables[0], tables[1], trim, fill=FILL, mask_fill=9)


class Trains:
    def __init__(self, capi):
        extra = [clicks(100, 10, 200), clicks(100, 10, 201), np.zeros(100, np.float32), clicks(200, 10, 202)]
        extra[3][50] = np.nan
        parts = [clicks(r, per, 100 + i) for i, (r, per) in enumerate(CLIPS)] + extra
        self.x = np.concatenate([np.zeros(3, np.float32)] + parts + [np.ones(2, np.float32)])
        self.fo = (3 + np.concatenate([[0], np.cumsum([v.size for v in parts])])).astype(np.uint64)
        # a clip with p = 0, one with p > P, a silent one, one with a NaN row
        self.period = np.array([per for _, per in CLIPS] + [0, P + 1, 10, 10], np.uint32)
        self.tables = capi.beat_tables(P)
        self.ref = reference(self.x, self.period, self.tables, self.fo, P)
        self.got = device(capi, self.x, self.period, self.tables, self.fo, P)


@pytest.fixture(scope="module")
def t(capi):
    return Trains(capi)


def test_scores_and_outputs_are_the_statement_s(t):
    agree(t.got, t.ref, "the trains")
    F = t.x.size
    assert (t.got["mask"][:3] == 9).all() and (t.got["mask"][F - 2:] == 9).all()
    assert (t.got["local_score"][:3] == FILL).all() and (t.got["cum_score"][F - 2:] == FILL).all()


def test_beats_lie_on_the_clicks(t):
    off = t.got["peak_offsets"]
    for s in (0, 1, 3, 5, 6, 7, 8, 9):
        rows, per = CLIPS[s]
        a = int(t.fo[s])
        assert np.array_equal(t.got["peaks"][off[s]:off[s + 1]], a + np.arange(per // 2, rows, per)), s
    assert off[1] - off[0] == 17 and off[2] - off[1] == 15 and off[4] - off[3] == 23
    n = len(CLIPS)
    # the empty clip, the one-row clip, p = 0, p > P, silence, a NaN row: no beats
    for s in (2, 11, n, n + 1, n + 2, n + 3):
        assert off[s + 1] == off[s], s


def test_the_double_period_and_no_trim(t, capi):
    per = t.period.copy()
    per[3] = 86
    agree(device(capi, t.x, per, t.tables, t.fo, P), reference(t.x, per, t.tables, t.fo, P), "p = 86 on the 43-row train")
    got = device(capi, t.x, t.period, t.tables, t.fo, P, trim=False)
    agree(got, reference(t.x, t.period, t.tables, t.fo, P, trim=0), "trim 0")
    off = got["peak_offsets"]
    assert off[1] - off[0] == 18 and off[4] - off[3] == 24


def test_a_tie_takes_the_larger_distance(t, capi):
    from test_beats_host import tie_case
    z, gauss, penalty = tie_case(t.tables)
    got = device(capi, z, [4], (gauss, penalty), None, P)
    agree(got, reference(z, [4], (gauss, penalty), None, P), "ties")
    rows = got["peaks"][:got["peak_offsets"][1]]
    assert list(rows[(rows >= 46) & (rows < 74)]) == [50, 58, 66]


def test_float64_envelope(t, capi):
    x64 = t.x.astype(np.float64) * (1 + 2.0 ** -40)
    agree(device(capi, x64, t.period, t.tables, t.fo, P), reference(x64, t.period, t.tables, t.fo, P), "float64")


def test_sizes_across_the_kernels_edges(capi, big):
    """n = 63, 64, 65, 129 for the partials; n around 2 p and at 4 p + 1 for the ring of a small period; the largest
    period over a ring that wraps twice; clips that lie across the local score's tiles of 256 rows."""
    shapes = [(63, 5), (64, 5), (65, 5), (129, 5), (31, 16), (32, 16), (33, 16), (65, 16), (4100, 1023), (2047, 1023), (700, 300),
              (2600, 512), (3, 2)]
    parts = [clicks(n, p, 300 + i) for i, (n, p) in enumerate(shapes)]
    x = np.concatenate(parts)
    fo = np.concatenate([[0], np.cumsum([v.size for v in parts])]).astype(np.uint64)
    period = np.array([p for _, p in shapes], np.uint32)
    assert any(fo[i] // 256 != (fo[i + 1] - 1) // 256 for i in range(len(shapes)))
    got = device(capi, x, period, big, fo, 1023)
    ref = reference(x, period, big, fo, 1023)
    agree(got, ref, "edges")
    assert ref["peak_offsets"][9] > ref["peak_offsets"][8]  # p = 1023 on 4,100 rows has beats


def test_one_signal_without_a_table(t, capi):
    x = t.x[3:1503]
    one = device(capi, x, [86], t.tables, None, P)
    assert one["peak_offsets"].shape == (2,) and one["peak_offsets"][1] == 17
    agree(one, reference(x, [86], t.tables, None, P), "no table")
    tab = device(capi, x, [86], t.tables, np.array([0, 1500], np.uint64), P)
    assert all(np.array_equal(one[k], tab[k]) for k in one)


def test_capacity_and_starts(t, capi):
    total = int(t.ref["peak_offsets"][-1])
    starts = (np.arange(t.x.size, dtype=np.uint64) * 7 + 5)
    got = device(capi, t.x, t.period, t.tables, t.fo, P, capacity=10, starts=starts)
    assert total > 10 and got["peaks"].shape == (10,)
    agree(got, t.ref, "capacity 10")
    assert np.array_equal(got["peak_starts"].astype(np.uint64), starts[t.ref["peaks"][:10].astype(np.int64)])
    full = device(capi, t.x, t.period, t.tables, t.fo, P, starts=starts)
    assert np.array_equal(full["peak_starts"][:total].astype(np.uint64), starts[t.ref["peaks"].astype(np.int64)])
    assert (full["peaks"][total:] == 0).all() and (full["peak_starts"][total:] == 0).all()


def test_repeat_and_graph_replay(t, capi):
    import torch
    x = torch.from_numpy(t.x).cuda()
    per = torch.from_numpy(t.period.view(np.int32)).cuda()
    g_, p_ = (torch.from_numpy(v).cuda() for v in t.tables)
    fo = torch.from_numpy(t.fo.view(np.int64)).cuda()
    ws = torch.empty(capi.beats_workspace_bytes(t.x.size, len(t.fo) - 1), dtype=torch.uint8, device="cuda")
    again = device(capi, t.x, t.period, t.tables, t.fo, P)
    assert all(np.array_equal(again[k].view(np.uint8), t.got[k].view(np.uint8)) for k in t.got)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = capi.beats_torch(x, per, g_, p_, fo, max_period=P, scores=True, stream=s.cuda_stream, workspace=ws)
    torch.cuda.synchronize()
    F = t.x.size
    own = slice(3, F - 2)
    # (the tensors beats_torch makes are filled inside the capture: a replay fills them again, then runs the call)
    for _ in range(2):
        for v in res.values():
            v.fill_(7)
        ws.fill_(0xAB)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in res.items()}
        total = int(t.ref["peak_offsets"][-1])
        assert np.array_equal(out["peak_offsets"].astype(np.uint64), t.ref["peak_offsets"])
        assert np.array_equal(out["peaks"][:total].astype(np.uint64), t.ref["peaks"]) and (out["peaks"][total:] == 0).all()
        assert np.array_equal(out["mask"][own], t.ref["mask"][own]) and (out["mask"][:3] == 0).all()
        for k in ("local_score", "cum_score"):
            assert np.array_equal(out[k][own].view(np.uint64), t.ref[k][own].view(np.uint64)), k
            assert (out[k][:3] == 0.0).all() and (out[k][F - 2:] == 0.0).all()


def test_period_straight_from_the_tempo_call(capi, big):
    """envelope -> capi.tempo_torch -> its "lag" tensor, as it lies on the device, is the tracker's period."""
    import torch
    W = 384
    parts = [clicks(1500, 86, 100), clicks(900, 60, 101), np.zeros(0, np.float32), clicks(1000, 43, 103)]
    x = np.concatenate(parts)
    fo = np.concatenate([[0], np.cumsum([v.size for v in parts])]).astype(np.uint64)
    xd = torch.from_numpy(x).cuda()
    fod = torch.from_numpy(fo.view(np.int64)).cuda()
    tempo = capi.tempo_torch(xd, torch.from_numpy(capi.tempogram_window(W)).cuda(), torch.from_numpy(capi.tempo_prior(RATE, W)).cuda(), fod)
    lag = tempo["lag"]
    assert lag.is_cuda and lag.dtype == torch.int32
    res = capi.beats_torch(xd, lag, big[0], big[1], fod, scores=True, score_fill=FILL, mask_fill=9)
    torch.cuda.synchronize()
    lags = lag.cpu().numpy()
    assert list(lags) == [86, 60, 0, 86]
    agree({k: v.cpu().numpy() for k, v in res.items()}, reference(x, lags.astype(np.uint32), big, fo, 1023), "chained")
    off = res["peak_offsets"].cpu().numpy()
    assert list(np.diff(off)) == [17, 15, 0, 11]
