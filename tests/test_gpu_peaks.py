"""The peak picker (mgx_peaks_device, include/meyda_gpu.h) against the numpy statement of its definition
(tests/peaks_ref.py). Every output is an integer, and the definition fixes every rounding and the order of every
addition: mask, peak_offsets, peaks and peak_starts are compared for equality."""
import numpy as np
import pytest

import peaks_ref

pytestmark = pytest.mark.gpu

F = 301
PRE_MAX = 3
SENTINEL = 9          # in the mask: a row the operator did not write
UNWRITTEN = -5        # in peaks and peak_starts
# an empty signal, a one-row signal, a signal of exactly PRE_MAX rows, and a long one that begins (row 70) and ends
# (row 290) inside a 64-row word; rows before the first and after the last signal
TABLE = np.array([5, 5, 6, 6 + PRE_MAX, 70, 290], np.uint64)
PARAM_SETS = [(0, 0, 0, 0, 0.0, 0), (0, 0, 0, 0, 0.0, 1), (3, 0, 10, 10, 0.07, 3), (64, 64, 64, 64, 0.0, 2), (2, 2, 4, 4, -0.5, 0),
              (1, 1, 3, 3, float("inf"), 0), (1, 1, 3, 3, float("-inf"), 2)]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def envelope(n, dtype, seed, quantised=False):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 5, n).astype(np.float64) if quantised else np.abs(rng.standard_normal(n))
    return x.astype(dtype)


def run(capi, x, fo, ps, capacity=None, starts=None):
    """The operator's four outputs as numpy; mask rows, peaks and peak_starts it did not write hold the sentinels."""
    import torch
    xd = torch.from_numpy(x).cuda()
    cap = max(x.size, 1) if capacity is None else capacity
    st = None if starts is None else torch.from_numpy(np.asarray(starts, np.uint64).view(np.int64)).cuda()
    # (peaks_torch zero-fills its lists: the sentinels are laid by a call on tensors of the test's own)
    S = 1 if fo is None else len(fo) - 1
    mask = torch.full((x.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    offs = torch.full((S + 1,), UNWRITTEN, dtype=torch.int64, device="cuda")
    peaks = torch.full((cap + 3,), UNWRITTEN, dtype=torch.int64, device="cuda")
    pst = torch.full((cap + 3,), UNWRITTEN, dtype=torch.int64, device="cuda")
    tb = None if fo is None else torch.from_numpy(np.asarray(fo, np.uint64).view(np.int64)).cuda()
    o = outputs(capi, mask, offs, peaks, cap, st, pst)
    nbytes = capi.peaks_workspace_bytes(x.size, 0 if fo is None else S)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    capi.peaks_device(xd.data_ptr(), x.size, x.dtype == np.float64, None if tb is None else tb.data_ptr(), 0 if fo is None else S,
                      capi.peak_params(**dict(zip(peaks_ref.PARAMS, ps))), o, ws.data_ptr(), nbytes,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), offs.cpu().numpy(), peaks.cpu().numpy(), pst.cpu().numpy()


def outputs(capi, mask, offs, peaks, cap, st, pst):
    import ctypes
    o = capi.PeakOutputs()
    o.struct_size = ctypes.sizeof(capi.PeakOutputs)
    o.mask, o.peak_offsets, o.peaks, o.capacity = mask.data_ptr(), offs.data_ptr(), peaks.data_ptr(), cap
    if st is not None:
        o.starts, o.peak_starts = st.data_ptr(), pst.data_ptr()
    return o


def check(capi, x, fo, ps, what, capacity=None, starts=None):
    mask, offs, peaks, pst = run(capi, x, fo, ps, capacity, starts)
    wm, wo, wp = peaks_ref.peaks(x, fo, fill=SENTINEL, **dict(zip(peaks_ref.PARAMS, ps)))
    assert np.array_equal(mask, wm), (what, "mask", np.nonzero(mask != wm)[0][:8])
    assert np.array_equal(offs.view(np.uint64), wo), (what, "peak_offsets", offs, wo)
    n = min(wp.size, peaks.size - 3 if capacity is None else capacity)
    assert np.array_equal(peaks[:n].view(np.uint64), wp[:n]), (what, "peaks")
    assert (peaks[n:] == UNWRITTEN).all(), (what, "peaks beyond the written ones")
    if starts is not None:
        assert np.array_equal(pst[:n].view(np.uint64), np.asarray(starts, np.uint64)[wp[:n].astype(np.int64)]), (what, "peak_starts")
    assert (pst[n if starts is not None else 0:] == UNWRITTEN).all(), (what, "peak_starts beyond the written ones")
    return wm, wo, wp


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("ps", PARAM_SETS, ids=[str(p) for p in PARAM_SETS])
def test_operator_is_the_definition(capi, dtype, ps):
    x = envelope(F, dtype, 3)
    starts = np.arange(F, dtype=np.uint64) * 64 + 17
    wm, wo, wp = check(capi, x, TABLE, ps, ps, starts=starts)
    assert (wm[:5] == SENTINEL).all() and (wm[290:] == SENTINEL).all() and (wm[5:290] != SENTINEL).all()
    if ps[:5] == (0, 0, 0, 0, 0.0):
        # every row of a signal is a candidate; with wait 1 every other one of each signal is a peak
        assert wp.size == (285 if ps[5] == 0 else 1 + 2 + 31 + 110)
    if ps[4] == float("inf"):
        assert wp.size == 0


def test_reaches_of_64_on_a_short_signal(capi):
    x = envelope(F, np.float32, 4)
    fo = np.array([100, 120, 130], np.uint64)  # 20 rows, then 10: every window leaves the signal on both sides
    wm, wo, wp = check(capi, x, fo, (64, 64, 64, 64, 0.0, 0), "reach 64")
    assert wo.tolist() == [0, 1, 2]  # the maximum of each signal, and it is above the mean
    check(capi, x, fo, (64, 0, 0, 64, -1.0, 1), "reach 64, one side")


@pytest.mark.parametrize("wait", [0, 1, 63, 64, 65, 1000])
def test_wait_across_words(capi, wait):
    """A quantised envelope: plateaus that cross word boundaries, ties inside the windows."""
    x = envelope(F, np.float32, 5, quantised=True)
    for ps in ((0, 0, 0, 0, 0.0, wait), (1, 1, 2, 2, 0.0, wait)):
        wm, wo, wp = check(capi, x, TABLE, ps, ps)
        check(capi, x, None, ps, (ps, "one signal"))
    if wait == 1000:
        assert wo.tolist() == [0, 0, 1, 2, 3, 4]  # one peak per signal that has rows


def test_nan_and_infinity(capi):
    x = envelope(F, np.float64, 6)
    x[[7, 100, 101, 200]] = np.nan
    x[[80, 150]] = np.inf
    x[[90, 151, 289]] = -np.inf
    x[69] = np.nan  # the last row of the signal before the long one: no row of the long one sees it
    fo = np.array([5, 70, 290], np.uint64)
    for ps in ((1, 1, 0, 0, 0.0, 0), (0, 0, 5, 5, -10.0, 0), (2, 2, 5, 5, 0.0, 3)):
        wm, wo, wp = check(capi, x, fo, ps, ps)
        assert (wm[[7, 69, 100, 101, 200]] == 0).all()
    # a NaN inside the averaging window rejects the row, in its own signal alone
    wm, _, _ = check(capi, x, fo, (0, 0, 5, 5, -10.0, 0), "averaging window")
    assert (wm[64:70] == 0).all() and (wm[70:75] == 1).all() and (wm[95:107] == 0).all() and wm[94] == 1 and wm[107] == 1


def test_capacity_below_the_total(capi):
    x = envelope(F, np.float32, 7)
    starts = np.arange(F, dtype=np.uint64)[::-1].copy()
    ps = (1, 1, 0, 0, 0.0, 0)
    total = int(peaks_ref.peaks(x, TABLE, **dict(zip(peaks_ref.PARAMS, ps)))[1][-1])
    assert total > 40
    for cap in (1, 40, total - 1, total, total + 1):
        check(capi, x, TABLE, ps, ("capacity", cap), capacity=cap, starts=starts)


def test_null_table_and_its_spelling(capi):
    x = envelope(F, np.float32, 8)
    for ps in PARAM_SETS[:4]:
        a = check(capi, x, None, ps, (ps, "NULL table"))
        b = check(capi, x, np.array([0, F], np.uint64), ps, (ps, "[0, F]"))
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_entries_above_the_rows(capi):
    x = envelope(F, np.float32, 9)
    for fo in ([0, 100, F + 1, 2 ** 40], [F, F + 5], [2 ** 63, 2 ** 64 - 1], [0, 0, 2 ** 64 - 1]):
        check(capi, x, np.array(fo, np.uint64), (3, 0, 10, 10, 0.07, 3), fo)


def test_a_table_that_is_not_non_decreasing(capi):
    """Unspecified values, but the call returns and nothing outside the arrays is written."""
    x = envelope(F, np.float32, 10)
    for fo in ([200, 100, 300, 50, 250], [F, 0, F, 0], [2 ** 64 - 1, 0, 17]):
        for ps in ((3, 0, 10, 10, 0.07, 3), (0, 0, 0, 0, 0.0, 0)):
            mask, offs, peaks, pst = run(capi, x, np.array(fo, np.uint64), ps, capacity=20)
            assert mask.size == F and (peaks[20:] == UNWRITTEN).all() and (pst == UNWRITTEN).all()
            assert ((peaks[:20] == UNWRITTEN) | ((peaks[:20] >= 0) & (peaks[:20] < F))).all()


@pytest.fixture(scope="module")
def long_envelope():
    return envelope(70000, np.float32, 11, quantised=True) + envelope(70000, np.float32, 12) * np.float32(0.25)


@pytest.mark.parametrize("shape", ["one signal", "2000 signals"])
def test_several_tiles_steps_and_scan_blocks(capi, long_envelope, shape):
    """70,000 rows: 274 tiles, 1,094 words (18 steps of 64 for one signal's wave), two scan blocks, the second of
    which begins inside a signal in both shapes (row 65,536 = 35 x 1872 + 16)."""
    x = long_envelope
    fo = np.array([0, 70000], np.uint64) if shape == "one signal" else np.arange(2001, dtype=np.uint64) * 35
    starts = (np.arange(70000, dtype=np.uint64) * 7) % 65521
    for ps in ((3, 0, 10, 10, 0.07, 3), (0, 0, 0, 0, 0.0, 1), (1, 1, 0, 0, 0.0, 100)):
        wm, wo, wp = check(capi, x, fo, ps, (shape, ps), starts=starts)
        assert wp.size > 64


def test_repeated_call_and_graph_replay(capi, long_envelope):
    import torch
    x = long_envelope[:5000]
    fo = np.array([3, 3, 1000, 1001, 4990], np.uint64)
    ps = dict(pre_max=3, post_max=0, pre_avg=10, post_avg=10, delta=0.07, wait=3)
    xd = torch.from_numpy(x).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    st = torch.arange(5000, dtype=torch.int64, device="cuda") * 3
    first = [t.cpu().numpy() for t in capi.peaks_torch(xd, tb, starts=st, mask_fill=SENTINEL, **ps)]
    again = [t.cpu().numpy() for t in capi.peaks_torch(xd, tb, starts=st, mask_fill=SENTINEL, **ps)]
    wm, wo, wp = peaks_ref.peaks(x, fo, fill=SENTINEL, **ps)
    for got in (first, again):
        assert np.array_equal(got[0], wm) and np.array_equal(got[1].view(np.uint64), wo)
        assert np.array_equal(got[2][:wp.size].view(np.uint64), wp) and (got[2][wp.size:] == 0).all()
        assert np.array_equal(got[3][:wp.size].view(np.uint64), wp * np.uint64(3))
    # a graph replay, on tensors (the workspace among them) that outlive the capture
    s = torch.cuda.Stream()
    mask = torch.full((5000,), SENTINEL, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(5, dtype=torch.int64, device="cuda")
    peaks = torch.zeros(5000, dtype=torch.int64, device="cuda")
    pst = torch.zeros(5000, dtype=torch.int64, device="cuda")
    nbytes = capi.peaks_workspace_bytes(5000, 4)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    o = outputs(capi, mask, offs, peaks, 5000, st, pst)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        capi.peaks_device(xd.data_ptr(), 5000, False, tb.data_ptr(), 4, capi.peak_params(**ps), o, ws.data_ptr(), nbytes, s.cuda_stream)
    torch.cuda.synchronize()
    for t, v in ((mask, SENTINEL), (offs, 0), (peaks, 0), (pst, 0), (ws, 0xFF)):
        t.fill_(v)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip((mask, offs, peaks, pst), first):
        assert np.array_equal(got.cpu().numpy(), want)


def test_no_rows(capi):
    import torch
    xd = torch.empty(0, dtype=torch.float32, device="cuda")
    tb = torch.zeros(4, dtype=torch.int64, device="cuda")
    offs = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    o = outputs(capi, torch.empty(0, dtype=torch.uint8, device="cuda"), offs, torch.full((2,), 7, dtype=torch.int64, device="cuda"), 2,
                None, None)
    capi.peaks_device(None, 0, False, tb.data_ptr(), 3, capi.peak_params(), o, None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert offs.tolist() == [0, 0, 0, 0]
