"""The tempogram operator (mgx_tempogram_device, include/meyda_gpu.h) against the numpy statement of its definition
(tests/tempo_ref.py): equality of bits, both norms. The definition fixes every rounding and the order of every
addition, and the division is the correctly rounded float64 one. The reference sums of a case are computed once and
shared by both norms."""
import numpy as np
import pytest

import tempo_ref

pytestmark = pytest.mark.gpu

F = 301
# K = 1 .. 16 lags a lane, W below, at and above a multiple of 64 and of K, L < W, the largest window
SHAPES = [(2, 1), (2, 2), (8, 8), (64, 64), (65, 65), (129, 64), (384, 384), (384, 100), (1000, 513), (1024, 1024)]
# rows 0..4 and 290..300 belong to no clip; an empty clip, a one-row clip, a three-row clip (shorter than W / 2 from
# W = 8 on), then 31, 100 and 150 rows
TABLE = np.array([5, 5, 6, 9, 40, 140, 290], np.uint64)
SENTINEL = 777.0
NORMS = {"none": tempo_ref.NORM_NONE, "lag0": tempo_ref.NORM_LAG0}


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def make_envelope(seed, rows=F):
    """|normal| scaled over +-20 binary orders row by row; a silent stretch of 135 rows (longer than W up to 129: the
    whole fifth clip and the start of the last; F = 301 has no room for one longer than 384), float32 denormals, a
    NaN and a +Infinity in the last clip, so that the clips before it stay finite."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal(rows)) * 2.0 ** rng.integers(-20, 21, rows)).astype(np.float32)
    if rows >= F:
        x[40:175] = 0.0
        x[12:18] = np.float32(1e-42)
        x[20] = np.float32(3e-45)
        x[200] = np.nan
        x[250] = np.inf
    return x


def make_window(W, seed):
    """The library's window with its first tap moved off 0 and one tap negative: a caller's window may be signed."""
    rng = np.random.default_rng(seed)
    h = tempo_ref.window_ref(W)
    h[0] = np.float32(0.125)
    h[W - 1] = -h[W - 1] - np.float32(0.03125)
    return (h * (1 + rng.random(W) * 2.0 ** -12)).astype(np.float32)


def run(capi, x, h, L, norm, table=None, extra=3):
    """The operator's rows over a sentinel-filled array, and the `extra` sentinel rows behind them left intact."""
    import torch
    xd = torch.from_numpy(x).cuda()
    hd = torch.from_numpy(h).cuda()
    buf = torch.full((x.shape[0] + extra, L), SENTINEL, dtype=torch.float32, device="cuda")
    capi.tempogram_torch(xd, hd, table, L, norm, out=buf[:x.shape[0]])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[x.shape[0]:] == SENTINEL).all(), "the rows after the last output row were written"
    return got[:x.shape[0]]


def same(got, want, what):
    """Equal bits; a NaN for a NaN (its payload is not part of the definition)."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.argwhere(np.isnan(got) != nan)[:4])
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (what, len(bad), bad[:4], [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


_sums = {}


def reference(key, x, h, L, table):
    """The sums of a case, computed once: both norms and every test of the case share them."""
    if key not in _sums:
        _sums[key] = tempo_ref.sums_ref(x, h, L, table)
    S, owned = _sums[key]
    return {name: tempo_ref.finish_ref(S, owned, norm, SENTINEL) for name, norm in NORMS.items()}


@pytest.mark.parametrize("W,L", SHAPES)
def test_one_signal(capi, W, L):
    x, h = make_envelope(W + L), make_window(W, W)
    want = reference(("one", W, L), x, h, L, None)
    for norm in NORMS:
        got = run(capi, x, h, L, norm)
        same(got, want[norm], (W, L, norm))
        # the NaN and the Infinity reach the rows whose window holds them and no other row
        reach = np.zeros(F, bool)
        for at in (200, 250):
            reach[max(at - (W - 1 - W // 2), 0):at + W // 2 + 1] = True
        assert np.isfinite(got[~reach]).all() and not np.isfinite(got[reach, 0]).any()
    if W <= 129:  # a silent window stays +0 under both norms
        assert all((want[norm][107] == 0).all() and not np.signbit(want[norm][107]).any() for norm in NORMS)
    fin = np.isfinite(want["none"][:, 0]) & (want["none"][:, 0] > 0)
    assert (want["lag0"][fin, 0] == 1.0).all()
    assert W > 129 or fin.sum() > 50  # (at the larger windows most rows of this one signal hold the NaN: the clips' turn)


@pytest.mark.parametrize("W,L", SHAPES)
def test_table_of_clips(capi, W, L):
    x, h = make_envelope(2 * W + L), make_window(W, W + 1)
    want = reference(("table", W, L), x, h, L, TABLE)
    for norm in NORMS:
        got = run(capi, x, h, L, norm, TABLE)
        same(got, want[norm], (W, L, norm))
        assert (got[:5] == SENTINEL).all() and (got[290:] == SENTINEL).all()  # rows of no clip are not written
        assert np.isfinite(got[5:140]).all()  # the last clip's NaN and Infinity stay in their own clip
        assert (got[40:140] == 0).all() and not np.signbit(got[40:140]).any()  # a silent clip stays +0
        assert not np.isfinite(got[200, 0]) and not np.isfinite(got[250, 0])


@pytest.mark.parametrize("W,L", [(8, 8), (129, 64), (384, 384)])
def test_float64_envelope(capi, W, L):
    """Values are taken as float64: an envelope that no float32 array holds."""
    x = make_envelope(3 * W).astype(np.float64) * (1.0 + 2.0 ** -30)
    h = make_window(W, W + 2)
    want = reference(("f64", W, L), x, h, L, TABLE)
    for norm in NORMS:
        same(run(capi, x, h, L, norm, TABLE), want[norm], ("float64", W, L, norm))
    rounded = reference(("f64 rounded", W, L), x.astype(np.float32), h, L, TABLE)
    assert not np.array_equal(want["none"][9:140], rounded["none"][9:140])


def test_non_monotone_table(capi):
    """A table that is no table: entries are limited to num_frames, no access leaves the arrays (the sentinel rows
    behind the output stay); the values are unspecified."""
    x, h = make_envelope(1), make_window(64, 1)
    for table in ([50, 20, 1301, 10, 2 ** 63, 100], [2 ** 64 - 1, 0, 301], [301, 0], [400, 500, 600]):
        run(capi, x, h, 64, "lag0", np.array(table, np.uint64))
    # a table of no signals writes nothing
    got = run(capi, x, h, 64, "lag0", np.array([0], np.uint64))
    assert (got == SENTINEL).all()


def test_many_rows_and_row_counts(capi):
    """More rows than one pass of the grid's waves, and row counts around a workgroup's four."""
    h = make_window(8, 3)
    x = make_envelope(4, rows=70001)
    table = np.array([0, 1, 30000, 30000, 65536, 70001], np.uint64)
    same(run(capi, x, h, 8, "lag0", table), tempo_ref.tempogram_ref(x, h, 8, tempo_ref.NORM_LAG0, table, SENTINEL), "70001 rows")
    h = make_window(129, 4)
    for rows in (1, 2, 3, 4, 5, 9):
        same(run(capi, x[:rows], h, 65, "none"), tempo_ref.tempogram_ref(x[:rows], h, 65, tempo_ref.NORM_NONE), rows)


def test_repeat_and_graph_replay(capi):
    import torch
    W = L = 384
    x, h = make_envelope(2 * W + L), make_window(W, W + 1)
    want = reference(("table", W, L), x, h, L, TABLE)["lag0"]
    same(run(capi, x, h, L, "lag0", TABLE), want, "first")
    same(run(capi, x, h, L, "lag0", TABLE), want, "repeated")
    s = torch.cuda.Stream()
    xd, hd = torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda()
    td = torch.from_numpy(TABLE.view(np.int64)).cuda()
    out = torch.full((F, L), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        capi.tempogram_torch(xd, hd, td, L, "lag0", stream=s.cuda_stream, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "graph replay")


def test_no_rows_and_a_refusal_launch_nothing(capi):
    import torch
    x = torch.ones(4, dtype=torch.float32, device="cuda")
    h = torch.ones(8, dtype=torch.float32, device="cuda")
    out = torch.full((4, 8), SENTINEL, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.MgxError):
        capi.tempogram_torch(x, h, None, 9, "lag0", out=torch.full((4, 9), SENTINEL, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        capi.tempogram_torch(x, h, None, 8, "max", out=out)
    capi.tempogram_device(x.data_ptr(), 0, False, None, 0, h.data_ptr(), 8, 8, 1, out.data_ptr())  # no rows: MGX_OK
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()
    capi.tempogram_torch(x, h, None, 8, "none", out=out)
    torch.cuda.synchronize()
    # y of row 0 is (0, 0, 0, 0, 1, 1, 1, 1): lag l has 4 - l products of 1
    assert out[0].cpu().tolist() == [4.0, 3.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0]
