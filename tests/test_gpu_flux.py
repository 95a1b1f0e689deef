"""The flux operator (mgx_flux_device, include/meyda_gpu.h) against the numpy statement of its definition
(tests/flux_ref.py). RECTIFIED and L1 are equality of bits: the definition fixes every rounding and the order of
every addition. In L2 the sum S is the oracle's too, but the last bit of the device's float64 square root is not
documented here, so the result has to be the rounding, to the rows' type, of sqrt(S) or of one of its two float64
neighbours (for float32 rows that is one value except at a rounding boundary)."""
import numpy as np
import pytest

import flux_ref

pytestmark = pytest.mark.gpu

F = 301
COLS = [1, 13, 26, 40, 63, 64, 65, 129, 256, 2048]
LAGS = [1, 2, 8]
SENTINEL = 777.0


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def table(lag):
    # an empty signal, a one-row signal, a signal of exactly `lag` rows, a long one; rows before and after every signal
    return np.array([2, 2, 3, 3 + lag, 20, F - 5], np.uint64)


def make_rows(cols, dtype, seed):
    """Values scaled over +-20 in the exponent, element by element; some equal to the element `lag` rows above."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((F, cols)) * 2.0 ** rng.integers(-20, 21, (F, cols))).astype(dtype)
    for lag in LAGS:
        keep = rng.random((F - lag, cols)) < 0.05
        x[lag:][keep] = x[:-lag][keep]
    return x


def run(capi, x, fo, mode, lag, fill=SENTINEL):
    import torch
    xd = torch.from_numpy(x).cuda()
    out = torch.full((x.shape[0],), fill, dtype=xd.dtype, device="cuda")
    capi.flux_torch(xd, None if fo is None else np.asarray(fo, np.uint64), mode, lag, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same(got, want, what):
    """Equal bits; a NaN for a NaN (its payload is not part of the definition)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.nonzero((got.view(u) != want.view(u)) & ~nan)[0]
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def check_l2(got, x, fo, lag, what, fill=SENTINEL):
    S, written = flux_ref.sums(x, fo, flux_ref.L2, lag)
    assert (got[~written] == fill).all(), what
    with np.errstate(all="ignore"):
        r = np.sqrt(S)
        cands = [c.astype(x.dtype) for c in (r, np.nextafter(r, 0.0), np.nextafter(r, np.inf))]
    ok = np.zeros(S.shape, bool)
    for c in cands:
        ok |= (got == c) | (np.isnan(got) & np.isnan(c))
    bad = np.nonzero(written & ~ok)[0]
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], cands[0][bad[:8]])
    # a root of an exactly representable square is exact whatever the last bit's rule
    sq = written & (r * r == S) & (r == np.floor(r))
    assert (got[sq] == r[sq].astype(x.dtype)).all(), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cols", COLS)
def test_operator_against_the_oracle(capi, cols, dtype):
    x = make_rows(cols, dtype, 1000 + cols)
    for lag in LAGS:
        fo = table(lag)
        first = [int(a) for a, b in zip(fo[:-1], fo[1:]) if b > a]
        for mode in ("rectified", "l1"):
            got = run(capi, x, fo, mode, lag)
            want = flux_ref.flux(x, fo, mode, lag, fill=SENTINEL)
            same(got, want, (cols, dtype.__name__, mode, lag))
            # sentinels stay in the rows of no signal; a signal's first row is exactly 0
            assert (got[:2] == SENTINEL).all() and (got[F - 5:] == SENTINEL).all() and (got[first] == 0).all()
            assert (got[20:F - 5] > 0).any()
        got = run(capi, x, fo, "l2", lag)
        check_l2(got, x, fo, lag, (cols, dtype.__name__, "l2", lag))
        assert (got[first] == 0).all()


@pytest.mark.parametrize("cols", [13, 129])
def test_null_table_repeat_and_wide_table(capi, cols):
    x = make_rows(cols, np.float32, 7)
    for mode in ("rectified", "l1"):
        got = run(capi, x, None, mode, 2)
        same(got, flux_ref.flux(x, None, mode, 2), ("NULL table", mode))
        same(run(capi, x, None, mode, 2), got, ("repeated", mode))
        # one signal given as a table is the NULL table's
        same(run(capi, x, [0, F], mode, 2), got, ("one signal", mode))
    # entries above num_frames are limited to it: nothing outside the arrays is touched, the rows are the oracle's
    fo = np.array([5, 100, F + 10, 2 ** 40, 2 ** 63], np.uint64)
    got = run(capi, x, fo, "l1", 8)
    same(got, flux_ref.flux(x, fo, "l1", 8, fill=SENTINEL), "entries above num_frames")
    assert (got[:5] == SENTINEL).all() and got[5] == 0 and got[100] == 0
    # a table that is not non-decreasing: unspecified values, and a call that returns
    got = run(capi, x, np.array([50, 10, 2 ** 62, 3, 200], np.uint64), "l1", 8)
    assert got.shape == (F,)
    # a table without a signal writes nothing
    assert (run(capi, x, [7], "l1", 1) == SENTINEL).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cols", [13, 40, 200])
def test_non_finite_rows(capi, cols, dtype):
    """NaN stays in its signal (rows t and t + lag of it); Inf against a finite value is Inf where the mode keeps the
    sign's side; a column that is -Infinity in both rows contributes 0."""
    rng = np.random.default_rng(cols)
    x = rng.standard_normal((60, cols)).astype(dtype)
    fo = np.array([0, 20, 40, 60], np.uint64)
    x[:, 0] = -np.inf           # a dead band in every row
    x[25, 3] = np.nan           # second signal
    x[38, cols - 1] = np.nan    # its last rows: row 40 is the third signal's first
    x[50, 5] = np.inf           # third signal
    x[55, 6] = -np.inf
    for lag in (1, 2):
        for mode in ("rectified", "l1"):
            got = run(capi, x, fo, mode, lag)
            same(got, flux_ref.flux(x, fo, mode, lag, fill=SENTINEL), (mode, lag))
            nan = np.zeros(60, bool)
            nan[[25, 25 + lag, 38]] = True
            nan[38 + lag] = 38 + lag < 40
            assert np.array_equal(np.isnan(got), nan), (mode, lag)
            assert np.isfinite(got[:20]).all() and np.isfinite(got[40:50]).all()  # the dead band poisons nothing
            assert got[50] == np.inf and got[50 + lag] == (np.inf if mode == "l1" else got[50 + lag])
            assert np.isfinite(got[50 + lag]) == (mode == "rectified")
            assert (got[55] == np.inf) == (mode == "l1") and got[55 + lag] == np.inf
        got = run(capi, x, fo, "l2", lag)
        check_l2(got, x, fo, lag, ("l2", lag))
        assert np.isfinite(got[:20]).all() and got[50] == np.inf and np.isnan(got[25])


def test_many_rows_more_than_one_tile_per_workgroup(capi):
    """40,000 narrow rows and 3,000 wide ones: several tiles, sub-wave groups, signals that begin inside a tile."""
    rng = np.random.default_rng(3)
    for rows, cols in ((40000, 5), (40000, 32), (3000, 600)):
        x = rng.standard_normal((rows, cols)).astype(np.float32)
        fo = np.array([0, 1, 1000, 1001, 1029, rows // 2 + 3, rows - 1], np.uint64)
        got = run(capi, x, fo, "l1", 8)
        same(got, flux_ref.flux(x, fo, "l1", 8, fill=SENTINEL), (rows, cols))


def test_graph_replay(capi):
    import torch
    x = make_rows(129, np.float32, 11)
    fo = table(2)
    want = run(capi, x, fo, "rectified", 2)
    s = torch.cuda.Stream()
    xd = torch.from_numpy(x).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    out = torch.full((F,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        capi.flux_torch(xd, tb, "rectified", 2, stream=s.cuda_stream, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "graph replay")
