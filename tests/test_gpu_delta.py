"""The delta operator on the device (mgx_delta_device, include/meyda_gpu.h) on synthetic rows; no plan needed.

The expected value is the header's definition evaluated in numpy float64: rows outside a signal repeat its first /
last row, the sum runs in ascending n, one division by D = W (W + 1) (2 W + 1) / 3. The second order is the same
operator over the delta rows as the device stored them.

Tolerance, derived: one rounding to the output type, and at most W + 3 float64 roundings of terms bounded by
M = max|x~| over the rows that enter the sum:
    float32: |got - ref| <= 2^-24 |ref| + 2^-45 M          float64: |got - ref| <= 2^-48 M
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# below, at and above 2 W + 1 for every W, and around any plausible tile
COUNTS = [0, 1, 2, 3, 8, 9, 16, 17, 31, 33, 255, 256, 257, 1031]
BEFORE, AFTER = 3, 5  # rows that belong to no signal
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def table(counts, before=BEFORE):
    return (before + np.concatenate([[0], np.cumsum(counts)])).astype(np.uint64)


def definition(x, fo, W):
    """(delta, M): the definition on float64 rows x (F, cols), and max|x~| over the rows each sum reads; rows that
    belong to no signal are NaN in delta."""
    x = x.astype(np.float64)
    out, M = np.full(x.shape, np.nan), np.zeros(x.shape)
    D = W * (W + 1) * (2 * W + 1) // 3
    with np.errstate(all="ignore"):
        for s in range(len(fo) - 1):
            a, b = int(fo[s]), int(fo[s + 1])
            if b <= a:
                continue
            t = np.arange(a, b)
            acc, m = np.zeros((b - a, x.shape[1])), np.zeros((b - a, x.shape[1]))
            for n in range(1, W + 1):
                up, um = x[np.minimum(t + n, b - 1)], x[np.maximum(t - n, a)]
                acc = acc + n * (up - um)
                m = np.fmax(m, np.fmax(np.abs(up), np.abs(um)))
            out[a:b], M[a:b] = acc / D, m
    return out, M


def within(got, ref, M, what):
    """The derived tolerance on the rows a signal owns (`ref` is NaN elsewhere)."""
    own = ~np.isnan(ref)
    g, r = got.astype(np.float64)[own], ref[own]
    bound = 2.0 ** -24 * np.abs(r) + 2.0 ** -45 * M[own] if got.dtype == np.float32 else 2.0 ** -48 * M[own]
    err = np.abs(g - r)
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run(capi, x, fo, W, want=(True, True), guard=0):
    """mgx_delta_device on host arrays: (delta, delta2) as numpy, None where not asked for; the outputs are filled
    with the sentinel first, `guard` elements after each array included (returned with it)."""
    import torch
    xs = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    F = x.shape[0]
    cols = x.shape[1] if x.ndim == 2 else 1
    tb = None if fo is None else torch.from_numpy(np.asarray(fo, np.uint64).view(np.int64)).cuda()
    outs = [torch.full((F * cols + guard,), SENTINEL, dtype=xs.dtype, device="cuda") if w else None for w in want]
    capi.delta_device(xs.data_ptr(), F, cols, x.dtype == np.float64, None if tb is None else tb.data_ptr(),
                      0 if tb is None else len(fo) - 1, W, *[None if o is None else o.data_ptr() for o in outs],
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    shape = (F * cols + guard,) if guard else x.shape
    return [None if o is None else o.cpu().numpy().reshape(shape) for o in outs]


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("cols", [1, 13, 40, 128])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_against_the_definition(capi, dtype, cols, W):
    fo = table(COUNTS)
    F = int(fo[-1]) + AFTER
    rng = np.random.default_rng(1000 * cols + W)
    # each column at its own level and offset, so that sums cancel and do not
    x = (rng.standard_normal((F, cols)) * (0.1 + 10 * rng.random(cols)) + 3 * rng.standard_normal(cols)).astype(dtype)
    d1, d2 = run(capi, x, fo, W)
    ref1, M1 = definition(x, fo, W)
    within(d1, ref1, M1, "delta")
    ref2, M2 = definition(d1, fo, W)  # the second order reads the delta rows as stored
    within(d2, ref2, M2, "delta2")
    # rows that belong to no signal keep what was there
    for d in (d1, d2):
        assert d.dtype == dtype
        assert (d[:BEFORE] == SENTINEL).all() and (d[int(fo[-1]):] == SENTINEL).all()
        assert not (d[BEFORE:int(fo[-1])] == SENTINEL).any()
    # a signal of one row: exactly 0 (positive zero), in both orders
    one = int(fo[COUNTS.index(1)])
    assert not bits(d1[one]).any() and not bits(d2[one]).any()
    # order 2 is a second call on the first call's output, bit for bit
    again1, _ = run(capi, d1, fo, W, want=(True, False))
    assert np.array_equal(bits(again1), bits(d2))
    # delta2 alone, and a repeated call
    _, alone = run(capi, x, fo, W, want=(False, True))
    assert np.array_equal(bits(alone), bits(d2))
    r1, r2 = run(capi, x, fo, W)
    assert np.array_equal(bits(r1), bits(d1)) and np.array_equal(bits(r2), bits(d2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_no_table_is_one_signal(capi, dtype):
    rng = np.random.default_rng(5)
    for F, cols in ((1, 13), (700, 13), (300, 1)):
        x = rng.standard_normal((F, cols)).astype(dtype)
        a = run(capi, x, None, 2)
        b = run(capi, x, np.array([0, F], np.uint64), 2)
        ref, M = definition(x, [0, F], 2)
        within(a[0], ref, M, "no table")
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v))
    # a 1-D array is one column
    v = rng.standard_normal(50).astype(dtype)
    a = run(capi, v, None, 3)
    b = run(capi, v.reshape(50, 1), None, 3)
    assert np.array_equal(bits(a[0]), bits(b[0].reshape(50))) and np.array_equal(bits(a[1]), bits(b[1].reshape(50)))
    # a table without a signal, and no rows at all: nothing written, MGX_OK
    d1, d2 = run(capi, x, np.array([7], np.uint64), 2)
    assert (d1 == SENTINEL).all() and (d2 == SENTINEL).all()
    for o in run(capi, np.empty((0, 13), dtype), None, 2, guard=8):
        assert (o == SENTINEL).all()


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_non_finite_values_stay_in_their_reach(capi, dtype, W):
    """One +Infinity and one NaN in the middle of the 40-row middle signal of three. By the definition a row's own
    value does not enter its delta (n starts at 1), so the first order is non-finite in the rows 1..W away from
    the planted one and finite in that row itself; the second order is non-finite in every row within 2 W (at
    W = 1: in the rows 0 and 2 away). No other row, column or signal is touched: every other value has the bits of
    the call on the clean rows."""
    cols, r_inf, r_nan, c_inf, c_nan = 13, 60, 59, 4, 9
    fo = np.array([0, 40, 80, 120], np.uint64)
    rng = np.random.default_rng(W)
    clean = rng.standard_normal((120, cols)).astype(dtype)
    x = clean.copy()
    x[r_inf, c_inf], x[r_nan, c_nan] = np.inf, np.nan
    want = run(capi, clean, fo, W)
    got = run(capi, x, fo, W)
    expect = ~np.isfinite(x)
    for k, (g, w) in enumerate(zip(got, want)):
        # a row is non-finite when a row 1..W away was in the order below (an infinity never cancels to a finite sum)
        reach = (k + 1) * W
        spread = np.zeros_like(expect)
        for n in range(1, W + 1):
            spread[n:] |= expect[:-n]
            spread[:-n] |= expect[n:]
        expect = spread
        assert np.array_equal(~np.isfinite(g), expect), (k, np.argwhere(~np.isfinite(g) != expect)[:8])
        assert np.array_equal(bits(g[~expect]), bits(w[~expect]))
        for r, c in ((r_inf, c_inf), (r_nan, c_nan)):
            hit = np.flatnonzero(expect[:, c])
            assert hit.min() == r - reach and hit.max() == r + reach
            # within the reach every row but, in the first order, the planted one (and at W = 1 its neighbours in the second)
            inside = np.arange(r - reach, r + reach + 1)
            holes = {0: [r], 1: [r - 1, r + 1] if W == 1 else []}[k]
            assert sorted(set(inside) - set(hit)) == holes
    assert np.isnan(got[0][r_nan - W:r_nan + W + 1, c_nan][np.arange(2 * W + 1) != W]).all()
    assert np.isinf(got[0][r_inf - 1, c_inf]) and np.isinf(got[0][r_inf + 1, c_inf])


@pytest.mark.parametrize("fo", [[0, 100, 5000, 300, 2 ** 63], [0, 300, 200, 700, 650], [900, 20, 10, 0, 1]],
                         ids=["above_num_frames", "decreasing", "all_decreasing"])
def test_bad_tables_stay_inside_the_arrays(capi, fo):
    """A table the host cannot see may hold anything: MGX_OK, values unspecified, nothing written past the arrays'
    ends (a guard of sentinels after each)."""
    F, cols, guard = 800, 13, 4096
    x = np.random.default_rng(3).standard_normal((F, cols)).astype(np.float32)
    for want in ((True, True), (False, True)):
        for o in run(capi, x, np.array(fo, np.uint64), 8, want=want, guard=guard):
            assert o is None or (o[F * cols:] == SENTINEL).all()
    # ... and where such a table is non-decreasing after the limit to num_frames it gives the definition
    if fo[2] == 5000:
        d1, _ = run(capi, x, np.array(fo[:3], np.uint64), 2)
        ref, M = definition(x, [0, 100, F], 2)
        within(d1, ref, M, "entry above num_frames")
