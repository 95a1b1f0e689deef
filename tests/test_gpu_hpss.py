"""The HPSS operator (mgx_hpss_device, include/meyda_gpu.h) against the numpy statement of its definition
(tests/hpss_ref.py): equality of bits over every element, every mode. MEDIANS compares a NaN's payload too (the output
is a copied element); a computed NaN is a NaN for a NaN. One table holds the clip lengths at which the kernel takes
another path: shorter than a quarter of the halo (repeated reflection), around the halo, around the tile height."""
import numpy as np
import pytest

import hpss_ref

pytestmark = pytest.mark.gpu

COLS = [1, 2, 31, 63, 64, 65, 512]
KERNELS = [(1, 1), (3, 3), (31, 31), (5, 17), (17, 5), (31, 1), (1, 31)]
MODES = ["medians", "soft1", "soft2", "hard"]
MARGINS = [(1.0, 1.0), (2.0, 1.5)]
SENTINEL = 777.0
LEAD, TRAIL, GUARD = 5, 7, 3


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def table_of(capi):
    """Clips of 0, 1, 2, 3, 15, 16, 17, 31 and 100 rows and of T - 1, T, T + 1 and 2 T + 1 rows (T: the tile's
    rows), behind LEAD rows of no signal; TRAIL more follow. Returns (offsets, F)."""
    T, _ = capi.hpss_tile()
    lengths = [3, 0, 1, 17, 2, T - 1, 15, 100, 16, T, 31, 2 * T + 1, T + 1]
    offsets = np.concatenate([[LEAD], LEAD + np.cumsum(lengths)]).astype(np.uint64)
    return offsets, int(offsets[-1]) + TRAIL


def make_rows(F, cols, seed, offsets):
    """Values with which a selection can go wrong: rows quantised to four values (ties dominate), both zeros mixed,
    all-zero clips and blocks, single NaNs (either sign, with payloads) and +Infinity at under half a window's
    density, a few negative values."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal((F, cols))) * 2.0 ** rng.integers(-12, 13, (F, cols))).astype(np.float32)
    quant = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), (F, cols))
    x = np.where((np.arange(F) % 3 == 0)[:, None], quant, x).astype(np.float32)
    zeros = rng.choice(np.array([0.0, -0.0], np.float32), (F, cols))
    x = np.where(rng.random((F, cols)) < 0.25, zeros, x).astype(np.float32)
    x[rng.random((F, cols)) < 0.02] = -1.5
    # all-zero regions: the 16-row clip whole, and a block of rows inside the longest clips (both medians zero there)
    lengths = np.diff(offsets.astype(np.int64))
    for a, n in zip(offsets[:-1].astype(np.int64), lengths):
        if n == 16:
            x[a:a + n] = 0.0
        if n >= 100:
            x[a + 20:a + 20 + 48] = np.where(rng.random((48, cols)) < 0.5, np.float32(0.0), np.float32(-0.0))
    b = x.view(np.uint32)
    b[rng.random((F, cols)) < 0.03] = 0x7FC01234
    b[rng.random((F, cols)) < 0.01] = 0xFFC00007
    b[rng.random((F, cols)) < 0.01] = 0x7F800055  # a signalling NaN: a selection copies it as it is
    x[rng.random((F, cols)) < 0.03] = np.inf
    return x


_cache = {}


def case(capi, cols, kernel):
    """The rows, the table and the reference medians of a (cols, kernel) pair, computed once."""
    key = (cols, kernel)
    if key not in _cache:
        offsets, F = table_of(capi)
        x = make_rows(F, cols, 7919 * cols + 31 * kernel[0] + kernel[1], offsets)
        H, P = hpss_ref.medians(x, offsets, *kernel)
        member = np.zeros(F, bool)
        member[int(offsets[0]):int(offsets[-1])] = True
        for arr in (x, H, P, member):
            arr.setflags(write=False)
        _cache[key] = (x, offsets, H, P, member)
    return _cache[key]


def run(capi, x, offsets, harmonic=True, percussive=True, **params):
    """The operator's outputs (None for one not asked for), written into one buffer of sentinels: GUARD rows, the
    harmonic rows, GUARD rows, the percussive rows, GUARD rows. The guards must keep the sentinel."""
    import torch
    F, cols = x.shape
    xd = torch.tensor(x, device="cuda")
    buf = torch.full((3 * GUARD + 2 * F, cols), SENTINEL, dtype=torch.float32, device="cuda")
    oh, op = buf[GUARD:GUARD + F], buf[2 * GUARD + F:2 * GUARD + 2 * F]
    capi.hpss_torch(xd, None if offsets is None else offsets, harmonic=harmonic, percussive=percussive,
                    out_harmonic=oh if harmonic else None, out_percussive=op if percussive else None, **params)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    for lo, hi in ((0, GUARD), (GUARD + F, 2 * GUARD + F), (2 * GUARD + 2 * F, 3 * GUARD + 2 * F)):
        assert (got[lo:hi] == SENTINEL).all(), "a guard row was written"
    h, p = got[GUARD:GUARD + F], got[2 * GUARD + F:2 * GUARD + 2 * F]
    if not harmonic:
        assert (h == SENTINEL).all()
    if not percussive:
        assert (p == SENTINEL).all()
    return (h if harmonic else None), (p if percussive else None)


def check(got, want, member, what, payload):
    assert (got[~member] == SENTINEL).all(), (what, "a row of no signal was written")
    hpss_ref.same_bits(np.ascontiguousarray(got[member]), np.ascontiguousarray(want[member]), what, payload)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cols", COLS)
def test_operator_against_the_statement(capi, cols, kernel):
    x, offsets, H, P, member = case(capi, cols, kernel)
    for mode in MODES:
        for mh, mp in (MARGINS if mode != "medians" else MARGINS[:1]):
            gh, gp = run(capi, x, offsets, kernel_size=kernel, mode=mode, margin=(mh, mp))
            wh, wp = hpss_ref.mask_outputs(x, H, P, hpss_ref.MODES[mode], mh, mp)
            check(gh, wh, member, ("harmonic", cols, kernel, mode, mh, mp), mode == "medians")
            check(gp, wp, member, ("percussive", cols, kernel, mode, mh, mp), mode == "medians")


def test_zero_rule_is_exercised(capi):
    """The all-zero regions give 0.5 x under unit margins and 0 under others: the reference holds both."""
    x, offsets, H, P, member = case(capi, 65, (31, 31))
    both_zero = (H == 0) & (P == 0) & member[:, None]
    assert both_zero.sum() > 100
    wh, _ = hpss_ref.mask_outputs(x, H, P, hpss_ref.SOFT2, 1.0, 1.0)
    with np.errstate(invalid="ignore"):  # (a signalling NaN among the elements)
        half = (x[both_zero].astype(np.float64) * 0.5).astype(np.float32)
    assert np.array_equal(wh[both_zero], half, equal_nan=True)
    wh, _ = hpss_ref.mask_outputs(x, H, P, hpss_ref.SOFT2, 2.0, 1.5)
    finite = both_zero & np.isfinite(x)
    assert (wh[finite] == 0).all()
    assert np.isfinite(H[member]).mean() > 0.9 and np.isnan(x[member]).sum() > 100 and np.isinf(x[member]).sum() > 100


def test_null_table_is_one_signal(capi):
    x = np.ascontiguousarray(case(capi, 65, (31, 31))[0][:150])
    for kernel, mode in (((31, 31), "soft2"), ((17, 5), "medians")):
        a = run(capi, x, None, kernel_size=kernel, mode=mode)
        b = run(capi, x, np.array([0, 150], np.uint64), kernel_size=kernel, mode=mode)
        want = hpss_ref.hpss(x, None, *kernel, mode)
        for g1, g2, w in zip(a, b, want):
            hpss_ref.same_bits(g1, g2, ("no table", kernel, mode), payload=True)
            hpss_ref.same_bits(g1, w, ("one signal", kernel, mode), payload=mode == "medians")
    # an entry above the rows is limited to them
    c = run(capi, x, np.array([0, 2 ** 40], np.uint64), kernel_size=(31, 31), mode="soft2")
    d = run(capi, x, None, kernel_size=(31, 31), mode="soft2")
    for g1, g2 in zip(c, d):
        hpss_ref.same_bits(g1, g2, "limited", payload=True)


@pytest.mark.parametrize("mode", MODES)
def test_one_output_equals_two(capi, mode):
    x, offsets, _, _, _ = case(capi, 65, (31, 31))
    h2, p2 = run(capi, x, offsets, kernel_size=(31, 31), mode=mode, margin=(2.0, 1.5))
    h1, none = run(capi, x, offsets, percussive=False, kernel_size=(31, 31), mode=mode, margin=(2.0, 1.5))
    assert none is None
    none, p1 = run(capi, x, offsets, harmonic=False, kernel_size=(31, 31), mode=mode, margin=(2.0, 1.5))
    assert none is None
    hpss_ref.same_bits(h1, h2, ("harmonic alone", mode), payload=True)
    hpss_ref.same_bits(p1, p2, ("percussive alone", mode), payload=True)


def test_repeat_and_graph_replay(capi):
    import torch
    x, offsets, _, _, _ = case(capi, 512, (31, 31))
    want = run(capi, x, offsets)
    again = run(capi, x, offsets)
    for a, b in zip(again, want):
        hpss_ref.same_bits(a, b, "repeated", payload=True)
    F, cols = x.shape
    s = torch.cuda.Stream()
    xd = torch.tensor(x, device="cuda")
    od = torch.from_numpy(offsets.view(np.int64)).cuda()
    oh = torch.full((F, cols), SENTINEL, dtype=torch.float32, device="cuda")
    op = torch.full((F, cols), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        capi.hpss_torch(xd, od, stream=s.cuda_stream, out_harmonic=oh, out_percussive=op)
    torch.cuda.synchronize()
    oh.fill_(SENTINEL)
    op.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    hpss_ref.same_bits(oh.cpu().numpy(), want[0], "graph replay, harmonic", payload=True)
    hpss_ref.same_bits(op.cpu().numpy(), want[1], "graph replay, percussive", payload=True)


def test_any_table_stays_inside_the_arrays(capi):
    """A table that is not non-decreasing gives unspecified values, and no access outside the arrays: the guard
    rows around and between the outputs keep their sentinel (run checks them)."""
    x = np.ascontiguousarray(case(capi, 65, (31, 31))[0][:200])
    for table in ([50, 20, 190, 10, 2 ** 40, 100], [2 ** 63, 0, 200], [199, 198, 197, 0], [7, 7, 7], [300, 400]):
        for kernel in ((31, 31), (3, 3)):
            h, p = run(capi, x, np.array(table, np.uint64), kernel_size=kernel, mode="soft2")
            assert h.shape == p.shape == (200, 65)


def test_refusals_and_no_rows(capi):
    import torch
    x = torch.zeros((4, 128), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.MgxError):
        capi.hpss_torch(x, kernel_size=4)
    with pytest.raises(capi.MgxError):
        capi.hpss_torch(x, margin=0.5)
    with pytest.raises(capi.MgxError):
        capi.hpss_torch(x, harmonic=False, percussive=False)
    with pytest.raises(capi.MgxError):
        capi.hpss_device(x.data_ptr(), 4, 128, None, 0, capi.hpss_params(), x.data_ptr(), None)
    # a table of one entry: no signal, nothing written
    out = torch.full((4, 128), SENTINEL, dtype=torch.float32, device="cuda")
    capi.hpss_torch(x, np.array([0], np.uint64), out_harmonic=out, percussive=False)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
