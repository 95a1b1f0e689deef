"""The chroma operator (mgx_chroma_device, include/meyda_gpu.h) against the numpy statement of its definition
(tests/chroma_ref.py): equality of bits, both norms. The definition fixes every rounding and the order of every
addition, and the division is the correctly rounded float64 one."""
import ctypes

import numpy as np
import pytest

import chroma_ref

pytestmark = pytest.mark.gpu

F = 301
COLS = [1, 63, 64, 65, 128, 512, 2048]
BINS = [1, 12, 13, 36]
SENTINEL = 777.0


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def make_rows(cols, seed, rows=F):
    """|normal| scaled over +-20 in the exponent, element by element."""
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((rows, cols))) * 2.0 ** rng.integers(-20, 21, (rows, cols))).astype(np.float32)


def positive_bank(C, cols, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((C, cols)) * 2.0 ** rng.integers(-6, 1, (C, cols))).astype(np.float32)


def run(capi, x, w, norm, extra=3):
    """The operator's rows and the `extra` sentinel rows behind them."""
    import torch
    xd = torch.from_numpy(x).cuda()
    wd = torch.from_numpy(w).cuda()
    buf = torch.full((x.shape[0] + extra, w.shape[0]), SENTINEL, dtype=torch.float32, device="cuda")
    capi.chroma_torch(xd, wd, norm, out=buf[:x.shape[0]])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[x.shape[0]:] == SENTINEL).all(), "the rows after the last output row were written"
    return got[:x.shape[0]]


def same(got, want, what):
    """Equal bits; a NaN for a NaN (its payload is not part of the definition)."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~nan)
    assert bad.size == 0, (what, len(bad), bad[:4], [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def both_norms(capi, x, w, what):
    S = chroma_ref.ordered_sums(x, w)
    with np.errstate(all="ignore"):
        want = {"none": S.astype(np.float32), "max": chroma_ref.normalise(S).astype(np.float32)}
    got = {}
    for norm in ("none", "max"):
        got[norm] = run(capi, x, w, norm)
        same(got[norm], want[norm], (what, norm))
    return got, want


@pytest.mark.parametrize("C", BINS)
@pytest.mark.parametrize("cols", COLS)
def test_operator_against_the_oracle(capi, cols, C):
    x = make_rows(cols, 1000 + cols)
    x[7] = 0.0                       # a silent buffer
    x[11, 0] = np.nan                # NaN: its own row only
    x[13, cols - 1] = np.inf         # an overflowed amplitude
    x[17] = np.float32(1e-42)        # float32 denormals
    x[19, ::2] = np.float32(3e-45)
    w = positive_bank(C, cols, 7 * cols + C)
    got, want = both_norms(capi, x, w, (cols, C))
    for norm in ("none", "max"):
        g = got[norm]
        assert (g[7] == 0).all() and not np.signbit(g[7]).any()
        assert np.isnan(g[11]).all() and np.isfinite(g[10]).all() and np.isfinite(g[12]).all()
        assert (g[13] == np.inf).all()
    fin = np.isfinite(x).all(axis=1) & (x > 0).any(axis=1)
    assert (got["max"][fin].max(axis=1) == 1.0).all()  # (the denormal rows too: the division is in float64)


@pytest.mark.parametrize("C", [12, 13])
@pytest.mark.parametrize("cols", [65, 512])
def test_signed_bank(capi, cols, C):
    """A caller's signed bank: rows whose sums are all <= 0 stay undivided, and no -0 comes out."""
    rng = np.random.default_rng(cols + C)
    x = make_rows(cols, 5)
    w = rng.standard_normal((C, cols)).astype(np.float32)
    w[:, 0] = -np.abs(w[:, 0])
    x[3] = 0.0
    x[3, 0] = 2.0                    # every sum negative: m <= 0
    x[5] = 0.0
    x[5, :2] = [1.0, -0.0]
    x[9, 1], x[9, 2] = np.inf, np.inf   # Inf - Inf under a signed bank: NaN and Inf side by side
    got, want = both_norms(capi, x, w, ("signed", cols, C))
    assert (got["max"][3] < 0).all() and np.array_equal(got["max"][3], got["none"][3])
    assert not (np.signbit(got["none"]) & (got["none"] == 0)).any()
    assert not (np.signbit(got["max"]) & (got["max"] == 0)).any()


@pytest.mark.parametrize("n", [256, 1024])
def test_library_table(capi, n):
    """The library's own bank (cols = 128 and 512), C = 12 and 36, over amplitude-like rows."""
    cols = n // 2
    x = make_rows(cols, n)
    for C in (12, 36):
        w = capi.chroma_weights(n, 44100.0, num_chroma=C)
        assert w.shape == (C, cols)
        both_norms(capi, x, w, ("library table", n, C))


def test_many_rows_and_row_counts(capi):
    """More rows than one pass of the grid's waves, and row counts that leave a wave's last group of rows partly empty."""
    w12, w36 = positive_bank(12, 128, 1), positive_bank(36, 128, 2)
    x = make_rows(128, 9, rows=40003)
    same(run(capi, x, w12, "max"), chroma_ref.chroma(x, w12, "max"), "40003 rows, C = 12")
    same(run(capi, x[:20001], w36, "max"), chroma_ref.chroma(x[:20001], w36, "max"), "20001 rows, C = 36")
    for rows in (1, 2, 3, 4, 5, 15, 16, 17):
        same(run(capi, x[:rows], w12, "max"), chroma_ref.chroma(x[:rows], w12, "max"), (rows, 12))
        same(run(capi, x[:rows], w36, "none"), chroma_ref.chroma(x[:rows], w36, "none"), (rows, 36))


def test_repeat_and_graph_replay(capi):
    import torch
    x = make_rows(512, 11)
    w = capi.chroma_weights(1024, 44100.0)
    want = run(capi, x, w, "max")
    same(run(capi, x, w, "max"), want, "repeated")
    same(want, chroma_ref.chroma(x, w, "max"), "oracle")
    s = torch.cuda.Stream()
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
    out = torch.full((F, 12), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        capi.chroma_torch(xd, wd, "max", stream=s.cuda_stream, out=out)
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    same(out.cpu().numpy(), want, "graph replay")


def test_refusals_and_no_rows(capi):
    import torch
    x = torch.zeros((4, 128), dtype=torch.float32, device="cuda")
    w = torch.ones((12, 128), dtype=torch.float32, device="cuda")
    out = torch.full((4, 12), SENTINEL, dtype=torch.float32, device="cuda")
    L = capi.lib()
    call = lambda rows=x.data_ptr(), F=4, cols=128, wp=w.data_ptr(), C=12, norm=1, o=out.data_ptr(): L.mgx_chroma_device(
        ctypes.c_void_p(rows), F, cols, ctypes.c_void_p(wp), C, norm, ctypes.c_void_p(o), None)
    for kw in (dict(cols=0), dict(C=0), dict(C=37), dict(norm=2), dict(wp=None), dict(o=None), dict(o=x.data_ptr()),
               dict(o=w.data_ptr()), dict(rows=None)):
        assert call(**kw) == -1, kw
        assert len(L.mgx_last_error()) > 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()  # a refused call launched nothing
    assert call(F=0) == 0 and call(F=0, rows=None) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all().item()
    with pytest.raises(ValueError):
        capi.chroma_torch(x, w, "l2")
    assert call() == 0
    torch.cuda.synchronize()
    assert (out == 0).all().item()
