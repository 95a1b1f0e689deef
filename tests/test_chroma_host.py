"""Chroma (mgx_chroma_weights, mgx_chroma_device, mgx_chroma_host; include/meyda_gpu.h) as far as it can be checked
on the host: the filter bank against its numpy statement, the pitch classes it finds, the numpy oracle of the
operator against an exact sum and on its rules, the structs and the exports, and every refusal that comes before a
device call (the operator takes no plan, and the host call checks its request ahead of the plan)."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import chroma_ref
from meyda_amd import capi

E_INVALID, E_POW2 = -1, -2
NEW = ["mgx_chroma_params_init", "mgx_chroma_weights", "mgx_chroma_device", "mgx_chroma_host"]


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def ulp_apart(a, b):
    """The distance of two positive finite float32 arrays in units of the last place."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_structs_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    # two uint32, three doubles, two uint32
    assert ctypes.sizeof(capi.ChromaParams) == 40
    assert capi.ChromaParams.a440.offset == 8 and capi.ChromaParams.base_c.offset == 32
    # four uint32, three pointers
    assert ctypes.sizeof(capi.ChromaRequest) == 40
    assert capi.ChromaRequest.weights.offset == 16 and capi.ChromaRequest.summary.offset == 32
    assert capi.CHROMA_MAX_BINS == 36 and capi.CHROMA_NORMS == {"none": 0, "max": 1}
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"chroma") == -1


def test_params_init():
    p = capi.ChromaParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    capi.lib().mgx_chroma_params_init(ctypes.byref(p))
    assert p.struct_size == 40 and p.num_chroma == 12 and p.a440 == 440.0 and p.center_octave == 5.0
    assert p.octave_width == 2.0 and p.base_c == 1 and p.reserved == 0
    capi.lib().mgx_chroma_params_init(None)  # nothing to set: no fault


@pytest.mark.parametrize("n,sr", list(itertools.product([256, 1024, 4096], [44100.0, 16000.0])))
def test_weights_agree_with_the_numpy_statement(n, sr):
    """Both sides work in float64 from the same formula, and the exp and log2 of two libms differ by parts in
    10^16: only an entry on a float32 rounding boundary can differ, by one unit of the last place."""
    for C, base_c, ow in itertools.product([1, 12, 13, 36], [True, False], [0.0, 2.0]):
        got = capi.chroma_weights(n, sr, num_chroma=C, base_c=base_c, octave_width=ow)
        ref = chroma_ref.weights(n, sr, num_chroma=C, base_c=base_c, octave_width=ow)
        assert got.shape == (C, n // 2) and got.dtype == np.float32
        assert ulp_apart(got, ref).max() <= 1, (C, base_c, ow, ulp_apart(got, ref).max())
        if ow == 0.0:
            ss = np.sum(got.astype(np.float64) ** 2, axis=0)
            assert np.abs(ss - 1.0).max() <= 4 * 2.0 ** -24, (C, base_c, np.abs(ss - 1.0).max())


@pytest.mark.parametrize("C", [1, 12, 13, 36])
def test_weights_finite_and_positive(C):
    """Every entry is finite and greater than 0. In float64 the construction is positive everywhere; where a bin is a
    semitone or narrower bw(k) = 1, |d| reaches C / 2 and w = exp(-2 d^2) falls below the smallest float32 from
    |d| = 7.2 on (C >= 15; exp(-648) at C = 36), and there the one rounding gives the smallest float32, not +0."""
    for n, sr, base_c, ow in itertools.product([256, 1024, 4096], [44100.0, 16000.0], [True, False], [0.0, 2.0]):
        got = capi.chroma_weights(n, sr, num_chroma=C, base_c=base_c, octave_width=ow)
        assert np.isfinite(got).all(), (n, sr, base_c, ow)
        assert (got > 0).all(), (n, sr, base_c, ow, int((got == 0).sum()), got.size)
        if C == 36:  # the far rows of the narrow bins are there, as the smallest float32
            assert (got == np.float32(1e-45)).sum() > got.size // 4 and got.max() > 0.1


def test_weights_other_parameters():
    got = capi.chroma_weights(1024, 22050.0, a440=432.0, center_octave=4.0, octave_width=1.5)
    ref = chroma_ref.weights(1024, 22050.0, a440=432.0, center_octave=4.0, octave_width=1.5)
    assert ulp_apart(got, ref).max() <= 1


@pytest.mark.parametrize("n,sr", [(1024, 44100.0), (4096, 44100.0), (4096, 16000.0)])
def test_pitch_classes(n, sr):
    """Hann-windowed sines at A4, C4 and E5 peak in rows 9, 0 and 4 of the library's table (row 0 is C)."""
    w = capi.chroma_weights(n, sr)
    t = np.arange(n) / sr
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    for freq, row in ((440.0, 9), (261.6255653005986, 0), (659.2551138257398, 4)):
        amp = np.abs(np.fft.rfft(hann * np.sin(2 * np.pi * freq * t)))[:n // 2].astype(np.float32)
        c = chroma_ref.chroma(amp[None, :], w, "max")[0]
        assert int(np.argmax(c)) == row and c[row] == 1.0, (freq, c)


def test_weights_refusals():
    L = capi.lib()
    out = (ctypes.c_float * (36 * 2048))()

    def call(n=1024, sr=44100.0, out=out, null_params=False, **kw):
        p = capi.ChromaParams()
        L.mgx_chroma_params_init(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return L.mgx_chroma_weights(n, sr, None if null_params else ctypes.byref(p), out)
    assert call() == 0
    assert b"struct_size" in refused(call(struct_size=39))
    assert b"struct_size" in refused(call(struct_size=0))
    for C in (0, 37, 2 ** 31):
        assert b"num_chroma" in refused(call(num_chroma=C))
    for sr in (0.0, -44100.0, math.inf, math.nan):
        assert b"sample_rate" in refused(call(sr=sr))
    for a in (0.0, -440.0, math.inf, math.nan):
        assert b"a440" in refused(call(a440=a))
    for ow in (-1.0, math.inf, math.nan):
        assert b"octave_width" in refused(call(octave_width=ow))
    assert call(octave_width=0.0) == 0
    assert b"NULL" in refused(call(out=None))
    assert b"NULL" in refused(call(null_params=True))
    for n in (0, 1, 2, 3, 6, 1000, 1025):
        assert b"power of two" in refused(call(n=n), E_POW2)
    assert call(n=4) == 0


def test_operator_refusals():
    """Every refusal of mgx_chroma_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    rows, w, out = (ctypes.c_void_p(256 * k) for k in (1, 2, 3))
    names = ("rows", "F", "cols", "w", "C", "norm", "out", "st")
    call = lambda **kw: L.mgx_chroma_device(*[{**dict(rows=rows, F=10, cols=128, w=w, C=12, norm=1, out=out, st=None), **kw}[k]
                                              for k in names])
    assert b"cols" in refused(call(cols=0))
    for C in (0, 37, 2 ** 31):
        assert b"num_chroma" in refused(call(C=C))
    for norm in (2, 3, 2 ** 31):
        assert b"norm" in refused(call(norm=norm))
    assert b"weights is NULL" in refused(call(w=None))
    assert b"chroma is NULL" in refused(call(out=None))
    assert b"same array as rows" in refused(call(out=rows))
    assert b"same array as weights" in refused(call(out=w))
    assert b"rows is NULL" in refused(call(rows=None))
    # refused whatever the number of rows; with valid arguments no rows is MGX_OK, nothing launched
    refused(call(F=0, cols=0))
    refused(call(F=0, norm=2))
    assert call(F=0) == 0 and call(F=0, rows=None) == 0


def test_host_request_refusals():
    """The request is checked ahead of the plan, so these need no device."""
    L = capi.lib()
    w = np.ones((12, 128), np.float32)
    pf = np.zeros((4, 12), np.float32)
    sm = np.zeros((1, 4, 12), np.float64)

    def call(S=1, null_req=False, **kw):
        r = capi.ChromaRequest()
        r.struct_size = ctypes.sizeof(capi.ChromaRequest)
        r.num_chroma, r.norm, r.weights, r.per_frame, r.summary = 12, 1, w.ctypes.data, pf.ctypes.data, sm.ctypes.data
        for k, v in kw.items():
            setattr(r, k, v)
        return L.mgx_chroma_host(None, None, 0, None, 0, None, S, None if null_req else ctypes.byref(r))
    assert b"request is NULL" in refused(call(null_req=True))
    assert b"struct_size" in refused(call(struct_size=32))
    for C in (0, 37):
        assert b"num_chroma" in refused(call(num_chroma=C))
    assert b"norm" in refused(call(norm=2))
    assert b"weights is NULL" in refused(call(weights=None))
    assert b"both NULL" in refused(call(per_frame=None, summary=None))
    assert b"num_signals = 0" in refused(call(S=0))
    assert b"plan is NULL" in refused(call())


def test_binding_refusals():
    with pytest.raises(TypeError):
        capi.chroma_weights(1024, 44100.0, bins=12)
    with pytest.raises(capi.MgxError):
        capi.chroma_weights(1000, 44100.0)
    with pytest.raises(capi.MgxError):
        capi.chroma_weights(1024, 44100.0, num_chroma=37)


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 129, 2048])
def test_oracle_against_an_exact_sum(cols):
    """Non-negative amplitudes under the library's positive table: every product is exact and non-negative, and a
    value passes through at most ceil(cols / 64) - 1 additions of its partial and 6 halvings, so the ordered sum is
    within (ceil(cols / 64) + 5) 2^-53, relatively, of the exact sum, which math.fsum gives."""
    rng = np.random.default_rng(cols)
    F, C = 6, 12
    w = capi.chroma_weights(4096, 44100.0)[:, :cols]
    x = (np.abs(rng.standard_normal((F, cols))) * 2.0 ** rng.integers(-20, 21, (F, cols))).astype(np.float32)
    S = chroma_ref.ordered_sums(x, w)
    bound = (-(-cols // 64) + 5) * 2.0 ** -53
    for t in range(F):
        for c in range(C):
            exact = math.fsum((x[t].astype(np.float64) * w[c].astype(np.float64)).tolist())
            assert exact > 0 and abs(S[t, c] - exact) <= bound * exact, (t, c, S[t, c], exact)
    got = chroma_ref.chroma(x, w, "max")
    assert got.dtype == np.float32 and got.max() == 1.0 and (got.max(axis=1) == 1.0).all()


def test_oracle_rules():
    inf, nan = np.inf, np.nan
    w = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0]], np.float32)
    # a zero row stays zero, and +0
    z = chroma_ref.chroma(np.zeros((1, 3), np.float32), w, "max")
    assert (z == 0).all() and not np.signbit(z).any()
    # a NaN never becomes the maximum: the others are divided by the largest of them (on the sums themselves: a NaN
    # amplitude is NaN under every finite weight, 0 included, so a row's sums are NaN together)
    r = chroma_ref.normalise(np.array([[nan, 4.0, 2.0, nan], [-inf, -1.0, nan, -2.0]]))
    assert np.isnan(r[0, 0]) and r[0, 1] == 1.0 and r[0, 2] == 0.5 and np.isnan(r[0, 3])
    assert r[1, 0] == -inf and r[1, 1] == -1.0 and np.isnan(r[1, 2]) and r[1, 3] == -2.0
    r = chroma_ref.chroma(np.array([[nan, 4.0, 2.0]], np.float32), w, "max")[0]
    assert np.isnan(r).all()
    # an infinite maximum leaves the row undivided
    r = chroma_ref.normalise(np.array([[inf, 4.0, 2.0, inf]]))[0]
    assert r[0] == inf and r[1] == 4.0 and r[2] == 2.0 and r[3] == inf
    r = chroma_ref.chroma(np.array([[inf, 4.0, 2.0]], np.float32), np.array([[1, 1, 1], [2, 1, 1], [-1, 1, 1]], np.float32), "max")[0]
    assert r[0] == inf and r[1] == inf and r[2] == -inf
    # a maximum <= 0 (a signed bank) leaves the row undivided
    r = chroma_ref.chroma(np.array([[1.0, 4.0, 2.0]], np.float32), -w, "max")[0]
    assert list(r) == [-1.0, -4.0, -2.0, -5.0]
    # all NaN: nothing to divide by
    assert np.isnan(chroma_ref.chroma(np.full((1, 3), nan, np.float32), w, "max")).all()
    # no -0 comes out: a partial starts at +0, and +0 + -0 is +0
    r = chroma_ref.chroma(np.array([[0.0, 1.0, 0.0]], np.float32), -w, "none")[0]
    assert r[0] == 0 and not np.signbit(r[0]) and r[1] == -1.0
    r = chroma_ref.chroma(np.array([[-0.0, -0.0, -0.0]], np.float32), w, "max")[0]
    assert (r == 0).all() and not np.signbit(r).any()
    # norm none is the plain ordered sum
    r = chroma_ref.chroma(np.array([[1.0, 4.0, 2.0]], np.float32), w, "none")[0]
    assert list(r) == [1.0, 4.0, 2.0, 5.0]
    # 0 x Inf in a column that exists is NaN, in its own row only
    r = chroma_ref.chroma(np.array([[inf, 1.0, 1.0], [1.0, 1.0, 1.0]], np.float32), w, "none")
    assert np.isnan(r[0, 1]) and r[0, 0] == inf and np.isfinite(r[1]).all()
