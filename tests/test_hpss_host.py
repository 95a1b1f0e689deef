"""HPSS (mgx_hpss_device, mgx_hpss_host; include/meyda_gpu.h) as far as it can be checked on the host: the two numpy
statements of the definition against each other and against scipy's median filter, the mask arithmetic against
librosa's float32 formulation, the structs and the exports, and every refusal that comes before a device call (the
operator takes no plan, and the host call checks its parameters and requests ahead of the plan)."""
import ctypes

import numpy as np
import pytest

import hpss_ref
from meyda_amd import capi

E_INVALID, E_UNSUPPORTED = -1, -3
NEW = ["mgx_hpss_params_init", "mgx_hpss_tile", "mgx_hpss_device", "mgx_hpss_host"]


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def awkward_rows(F, cols, seed):
    """Ties, both zeros, a few NaNs (either sign, with payloads) and infinities."""
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 1.0, 3.0, -2.0], np.float32), (F, cols)).astype(np.float32)
    x = np.where(rng.random((F, cols)) < 0.3, rng.standard_normal((F, cols)).astype(np.float32), x)
    b = x.view(np.uint32)
    b[rng.random((F, cols)) < 0.04] = 0x7FC00123
    b[rng.random((F, cols)) < 0.02] = 0xFFC00001
    x[rng.random((F, cols)) < 0.04] = np.inf
    x[rng.random((F, cols)) < 0.02] = -np.inf
    return x


def test_structs_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    # four uint32, two floats
    assert ctypes.sizeof(capi.HpssParams) == 24
    assert capi.HpssParams.mode.offset == 12 and capi.HpssParams.margin_percussive.offset == 20
    assert capi.HPSS_MAX_KERNEL == 31 and capi.HPSS_MODES == {"medians": 0, "soft1": 1, "soft2": 2, "hard": 3}
    assert capi.HPSS_MODES == hpss_ref.MODES
    T, W = capi.hpss_tile()
    assert T >= 1 and W >= 1
    capi.lib().mgx_hpss_tile(None, None)  # nothing to set: no fault
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"hpss") == -1


def test_params_init():
    p = capi.HpssParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    capi.lib().mgx_hpss_params_init(ctypes.byref(p))
    assert p.struct_size == 24 and p.kernel_time == 31 and p.kernel_freq == 31 and p.mode == 2
    assert p.margin_harmonic == 1.0 and p.margin_percussive == 1.0
    capi.lib().mgx_hpss_params_init(None)  # nothing to set: no fault
    q = capi.hpss_params(kernel_size=(5, 17), power=float("inf"), margin=(2, 1.5))
    assert (q.kernel_time, q.kernel_freq, q.mode, q.margin_harmonic, q.margin_percussive) == (5, 17, 3, 2.0, 1.5)
    q = capi.hpss_params(kernel_size=7, mode="medians", margin=3)
    assert (q.kernel_time, q.kernel_freq, q.mode, q.margin_harmonic, q.margin_percussive) == (7, 7, 0, 3.0, 3.0)
    assert capi.hpss_params(power=1).mode == 1 and capi.hpss_params(power=2).mode == 2
    with pytest.raises(ValueError):
        capi.hpss_params(power=3)
    with pytest.raises(ValueError):
        capi.hpss_params(mode="soft3")
    with pytest.raises(TypeError):
        capi.hpss_params(mode="hard", power=2)
    with pytest.raises(TypeError):
        capi.hpss_params(kernel_size=(3, 5, 7))


def test_keys_are_the_total_order():
    bits = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                     0x3F800000, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF], np.uint32)
    k = hpss_ref.keys(bits.view(np.float32))
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert [hpss_ref._key1(int(b)) for b in bits] == k.tolist()


def test_reflection():
    assert [int(hpss_ref.reflect(u, 4)) for u in range(-9, 13)] == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3]
    assert [hpss_ref._reflect1(u, 4) for u in range(-9, 13)] == [int(hpss_ref.reflect(u, 4)) for u in range(-9, 13)]
    assert [int(hpss_ref.reflect(u, 1)) for u in range(-3, 4)] == [0] * 7


@pytest.mark.parametrize("kt,kf", [(1, 1), (3, 3), (31, 31), (5, 17), (17, 5), (31, 1), (1, 31)])
def test_the_two_statements_agree(kt, kf):
    offsets = [2, 2, 3, 5, 8, 19, 26]  # clips of 0, 1, 2, 3, 11 and 7 rows; rows of no signal at both ends
    for cols in (1, 2, 9):
        x = awkward_rows(29, cols, 31 * kt + kf + cols)
        H, P = hpss_ref.medians(x, offsets, kt, kf)
        Hl, Pl = hpss_ref.medians_loops(x, offsets, kt, kf)
        hpss_ref.same_bits(H, Hl, ("H", kt, kf, cols), payload=True)
        hpss_ref.same_bits(P, Pl, ("P", kt, kf, cols), payload=True)
        for mode in (1, 2, 3):
            for mh, mp in ((1.0, 1.0), (2.0, 1.5)):
                a = hpss_ref.mask_outputs(x, H, P, mode, mh, mp)
                b = hpss_ref.mask_loops(x, H, P, mode, mh, mp)
                hpss_ref.same_bits(a[0], b[0], ("harmonic", kt, kf, cols, mode, mh))
                hpss_ref.same_bits(a[1], b[1], ("percussive", kt, kf, cols, mode, mp))
    # one signal without a table is the table [0, F]
    x = awkward_rows(9, 5, 99)
    for a, b in zip(hpss_ref.medians(x, None, kt, kf), hpss_ref.medians(x, [0, 9], kt, kf)):
        hpss_ref.same_bits(a, b, "no table", payload=True)


def test_the_median_is_an_element_and_ignores_a_lone_nan():
    x = np.array([[1.0], [np.nan], [2.0], [np.inf], [3.0]], np.float32)
    H, _ = hpss_ref.medians(x, None, 3, 1)
    # windows (reflected): [1 1 nan] [1 nan 2] [nan 2 inf] [2 inf 3] [inf 3 3]
    assert H[:, 0].tolist() == [1.0, 2.0, np.inf, 3.0, 3.0]
    z = np.array([[0.0, -0.0, -0.0]], np.float32)
    _, P = hpss_ref.medians(z, None, 1, 3)
    assert np.signbit(P[0]).tolist() == [False, True, True]  # [+0 +0 -0] [+0 -0 -0] [-0 -0 -0]
    yh, yp = hpss_ref.hpss(np.zeros((4, 4), np.float32) + 2, None, 3, 3, "soft2")
    assert (yh == 1.0).all() and (yp == 1.0).all()
    # both medians zero: 0.5 under unit margins, else 0
    x = np.zeros((5, 5), np.float32)
    x[2, 2] = 8.0
    yh, yp = hpss_ref.hpss(x, None, 3, 3, "soft2")
    assert yh[2, 2] == 4.0 and yp[2, 2] == 4.0
    yh, yp = hpss_ref.hpss(x, None, 3, 3, "soft2", 2.0, 1.0)
    assert yh[2, 2] == 0.0 and yp[2, 2] == 0.0
    yh, yp = hpss_ref.hpss(x, None, 3, 3, "hard")
    assert yh[2, 2] == 0.0 and yp[2, 2] == 0.0


def test_statement_agrees_with_scipy():
    """scipy.ndimage.median_filter(mode='reflect') on finite non-negative rows, for clips of at least K div 2 rows
    (below that scipy's far extension is not always the periodic reflection)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 15, 16, 19, 40):
        for cols in (1, 6, 33):
            x = np.round(np.abs(rng.standard_normal((n, cols))) * 4).astype(np.float32) / 4  # ties
            for K in (1, 3, 5, 17, 31):
                if n >= K // 2:
                    H, _ = hpss_ref.medians(x, None, K, 1)
                    hpss_ref.same_bits(H, ndimage.median_filter(x, size=(K, 1), mode="reflect"), ("time", n, cols, K))
                if cols >= K // 2:
                    _, P = hpss_ref.medians(x, None, 1, K)
                    hpss_ref.same_bits(P, ndimage.median_filter(x, size=(1, K), mode="reflect"), ("freq", n, cols, K))


def test_masks_against_the_float32_formulation():
    """librosa.util.softmask in float32 (both terms divided by their maximum first) against the definition's
    float64 with one rounding: float32 pays a rounding per division, power, sum and quotient, a few 2^-24 in all;
    the bound is 1e-6 relative."""
    rng = np.random.default_rng(11)
    H = (np.abs(rng.standard_normal((64, 64))) * 2.0 ** rng.integers(-10, 11, (64, 64))).astype(np.float32)
    P = (np.abs(rng.standard_normal((64, 64))) * 2.0 ** rng.integers(-10, 11, (64, 64))).astype(np.float32)
    x = np.ones_like(H)
    worst = 0.0
    for mode, power in ((hpss_ref.SOFT1, 1), (hpss_ref.SOFT2, 2)):
        for mh, mp in ((1.0, 1.0), (2.0, 1.5)):
            got = hpss_ref.mask_outputs(x, H, P, mode, mh, mp)
            for y, (X, Xref) in zip(got, ((H, P * np.float32(mh)), (P, H * np.float32(mp)))):
                Z = np.maximum(X, Xref)
                m, r = (X / Z) ** np.float32(power), (Xref / Z) ** np.float32(power)
                want = m / (m + r)
                assert want.dtype == np.float32
                rel = np.abs(y.astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)
                worst = max(worst, float(rel.max()))
    print("worst relative difference: %.3g" % worst)
    assert worst <= 1e-6


def hpss_struct(**kw):
    p = capi.HpssParams()
    capi.lib().mgx_hpss_params_init(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [(dict(struct_size=20), b"struct_size"), (dict(struct_size=0), b"struct_size"),
              (dict(kernel_time=0), b"kernel_time"), (dict(kernel_time=2), b"kernel_time"), (dict(kernel_time=30), b"kernel_time"),
              (dict(kernel_time=33), b"kernel_time"), (dict(kernel_freq=0), b"kernel_freq"), (dict(kernel_freq=16), b"kernel_freq"),
              (dict(kernel_freq=33), b"kernel_freq"), (dict(kernel_freq=2 ** 31 + 1), b"kernel_freq"),
              (dict(mode=4), b"mode"), (dict(mode=2 ** 31), b"mode"),
              (dict(margin_harmonic=float("nan")), b"margin_harmonic"), (dict(margin_harmonic=float("inf")), b"margin_harmonic"),
              (dict(margin_harmonic=0.999), b"margin_harmonic"), (dict(margin_percussive=float("nan")), b"margin_percussive"),
              (dict(margin_percussive=float("inf")), b"margin_percussive"), (dict(margin_percussive=-2.0), b"margin_percussive")]


def test_device_argument_refusals():
    """Every refusal of mgx_hpss_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    rows, h, p, tab = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    names = ("rows", "F", "cols", "tab", "S", "params", "h", "p", "st")

    def call(**kw):
        a = {**dict(rows=rows, F=10, cols=128, tab=None, S=0, params=ctypes.byref(hpss_struct()), h=h, p=p, st=None), **kw}
        return L.mgx_hpss_device(*[a[k] for k in names])
    for bad, word in BAD_PARAMS:
        assert word in refused(call(params=ctypes.byref(hpss_struct(**bad)))), bad
    assert b"params is NULL" in refused(call(params=None))
    assert b"cols" in refused(call(cols=0))
    assert b"both NULL" in refused(call(h=None, p=None))
    assert b"same array" in refused(call(p=h))
    assert b"rows' own array" in refused(call(h=rows))
    assert b"rows' own array" in refused(call(p=rows))
    assert b"frame_offsets is NULL" in refused(call(S=3))
    assert b"rows is NULL" in refused(call(rows=None))
    # refused whatever the number of rows; with valid arguments no rows is MGX_OK, nothing launched
    refused(call(F=0, cols=0))
    refused(call(F=0, params=ctypes.byref(hpss_struct(kernel_time=4))))
    refused(call(F=0, S=2))
    assert call(F=0) == 0 and call(F=0, rows=None) == 0 and call(F=0, h=None) == 0 and call(F=0, tab=tab, S=2) == 0


def test_host_argument_refusals():
    """The parameters and the requests are checked ahead of the plan, so these need no device."""
    L = capi.lib()
    w = np.ones((12, 128), np.float32)
    pf = np.zeros((4, 12), np.float32)
    sm = np.zeros((1, 4, 12), np.float64)
    fl = np.zeros(4, np.float32)
    fs = np.zeros((1, 4), np.float64)
    out = np.zeros((4, 128), np.float32)

    def chroma(**kw):
        r = capi.ChromaRequest()
        r.struct_size = ctypes.sizeof(capi.ChromaRequest)
        r.num_chroma, r.norm, r.weights, r.per_frame, r.summary = 12, 1, w.ctypes.data, pf.ctypes.data, sm.ctypes.data
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.byref(r)

    def flux(**kw):
        r = capi.FluxRequest()
        r.struct_size = ctypes.sizeof(capi.FluxRequest)
        r.field, r.mode, r.lag, r.per_frame, r.summary = 15, 0, 1, fl.ctypes.data, fs.ctypes.data
        for k, v in kw.items():
            setattr(r, k, v)
        return ctypes.byref(r)

    def call(S=1, params=None, c=None, f=None, h=out.ctypes.data, p=None):
        return L.mgx_hpss_host(None, None, 0, None, 0, None, S, params if params is not None else ctypes.byref(hpss_struct()), c, f, h, p)
    for bad, word in BAD_PARAMS:
        assert word in refused(call(params=ctypes.byref(hpss_struct(**bad)))), bad
    assert b"params is NULL" in refused(L.mgx_hpss_host(None, None, 0, None, 0, None, 1, None, None, None, out.ctypes.data, None))
    assert b"all NULL" in refused(call(h=None))
    assert b"same array" in refused(call(p=out.ctypes.data))
    assert b"struct_size" in refused(call(c=chroma(struct_size=32)))
    for C in (0, 37):
        assert b"num_chroma" in refused(call(c=chroma(num_chroma=C)))
    assert b"norm" in refused(call(c=chroma(norm=2)))
    assert b"weights is NULL" in refused(call(c=chroma(weights=None)))
    assert b"both NULL" in refused(call(c=chroma(per_frame=None, summary=None)))
    assert b"num_signals = 0" in refused(call(S=0, c=chroma()))
    assert b"struct_size" in refused(call(f=flux(struct_size=24)))
    assert b"mode" in refused(call(f=flux(mode=3)))
    for lag in (0, 9):
        assert b"lag" in refused(call(f=flux(lag=lag)))
    assert b"both NULL" in refused(call(f=flux(per_frame=None, summary=None)))
    assert b"num_signals = 0" in refused(call(S=0, f=flux()))
    for field in (13, 14, 16, 19):
        assert b"MGX_AMPLITUDE_SPECTRUM" in refused(call(f=flux(field=field)), E_UNSUPPORTED)
    refused(call(f=flux(field=3)), E_UNSUPPORTED)
    # everything in order up to the plan
    assert b"plan is NULL" in refused(call())
    assert b"plan is NULL" in refused(call(c=chroma(), f=flux(), h=None))
