"""Tempo (mgx_tempogram_device, mgx_tempo_device, mgx_tempo_host, mgx_tempogram_window, mgx_tempo_prior;
include/meyda_gpu.h) as far as it can be checked on the host: the numpy statement of the tempogram against loops
written from the definition, the structs and the exports, the window and the prior against their statements, the
pick's rules, and every refusal that comes before a launch (the device calls take no plan, and the host call
checks its parameters ahead of the plan)."""
import ctypes
import math

import numpy as np
import pytest

import tempo_ref
from meyda_amd import capi

E_INVALID = -1
NEW = ["mgx_tempo_params_init", "mgx_tempogram_window", "mgx_tempo_prior", "mgx_tempogram_device", "mgx_tempo_workspace_bytes",
       "mgx_tempo_device", "mgx_tempo_host"]


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def envelope(F, seed):
    """Non-negative values over +-20 binary orders with a silent stretch, float32 denormals, a NaN and a +Infinity."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal(F)) * 2.0 ** rng.integers(-20, 21, F)).astype(np.float32)
    x[F // 3:F // 3 + 5] = 0.0
    x[1] = np.float32(3e-43)
    x[F - 2] = np.nan
    x[F // 2] = np.inf
    return x


@pytest.mark.parametrize("W,L", [(2, 1), (2, 2), (5, 3), (8, 8), (16, 9)])
@pytest.mark.parametrize("norm", [tempo_ref.NORM_NONE, tempo_ref.NORM_LAG0])
def test_statement_against_loops(W, L, norm):
    F = 40
    x = envelope(F, W * 100 + L)
    h = tempo_ref.window_ref(W)
    h[0] = np.float32(0.25)  # (the periodic Hann window starts at 0: give the first tap a say)
    for table in (None, [3, 3, 4, 4 + W // 2, 30, 38]):
        got = tempo_ref.tempogram_ref(x, h, L, norm, table, fill=7.0)
        want = tempo_ref.tempogram_loops(x, h, L, norm, table, fill=7.0)
        assert got.shape == (F, L) and got.dtype == np.float32
        assert np.array_equal(bits(got), bits(want)), (W, L, norm, table)
    # the same on a float64 envelope: values are taken as float64
    x64 = envelope(F, 5).astype(np.float64) * (1.0 + 2.0 ** -30)
    assert np.array_equal(bits(tempo_ref.tempogram_ref(x64, h, L, norm)), bits(tempo_ref.tempogram_loops(x64, h, L, norm)))


def test_statement_rules():
    h = np.ones(4, np.float32)
    # a silent window stays +0 under both norms; lag 0 of a normalised row is exactly 1
    z = tempo_ref.tempogram_ref(np.zeros(6, np.float32), h, 4, tempo_ref.NORM_LAG0)
    assert (z == 0).all() and not np.signbit(z).any()
    r = tempo_ref.tempogram_ref(np.array([1, 2, 3, 4, 5, 6], np.float32), h, 4, tempo_ref.NORM_LAG0)
    assert (r[:, 0] == 1.0).all()
    # outside the signal the envelope is +0, not an edge repeat: row 0 sees y = (0, 0, x0, x1)
    r = tempo_ref.tempogram_ref(np.array([3, 5, 7, 11], np.float32), h, 4, tempo_ref.NORM_NONE)
    assert list(r[0]) == [9.0 + 25.0, 15.0, 0.0, 0.0]
    # an infinite value reaches the rows whose window holds it, in its own signal, and no other row; a lag whose
    # terms do not hold it stays finite
    x = np.ones(12, np.float32)
    x[2] = np.inf
    r = tempo_ref.tempogram_ref(x, h, 4, tempo_ref.NORM_NONE, [0, 6, 12])
    assert np.isfinite(r[6:]).all() and (r[1:5, 0] == np.inf).all() and np.isfinite(r[0]).all() and np.isfinite(r[5]).all()
    # row 3: y = (1, inf, 1, 1): lag 3 is y(0) y(3) alone and stays finite; row 1: y = (+0, 1, 1, inf): lag 3 is 0 x inf
    assert r[3, 3] == 1.0 and np.isnan(r[1, 3])


def test_structs_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    # four uint32, a double
    assert ctypes.sizeof(capi.TempoParams) == 24 and capi.TempoParams.gain.offset == 16
    assert capi.TEMPOGRAM_MAX_WIN == 1024 and capi.TEMPO_CHUNK_ROWS == 65536 and capi.TEMPOGRAM_NORMS == {"none": 0, "lag0": 1}
    p = capi.TempoParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    capi.lib().mgx_tempo_params_init(ctypes.byref(p))
    assert (p.struct_size, p.win_length, p.num_lags, p.norm, p.gain) == (24, 384, 384, 1, 1e6)
    capi.lib().mgx_tempo_params_init(None)  # nothing to set: no fault
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"tempo") == -1 and capi.lib().mgx_feature_index(b"tempogram") == -1


@pytest.mark.parametrize("W", [2, 3, 8, 65, 384, 1000, 1024])
def test_window(W):
    """Compared after the float32 rounding: both sides form 0.5 - 0.5 cos in float64; two libms' cosines may differ in
    the last place of float64, which the rounding to float32 hides except on a rounding boundary."""
    got, ref = capi.tempogram_window(W), tempo_ref.window_ref(W)
    assert got.dtype == np.float32 and got.shape == (W,)
    assert np.array_equal(bits(got), bits(ref)), int((bits(got) != bits(ref)).sum())
    assert got[0] == 0.0 and (W % 2 or got[W // 2] == 1.0)


@pytest.mark.parametrize("rate,L,start,std,mx", [(172.265625, 384, 120.0, 1.0, 320.0), (86.1328125, 1024, 100.0, 0.5, 0.0),
                                                 (31.25, 2, 120.0, 1.0, 320.0), (1000.0, 1, 60.0, 2.0, 10.0)])
def test_prior(rate, L, start, std, mx):
    """A relative 4 x 2^-52: libm and numpy may differ in the last place of log2 and exp."""
    got, ref = capi.tempo_prior(rate, L, start, std, mx), tempo_ref.prior_ref(rate, L, start, std, mx)
    assert got.dtype == np.float64 and got.shape == (L,) and got[0] == 0.0
    assert (np.abs(got - ref) <= 4 * 2.0 ** -52 * np.abs(ref)).all(), np.abs(got / ref - 1)[1:].max()
    assert ((got == 0) == (ref == 0)).all()
    print("prior entries that differ at all: %d of %d" % (int((got != ref).sum()), L))
    if mx > 0 and L > 1:
        l = np.arange(1, L)
        assert ((got[1:] == 0) == (60.0 * rate / l > mx)).all()


def test_window_and_prior_refusals():
    L = capi.lib()
    h = (ctypes.c_float * 1024)()
    p = (ctypes.c_double * 16)()
    for W in (0, 1, 1025, 2 ** 31):
        assert b"win_length" in refused(L.mgx_tempogram_window(W, h))
    assert b"NULL" in refused(L.mgx_tempogram_window(8, None))
    assert L.mgx_tempogram_window(2, h) == 0 and L.mgx_tempogram_window(1024, h) == 0
    ok = dict(rate=100.0, start=120.0, std=1.0, mx=320.0, n=16, out=p)
    call = lambda **kw: L.mgx_tempo_prior(*[{**ok, **kw}[k] for k in ("rate", "start", "std", "mx", "n", "out")])
    assert call() == 0 and call(mx=0.0) == 0
    for v in (0.0, -1.0, math.inf, math.nan):
        assert b"frame_rate" in refused(call(rate=v))
        assert b"start_bpm" in refused(call(start=v))
        assert b"std_octaves" in refused(call(std=v))
    for v in (-1.0, math.nan):
        assert b"max_bpm" in refused(call(mx=v))
    assert b"num_lags" in refused(call(n=0))
    assert b"NULL" in refused(call(out=None))
    with pytest.raises(capi.MgxError):
        capi.tempogram_window(1)
    with pytest.raises(ValueError):
        capi.tempo_params(norm="max")


def test_pick_rules():
    pick, loop = tempo_ref.pick_ref, tempo_ref.pick_loop
    nan, inf = np.nan, np.inf
    p = np.array([0.0, 0.5, 1.0, 1.0, 0.25])
    cases = [
        ([1.0, 1.0, 1.0, 1.0, 1.0], p, 1e6, 2),    # the lowest lag on ties
        ([1.0, nan, 0.5, 0.5, 8.0], p, 1e6, 4),    # a NaN never wins
        ([1.0, nan, nan, nan, nan], p, 1e6, 0),    # p(0) = 0 excludes lag 0; nothing else is positive
        ([0.0, 0.0, 0.0, 0.0, 0.0], np.zeros(5), 1e6, 0),  # no positive score: none
        ([0.0, 0.0, 0.0, 0.0, 0.0], p, 1e6, 2),    # an all-zero mean scores the prior itself
        ([0.0, 0.0, 0.0, 0.0, 0.0], p, 0.0, 2),
        ([-1.0, -1.0, -1.0, -1.0, -1.0], p, 1e6, 0),  # negative scores never beat +0
        ([1.0, inf, 1.0, 1.0, 1.0], p, 1e6, 1),
        ([nan] * 5, p, 1e6, 0),                    # an empty clip's mean
    ]
    for m, pr, g, want in cases:
        assert loop(m, pr, g) == want, (m, want)
        assert int(pick(np.array([m]), pr, g)[0]) == want, (m, want)
    rng = np.random.default_rng(7)
    m = rng.standard_normal((50, 33)) * 1e-5
    m[rng.random(m.shape) < 0.1] = nan
    pr = tempo_ref.prior_ref(50.0, 33)
    assert [int(v) for v in pick(m, pr)] == [loop(r, pr) for r in m]


def test_tempogram_device_refusals():
    """Every refusal of mgx_tempogram_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    env, tab, win, out = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    names = ("env", "F", "f64", "tab", "S", "win", "W", "L", "norm", "out", "st")
    ok = dict(env=env, F=10, f64=0, tab=tab, S=2, win=win, W=8, L=8, norm=1, out=out, st=None)
    call = lambda **kw: L.mgx_tempogram_device(*[{**ok, **kw}[k] for k in names])
    assert b"envelope_f64" in refused(call(f64=2))
    for W in (0, 1, 1025, 2 ** 31):
        assert b"win_length" in refused(call(W=W, L=1))
    for nl in (0, 9, 2 ** 31):
        assert b"num_lags" in refused(call(L=nl))
    for norm in (2, 2 ** 31):
        assert b"norm" in refused(call(norm=norm))
    assert b"window is NULL" in refused(call(win=None))
    assert b"tempogram is NULL" in refused(call(out=None))
    assert b"same array as envelope" in refused(call(out=env))
    assert b"same array as window" in refused(call(out=win))
    assert b"frame_offsets is NULL" in refused(call(tab=None))
    assert b"envelope is NULL" in refused(call(env=None))
    # refused whatever the number of rows; with valid arguments no rows is MGX_OK, nothing launched
    refused(call(F=0, W=1))
    refused(call(F=0, norm=2))
    assert call(F=0) == 0 and call(F=0, env=None) == 0 and call(F=0, tab=None, S=0) == 0


def tempo_params(**kw):
    p = capi.TempoParams()
    capi.lib().mgx_tempo_params_init(ctypes.byref(p))
    p.win_length = p.num_lags = 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("struct_size", 20, b"struct_size"), ("struct_size", 0, b"struct_size"), ("win_length", 1, b"win_length"),
              ("win_length", 1025, b"win_length"), ("num_lags", 0, b"num_lags"), ("num_lags", 9, b"num_lags"), ("norm", 2, b"norm"),
              ("gain", -1.0, b"gain"), ("gain", math.inf, b"gain"), ("gain", math.nan, b"gain")]


def test_tempo_device_refusals():
    L = capi.lib()
    env, tab, win, pri, tg, sm, lg, ws = (ctypes.c_void_p(256 * k) for k in range(1, 9))
    names = ("env", "F", "f64", "tab", "S", "par", "win", "pri", "tg", "sm", "lg", "ws", "wsb", "st")
    ok = dict(env=env, F=10, f64=0, tab=tab, S=2, par=None, win=win, pri=pri, tg=tg, sm=sm, lg=lg, ws=ws, wsb=1 << 40, st=None)

    def call(params=None, **kw):
        a = {**ok, **kw}
        a["par"] = None if params == "null" else ctypes.byref(params if params is not None else tempo_params())
        return L.mgx_tempo_device(*[a[k] for k in names])
    assert b"params is NULL" in refused(call("null"))
    for field, value, word in BAD_PARAMS:
        assert word in refused(call(tempo_params(**{field: value}))), (field, value)
    assert b"envelope_f64" in refused(call(f64=2))
    assert b"window is NULL" in refused(call(win=None))
    assert b"frame_offsets is NULL" in refused(call(tab=None))
    assert b"envelope is NULL" in refused(call(env=None))
    assert b"all NULL" in refused(call(tg=None, sm=None, lg=None))
    assert b"without prior" in refused(call(pri=None))
    assert b"same array as envelope" in refused(call(tg=env))
    assert b"same array as window" in refused(call(tg=win))
    need = ctypes.c_uint64()
    assert L.mgx_tempo_workspace_bytes(10, 2, ctypes.byref(tempo_params()), 1, ctypes.byref(need)) == 0
    assert b"workspace" in refused(call(wsb=need.value - 1))
    assert b"workspace" in refused(call(ws=None))
    assert b"aligned" in refused(call(ws=ctypes.c_void_p(2048 + 128)))
    # without a tempogram output the call needs a pass of rows more
    more = ctypes.c_uint64()
    assert L.mgx_tempo_workspace_bytes(10, 2, ctypes.byref(tempo_params()), 0, ctypes.byref(more)) == 0
    assert more.value == need.value + 512 and b"workspace" in refused(call(tg=None, wsb=need.value))


def test_workspace_bytes():
    """The stated bytes: a multiple of 256, non-decreasing, and without a tempogram output bounded in num_frames x L
    by one pass of rows."""
    L = capi.lib()
    b = ctypes.c_uint64()
    up = lambda v: -(-v // 256) * 256

    def stated(F, S, nl, keep):
        S = S or 1
        return (up((S + 1) * 8) + up(S * nl * 8) + up((F // 256 + S + 1) * 5 * nl * 8) + up(S * 4 * nl * 8)
                + (0 if keep else up(min(F, 65536) * nl * 4)))
    for F, S, nl in ((0, 0, 1), (10, 2, 8), (70000, 3, 8), (262144, 512, 384), (10 ** 7, 1, 384)):
        for keep in (0, 1):
            assert L.mgx_tempo_workspace_bytes(F, S, ctypes.byref(tempo_params(win_length=max(nl, 2), num_lags=nl)), keep,
                                               ctypes.byref(b)) == 0
            assert b.value == stated(F, S, nl, keep) and b.value % 256 == 0, (F, S, nl, keep, b.value)
    assert up(65536 * 384 * 4) == 100663296
    p = tempo_params()
    assert b"bytes is NULL" in refused(L.mgx_tempo_workspace_bytes(10, 1, ctypes.byref(p), 0, None))
    assert b"keep_rows" in refused(L.mgx_tempo_workspace_bytes(10, 1, ctypes.byref(p), 2, ctypes.byref(b)))
    assert b"params is NULL" in refused(L.mgx_tempo_workspace_bytes(10, 1, None, 0, ctypes.byref(b)))
    for field, value, word in BAD_PARAMS:
        assert word in refused(L.mgx_tempo_workspace_bytes(10, 1, ctypes.byref(tempo_params(**{field: value})), 0, ctypes.byref(b)))


def test_tempo_host_refusals():
    """The parameters are checked ahead of the plan and the request, so these need no device."""
    L = capi.lib()
    h = np.ones(8, np.float32)
    pr = np.ones(8, np.float64)
    sm = np.zeros((1, 4, 8), np.float64)
    lg = np.zeros(1, np.uint32)
    fr = capi.FluxRequest()
    fr.struct_size = ctypes.sizeof(capi.FluxRequest)
    names = ("plan", "x", "nx", "st", "F", "tab", "S", "fr", "par", "win", "pri", "sm", "lg")
    ok = dict(plan=None, x=None, nx=0, st=None, F=0, tab=None, S=1, fr=ctypes.byref(fr), par=None, win=h.ctypes.data,
              pri=pr.ctypes.data, sm=sm.ctypes.data, lg=lg.ctypes.data)

    def call(params=None, **kw):
        a = {**ok, **kw}
        a["par"] = None if params == "null" else ctypes.byref(params if params is not None else tempo_params())
        return L.mgx_tempo_host(*[a[k] for k in names])
    assert b"params is NULL" in refused(call("null"))
    for field, value, word in BAD_PARAMS:
        assert word in refused(call(tempo_params(**{field: value}))), (field, value)
    assert b"num_signals is 0" in refused(call(S=0))
    assert b"flux is NULL" in refused(call(fr=None))
    assert b"window is NULL" in refused(call(win=None))
    assert b"both NULL" in refused(call(sm=None, lg=None))
    assert b"without prior" in refused(call(pri=None))
    assert call(pri=None, lg=None) != 0  # (the prior is the pick's alone; what refuses now is the request or the plan)
    assert b"without prior" not in capi.lib().mgx_last_error()
    refused(call())  # the request names no field of a NULL plan
