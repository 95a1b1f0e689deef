"""Beats (mgx_beat_tables, mgx_beats_workspace_bytes, mgx_beats_device, mgx_beats_host; include/meyda_gpu.h) as far as
they can be checked on the host: the structs and the exports, the tables against the numpy statement
(tests/beat_ref.py), lo(p), the statement's vectorised form against its plain loops on the click trains and on every
rule, and every refusal that comes before a launch (the device call takes no plan, and the host call checks its
parameters ahead of the plan)."""
import ctypes
import math

import numpy as np
import pytest

import beat_ref
from meyda_amd import capi
from test_gpu_tempo import clicks

E_INVALID = -1
NEW = ["mgx_beat_params_init", "mgx_beat_tables", "mgx_beats_workspace_bytes", "mgx_beats_device", "mgx_beats_host"]


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def test_structs_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    assert ctypes.sizeof(capi.BeatParams) == 16 and ctypes.sizeof(capi.PeakOutputs) == 56
    assert capi.BEAT_MAX_PERIOD == 1023 == beat_ref.MAX_PERIOD
    p = capi.BeatParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    capi.lib().mgx_beat_params_init(ctypes.byref(p))
    assert (p.struct_size, p.max_period, p.trim, p.reserved) == (16, 1023, 1, 0)
    capi.lib().mgx_beat_params_init(None)  # nothing to set: no fault
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"beats") == -1


@pytest.mark.parametrize("P", [1, 2, 7, 128, 1023])
def test_tables(P):
    """penalty within a relative 4 x 2^-52 (two libms' logs), -Infinity in the same places; gauss with equal bits after
    the float32 rounding, which hides a last place of float64 except on a rounding boundary."""
    gauss, penalty = capi.beat_tables(P)
    rg, rp = beat_ref.tables(P)
    assert gauss.dtype == np.float32 and gauss.shape == ((P + 1) * (P + 2) // 2,)
    assert penalty.dtype == np.float64 and penalty.shape == ((P + 1) ** 2,)
    inf = np.isneginf(rp)
    assert np.array_equal(np.isneginf(penalty), inf) and np.isfinite(penalty[~inf]).all()
    assert (np.abs(penalty[~inf] - rp[~inf]) <= 4 * 2.0 ** -52 * np.abs(rp[~inf])).all()
    print("penalty entries that differ at all: %d of %d" % (int((penalty[~inf] != rp[~inf]).sum()), int((~inf).sum())))
    assert np.array_equal(gauss.view(np.uint32), rg.view(np.uint32)), int((gauss != rg).sum())
    assert np.array_equal(gauss == 0, rg == 0) and not np.signbit(gauss).any()
    print("gauss entries that differ at all: %d of %d" % (int((gauss != rg).sum()), gauss.size))
    # entry 0 and the row of p = 0; every period's first weight is 1 and its penalty at d = p is -0
    assert gauss[0] == 1.0 and np.isneginf(penalty[0])
    for p in {1, P}:
        assert gauss[p * (p + 1) // 2] == 1.0 and penalty[p * p + p] == 0.0
        assert np.isneginf(penalty[p * p:p * p + beat_ref.lo(p)]).all() and np.isfinite(penalty[p * p + beat_ref.lo(p):(p + 1) ** 2]).all()
    # the tightness scales the penalty
    if P == 7:
        assert np.array_equal(capi.beat_tables(P, 50.0)[1][~inf] * 2.0, penalty[~inf])


def test_lo():
    assert [beat_ref.lo(p) for p in (1, 2, 3, 5, 7, 9)] == [1, 1, 2, 2, 4, 4]
    for p in range(1, 1024):
        assert beat_ref.lo(p) == max(1, int(np.round(p / 2)))


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)) and u.dtype == v.dtype
               for u, v in zip(a, b))


@pytest.fixture(scope="module")
def tables():
    return beat_ref.tables(128)


TRAINS = [(1500, 86, 100, 86, 17), (900, 60, 101, 60, 15), (1000, 43, 103, 43, 23), (1000, 43, 103, 86, 11), (300, 7, 105, 7, None),
          (130, 5, 106, 5, None), (65, 3, 107, 3, None), (40, 2, 108, 2, None), (9, 1, 109, 1, None)]


@pytest.mark.parametrize("rows,period,seed,p,count", TRAINS)
def test_the_two_statements_agree_on_the_trains(tables, rows, period, seed, p, count):
    x = clicks(rows, period, seed)
    on = np.arange(period // 2, rows, period)
    for trim in (1, 0):
        a, b = beat_ref.signal_ref(x, p, 128, *tables, trim), beat_ref.signal_loop(x, p, 128, *tables, trim)
        assert same(a, b), (rows, p, trim)
        if trim and p == period:
            assert np.array_equal(a[2], on)  # a beat on every click
        if trim and count is not None:
            assert a[2].size == count
        if trim and p == 2 * period:
            assert np.array_equal(a[2], on[1::2]) or np.array_equal(a[2], on[0::2][:count])  # every second click
    # without the trim the 86-row and the 43-row train gain one trailing beat
    if (rows, p) in ((1500, 86), (1000, 43)):
        assert beat_ref.signal_ref(x, p, 128, *tables, 0)[2].size == count + 1


def tie_case(tables):
    """A clip where ties decide the beats, at p = 4: every distance is made to cost the same, and 40 silent rows lie
    between two click trains. There the local score is +0, so the rows 2 .. 8 behind the last click all inherit its
    score less the cost: equal values, and from then on every row chooses among equals. Returns (x, gauss, penalty)."""
    gauss, penalty = tables
    penalty = penalty.copy()
    penalty[4 * 4 + 2:4 * 4 + 9] = -1.0
    return np.concatenate([clicks(40, 4, 3), np.zeros(40, np.float32), clicks(40, 4, 4)]), gauss, penalty


def test_the_two_statements_agree_on_the_rules(tables):
    both = lambda x, p, trim=1, P=128: (beat_ref.signal_ref(x, p, P, *tables, trim), beat_ref.signal_loop(x, p, P, *tables, trim))
    x = clicks(200, 10, 1)

    def none(x, p, P=128):
        a, b = both(x, p, P=P)
        assert same(a, b) and a[2].size == 0
        return a
    # n < 2, p = 0, p > P: no beats, +0 in both scores
    for v, p, P in ((x[:1], 10, 128), (x[:0], 10, 128), (x, 0, 128), (x, 129, 128), (x, 11, 10)):
        a = none(v, p, P)
        assert not a[0].any() and not a[1].any() and a[0].size == v.size
    # silence and a constant: sd is not positive
    none(np.zeros(100, np.float32), 10)
    none(np.full(100, 3.0, np.float32), 10)
    # a NaN row and an infinite row: sd is not finite
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[50] = bad
        none(y, 10)
    # a square that overflows: sd is infinite; and the largest quotient there can be, one row far above the others,
    # stays near sqrt(n): xn is always finite
    y = np.zeros(300, np.float64)
    y[::10] = 1e-30
    y[5] = 1e300
    none(y, 10)
    y[5] = 1e150
    a, b = both(y, 10)
    assert same(a, b) and np.isfinite(a[0]).all() and a[0].max() <= 2 * math.sqrt(300)
    # a tie in the recurrence, where the larger d wins
    z, g, pen2 = tie_case(tables)
    a, b = beat_ref.signal_ref(z, 4, 128, g, pen2), beat_ref.signal_loop(z, 4, 128, g, pen2)
    assert same(a, b)
    inside = a[2][(a[2] >= 46) & (a[2] < 74)]
    assert list(inside) == [50, 58, 66]  # steps of 2 p = 8, the largest distance; the smallest would be 2
    # an even and an odd count of local maxima
    seen = set()
    for seed in range(40):
        w = clicks(97, 6, 500 + seed)
        a, b = both(w, 6)
        assert same(a, b)
        C = a[1]
        m = int(((C[1:-1] > C[:-2]) & (C[1:-1] >= C[2:])).sum() + (C[-1] > C[-2]))
        seen.add(m & 1)
    assert seen == {0, 1}
    # trim 0 against 1: the untrimmed beats hold the trimmed ones
    a1, a0 = both(x, 10, 1)[0], both(x, 10, 0)[0]
    assert same(both(x, 10, 0)[0], both(x, 10, 0)[1]) and set(a1[2]) <= set(a0[2]) and a0[2].size >= a1[2].size > 0
    # a float64 envelope is taken as it is
    x64 = x.astype(np.float64) * (1 + 2.0 ** -40)
    assert same(*both(x64, 10))


def test_whole_array(tables):
    """beats_ref: the table limited to the rows, rows of no signal keep the fill."""
    x = np.concatenate([np.zeros(3, np.float32), clicks(200, 10, 1), clicks(90, 5, 2), np.ones(2, np.float32)])
    fo = [3, 203, 203, 293]
    r = beat_ref.beats_ref(x, [10, 7, 5], fo, 128, *tables, fill=-1.0, mask_fill=9)
    l = beat_ref.beats_ref(x, [10, 7, 5], fo, 128, *tables, fill=-1.0, mask_fill=9, one=beat_ref.signal_loop)
    assert all(np.array_equal(r[k].view(np.uint8), l[k].view(np.uint8)) for k in r)
    assert (r["mask"][:3] == 9).all() and (r["mask"][293:] == 9).all() and (r["local_score"][:3] == -1.0).all()
    assert r["peak_offsets"][1] == r["peak_offsets"][2] and r["peaks"].size == r["peak_offsets"][3] == r["mask"][3:293].sum()
    assert (np.diff(r["peaks"].astype(np.int64)) > 0).all()


def test_table_refusals():
    L = capi.lib()
    g = (ctypes.c_float * 8)()
    w = (ctypes.c_double * 16)()
    for P in (0, 1024, 2 ** 31):
        assert b"max_period" in refused(L.mgx_beat_tables(P, 100.0, g, w))
    for v in (0.0, -1.0, math.inf, math.nan):
        assert b"tightness" in refused(L.mgx_beat_tables(2, v, g, w))
    assert b"gauss is NULL" in refused(L.mgx_beat_tables(2, 100.0, None, w))
    assert b"penalty is NULL" in refused(L.mgx_beat_tables(2, 100.0, g, None))
    assert L.mgx_beat_tables(2, 100.0, g, w) == 0 and g[0] == 1.0 and g[6] == 0.0 and g[7] == 0.0 and w[9] == 0.0
    with pytest.raises(capi.MgxError):
        capi.beat_tables(0)
    with pytest.raises(capi.MgxError):
        capi.beat_tables(1024)


def beat_params(**kw):
    p = capi.BeatParams()
    capi.lib().mgx_beat_params_init(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [("struct_size", 12, b"struct_size"), ("struct_size", 0, b"struct_size"), ("max_period", 0, b"max_period"),
              ("max_period", 1024, b"max_period"), ("trim", 2, b"trim"), ("trim", 2 ** 31, b"trim")]


def peak_outputs(**kw):
    o = capi.PeakOutputs()
    o.struct_size = ctypes.sizeof(capi.PeakOutputs)
    o.mask, o.peak_offsets, o.peaks, o.capacity = 256 * 20, 256 * 21, 256 * 22, 10
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_beats_device_refusals():
    """Every refusal of mgx_beats_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    env, tab, per, gs, pn, ls, cs, ws = (ctypes.c_void_p(256 * k) for k in range(1, 9))
    names = ("env", "F", "f64", "tab", "S", "per", "par", "gs", "pn", "ls", "cs", "out", "ws", "wsb", "st")
    ok = dict(env=env, F=10, f64=0, tab=tab, S=2, per=per, par=None, gs=gs, pn=pn, ls=ls, cs=cs, out=None, ws=ws, wsb=1 << 40, st=None)

    def call(params=None, out=None, **kw):
        a = {**ok, **kw}
        a["par"] = None if params == "null" else ctypes.byref(params if params is not None else beat_params())
        a["out"] = None if out == "null" else ctypes.byref(out if out is not None else peak_outputs())
        return L.mgx_beats_device(*[a[k] for k in names])
    assert b"params is NULL" in refused(call("null"))
    for field, value, word in BAD_PARAMS:
        assert word in refused(call(beat_params(**{field: value}))), (field, value)
    assert b"out is NULL" in refused(call(out="null"))
    assert b"mgx_peak_outputs.struct_size" in refused(call(out=peak_outputs(struct_size=48)))
    assert b"envelope_f64" in refused(call(f64=2))
    assert b"period is NULL" in refused(call(per=None))
    assert b"gauss is NULL" in refused(call(gs=None))
    assert b"penalty is NULL" in refused(call(pn=None))
    assert b"all NULL" in refused(call(out=peak_outputs(mask=None, peak_offsets=None, peaks=None)))
    assert b"capacity 0" in refused(call(out=peak_outputs(capacity=0)))
    assert b"without starts" in refused(call(out=peak_outputs(peak_starts=256 * 30)))
    assert b"without peaks" in refused(call(out=peak_outputs(peak_starts=256 * 30, starts=256 * 31, peaks=None)))
    assert b"frame_offsets is NULL" in refused(call(tab=None))
    assert b"envelope is NULL" in refused(call(env=None))
    need = ctypes.c_uint64()
    assert L.mgx_beats_workspace_bytes(10, 2, ctypes.byref(need)) == 0 and need.value > 0
    assert b"workspace" in refused(call(wsb=need.value - 1))
    assert b"workspace" in refused(call(ws=None))
    assert b"aligned" in refused(call(ws=ctypes.c_void_p(2048 + 128)))
    # refused whatever the number of rows
    refused(call(beat_params(trim=2), F=0))
    refused(call(F=0, per=None))
    # the optional scores are optional
    assert b"workspace" in refused(call(ls=None, cs=None, wsb=0))


def test_workspace_bytes():
    L = capi.lib()
    b = ctypes.c_uint64()
    assert b"bytes is NULL" in refused(L.mgx_beats_workspace_bytes(10, 1, None))
    assert capi.beats_workspace_bytes(0, 0) == 0 and capi.beats_workspace_bytes(0, 5) == 0
    last = 0
    for F in (1, 63, 64, 65, 1000, 65536, 10 ** 6, 10 ** 7):
        row = 0
        for S in (0, 1, 2, 100, 10 ** 4, 10 ** 6):
            v = capi.beats_workspace_bytes(F, S)
            assert v % 256 == 0 and v >= row and v >= capi.peaks_workspace_bytes(F, S) + 20 * F + 16 * max(S, 1)
            row = v
        assert capi.beats_workspace_bytes(F, 1) >= last
        last = capi.beats_workspace_bytes(F, 1)
    assert capi.beats_workspace_bytes(10 ** 6, 1) < 22 * 10 ** 6  # about twenty bytes a row


def tempo_params(**kw):
    p = capi.TempoParams()
    capi.lib().mgx_tempo_params_init(ctypes.byref(p))
    p.win_length = p.num_lags = 8
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_beats_host_refusals():
    """The parameters are checked ahead of the plan and the request, so these need no device."""
    L = capi.lib()
    h = np.ones(8, np.float32)
    pr = np.ones(8, np.float64)
    gs, pn = capi.beat_tables(7)
    lg = np.zeros(1, np.uint32)
    off = np.zeros(2, np.uint64)
    rows = np.zeros(4, np.uint64)
    fr = capi.FluxRequest()
    fr.struct_size = ctypes.sizeof(capi.FluxRequest)
    names = ("plan", "x", "nx", "st", "F", "tab", "S", "fr", "tp", "win", "pri", "bp", "gs", "pn", "lg", "off", "rows", "cap")
    ok = dict(plan=None, x=None, nx=0, st=None, F=0, tab=None, S=1, fr=ctypes.byref(fr), tp=None, win=h.ctypes.data, pri=pr.ctypes.data,
              bp=None, gs=gs.ctypes.data, pn=pn.ctypes.data, lg=lg.ctypes.data, off=off.ctypes.data, rows=rows.ctypes.data, cap=4)

    def call(tp=None, bp=None, **kw):
        a = {**ok, **kw}
        a["tp"] = None if tp == "null" else ctypes.byref(tp if tp is not None else tempo_params())
        a["bp"] = None if bp == "null" else ctypes.byref(bp if bp is not None else beat_params(max_period=7))
        return L.mgx_beats_host(*[a[k] for k in names])
    assert b"params is NULL" in refused(call("null"))
    assert b"params is NULL" in refused(call(bp="null"))
    assert b"win_length" in refused(call(tempo_params(win_length=1)))
    assert b"gain" in refused(call(tempo_params(gain=math.nan)))
    for field, value, word in BAD_PARAMS:
        assert word in refused(call(bp=beat_params(**{field: value}))), (field, value)
    assert b"max_period" in refused(call(bp=beat_params(max_period=6)))  # lags reach 7
    assert b"num_signals is 0" in refused(call(S=0))
    assert b"flux is NULL" in refused(call(fr=None))
    assert b"window is NULL" in refused(call(win=None))
    assert b"prior is NULL" in refused(call(pri=None))
    assert b"gauss is NULL" in refused(call(gs=None))
    assert b"penalty is NULL" in refused(call(pn=None))
    assert b"peak_offsets is NULL" in refused(call(off=None))
    assert b"peaks is NULL" in refused(call(rows=None))
    assert b"capacity 0" in refused(call(cap=0))
    assert call(lg=None) != 0 and b"flux[0]" in capi.lib().mgx_last_error()  # (the lag output is optional: the request refuses)
    refused(call())  # the request names no field of a NULL plan
