"""Onsets (mgx_peaks_device, mgx_onsets_host; include/meyda_gpu.h) as far as they can be checked on the host: the
numpy oracle against a per-row loop written from the definition, the structs and the exports, every refusal that
comes before a device call (the operator takes no plan; the host call checks its own arguments ahead of the plan),
and the workspace's bytes. No test here makes a launch."""
import ctypes

import numpy as np
import pytest

import peaks_ref
from meyda_amd import capi

E_INVALID = -1
NEW = ["mgx_peaks_workspace_bytes", "mgx_peaks_device", "mgx_onsets_host"]


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def direct(x, fo, pre_max, post_max, pre_avg, post_avg, delta, wait, fill):
    """The definition, row by row, in Python floats (IEEE float64)."""
    x = [float(v) for v in np.asarray(x).astype(np.float64)]
    F = len(x)
    bounds = [(0, F)] if fo is None else [(min(int(fo[s]), F), min(int(fo[s + 1]), F)) for s in range(len(fo) - 1)]
    mask, offsets, out = [fill] * F, [0], []
    for a, b in bounds:
        last = None
        for t in range(a, b):
            mask[t] = 0
            xc = lambda u: x[min(max(u, a), b - 1)]
            if any(xc(u) > x[t] for u in range(t - pre_max, t + post_max + 1)):
                continue
            m = 0.0
            for u in range(t - pre_avg, t + post_avg + 1):
                m += xc(u)
            m = float(np.float64(m) / np.float64(pre_avg + post_avg + 1))
            if not x[t] >= m + delta:
                continue
            if last is None or t - last > wait:
                last = t
                mask[t] = 1
                out.append(t)
        offsets.append(len(out))
    return np.array(mask, np.uint8), np.array(offsets, np.uint64), np.array(out, np.uint64)


TABLES = [None, [0, 150], [3, 3, 4, 6, 60, 147], [0, 0, 1, 2, 2, 150, 150], [10, 75, 139, 400]]
PARAM_SETS = [(0, 0, 0, 0, 0.0, 0), (0, 0, 0, 0, 0.0, 1), (3, 0, 10, 10, 0.07, 3), (3, 3, 5, 6, 0.0, 2), (64, 64, 64, 64, -0.5, 5),
              (1, 1, 0, 0, 0.0, 63), (2, 4, 1, 0, float("-inf"), 64), (0, 0, 3, 3, float("inf"), 0)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_oracle_against_the_definition(dtype, kind):
    """Tables with an empty signal, a one-row signal ([3, 4)), a signal shorter than every window ([4, 6)), rows of
    no signal on either side and entries above the rows; a quantised envelope of five integers has plateaus and ties."""
    rng = np.random.default_rng(7 if kind == "random" else 8)
    F = 150
    x = rng.standard_normal(F) if kind == "random" else rng.integers(0, 5, F).astype(np.float64)
    x = x.astype(dtype)
    for fo in TABLES:
        for ps in PARAM_SETS:
            kw = dict(zip(peaks_ref.PARAMS, ps))
            got = peaks_ref.peaks(x, fo, fill=9, **kw)
            want = direct(x, fo, *ps, fill=9)
            for g, w, name in zip(got, want, ("mask", "peak_offsets", "peaks")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, fo, ps)
    # every row of a constant signal is a candidate; wait thins them
    m, o, p = peaks_ref.peaks(np.ones(10, dtype), None, wait=3)
    assert p.tolist() == [0, 4, 8] and o.tolist() == [0, 3] and m.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0]


def test_oracle_rules():
    nan, inf = np.nan, np.inf
    #            0    1    2    3    4    5     6    7    8    9
    x = np.array([1.0, 5.0, nan, 7.0, 2.0, -inf, inf, 0.0, 3.0, 9.0])
    # a NaN row is no peak, a NaN neighbour does not block the maximum ...
    m, o, p = peaks_ref.peaks(x, [0, 5, 10], pre_max=1, post_max=1)
    assert p.tolist() == [1, 3, 6, 9] and o.tolist() == [0, 2, 4]
    # ... and a NaN in the averaging window rejects the row, in its own signal alone
    m, o, p = peaks_ref.peaks(x, [0, 5, 10], pre_avg=1, post_avg=0, delta=-100.0)
    assert m[:5].tolist() == [1, 1, 0, 0, 1]
    assert m[5:].tolist() == [1, 0, 0, 1, 1]  # -inf >= -inf - 100; inf against a mean of NaN (-inf + inf); 0 against inf
    # rows of no signal keep the fill, an empty signal has no peaks
    m, o, p = peaks_ref.peaks(x, [1, 1, 2], fill=7)
    assert m.tolist() == [7, 1] + [7] * 8 and o.tolist() == [0, 0, 1] and p.tolist() == [1]


def test_structs_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    assert hasattr(capi, "peaks_torch") and hasattr(capi, "peaks_device") and hasattr(capi.Plan, "onsets")
    # six uint32 and a double; two uint32, three pointers, a uint64, two pointers
    assert ctypes.sizeof(capi.PeakParams) == 32 and capi.PeakParams.delta.offset == 24 and capi.PeakParams.wait.offset == 20
    assert ctypes.sizeof(capi.PeakOutputs) == 56
    assert [getattr(capi.PeakOutputs, k).offset for k in ("mask", "peak_offsets", "peaks", "capacity", "starts", "peak_starts")] == \
        [8, 16, 24, 32, 40, 48]
    assert capi.PEAK_MAX_REACH == 64
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"onsets") == -1 and capi.lib().mgx_feature_index(b"peaks") == -1
    assert ctypes.sizeof(capi.FluxRequest) == 32 and ctypes.sizeof(capi.DeltaSummaries) == 24


def outputs(**kw):
    o = capi.PeakOutputs()
    o.struct_size = ctypes.sizeof(capi.PeakOutputs)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_operator_refusals():
    """Every refusal of mgx_peaks_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    env, tb, ws, mask, offs, pk, st, pst = (256 * k for k in range(1, 9))
    full = dict(mask=mask, peak_offsets=offs, peaks=pk, capacity=10)

    def call(params=None, out=None, env=env, F=10, f64=0, tb=tb, S=2, ws=ws, wsb=1 << 20):
        params = capi.peak_params() if params is None else params
        out = outputs(**full) if out is None else out
        return L.mgx_peaks_device(env, F, f64, tb, S, ctypes.byref(params), ctypes.byref(out), ws, wsb, None)
    for wrong in (0, 24, 40):
        p = capi.peak_params()
        p.struct_size = wrong
        assert b"mgx_peak_params.struct_size" in refused(call(params=p))
        o = outputs(**full)
        o.struct_size = wrong
        assert b"mgx_peak_outputs.struct_size" in refused(call(out=o))
    for name in ("pre_max", "post_max", "pre_avg", "post_avg"):
        for v in (65, 2 ** 31):
            assert name.encode() in refused(call(params=capi.peak_params(**{name: v})))
        assert call(params=capi.peak_params(**{name: 64}), F=0, out=outputs(mask=mask)) == 0
    assert b"NaN" in refused(call(params=capi.peak_params(delta=float("nan"))))
    assert b"envelope_f64" in refused(call(f64=2))
    assert b"all NULL" in refused(call(out=outputs()))
    assert b"capacity" in refused(call(out=outputs(peaks=pk, capacity=0)))
    assert b"without starts" in refused(call(out=outputs(peaks=pk, capacity=4, peak_starts=pst)))
    assert b"without peaks" in refused(call(out=outputs(mask=mask, starts=st, peak_starts=pst)))
    assert b"frame_offsets" in refused(call(tb=None))
    assert b"envelope is NULL" in refused(call(env=None))
    need = capi.peaks_workspace_bytes(10, 2)
    assert need > 0
    assert b"workspace" in refused(call(wsb=need - 1))
    assert b"workspace" in refused(call(ws=None))
    assert b"aligned" in refused(call(ws=ws + 128))
    assert L.mgx_peaks_device(env, 10, 0, tb, 2, None, ctypes.byref(outputs(**full)), ws, need, None) == E_INVALID
    assert L.mgx_peaks_device(env, 10, 0, tb, 2, ctypes.byref(capi.peak_params()), None, ws, need, None) == E_INVALID
    # refused whatever the number of rows; with valid arguments and no offsets to clear, no rows is MGX_OK, nothing launched
    refused(call(F=0, f64=2))
    refused(call(F=0, out=outputs()))
    refused(call(F=0, params=capi.peak_params(wait=1, pre_avg=65)))
    assert call(F=0, out=outputs(mask=mask), ws=None, wsb=0) == 0
    assert call(F=0, out=outputs(mask=mask), env=None, tb=None, S=0, ws=None, wsb=0) == 0


def test_host_call_refusals_ahead_of_the_plan():
    """mgx_onsets_host checks the picker's arguments before the flux call's, and that one its request before the plan."""
    L = capi.lib()
    N = 256
    x = np.zeros(N, np.float32)
    st = np.zeros(1, np.uint64)
    fo = np.array([0, 1], np.uint64)
    offs = np.full(2, 7, np.uint64)
    pk = np.full(4, 7, np.uint64)
    req = capi.FluxRequest()
    req.struct_size = ctypes.sizeof(capi.FluxRequest)
    req.field, req.mode, req.lag = 19, 0, 1

    def call(params=None, S=1, flux=req, offsets=offs.ctypes.data, peaks=pk.ctypes.data, cap=4):
        params = capi.peak_params() if params is None else params
        return L.mgx_onsets_host(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, S, None if flux is None else ctypes.byref(flux),
                                 ctypes.byref(params), offsets, peaks, cap)
    p = capi.peak_params()
    p.struct_size = 24
    assert b"mgx_peak_params.struct_size" in refused(call(params=p))
    assert b"post_avg" in refused(call(params=capi.peak_params(post_avg=65)))
    assert b"NaN" in refused(call(params=capi.peak_params(delta=float("nan"))))
    assert b"num_signals" in refused(call(S=0))
    assert b"flux is NULL" in refused(call(flux=None))
    assert b"peak_offsets" in refused(call(offsets=None))
    assert b"capacity" in refused(call(peaks=None, cap=4))
    assert b"capacity" in refused(call(cap=0))
    bad = capi.FluxRequest()
    bad.struct_size, bad.field, bad.mode, bad.lag = 24, 19, 0, 1
    assert b"mgx_flux_request.struct_size" in refused(call(flux=bad))
    bad.struct_size, bad.lag = 32, 9
    assert b"lag" in refused(call(flux=bad))
    bad.lag, bad.field = 1, 3
    assert b"field" in refused(call(flux=bad), -3)
    # a request that names neither array is this call's own, and reaches the plan; so does the count-only form
    assert b"NULL plan" in refused(call())
    assert b"NULL plan" in refused(call(peaks=None, cap=0))
    assert (offs == 7).all() and (pk == 7).all()  # a refused call writes nothing
    # ... while the summary call still refuses such a request
    so = capi.SummaryOutputs()
    so.struct_size = ctypes.sizeof(capi.SummaryOutputs)
    assert b"both NULL" in refused(L.mgx_summarize_flux_host(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, 1, None, None,
                                                             ctypes.byref(so), None, ctypes.byref(req), 1))


def test_workspace_bytes():
    L = capi.lib()
    assert L.mgx_peaks_workspace_bytes(10, 1, None) == E_INVALID
    prev = 0
    for F in [0, 1, 63, 64, 65, 300, 65536, 65537, 262144, 2 ** 31 + 5, 2 ** 40]:
        row = [capi.peaks_workspace_bytes(F, S) for S in (0, 1, 2, 1000, 2 ** 33)]
        assert all(b % 256 == 0 for b in row)
        assert all(b1 >= b0 for b0, b1 in zip(row, row[1:]))
        assert row[0] >= prev
        if F > 0:
            assert row[0] >= 2 * ((F + 63) // 64) * 8  # two bitmaps of one bit per row at the least
        prev = row[-1]
    assert capi.peaks_workspace_bytes(0, 0) == 0
