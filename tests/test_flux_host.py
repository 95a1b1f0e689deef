"""Spectral flux (mgx_flux_device, mgx_summarize_flux_*; include/meyda_gpu.h) as far as it can be checked on the
host: the numpy oracle against an exact sum, the struct and the exports, every refusal that comes before a device
call (the operator takes no plan, and the requests are checked ahead of the plan as the summary and delta structs
are), and the workspace's bytes. The checks that read the plan's sizes need a plan, and a plan needs a device: those
tests make no launch, and are skipped where mgx_plan_create finds no device."""
import ctypes
import math

import numpy as np
import pytest

import flux_ref
from meyda_amd import capi

N = 256
E_INVALID, E_UNSUPPORTED = -1, -3
NEW = ["mgx_flux_device", "mgx_summarize_flux_workspace_bytes", "mgx_summarize_flux_device", "mgx_summarize_flux_host"]


def summary(**ptrs):
    s = capi.SummaryOutputs()
    s.struct_size = ctypes.sizeof(capi.SummaryOutputs)
    for k, v in ptrs.items():
        setattr(s, k, v)
    return s


def requests(*rs):
    """A FluxRequest array of dicts(field, mode, lag, per_frame, summary), struct_size set."""
    a = (capi.FluxRequest * max(len(rs), 1))()
    for i, r in enumerate(rs):
        a[i].struct_size = ctypes.sizeof(capi.FluxRequest)
        a[i].field, a[i].mode, a[i].lag = r.get("field", 14), r.get("mode", 0), r.get("lag", 1)
        a[i].per_frame, a[i].summary = r.get("per_frame"), r.get("summary")
    return a


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


@pytest.mark.parametrize("cols", [1, 13, 40, 63, 64, 65, 129, 2048])
def test_oracle_against_an_exact_sum(cols):
    """Every term is non-negative, and a value passes through at most ceil(cols / 64) - 1 additions of its partial
    and 6 halvings: the ordered sum is within (ceil(cols / 64) + 5) 2^-53, relatively, of the exact sum of the
    rounded terms, which math.fsum gives. The L2 mode is compared before its root."""
    rng = np.random.default_rng(cols)
    F, lag = 24, 2
    x = rng.standard_normal((F, cols)) * 2.0 ** rng.integers(-20, 21, (F, cols))
    x[5] = x[3]  # a row equal to its earlier row: flux exactly 0
    bound = (-(-cols // 64) + 5) * 2.0 ** -53
    for mode in (flux_ref.RECTIFIED, flux_ref.L1, flux_ref.L2):
        S, written = flux_ref.sums(x, None, mode, lag)
        assert written.all() and S[0] == 0 and S[5] == 0 and (mode == flux_ref.RECTIFIED or (S[1:5] > 0).all())
        for t in range(F):
            p = max(t - lag, 0)
            exact = math.fsum(flux_ref.terms(x[t], x[p], mode).tolist())
            assert abs(S[t] - exact) <= bound * exact, (mode, t, S[t], exact)
        got = flux_ref.flux(x.astype(np.float32), None, mode, lag)
        assert got.dtype == np.float32 and got[0] == 0


def test_oracle_rules():
    inf = np.inf
    x = np.array([[1.0, -inf, 2.0], [1.0, -inf, 5.0], [np.nan, -inf, 5.0], [3.0, -inf, 1.0], [inf, -inf, 1.0], [9.0, 9.0, 9.0]])
    fo = [1, 1, 5, 5]  # row 0 and row 5 belong to no signal; signals 0 and 2 are empty
    r = flux_ref.flux(x, fo, "rectified", 1, fill=7.0)
    assert r[0] == 7 and r[5] == 7 and r[1] == 0 and np.isnan(r[2]) and np.isnan(r[3]) and r[4] == inf
    a = flux_ref.flux(x, fo, "l1", 2, fill=7.0)
    assert a[1] == 0 and np.isnan(a[2]) and a[3] == 2.0 + 4.0 and np.isnan(a[4])
    q = flux_ref.flux(x[:2], None, "l2", 1)
    assert q[0] == 0 and q[1] == 3.0


def test_struct_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    # four uint32, two pointers
    assert ctypes.sizeof(capi.FluxRequest) == 32
    assert capi.FluxRequest.per_frame.offset == 16 and capi.FluxRequest.summary.offset == 24
    assert capi.FLUX_MAX_LAG == 8 and capi.FLUX_MAX_REQUESTS == 4 and capi.FLUX_MODES == {"rectified": 0, "l1": 1, "l2": 2}
    # not a feature, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"spectralFlux") == -1 and capi.lib().mgx_feature_index(b"flux") == -1
    assert ctypes.sizeof(capi.AuxOutputs) == 16 and ctypes.sizeof(capi.DeltaSummaries) == 24


def test_operator_refusals():
    """Every refusal of mgx_flux_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    rows, out, tb = (ctypes.c_void_p(256 * k) for k in (1, 2, 3))
    names = ("rows", "F", "cols", "f64", "tb", "S", "mode", "lag", "out", "st")
    call = lambda **kw: L.mgx_flux_device(*[{**dict(rows=rows, F=10, cols=13, f64=0, tb=tb, S=2, mode=0, lag=1, out=out, st=None),
                                             **kw}[k] for k in names])
    assert b"cols" in refused(call(cols=0))
    for m in (3, 4, 2 ** 31):
        assert b"mode" in refused(call(mode=m))
    for lag in (0, 9, 2 ** 31):
        assert b"lag" in refused(call(lag=lag))
    assert b"rows_f64" in refused(call(f64=2))
    assert b"flux is NULL" in refused(call(out=None))
    assert b"own array" in refused(call(out=rows))
    assert b"frame_offsets" in refused(call(tb=None))
    assert b"rows is NULL" in refused(call(rows=None))
    # refused whatever the number of rows; with valid arguments no rows is MGX_OK, nothing launched
    refused(call(F=0, lag=0))
    refused(call(F=0, cols=0))
    refused(call(F=0, out=None))
    assert call(F=0) == 0 and call(F=0, rows=None, tb=None, S=0) == 0


def test_request_refusals_ahead_of_the_plan():
    """The requests, like the summary and delta structs, are checked before the plan is looked at; then a NULL plan is."""
    L = capi.lib()
    x = np.zeros(N, np.float32)
    st = np.zeros(1, np.uint64)
    fo = np.array([0, 1], np.uint64)
    dst = np.full(16, 7.0)
    col = np.full(4, 7.0, np.float32)
    b = ctypes.c_uint64(99)
    base = summary()
    D, C = dst.ctypes.data, col.ctypes.data

    def calls(S):
        host = lambda s, r, n: L.mgx_summarize_flux_host(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, S, None, None, s,
                                                         None, r, n)
        dev = lambda s, r, n: L.mgx_summarize_flux_device(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, S, None, None, s,
                                                          None, r, n, None, 0, None)
        size = lambda s, r, n: L.mgx_summarize_flux_workspace_bytes(None, None, None, s, None, r, n, 1, S, ctypes.byref(b))
        return host, dev, size
    for call in calls(1):
        ok = dict(summary=D, per_frame=C)
        assert b"summary is NULL" in refused(call(None, requests(ok), 1))
        assert b"num_flux" in refused(call(ctypes.byref(base), requests(ok, ok, ok, ok, ok), 5))
        assert b"flux is NULL" in refused(call(ctypes.byref(base), None, 1))
        for wrong in (0, 24, 40):
            r = requests(ok, ok)
            r[1].struct_size = wrong
            assert b"mgx_flux_request.struct_size" in refused(call(ctypes.byref(base), r, 2))
        for m in (3, 2 ** 31):
            assert b"mode" in refused(call(ctypes.byref(base), requests(dict(ok, mode=m)), 1))
        for lag in (0, 9):
            assert b"lag" in refused(call(ctypes.byref(base), requests(ok, dict(ok, lag=lag)), 2))
        assert b"both NULL" in refused(call(ctypes.byref(base), requests(dict()), 1))
        # the scalars, the complex spectrum and anything beyond the registry have no flux
        for field in (0, 12, 17, 18, 20, 2 ** 31):
            assert b"field" in refused(call(ctypes.byref(base), requests(dict(ok, field=field)), 1), E_UNSUPPORTED)
        # ... and valid ones reach the plan
        for field in (13, 14, 15, 16, 19):
            assert b"NULL plan" in refused(call(ctypes.byref(base), requests(dict(ok, field=field, mode=2, lag=8)), 1))
        assert b"NULL plan" in refused(call(ctypes.byref(base), requests(dict(per_frame=C)), 1))
        assert b"NULL plan" in refused(call(ctypes.byref(base), None, 0))  # (no request: the deltas call, which says the same)
    for call in calls(0):
        assert b"num_signals" in refused(call(ctypes.byref(base), requests(dict(summary=D)), 1))
        assert b"NULL plan" in refused(call(ctypes.byref(base), requests(dict(per_frame=C)), 1))
    assert (dst == 7.0).all() and (col == 7.0).all() and b.value == 99  # a refused call writes nothing


@pytest.fixture(scope="module")
def plan():
    if capi.device_count() == 0:
        pytest.skip("mgx_plan_create needs a device (these checks make no launch)")
    p = capi.Plan(buffer_size=N, num_mel_bands=40)
    yield p
    p.close()


def test_workspace_bytes(plan):
    S = 5
    alloc = lambda shape: np.empty(shape)
    _, so = plan._summary_outputs(S, ["rms", "mfcc", "amplitudeSpectrum"], alloc)
    _, empty = plan._summary_outputs(S, [], alloc)
    _, _, ds = plan._delta_summaries(S, ["mfcc", "melBands"], (2, 2), alloc)
    _, none = plan._host_outputs(0, [])
    _, some = plan._host_outputs(1, ["melBands"])
    dst, col = np.empty((S, 4)), np.empty(1, np.float32)
    D, C = dst.ctypes.data, col.ctypes.data
    amp, mel, power = 15, 19, 16
    size = plan.summarize_flux_workspace_bytes
    prev = {}
    for F in [0, 1, 255, 256, 257, 5000]:
        for o in (none, some):
            for d in (None, ds):
                # no request: the deltas call's bytes
                assert size(o, so, d, None, 0, F, S) == plan.summarize_deltas_workspace_bytes(o, so, d, F, S)
        cases = {
            "pooled_field": (none, so, None, requests(dict(field=amp, summary=D))),
            "pooled_field_col": (none, so, None, requests(dict(field=amp, per_frame=C))),
            "new_field": (none, so, None, requests(dict(field=power, summary=D))),
            "two_of_one_field": (none, so, None, requests(dict(field=power, summary=D), dict(field=power, mode=2, lag=8, summary=D))),
            "delta_field": (none, so, ds, requests(dict(field=mel, summary=D))),
            "per_frame_field": (some, empty, None, requests(dict(field=mel, summary=D))),
            "no_base": (none, empty, None, requests(dict(field=mel, summary=D))),
        }
        for key, (o, s, d, r) in cases.items():
            b = size(o, s, d, r, len(r), F, S)
            assert b % 256 == 0 and b >= prev.get(key, 0), (key, F)
            prev[key] = b
        if F == 0:
            assert set(prev.values()) == {0}  # nothing to keep
            continue
        plain = plan.summary_workspace_bytes(none, so, F, S)
        own = 8 * S + 8 * 5 * (F // 256 + S + 1)  # one column's shifts and partials
        slack = 256 * 8
        # a field that is already pooled: the flux column and its pooling, no row of the spectrum again
        assert plain + 4 * F + own <= prev["pooled_field"] <= plain + 4 * F + own + slack
        assert F < 255 or prev["pooled_field"] < plain + 4 * F * (N // 2)
        # with per_frame the caller holds the column, and nothing is pooled
        assert plain <= prev["pooled_field_col"] <= plain + slack
        # a field nothing else keeps: its rows once, whatever the number of requests on it
        assert plain + 4 * F * (N // 2) + 4 * F + own <= prev["new_field"] <= plain + 4 * F * (N // 2) + 4 * F + own + slack
        assert prev["two_of_one_field"] <= prev["new_field"] + 4 * F + own + slack
        # a field the deltas keep is shared too
        withd = plan.summarize_deltas_workspace_bytes(none, so, ds, F, S)
        assert withd + 4 * F + own <= prev["delta_field"] <= withd + 4 * F + own + slack
        # rows the caller holds are not kept again
        assert prev["per_frame_field"] < prev["no_base"] and prev["no_base"] >= prev["per_frame_field"] + 4 * F * 40
    # no signal: the gather call, nothing kept
    assert size(none, so, None, requests(dict(field=mel, per_frame=C)), 1, 1000, 0) == 0


def test_device_call_refuses_a_small_workspace(plan):
    """Refused on the host, before anything is launched (the pointers are never read)."""
    L = capi.lib()
    alloc = lambda shape: np.empty(shape)
    _, so = plan._summary_outputs(2, ["rms"], alloc)
    _, none = plan._host_outputs(0, [])
    r = requests(dict(field=14, summary=256))
    need = plan.summarize_flux_workspace_bytes(none, so, None, r, 1, 8, 2)
    assert need > plan.summary_workspace_bytes(none, so, 8, 2) > 0
    args = (plan._h, ctypes.c_void_p(256), 8 * N, ctypes.c_void_p(256), 8, ctypes.c_void_p(256), 2, None, None, ctypes.byref(so),
            None, r, 1)
    assert b"workspace" in refused(L.mgx_summarize_flux_device(*args, ctypes.c_void_p(256), need - 1, None))
    refused(L.mgx_summarize_flux_device(*args, None, need, None))
    assert b"aligned" in refused(L.mgx_summarize_flux_device(*args, ctypes.c_void_p(264), need, None))
    assert b"frame_offsets is NULL" in refused(L.mgx_summarize_flux_device(*args[:5], None, *args[6:], ctypes.c_void_p(256), need, None))


def test_host_call_refuses_bad_tables_before_any_copy(plan):
    L = capi.lib()
    x = np.zeros(4 * N, np.float32)
    st = np.array([0, N, 2 * N, 3 * N], np.uint64)
    dst = np.full(3 * 4, 7.0)
    col = np.full(4, 7.0, np.float32)
    r = requests(dict(field=15, summary=dst.ctypes.data, per_frame=col.ctypes.data))
    base = summary()
    call = lambda starts, nf, fo, ns: L.mgx_summarize_flux_host(plan._h, x.ctypes.data, x.size, starts.ctypes.data, nf,
                                                                fo.ctypes.data, ns, None, None, ctypes.byref(base), None, r, 1)
    assert b"frame_offsets[2]" in refused(call(st, 4, np.array([0, 3, 2, 4], np.uint64), 3))
    assert b"frame_offsets[3]" in refused(call(st, 4, np.array([0, 2, 4, 5], np.uint64), 3))
    bad = st.copy()
    bad[2] = 3 * N + 1
    assert b"starts[2]" in refused(call(bad, 4, np.array([0, 2, 3, 4], np.uint64), 3))
    assert (dst == 7.0).all() and (col == 7.0).all()


def test_bindings_bookkeeping():
    """Plan._flux_requests and the flux= argument of Plan.summarize_signals on a stand-in for the plan."""
    class P:
        n = N
        desc = capi.make_desc(buffer_size=N, num_mel_bands=40)
        _flux_requests = capi.Plan._flux_requests
        seen = None

        def summarize_gather(self, samples, starts, frame_offsets, features, per_frame=(), deltas=None, flux=None):
            P.seen = (features, per_frame, deltas, flux)
            return ({}, {}, {}, {}, []) if deltas is not None else ({}, {}, [])

    a64, a32 = (lambda shape: np.empty(shape, np.float64)), (lambda shape: np.zeros(shape, np.float32))
    flux = [dict(feature="melBands"), dict(feature="amplitudeSpectrum", mode="l2", lag=8, per_frame=True, summary=False)]
    reqs, res = P()._flux_requests(10, 3, flux, a64, a32)
    assert [(r.struct_size, r.field, r.mode, r.lag) for r in reqs] == [(32, 19, 0, 1), (32, 15, 2, 8)]
    assert res[0]["summary"].shape == (3, 4) and res[0]["per_frame"] is None and reqs[0].summary == res[0]["summary"].ctypes.data
    assert res[1]["summary"] is None and res[1]["per_frame"].shape == (10,) and res[1]["per_frame"].dtype == np.float32
    assert not reqs[0].per_frame and not reqs[1].summary and reqs[1].per_frame == res[1]["per_frame"].ctypes.data
    for bad in (dict(feature="rms"), dict(feature="mfcc", mode="l3")):
        with pytest.raises(ValueError):
            P()._flux_requests(10, 3, [bad], a64, a32)
    sigs = [np.zeros(2 * N, np.float32), np.zeros(N, np.float32)]
    # one more element behind what the call returns without the argument
    assert len(capi.Plan.summarize_signals(P(), sigs, 64, ["mfcc"], flux=flux)) == 3
    assert len(capi.Plan.summarize_signals(P(), sigs, 64, ["mfcc"], per_frame=["zcr"], flux=flux)) == 4
    assert len(capi.Plan.summarize_signals(P(), sigs, 64, ["mfcc"], per_frame=["zcr"], deltas=(2, 2), flux=flux)) == 5
    assert P.seen == (["mfcc"], ["zcr"], (2, 2), flux)


def test_facade_refusals():
    """The facade checks the flux option before any plan (no device) is made."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(os.path.join(root, "meyda_amd", "addon", "meyda_napi.node")):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    js = """
const assert = require('assert');
const Meyda = require(%r);
const N = %d, hop = 64;
const m = new Meyda({ sampleRate: 44100 }, null, N, null);
const x = new Float32Array(4 * N);
const ok = { feature: 'mfcc' };
for (const form of ['getSignalSummaries', 'getSignalSummariesAsync']) {
  for (const flux of [[], [ok, ok, ok, ok, ok], ok, 'mfcc', null]) assert.throws(() => m[form](['rms'], [x], hop, { flux }), RangeError);
  for (const flux of [[{ feature: 'rms' }], [{ feature: 'buffer' }], [{}], ['mfcc'], [null]]) assert.throws(() => m[form](['rms'], [x], hop, { flux }), TypeError);
  for (const mode of ['l3', 0, null]) assert.throws(() => m[form](['rms'], [x], hop, { flux: [{ feature: 'mfcc', mode }] }), RangeError);
  for (const lag of [0, 9, -1, 1.5, '2', null]) assert.throws(() => m[form](['rms'], [x], hop, { flux: [{ feature: 'mfcc', lag }] }), RangeError);
  // the checks of the call without the option come first, as they did, and the delta options keep their errors
  assert.throws(() => m[form](['buffer'], [x], hop, { flux: [ok] }), (e) => e instanceof TypeError && /has no summary/.test(e.message));
  assert.throws(() => m[form](['rms'], [x], 0, { flux: [ok] }), RangeError);
  assert.throws(() => m[form](['rms'], [x], hop, { flux: [ok], deltaWidth: 9 }), RangeError);
  for (const bad of [2, 'flux', true]) assert.throws(() => m[form](['rms'], [x], hop, bad), TypeError);
}
console.log('ok');
""" % (os.path.join(root, "meyda_amd", "js", "meyda.js"), N)
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=60, cwd=root)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
