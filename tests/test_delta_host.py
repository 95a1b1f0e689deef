"""Deltas (mgx_delta_device, mgx_summarize_deltas_*; include/meyda_gpu.h) as far as they can be checked on the
host: the struct and the exports, every refusal that comes before a device call (the operator takes no plan, and
the delta struct is checked ahead of the plan as the summary struct is), and the workspace's bytes. The checks
that read the plan's sizes need a plan, and a plan needs a device: those tests make no launch, and are skipped
where mgx_plan_create finds no device."""
import ctypes

import numpy as np
import pytest

from meyda_amd import capi

N = 256
E_INVALID, E_UNSUPPORTED = -1, -3
NEW = ["mgx_delta_device", "mgx_summarize_deltas_workspace_bytes", "mgx_summarize_deltas_device", "mgx_summarize_deltas_host"]


def summary(**ptrs):
    s = capi.SummaryOutputs()
    s.struct_size = ctypes.sizeof(capi.SummaryOutputs)
    for k, v in ptrs.items():
        setattr(s, k, v)
    return s


def deltas(width=2, delta=None, delta2=None):
    d = capi.DeltaSummaries()
    d.struct_size = ctypes.sizeof(capi.DeltaSummaries)
    d.width = width
    if delta is not None:
        d.delta = ctypes.pointer(delta)
    if delta2 is not None:
        d.delta2 = ctypes.pointer(delta2)
    return d


def refused(rc, code=E_INVALID):
    assert rc == code, (rc, capi.lib().mgx_last_error())
    msg = capi.lib().mgx_last_error()
    assert len(msg) > 0
    return msg


def test_struct_and_exports():
    for sym in NEW:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    # two uint32, two pointers
    assert ctypes.sizeof(capi.DeltaSummaries) == 24
    assert capi.DeltaSummaries.delta.offset == 8 and capi.DeltaSummaries.delta2.offset == 16
    assert capi.DELTA_MAX_WIDTH == 8
    # not features, and no new ABI: the registry and the version are as they were
    assert len(capi.FEATURE_NAMES) == 20 and capi.lib().mgx_abi_version() == 2
    assert capi.lib().mgx_feature_index(b"delta") == -1


def test_operator_refusals():
    """Every refusal of mgx_delta_device comes before any launch: the pointers are never read."""
    L = capi.lib()
    rows, d1, d2, tb = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    call = lambda **kw: L.mgx_delta_device(*[{**dict(rows=rows, F=10, cols=13, f64=0, tb=tb, S=2, W=2, d1=d1, d2=d2, st=None),
                                              **kw}[k] for k in ("rows", "F", "cols", "f64", "tb", "S", "W", "d1", "d2", "st")])
    assert b"cols" in refused(call(cols=0))
    for w in (0, 9, 2 ** 31):
        assert b"width" in refused(call(W=w))
    assert b"rows_f64" in refused(call(f64=2))
    assert b"rows" in refused(call(rows=None))
    assert b"NULL" in refused(call(d1=None, d2=None))
    refused(call(d1=rows))
    refused(call(d2=rows))
    refused(call(d1=None, d2=rows))
    assert b"same" in refused(call(d2=d1))
    assert b"frame_offsets" in refused(call(tb=None))
    # refused whatever the number of rows; with valid arguments no rows is MGX_OK, nothing launched
    refused(call(F=0, W=0))
    refused(call(F=0, cols=0))
    assert call(F=0) == 0 and call(F=0, rows=None, tb=None, S=0, d1=None) == 0


def test_summary_refusals_ahead_of_the_plan():
    """The delta struct, like the summary struct, is checked before the plan is looked at; then a NULL plan is."""
    L = capi.lib()
    x = np.zeros(N, np.float32)
    st = np.zeros(1, np.uint64)
    fo = np.array([0, 1], np.uint64)
    dst = np.full(4 * N, 7.0)
    b = ctypes.c_uint64(99)
    base = summary()
    host = lambda s, d: L.mgx_summarize_deltas_host(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, 1, None, None, s, d)
    dev = lambda s, d: L.mgx_summarize_deltas_device(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, 1, None, None, s, d,
                                                     None, 0, None)
    size = lambda s, d: L.mgx_summarize_deltas_workspace_bytes(None, None, None, s, d, 1, 1, ctypes.byref(b))
    for call in (host, dev, size):
        named = summary(mfcc=dst.ctypes.data)
        assert b"summary is NULL" in refused(call(None, ctypes.byref(deltas(delta=named))))
        for wrong in (0, 16, 32):
            d = deltas(delta=named)
            d.struct_size = wrong
            assert b"mgx_delta_summaries.struct_size" in refused(call(ctypes.byref(base), ctypes.byref(d)))
        for w in (0, 9):
            assert b"width" in refused(call(ctypes.byref(base), ctypes.byref(deltas(width=w, delta=named))))
        for k in ("delta", "delta2"):
            bad = summary(mfcc=dst.ctypes.data)
            bad.struct_size -= 8
            assert b"struct_size" in refused(call(ctypes.byref(base), ctypes.byref(deltas(**{k: bad}))))
            bad = summary(mfcc=dst.ctypes.data)
            bad.reserved = 1
            assert b"reserved" in refused(call(ctypes.byref(base), ctypes.byref(deltas(**{k: bad}))))
            # a spectrum's deltas are not pooled
            for spec in ("amplitude_spectrum", "power_spectrum"):
                msg = refused(call(ctypes.byref(base), ctypes.byref(deltas(**{k: summary(**{spec: dst.ctypes.data})}))), E_UNSUPPORTED)
                assert b"spectrum" in msg and k.encode() in msg
        # ... and a valid one reaches the plan
        assert b"NULL plan" in refused(call(ctypes.byref(base), ctypes.byref(deltas(delta=named, delta2=named))))
        assert b"NULL plan" in refused(call(ctypes.byref(base), None))
    assert (dst == 7.0).all() and b.value == 99  # a refused call writes nothing


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
    _, _, ds = plan._delta_summaries(S, ["mfcc", "melBands", "zcr"], (2, 2), alloc)
    _, _, ds1 = plan._delta_summaries(S, ["mfcc", "melBands", "zcr"], (2, 1), alloc)
    _, none = plan._host_outputs(0, [])
    _, some = plan._host_outputs(1, ["mfcc", "zcr"])
    cols = 13 + 40 + 1
    prev = {}
    for F in [0, 1, 255, 256, 257, 5000]:
        for o in (none, some):
            plain = plan.summary_workspace_bytes(o, so, F, S)
            assert plan.summarize_deltas_workspace_bytes(o, so, None, F, S) == plain  # deltas = NULL: the summary call's
            assert plan.summarize_deltas_workspace_bytes(o, so, deltas(), F, S) == plain  # no field named in either
        for key, (o, s, d) in {"both": (none, so, ds), "first": (none, so, ds1), "per_frame": (some, so, ds),
                               "no_base": (none, empty, ds)}.items():
            b = plan.summarize_deltas_workspace_bytes(o, s, d, F, S)
            assert b % 256 == 0 and b >= prev.get(key, 0), (key, F)
            prev[key] = b
        if F == 0:
            assert set(prev.values()) == {0}  # nothing to keep
            continue
        plain = plan.summary_workspace_bytes(none, so, F, S)
        # the delta rows (and the rows of melBands and zcr, which the base call does not hold) come on top: 4 bytes
        # a column a frame and order, then the deltas' own shifts and partials
        own = 8 * S * cols + 8 * 5 * cols * (F // 256 + S + 1)
        assert prev["first"] >= plain + 4 * F * (cols + 41) + own
        assert prev["both"] >= prev["first"] + 4 * F * cols + own
        assert prev["both"] <= plain + 4 * F * (2 * cols + 41) + 2 * own + 256 * 64
        assert prev["per_frame"] < prev["both"]  # rows the caller holds are not kept again
        assert 0 < prev["no_base"] < prev["both"]
    # no signal: the gather call, nothing kept
    assert plan.summarize_deltas_workspace_bytes(none, so, ds, 1000, 0) == 0


def test_device_call_refuses_a_small_workspace(plan):
    """Refused on the host, before anything is launched (the pointers are never read)."""
    L = capi.lib()
    alloc = lambda shape: np.empty(shape)
    _, so = plan._summary_outputs(2, ["rms"], alloc)
    _, _, ds = plan._delta_summaries(2, ["mfcc"], (2, 2), alloc)
    _, none = plan._host_outputs(0, [])
    need = plan.summarize_deltas_workspace_bytes(none, so, ds, 8, 2)
    assert need > plan.summary_workspace_bytes(none, so, 8, 2) > 0
    args = (plan._h, ctypes.c_void_p(256), 8 * N, ctypes.c_void_p(256), 8, ctypes.c_void_p(256), 2, None, None, ctypes.byref(so),
            ctypes.byref(ds))
    # (the summary call's bytes are not enough)
    assert b"workspace" in refused(L.mgx_summarize_deltas_device(*args, ctypes.c_void_p(256), need - 1, None))
    refused(L.mgx_summarize_deltas_device(*args, ctypes.c_void_p(256), plan.summary_workspace_bytes(none, so, 8, 2), None))
    refused(L.mgx_summarize_deltas_device(*args, None, need, None))
    assert b"aligned" in refused(L.mgx_summarize_deltas_device(*args, ctypes.c_void_p(264), need, None))
    assert b"frame_offsets is NULL" in refused(L.mgx_summarize_deltas_device(*args[:5], None, *args[6:], ctypes.c_void_p(256), need, None))


def test_host_call_refuses_bad_tables_before_any_copy(plan):
    L = capi.lib()
    x = np.zeros(4 * N, np.float32)
    st = np.array([0, N, 2 * N, 3 * N], np.uint64)
    dst = np.full(3 * 4 * 13, 7.0)
    ds = deltas(delta=summary(mfcc=dst.ctypes.data))
    base = summary()
    call = lambda starts, nf, fo, ns: L.mgx_summarize_deltas_host(plan._h, x.ctypes.data, x.size, starts.ctypes.data, nf,
                                                                  fo.ctypes.data, ns, None, None, ctypes.byref(base), ctypes.byref(ds))
    assert b"frame_offsets[2]" in refused(call(st, 4, np.array([0, 3, 2, 4], np.uint64), 3))
    assert b"frame_offsets[3]" in refused(call(st, 4, np.array([0, 2, 4, 5], np.uint64), 3))
    bad = st.copy()
    bad[2] = 3 * N + 1
    assert b"starts[2]" in refused(call(bad, 4, np.array([0, 2, 3, 4], np.uint64), 3))
    assert (dst == 7.0).all()


def test_bindings_bookkeeping():
    """Plan._delta_summaries and the deltas= argument of Plan.summarize_signals on a stand-in for the plan."""
    class P:
        n = N
        desc = capi.make_desc(buffer_size=N, num_mel_bands=40)
        _summary_outputs = capi.Plan._summary_outputs
        seen = None

        def summarize_gather(self, samples, starts, frame_offsets, features, per_frame=(), deltas=None):
            P.seen = (features, per_frame, deltas)
            return {}, {}, {}, {}

    d1, d2, ds = capi.Plan._delta_summaries(P(), 3, ["rms", "loudness", "mfcc", "melBands"], (3, 2), lambda shape: np.empty(shape))
    assert ds.struct_size == 24 and ds.width == 3
    shapes = {"rms": (3, 4, 1), "loudness.specific": (3, 4, 24), "loudness.total": (3, 4, 1), "mfcc": (3, 4, 13), "melBands": (3, 4, 40)}
    assert {k: v.shape for k, v in d1.items()} == shapes == {k: v.shape for k, v in d2.items()}
    assert ds.delta.contents.mfcc == d1["mfcc"].ctypes.data and ds.delta2.contents.mfcc == d2["mfcc"].ctypes.data
    assert ds.delta2.contents.scalars[10] == d2["loudness.total"].ctypes.data
    d1, d2, ds = capi.Plan._delta_summaries(P(), 3, ["rms"], (1, 1), lambda shape: np.empty(shape))
    assert d2 is None and not ds.delta2 and ds.delta.contents.scalars[0] == d1["rms"].ctypes.data
    for order in (0, 3):
        with pytest.raises(ValueError):
            capi.Plan._delta_summaries(P(), 3, ["rms"], (2, order), lambda shape: np.empty(shape))
    sigs = [np.zeros(2 * N, np.float32), np.zeros(N, np.float32)]
    assert len(capi.Plan.summarize_signals(P(), sigs, 64, ["mfcc"], per_frame=["zcr"], deltas=(2, 2))) == 4
    assert P.seen == (["mfcc"], ["zcr"], (2, 2))


def test_facade_refusals():
    """The facade checks the options before any plan (no device) is made."""
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
for (const form of ['getSignalSummaries', 'getSignalSummariesAsync']) {
  for (const w of [0, 9, -1, 1.5, '2', null]) assert.throws(() => m[form](['rms'], [x], hop, { deltaWidth: w }), RangeError);
  for (const o of [0, 3, 1.5, '2', null]) assert.throws(() => m[form](['rms'], [x], hop, { deltaOrder: o }), RangeError);
  for (const bad of [2, 'delta', true]) assert.throws(() => m[form](['rms'], [x], hop, bad), TypeError);
  // the checks of the call without the option come first, as they did
  assert.throws(() => m[form](['buffer'], [x], hop, { deltaOrder: 2 }), (e) => e instanceof TypeError && /has no summary/.test(e.message));
  assert.throws(() => m[form](['rms'], [x], 0, { deltaOrder: 2 }), RangeError);
}
console.log('ok');
""" % (os.path.join(root, "meyda_amd", "js", "meyda.js"), N)
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=60, cwd=root)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
