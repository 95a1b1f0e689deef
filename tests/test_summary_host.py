"""Per-signal summaries (mgx_summary_workspace_bytes, mgx_summarize_device / _host; include/meyda_gpu.h) as far
as they can be checked on the host: the struct and the exports, the refusals that need no plan (the summary
struct is checked ahead of it), the bindings' bookkeeping on a stand-in for the plan, and the facade's
refusals. The refusals that read the plan's buffer size (the tables, the workspace's size) need a plan, and a
plan needs a device: those tests make no launch, and are skipped where mgx_plan_create finds no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from meyda_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")
N = 256
E_INVALID = -1


def summary(**ptrs):
    s = capi.SummaryOutputs()
    s.struct_size = ctypes.sizeof(capi.SummaryOutputs)
    for k, v in ptrs.items():
        setattr(s, k, v)
    return s


def test_struct_and_exports():
    # two uint32, 13 scalar pointers, five array pointers
    assert ctypes.sizeof(capi.SummaryOutputs) == 8 + 8 * (capi.NUM_SCALARS + 5)
    assert capi.SummaryOutputs.mel_bands.offset == 8 + 8 * (capi.NUM_SCALARS + 4)
    for sym in ("mgx_summary_workspace_bytes", "mgx_summarize_device", "mgx_summarize_host"):
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    assert capi.STATS == ["mean", "variance", "min", "max"]
    hdr = open(os.path.join(ROOT, "include", "meyda_gpu.h")).read()
    for k, name in enumerate(["MGX_STAT_MEAN", "MGX_STAT_VARIANCE", "MGX_STAT_MIN", "MGX_STAT_MAX", "MGX_NUM_STATS"]):
        assert "%s = %d" % (name, k) in hdr
    # not a feature index: the registry is as it was
    assert "MGX_NUM_FEATURES = 20" in hdr and len(capi.FEATURE_NAMES) == 20
    assert capi.lib().mgx_feature_index(b"mean") == -1


def test_refusals_ahead_of_the_plan():
    """NULL summary and a wrong struct_size are refused before the plan is looked at; then a NULL plan is."""
    L = capi.lib()
    x = np.zeros(N, np.float32)
    st = np.zeros(1, np.uint64)
    fo = np.array([0, 1], np.uint64)
    dst = np.full(4, 7.0)
    b = ctypes.c_uint64(99)
    host = lambda s: L.mgx_summarize_host(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, 1, None, None, s)
    dev = lambda s: L.mgx_summarize_device(None, x.ctypes.data, N, st.ctypes.data, 1, fo.ctypes.data, 1, None, None, s, None, 0,
                                           None)
    size = lambda s: L.mgx_summary_workspace_bytes(None, None, None, s, 1, 1, ctypes.byref(b))
    for call in (host, dev, size):
        assert call(None) == E_INVALID
        assert b"summary is NULL" in L.mgx_last_error()
        for wrong in (0, ctypes.sizeof(capi.SummaryOutputs) - 8, ctypes.sizeof(capi.SummaryOutputs) + 8):
            s = summary()
            s.scalars[0] = dst.ctypes.data
            s.struct_size = wrong
            assert call(ctypes.byref(s)) == E_INVALID
            assert b"struct_size" in L.mgx_last_error()
        s = summary()
        s.reserved = 1
        assert call(ctypes.byref(s)) == E_INVALID and b"reserved" in L.mgx_last_error()
        s = summary()
        s.scalars[0] = dst.ctypes.data
        assert call(ctypes.byref(s)) == E_INVALID and b"NULL plan" in L.mgx_last_error()
    assert L.mgx_summary_workspace_bytes(None, None, None, ctypes.byref(summary()), 1, 1, None) == E_INVALID
    assert (dst == 7.0).all() and b.value == 99  # a refused call writes nothing


@pytest.fixture(scope="module")
def plan():
    if capi.device_count() == 0:
        pytest.skip("mgx_plan_create needs a device (these checks make no launch)")
    p = capi.Plan(buffer_size=N, num_mel_bands=40)
    yield p
    p.close()


def test_host_call_refuses_bad_tables_before_any_copy(plan):
    L = capi.lib()
    x = np.zeros(4 * N, np.float32)
    st = np.array([0, N, 2 * N, 3 * N], np.uint64)
    dst = np.full(3 * 4, 7.0)
    s = summary()
    s.scalars[0] = dst.ctypes.data
    call = lambda starts, nf, fo, ns: L.mgx_summarize_host(plan._h, x.ctypes.data, x.size, starts.ctypes.data, nf,
                                                           fo.ctypes.data, ns, None, None, ctypes.byref(s))
    assert call(st, 4, np.array([0, 3, 2, 4], np.uint64), 3) == E_INVALID  # decreasing
    assert b"frame_offsets[2]" in L.mgx_last_error()
    assert call(st, 4, np.array([0, 2, 4, 5], np.uint64), 3) == E_INVALID  # last offset above num_frames
    assert b"frame_offsets[3]" in L.mgx_last_error() and b"4 buffers" in L.mgx_last_error()
    bad = st.copy()
    bad[2] = 3 * N + 1  # a start whose buffer leaves the samples
    assert call(bad, 4, np.array([0, 2, 3, 4], np.uint64), 3) == E_INVALID
    assert b"starts[2]" in L.mgx_last_error()
    assert L.mgx_summarize_host(plan._h, x.ctypes.data, x.size, st.ctypes.data, 4, None, 3, None, None, ctypes.byref(s)) == E_INVALID
    assert b"frame_offsets is NULL" in L.mgx_last_error()
    assert L.mgx_summarize_host(plan._h, x.ctypes.data, x.size, None, 4, st.ctypes.data, 3, None, None, ctypes.byref(s)) == E_INVALID
    assert L.mgx_summarize_host(plan._h, x.ctypes.data, N - 1, st.ctypes.data, 1, st.ctypes.data, 1, None, None,
                                ctypes.byref(s)) == E_INVALID
    assert (dst == 7.0).all()


def test_workspace_bytes(plan):
    feats = ["rms", "spectralRolloff", "loudness", "mfcc", "amplitudeSpectrum", "melBands"]
    _, so = plan._summary_outputs(5, feats, lambda shape: np.empty(shape))
    cols = 1 + 1 + 24 + 1 + 13 + N // 2 + 40
    _, none = plan._host_outputs(0, [])
    _, every = plan._host_outputs(1, feats)  # (only whether a pointer is NULL is read)
    _, some = plan._host_outputs(1, ["mfcc", "melBands", "rms"])
    prev = prev_all = 0
    for F in [0, 1, 255, 256, 257, 1000, 4096, 100000]:
        b, b_all, b_some = (plan.summary_workspace_bytes(o, so, F, 5) for o in (none, every, some))
        assert b % 256 == 0 and b_all % 256 == 0 and b_some % 256 == 0
        assert b >= prev and b_all >= prev_all  # non-decreasing in num_frames
        assert b_all <= b_some <= b
        if F == 0:  # nothing to keep: no per-frame array, no partial
            assert b == b_all == b_some == 0
        else:
            # with every pooled field requested per frame only the table, the shifts and the partials are left:
            # at least their own bytes, at most those and four roundings to 256
            own = 8 * (5 + 1) + 8 * 5 * cols + 8 * 5 * cols * (F // 256 + 5 + 1)
            assert own <= b_all <= own + 4 * 256
            # ... and without them the per-frame arrays come on top: 4 bytes a column a frame
            assert b - b_all >= 4 * cols * F and b - b_all <= 4 * cols * F + 256 * (len(capi.FIELDS) + 2)
        prev, prev_all = b, b_all
    # no pooled field, or no signal: nothing
    assert plan.summary_workspace_bytes(every, summary(), 1000, 5) == 0
    assert plan.summary_workspace_bytes(none, so, 1000, 0) == 0


def test_device_call_refuses_a_small_workspace(plan):
    """Refused on the host, before anything is launched (the pointers are never read)."""
    L = capi.lib()
    _, so = plan._summary_outputs(2, ["rms"], lambda shape: np.empty(shape))
    _, none = plan._host_outputs(0, [])
    need = plan.summary_workspace_bytes(none, so, 8, 2)
    assert need > 0
    args = (plan._h, ctypes.c_void_p(256), 8 * N, ctypes.c_void_p(256), 8, ctypes.c_void_p(256), 2, None, None, ctypes.byref(so))
    assert L.mgx_summarize_device(*args, ctypes.c_void_p(256), need - 1, None) == E_INVALID
    assert b"workspace" in L.mgx_last_error()
    assert L.mgx_summarize_device(*args, None, need, None) == E_INVALID
    assert L.mgx_summarize_device(*args, ctypes.c_void_p(264), need, None) == E_INVALID
    assert b"aligned" in L.mgx_last_error()


def test_summary_outputs_bookkeeping():
    """Plan._summary_outputs and Plan.summarize_signals on a stand-in for the plan."""
    class P:
        n = N
        desc = capi.make_desc(buffer_size=N, num_mel_bands=40)
        seen = None

        def summarize_gather(self, samples, starts, frame_offsets, features, per_frame=()):
            P.seen = (samples, starts, frame_offsets, features, per_frame)
            return {"rms": np.zeros((len(frame_offsets) - 1, 4, 1))}, {"zcr": np.zeros(len(starts))}

    out, so = capi.Plan._summary_outputs(P(), 3, ["rms", "loudness", "mfcc", "powerSpectrum", "melBands"],
                                         lambda shape: np.empty(shape, np.float64))
    shapes = {k: v.shape for k, v in out.items()}
    assert shapes == {"rms": (3, 4, 1), "loudness.specific": (3, 4, 24), "loudness.total": (3, 4, 1), "mfcc": (3, 4, 13),
                      "powerSpectrum": (3, 4, N // 2), "melBands": (3, 4, 40)}
    assert so.struct_size == ctypes.sizeof(capi.SummaryOutputs) and so.reserved == 0
    assert so.scalars[0] == out["rms"].ctypes.data and so.scalars[10] == out["loudness.total"].ctypes.data
    assert so.loudness_specific == out["loudness.specific"].ctypes.data and so.mel_bands == out["melBands"].ctypes.data
    assert so.power_spectrum == out["powerSpectrum"].ctypes.data and not so.amplitude_spectrum and not so.scalars[1]
    for bad in ("complexSpectrum", "buffer", "nonsense"):
        with pytest.raises(ValueError):
            capi.Plan._summary_outputs(P(), 1, [bad], lambda shape: np.empty(shape))
    hop = 64
    lens = [0, N - 1, N, N + hop, 3 * N + 1]
    sigs = [np.full(v, s, np.float32) for s, v in enumerate(lens)]
    summ, fo = capi.Plan.summarize_signals(P(), sigs, hop, ["rms"])
    samples, starts, fo_seen, feats, per_frame = P.seen
    counts = [capi.signal_frames(v, N, hop) for v in lens]
    assert fo.tolist() == fo_seen.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert feats == ["rms"] and per_frame == () and np.array_equal(samples, np.concatenate(sigs)) and len(starts) == fo[-1]
    assert summ["rms"].shape == (len(lens), 4, 1)
    summ, fo, rows = capi.Plan.summarize_signals(P(), sigs, hop, ["rms"], per_frame=["zcr"])
    assert P.seen[4] == ["zcr"] and rows["zcr"].shape == (fo[-1],)


def test_facade_refusals():
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    js = """
const assert = require('assert');
const Meyda = require(%r);
const N = %d, hop = 64;
// refused before any plan (no device) is made
const m = new Meyda({ sampleRate: 44100 }, null, N, null);
const x = new Float32Array(4 * N);
for (const bad of ['complexSpectrum', 'buffer', ['rms', 'complexSpectrum'], ['buffer', 'mfcc']]) {
  assert.throws(() => m.getSignalSummaries(bad, [x], hop), (e) => e instanceof TypeError && /has no summary/.test(e.message));
  assert.throws(() => m.getSignalSummariesAsync(bad, [x], hop), (e) => e instanceof TypeError && /has no summary/.test(e.message));
}
assert.throws(() => m.getSignalSummaries(['nonsense'], [x], hop), TypeError);
assert.throws(() => m.getSignalSummaries(['rms'], x, hop), TypeError);
for (const h of [0, -1, 1.5, '4', undefined]) assert.throws(() => m.getSignalSummaries(['rms'], [x], h), RangeError);
const g = new Meyda({ sampleRate: 44100 }, null, N, null, { devices: [0, 1] });
assert.throws(() => g.getSignalSummaries(['rms'], [x], hop), /not supported with options\\.devices/);
assert.throws(() => g.getSignalSummariesAsync(['rms'], [x], hop), /not supported with options\\.devices/);
console.log('ok');
""" % (os.path.join(ROOT, "meyda_amd", "js", "meyda.js"), N)
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
