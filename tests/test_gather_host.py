"""Buffers at given sample offsets (mgx_signals_frame_starts, mgx_extract_gather_*; include/meyda_gpu.h) as far
as they can be checked without a device: the starts helper against mgx_signal_frames and its own definition,
the argument checks that run before any device call, the bindings' bookkeeping and the facade's checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from meyda_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "meyda_amd", "addon", "meyda_napi.node")
N = 512


def lengths(n, hop):
    return [0, n - 1, n, n + hop - 1, n + hop, n + 5 * hop, 3 * n + 1]


def u64p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("hop", [1, N // 4, N, N + 3])
def test_signals_frame_starts(hop):
    L = capi.lib()
    lens = lengths(N, hop)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    counts = [capi.signal_frames(v, N, hop) for v in lens]
    assert counts[:3] == [0, 0, 1] and counts[3:6] == [1, 2, 6]
    total = ctypes.c_uint64(12345)
    # count only
    assert L.mgx_signals_frame_starts(u64p(off), len(lens), N, hop, None, None, 0, ctypes.byref(total)) == 0
    assert total.value == sum(counts)
    starts = np.full(sum(counts) + 1, 0xABCD, np.uint64)
    fo = np.zeros(len(lens) + 1, np.uint64)
    total2 = ctypes.c_uint64()
    assert L.mgx_signals_frame_starts(u64p(off), len(lens), N, hop, u64p(fo), u64p(starts), sum(counts),
                                      ctypes.byref(total2)) == 0
    assert total2.value == total.value
    assert fo.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    want = [int(off[s]) + k * hop for s in range(len(lens)) for k in range(counts[s])]
    assert starts[:-1].tolist() == want
    assert starts[-1] == 0xABCD  # nothing past the total
    # no buffer crosses its signal's end
    for s in range(len(lens)):
        for f in range(int(fo[s]), int(fo[s + 1])):
            assert off[s] <= starts[f] and starts[f] + N <= off[s + 1]
    # the Python helper: by lengths and by offsets
    st, fo2 = capi.signals_frame_starts(lens, N, hop)
    assert st.dtype == np.uint64 and st.tolist() == want and fo2.tolist() == fo.tolist()
    st, fo2 = capi.signals_frame_starts(off, N, hop, offsets=True)
    assert st.tolist() == want and fo2.tolist() == fo.tolist()


def test_signals_frame_starts_of_nothing():
    st, fo = capi.signals_frame_starts([], N, 7)
    assert st.size == 0 and fo.tolist() == [0]


def test_signals_frame_starts_errors():
    L = capi.lib()
    off = np.array([0, 2 * N, 5 * N], np.uint64)
    total = ctypes.c_uint64(77)
    starts = np.full(8, 0xABCD, np.uint64)
    fo = np.full(3, 0xABCD, np.uint64)
    args = (u64p(fo), u64p(starts))
    assert L.mgx_signals_frame_starts(u64p(off), 2, N, 0, *args, 8, ctypes.byref(total)) == -1
    assert b"hop" in L.mgx_last_error()
    bad = np.array([0, 3 * N, 2 * N], np.uint64)
    assert L.mgx_signals_frame_starts(u64p(bad), 2, N, N, *args, 8, ctypes.byref(total)) == -1
    assert b"offsets[2]" in L.mgx_last_error()
    assert L.mgx_signals_frame_starts(u64p(off), 2, N, N, *args, 4, ctypes.byref(total)) == -1  # 5 buffers
    assert b"5 buffers" in L.mgx_last_error()
    assert L.mgx_signals_frame_starts(u64p(off), 2, N, N, *args, 8, None) == -1
    assert L.mgx_signals_frame_starts(None, 2, N, N, *args, 8, ctypes.byref(total)) == -1
    # a refused call writes nothing
    assert total.value == 77 and (starts == 0xABCD).all() and (fo == 0xABCD).all()
    assert L.mgx_signals_frame_starts(u64p(off), 2, N, N, *args, 5, ctypes.byref(total)) == 0 and total.value == 5
    with pytest.raises(capi.MgxError) as e:
        capi.signals_frame_starts([N], N, 0)
    assert e.value.status == -1


def test_extract_calls_refuse_a_null_plan():
    L = capi.lib()
    o = capi.Outputs()
    a = capi.AuxOutputs()
    a.struct_size = ctypes.sizeof(capi.AuxOutputs)
    starts = np.zeros(1, np.uint64)
    x = np.zeros(N, np.float32)
    assert L.mgx_extract_gather_device(None, x.ctypes.data, N, u64p(starts), 1, ctypes.byref(o), ctypes.byref(a), None) == -1
    assert b"NULL" in L.mgx_last_error()
    assert L.mgx_extract_gather_host(None, x.ctypes.data, N, u64p(starts), 1, ctypes.byref(o), None) == -1
    assert b"NULL" in L.mgx_last_error()
    assert L.mgx_extract_gather_host(None, x.ctypes.data, N, u64p(starts), 1, None, None) == -1


def test_binding_name_lists():
    for sym in ("mgx_signals_frame_starts", "mgx_extract_gather_device", "mgx_extract_gather_host"):
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym)
    assert capi.lib().mgx_abi_version() == 2 and len(capi.FEATURE_NAMES) == 20


def test_extract_signals_bookkeeping():
    """Plan.extract_signals on a stand-in for the plan: the concatenated samples, the helper's starts and the
    frame offsets reach extract_gather, and come back with its outputs."""
    hop = 128
    lens = lengths(N, hop)
    sigs = [np.full(v, s, np.float32) for s, v in enumerate(lens)]

    class P:
        n = N
        seen = None

        def extract_gather(self, samples, starts, features):
            P.seen = (samples, starts, features)
            return {"rms": np.arange(len(starts), dtype=np.float32)}

    out, fo = capi.Plan.extract_signals(P(), sigs, hop, ["rms"])
    samples, starts, feats = P.seen
    assert feats == ["rms"] and samples.dtype == np.float32 and samples.size == sum(lens)
    assert np.array_equal(samples, np.concatenate(sigs))
    counts = [capi.signal_frames(v, N, hop) for v in lens]
    assert fo.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert out["rms"].shape[0] == fo[-1] == len(starts)
    for s in range(len(lens)):  # every buffer holds its own signal's samples only
        for f in range(int(fo[s]), int(fo[s + 1])):
            b = samples[int(starts[f]):int(starts[f]) + N]
            assert b.size == N and (b == s).all()
    # a list of nothing
    out, fo = capi.Plan.extract_signals(P(), [], hop, ["rms"])
    assert fo.tolist() == [0] and P.seen[0].size == 0 and len(P.seen[1]) == 0


def test_facade_signals_frame_starts_and_range_errors():
    if not shutil.which("node"):
        pytest.skip("node is not installed")
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (make -C meyda_amd/addon)")
    hop = 128
    lens = lengths(N, hop)
    st, fo = capi.signals_frame_starts(lens, N, hop)
    js = """
const assert = require('assert');
const Meyda = require(%r);
const lens = %s, N = %d, hop = %d;
const t = Meyda.signalsFrameStarts(lens, N, hop);
assert.ok(t.starts instanceof Float64Array && t.frameOffsets instanceof Float64Array);
assert.deepStrictEqual(Array.from(t.starts), %s);
assert.deepStrictEqual(Array.from(t.frameOffsets), %s);
assert.deepStrictEqual(Array.from(Meyda.signalsFrameStarts(Uint32Array.from(lens), N, hop).starts), Array.from(t.starts));
assert.deepStrictEqual(Array.from(Meyda.signalsFrameStarts([], N, hop).frameOffsets), [0]);
for (const bad of [[-1], [1.5], [NaN], ['7'], [2 ** 53], [null]]) {
  assert.throws(() => Meyda.signalsFrameStarts(bad, N, hop), RangeError, String(bad));
}
assert.throws(() => Meyda.signalsFrameStarts([2 ** 53 - 1, 2 ** 53 - 1], N, hop), /add up to more than a safe integer/);
for (const h of [0, -1, 1.5, '4', undefined]) assert.throws(() => Meyda.signalsFrameStarts(lens, N, h), RangeError);
// starts are checked before any plan (no device) is made
const m = new Meyda({ sampleRate: 44100 }, null, N, null);
const x = new Float32Array(4 * N);
for (const bad of [[-1], [0, 1.5], [NaN], ['0'], [2 ** 53], [undefined]]) {
  assert.throws(() => m.getBatchGather(['rms'], x, bad), RangeError, String(bad));
  assert.throws(() => m.getBatchGatherAsync(['rms'], x, bad), RangeError, String(bad));
}
assert.throws(() => m.getBatchGather(['rms'], x, 3), TypeError);
const g = new Meyda({ sampleRate: 44100 }, null, N, null, { devices: [0, 1] });
assert.throws(() => g.getBatchGather(['rms'], x, [0]), /not supported with options\\.devices/);
assert.throws(() => g.getBatchSignals(['rms'], [x], hop), /not supported with options\\.devices/);
console.log('ok');
""" % (os.path.join(ROOT, "meyda_amd", "js", "meyda.js"), lens, N, hop, st.tolist(), fo.tolist())
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
