"""Buffers at given sample offsets (mgx_extract_gather_*, include/meyda_gpu.h): buffer f of the launch is samples
[starts[f], starts[f] + N) of one array (GatherTable::starts, after the KernelArgs). The defining property is the
signal launch's: every output equals, bit for bit and NaN for NaN, what the dense entry points give on the same
buffers stacked with numpy -- buffer indices, the schedule, the scalar windows and the tail pool are functions
of the buffer count alone, so only the load address differs. Every output array is prefilled with NaN on both
sides, so an output a plan's mode never writes compares equal instead of showing two allocations' stale bytes.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_melbands import device_frames
from test_gpu_signal import FAMILIES, SPECTRA, dense_frames, env_plan, on_device, same_device, same_host, signal

pytestmark = pytest.mark.gpu

SIZES = [256, 512, 1024, 2048]


@pytest.fixture(scope="module")
def capi():
    from meyda_amd import capi
    if capi.device_count() == 0:
        pytest.fail("no GPU visible to libmeyda_gpu.so")
    return capi


def feats_all(capi):
    return capi.ALL_FEATURES + SPECTRA + ["melBands"]


def stacked(x, starts, n):
    return np.stack([x[int(s):int(s) + n] for s in starts])


def draw_starts(S, n, F, seed):
    """F starts in [0, S - n]: the last legal start, 0, an odd one, the same again, a descending run of odd
    steps, then a seeded draw (a shorter table is this one's beginning)."""
    last = S - n
    odd = (last // 2) | 1
    head = [last, 0, odd, odd] + [last - 1 - 37 * k for k in range(6)]
    rest = np.random.default_rng(seed).integers(0, last + 1, max(0, F - len(head))).tolist()
    st = np.array((head + rest)[:F], np.uint64)
    assert st.max() <= last
    return st


def starts_tensor(st):
    import torch
    return torch.from_numpy(np.ascontiguousarray(st, dtype=np.uint64).view(np.int64)).cuda()


def nan_outputs(plan, F, feats):
    out, o = plan.alloc_outputs(F, feats)
    for t in out.values():
        t.fill_(float("nan"))
    return out, o


def dense_run(plan, frames, feats, stream=None):
    """The dense launch over the rows of `frames` (numpy), device outputs."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).cuda()
    out, o = nan_outputs(plan, t.shape[0], feats)
    plan.extract_device(t.data_ptr(), t.shape[0], o, stream or torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def gather_run(plan, xs, st, feats, num_samples=None, stream=None):
    """The gather launch over the device signal xs at the starts st (numpy), device outputs."""
    import torch
    sd = starts_tensor(st)
    out, o = nan_outputs(plan, len(st), feats)
    plan.extract_gather_device(xs.data_ptr(), xs.shape[0] if num_samples is None else num_samples, sd.data_ptr(), len(st), o,
                               stream or torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def gather_vs_dense(plan, x, st, feats, what):
    ref = dense_run(plan, stacked(x, st, plan.n), feats)
    got = gather_run(plan, on_device(x), st, feats)
    same_device(got, ref, what)
    return got


# ------------------------------------------------------------------ 1. the schedule's corners
@pytest.mark.parametrize("n", SIZES)
def test_gather_equals_dense_at_the_schedules_corners(capi, n):
    """One buffer, a partial wave batch, one batch, a batch plus one, a group of 16, a group plus one, several
    workgroups; then, on a grid capped at 8 workgroups, 3,001 buffers: 12+ groups per workgroup and 8+ batches
    per wave -- the scalar windows, the ranked shares and (N = 2048) the tail pool."""
    feats = feats_all(capi)
    S = 8 * n + 5
    x = signal(S, 31 * n)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        for F in (1, 3, 4, 5, 16, 17, 65):
            gather_vs_dense(plan, x, draw_starts(S, n, F, 1000 * n + F), feats, (n, F))
    finally:
        plan.close()
    plan = env_plan(capi, {"MGX_GRID_CAP": 8}, buffer_size=n, scalar_f64=True)
    try:
        gather_vs_dense(plan, x, draw_starts(S, n, 3001, 7 * n), feats, (n, 3001))
    finally:
        plan.close()


# ------------------------------------------------------------------ 2. identity
@pytest.mark.parametrize("n", SIZES)
def test_gather_at_multiples_of_a_hop_is_the_signal_launch(capi, n):
    feats = feats_all(capi)
    F = 67
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        for hop in (n // 4, n, n + 3):
            x = signal((F - 1) * hop + n + 9, n + hop)
            xs = on_device(x)
            assert capi.signal_frames(x.size, n, hop) == F
            ref, o = nan_outputs(plan, F, feats)
            plan.extract_signal_device(xs.data_ptr(), x.size, hop, o)
            got = gather_run(plan, xs, np.arange(F, dtype=np.uint64) * hop, feats)
            same_device(got, ref, (n, hop))
    finally:
        plan.close()


# ------------------------------------------------------------------ 3. ragged signals
@pytest.mark.parametrize("n", [512, 2048])
def test_ragged_signals_in_one_launch(capi, n):
    import torch
    feats = feats_all(capi)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        for hop in (n // 4, n):
            lens = [0, n - 1, n, n + hop - 1, n + hop, n + 5 * hop, 3 * n + 1]
            sigs = [signal(v, 100 * s + hop) for s, v in enumerate(lens)]
            st, fo = capi.signals_frame_starts(lens, n, hop)
            got = gather_run(plan, on_device(np.concatenate(sigs)), st, feats)
            per = []
            for s, x in enumerate(sigs):
                F = capi.signal_frames(x.size, n, hop)
                assert F == fo[s + 1] - fo[s]
                if F == 0:
                    continue
                ref, o = nan_outputs(plan, F, feats)
                xs = on_device(x)
                plan.extract_signal_device(xs.data_ptr(), x.size, hop, o)
                torch.cuda.synchronize()
                # the signal's slice of the one launch is its own launch's output: no buffer straddles a boundary
                same_device({k: v[int(fo[s]):int(fo[s + 1])] for k, v in got.items()}, ref, (n, hop, s))
                per.append(ref)
            same_device(got, {k: torch.cat([r[k] for r in per]) for k in got}, (n, hop, "all"))
    finally:
        plan.close()


# ------------------------------------------------------------------ 4. every kernel family
@pytest.mark.parametrize("name,n,kw,feats", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_gather_every_kernel_family(capi, name, n, kw, feats):
    F = 67
    S = 8 * n + 3
    kw = dict({"scalar_f64": True}, **kw)
    plan = capi.Plan(buffer_size=n, **kw)
    try:
        gather_vs_dense(plan, signal(S, 4242), draw_starts(S, n, F, 99), feats or feats_all(capi), name)
    finally:
        plan.close()


@pytest.mark.parametrize("nt_min_mb", [0, 1 << 20], ids=["nt", "plain"])
def test_gather_both_load_kinds(capi, nt_min_mb):
    """MGX_NT_MIN_MB forces either kind of frame load, for tables that re-read samples and tables that do not."""
    n = 1024
    plan = env_plan(capi, {"MGX_NT_MIN_MB": nt_min_mb}, buffer_size=n, scalar_f64=True)
    try:
        for F, S in ((203, 8 * n + 3), (5, 8 * n + 3)):
            gather_vs_dense(plan, signal(S, 9), draw_starts(S, n, F, 5), feats_all(capi), (nt_min_mb, F))
    finally:
        plan.close()


# ------------------------------------------------------------------ 5. the clamp
@pytest.mark.parametrize("n", [1024, 2048])
def test_a_start_past_the_last_buffer_reads_the_last_buffer(capi, n):
    """Starts in (S - N, S - N + pad - N] -- inside the NaN tail on_device allocates, so even unclamped they land
    in memory the test owns -- give exactly the outputs of the buffer at S - N, and no NaN."""
    import torch
    feats = feats_all(capi)
    S, pad = 8 * n + 5, 4096
    x = signal(S, 17 * n)
    last = S - n
    late = [last + 1, last + 2, last + 777, last + pad - n]
    st = np.array([0, last] + late + [5, last + 1] + late * 3, np.uint64)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = gather_run(plan, on_device(x, pad=pad), st, feats)
        ref = dense_run(plan, stacked(x, np.minimum(st, last), n), feats)
        same_device(got, ref, n)
        for k, v in got.items():
            assert not torch.isnan(v).any(), k
    finally:
        plan.close()


# ------------------------------------------------------------------ 6. the host path
@pytest.mark.parametrize("n,F", [(1024, 1), (1024, 2), (512, 512), (512, 513)])
def test_host_gather_equals_dense(capi, n, F):
    """One buffer (the inline-frame launch), two, the one-launch path's last size and the chunked path's first."""
    feats = feats_all(capi)
    S = 8 * n + 5
    x = signal(S, 5 * F + n)
    st = draw_starts(S, n, F, F)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        same_host(plan.extract_gather(x, st, feats), plan.extract(stacked(x, st, n), feats), (n, F))
    finally:
        plan.close()


@pytest.mark.parametrize("F", [3, 600])
def test_host_gather_refuses_a_start_out_of_range(capi, F):
    n = 512
    S = 8 * n
    x = signal(S, 3)
    st = draw_starts(S, n, F, 1)
    st[F - 2] = S - n + 1
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        out, o = plan._host_outputs(F, feats_all(capi))
        for a in out.values():
            a.view(np.uint8)[...] = 0xA5
        rc = capi.lib().mgx_extract_gather_host(plan._h, x.ctypes.data, S, st.ctypes.data, F, ctypes.byref(o), capi._aux_ref(o))
        assert rc == -1
        assert ("starts[%d]" % (F - 2)).encode() in capi.lib().mgx_last_error()
        for k, a in out.items():
            assert (a.view(np.uint8) == 0xA5).all(), k
        with pytest.raises(capi.MgxError) as e:  # fewer samples than one buffer
            plan.extract_gather(x[:n - 1], np.zeros(1, np.uint64), ["rms"])
        assert e.value.status == -1
        assert plan.extract_gather(x, np.zeros(0, np.uint64), ["rms"])["rms"].shape == (0,)
    finally:
        plan.close()


def test_host_gather_chunk_seam(capi):
    """70,000 buffers at hop 1 with one jump of more than a staging slot's span (65,536 N samples) after buffer
    67,000: the first chunk ends at its 65,536 buffers, the second at the jump, the third holds the rest."""
    n, F, jump_at = 256, 70000, 67000
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum", "melBands"]
    jump = 65536 * n + 1000
    st = np.arange(F, dtype=np.uint64)
    st[jump_at:] += np.uint64(jump)
    x = signal(int(st[-1]) + n + 3, 65536)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        got = plan.extract_gather(x, st, feats)
        ref = plan.extract(stacked(x, st, n), feats)
    finally:
        plan.close()
    for at in (65536, jump_at):
        seam = slice(at - 8, at + 8)
        same_host({k: v[seam] for k, v in got.items()}, {k: v[seam] for k, v in ref.items()}, ("seam", at))
    same_host(got, ref, "all")


# ------------------------------------------------------------------ 7. graph replay
def test_gather_graph_replay(capi):
    """A gather launch captured into a graph and replayed three times gives the same bytes each time."""
    import torch
    n, F = 2048, 4099  # (the tail pool's counter resets itself between replays)
    feats = ["mfcc", "melBands", "rms", "spectralCentroid"]
    frames = device_frames(capi, n, 64)
    samples = frames.reshape(-1)
    S = samples.shape[0]
    sd = starts_tensor(draw_starts(S, n, F, 12))
    plan = capi.Plan(buffer_size=n)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            warm, wo = plan.alloc_outputs(64, feats)
            plan.extract_device(frames.data_ptr(), 64, wo, s.cuda_stream)  # the stream's scratch set, uncaptured
            ref, ro = plan.alloc_outputs(F, feats)
            plan.extract_gather_device(samples.data_ptr(), S, sd.data_ptr(), F, ro, s.cuda_stream)
        torch.cuda.synchronize()
        out, o = plan.alloc_outputs(F, feats)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.extract_gather_device(samples.data_ptr(), S, sd.data_ptr(), F, o, s.cuda_stream)
        torch.cuda.synchronize()
        for rep in range(3):
            for t in out.values():
                t.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            for k in ref:
                assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), (rep, k)
        g.reset()
    finally:
        plan.close()


# ------------------------------------------------------------------ 8. stream order
def test_two_gather_launches_on_two_streams(capi):
    import torch
    n = 1024
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum", "melBands"]
    S = 203 * 256 + n
    x = signal(S, 88)
    tables = {seed: draw_starts(S, n, F, seed) for seed, F in ((1, 203), (2, 777))}
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        xs = on_device(x)
        ref = {k: dense_run(plan, stacked(x, st, n), feats) for k, st in tables.items()}
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        dev = {k: starts_tensor(st) for k, st in tables.items()}
        outs = {k: nan_outputs(plan, len(st), feats) for k, st in tables.items()}
        torch.cuda.synchronize()
        for k, s in ((1, s1), (2, s2)):
            plan.extract_gather_device(xs.data_ptr(), S, dev[k].data_ptr(), len(tables[k]), outs[k][1], s.cuda_stream)
        torch.cuda.synchronize()
        same_device(outs[1][0], ref[1], "table 1")
        same_device(outs[2][0], ref[2], "table 2")
    finally:
        plan.close()


def test_gather_torch_binding(capi):
    """Plan.extract_gather_torch: starts as a numpy array or an int64 device tensor."""
    import torch
    n, F = 512, 37
    S = 8 * n
    x = signal(S, 4)
    st = draw_starts(S, n, F, 4)
    plan = capi.Plan(buffer_size=n, scalar_f64=True)
    try:
        ref = plan.extract_torch(torch.from_numpy(stacked(x, st, n)).cuda(), ["rms", "mfcc", "melBands"])
        xs = on_device(x)
        a = plan.extract_gather_torch(xs, st, ["rms", "mfcc", "melBands"])
        b = plan.extract_gather_torch(xs, starts_tensor(st), ["rms", "mfcc", "melBands"])
        torch.cuda.synchronize()
        same_device(a, ref, "numpy starts")
        same_device(b, ref, "tensor starts")
    finally:
        plan.close()
