#!/usr/bin/env python3
"""Timing of the signal launches (mgx_extract_signal_*: overlapping buffers read in place at a hop) in ONE
process, interleaved rounds (cdna_hip_programming.md §5.4 rule 24), medians of per-round means:

 1. the signal launch at hop = N against mgx_extract_device on the same frames (the run-time stride's cost);
 2. what the hop buys, hop in {N, N/2, N/4} at a fixed frame count: the signal launch with the frames' loads
    forced non-temporal and forced plain (MGX_NT_MIN_MB, read at plan creation), the same frame count dense,
    and the device copy that materialises the dense frames (what a caller had to do before);
 3. the host path: mgx_extract_signal_host against mgx_extract_host of host-materialised frames, wall clock.

usage: signal_bench.py [--n N] [--frames F] [--rounds R] [--launches K] [--host-frames F] [--skip-host]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meyda_amd import capi  # noqa: E402

TIME_ONLY = ["rms", "energy", "zcr"]


def plan_with(env, **kw):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return capi.Plan(**kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def timed(fn, launches):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(launches):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def interleaved(variants, rounds, launches):
    """variants: [(name, fn)]; returns {name: [per-round ms per launch]} after a warm-up of every variant."""
    for _ in range(2):
        for _, fn in variants:
            for _ in range(launches):
                fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            res[name].append(timed(fn, launches))
    return res


def report(res, F, base):
    b = np.median(res[base])
    for name, v in res.items():
        m = np.median(v)
        print("  %-22s median %8.4f ms  min %8.4f  max %8.4f  (%+5.1f %% vs %s)  %7.1f M frames/s" %
              (name, m, np.min(v), np.max(v), (m / b - 1) * 100, base, F / m / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=262144)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    n, F = a.n, a.frames
    print("signal_bench: N = %d, %d frames, %d rounds x %d launches, device %s" %
          (n, F, a.rounds, a.launches, torch.cuda.get_device_name(0)))
    # one signal long enough for hop = N; the shorter hops read its head
    sig = torch.empty(F, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(sig, 0x6D657964)
    sig = sig.view(-1)
    stream = torch.cuda.current_stream().cuda_stream
    default = capi.Plan(buffer_size=n)
    nt = plan_with({"MGX_NT_MIN_MB": 0}, buffer_size=n)
    plain = plan_with({"MGX_NT_MIN_MB": 1 << 20}, buffer_size=n)

    for label, feats in (("all features", capi.ALL_FEATURES), ("time-only (rms, energy, zcr)", TIME_ONLY)):
        outs, o = default.alloc_outputs(F, feats)
        print("\n== 1. hop = N against mgx_extract_device on the same frames, %s" % label)
        res = interleaved([
            ("dense", lambda: default.extract_device(sig.data_ptr(), F, o, stream)),
            ("signal hop=N", lambda: default.extract_signal_device(sig.data_ptr(), F * n, n, o, stream)),
        ], a.rounds, a.launches)
        report(res, F, "dense")
        d = res["dense"]
        print("  (spread of the dense launch's own per-round means: %.2f %% of its median)" %
              ((np.max(d) - np.min(d)) / np.median(d) * 100))
        ref = {k: t.clone() for k, t in outs.items()}
        for t in outs.values():
            t.fill_(float("nan"))
        default.extract_device(sig.data_ptr(), F, o, stream)
        torch.cuda.synchronize()
        same = all(torch.equal(outs[k].view(torch.int32), ref[k].view(torch.int32)) for k in outs)
        print("  outputs of the two: %s" % ("identical" if same else "DIFFER"))

        print("\n== 2. what the hop buys, %s, %d frames each" % (label, F))
        for hop in (n, n // 2, n // 4):
            S = (F - 1) * hop + n
            x = sig[:S]
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dense = x.unfold(0, n, hop).contiguous()  # (warm-up: the allocation)
            torch.cuda.synchronize()
            mat = []
            for _ in range(a.rounds):
                t0.record()
                dense.copy_(x.unfold(0, n, hop))
                t1.record()
                torch.cuda.synchronize()
                mat.append(t0.elapsed_time(t1))
            print(" hop = %d: the signal is %.0f MiB, its dense frames %.0f MiB; materialising them on the device: "
                  "median %.3f ms" % (hop, S * 4 / 2 ** 20, F * n * 4 / 2 ** 20, np.median(mat)))
            res = interleaved([
                ("dense (materialised)", lambda: default.extract_device(dense.data_ptr(), F, o, stream)),
                ("signal nt", lambda: nt.extract_signal_device(x.data_ptr(), S, hop, o, stream)),
                ("signal plain", lambda: plain.extract_signal_device(x.data_ptr(), S, hop, o, stream)),
                ("signal default", lambda: default.extract_signal_device(x.data_ptr(), S, hop, o, stream)),
            ], a.rounds, a.launches)
            report(res, F, "dense (materialised)")
            del dense

    if not a.skip_host:
        hop, Fh = n // 4, a.host_frames
        print("\n== 3. host path, N = %d, hop = %d, %d frames, all features, wall clock per call" % (n, hop, Fh))
        x = sig[:(Fh - 1) * hop + n].cpu().numpy()
        t = time.perf_counter()
        dense = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(x, n)[::hop])
        print("  materialising the frames on the host: %.1f ms (%.0f MiB from %.0f MiB)" %
              ((time.perf_counter() - t) * 1e3, dense.nbytes / 2 ** 20, x.nbytes / 2 ** 20))
        for name, fn in (("mgx_extract_host (dense)", lambda: default.extract(dense, capi.ALL_FEATURES)),
                         ("mgx_extract_signal_host", lambda: default.extract_signal(x, hop, capi.ALL_FEATURES))):
            fn()  # (staging allocated)
            ts = []
            for _ in range(a.host_reps):
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
            print("  %-26s median %8.1f ms  min %8.1f  (%.1f M frames/s)" % (name, np.median(ts), np.min(ts), Fh / np.median(ts) / 1e3))
    for p in (default, nt, plain):
        p.close()


if __name__ == "__main__":
    main()
