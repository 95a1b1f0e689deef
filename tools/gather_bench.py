#!/usr/bin/env python3
"""The measurements of profiles/gather_starts.txt on one MI355X: what a launch over a table of starts
(mgx_extract_gather_*) costs, and that the launches which do not use one did not move.

A. unchanged launches: the tree's library against a build of the parent revision (tools/build_rev.sh REV NAME ->
   ab/lib_NAME.so), two plans of each so the spread between equal builds shows beside the difference; outputs
   compared bit for bit.
B. the gather launch with starts = f * hop against the signal launch at that hop (8 more bytes read per buffer).
C. the case it exists for: 1,024 signals of N + 255 hop samples (262,144 buffers): one gather launch against 1,024
   signal launches back to back on one stream (the corpus timed twice per round, the one launch 20 times), with the
   frames' loads forced plain and forced non-temporal; and on
   the host one mgx_extract_gather_host call against 1,024 mgx_extract_signal_host calls, wall clock.

Every variant of a section runs in one process, in interleaved rounds (device events); per variant the median, min
and spread (max - min over the rounds) are printed: a difference is read against that spread.
usage: gather_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--no-host] [--sections ABC] [--ahead LIB]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meyda_amd import capi  # noqa: E402

TIME_ONLY = ["rms", "energy", "zcr"]


def load_parent(path):
    L = ctypes.CDLL(path)
    L.mgx_plan_create.argtypes = [ctypes.POINTER(capi.PlanDesc), ctypes.POINTER(ctypes.c_void_p)]
    L.mgx_plan_destroy.argtypes = [ctypes.c_void_p]
    L.mgx_extract_signal_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                            ctypes.POINTER(capi.Outputs), ctypes.c_void_p]
    L.mgx_last_error.restype = ctypes.c_char_p
    if hasattr(L, "mgx_extract_gather_device"):  # (a build of this tree: --ahead)
        L.mgx_extract_gather_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.POINTER(capi.Outputs), ctypes.c_void_p, ctypes.c_void_p]
    return L


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


class RawPlan:
    """A plan of library L (the parent's or the tree's) with outputs for F frames; launches are signal launches
    (a dense batch is the signal at hop N: the same launch)."""

    def __init__(self, L, n, F, feats):
        self.L, self.n, self.F = L, n, F
        d = capi.make_desc(buffer_size=n)
        self.h = ctypes.c_void_p()
        rc = L.mgx_plan_create(ctypes.byref(d), ctypes.byref(self.h))
        assert rc == 0, (rc, L.mgx_last_error())
        lay = capi.Plan.__new__(capi.Plan)  # (alloc_outputs only)
        lay.desc, lay.n, lay.scalar_dtype, lay._h = d, n, np.float32, None
        self.out, self.o = lay.alloc_outputs(F, feats)

    def signal(self, x, S, hop, stream):
        rc = self.L.mgx_extract_signal_device(self.h, ctypes.c_void_p(x.data_ptr()), S, hop, ctypes.byref(self.o), ctypes.c_void_p(stream))
        assert rc == 0, (rc, self.L.mgx_last_error())

    def gather(self, x, S, st, stream):
        rc = self.L.mgx_extract_gather_device(self.h, ctypes.c_void_p(x.data_ptr()), S, ctypes.c_void_p(st.data_ptr()), self.F,
                                              ctypes.byref(self.o), None, ctypes.c_void_p(stream))
        assert rc == 0, (rc, self.L.mgx_last_error())

    def close(self):
        self.L.mgx_plan_destroy(self.h)
        self.out = None


def timed(fn, launches):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(launches):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def interleaved(variants, rounds, launches, warm=3):
    """variants: (name, fn) or (name, fn, calls): fn is called `launches` (or `calls`) times per timing."""
    variants = [(v[0], v[1], v[2] if len(v) > 2 else launches) for v in variants]
    for _ in range(warm):  # clock settle, every variant's code loaded and scratch allocated
        for _, fn, k in variants:
            for _ in range(k):
                fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, k in variants:
            res[name].append(timed(fn, k))
    return res


def report(res, F):
    names = list(res)
    b = np.median(res[names[0]])
    for name in names:
        v = res[name]
        m = np.median(v)
        print("  %-30s median %9.4f ms  min %9.4f  spread %7.4f  (%+6.2f %% vs %s)  %7.1f M frames/s" %
              (name, m, np.min(v), np.max(v) - np.min(v), (m / b - 1) * 100, names[0], F / m / 1e3))


def same_outputs(a, b):
    keys = sorted(a)
    diff = [k for k in keys if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    return "%d arrays %s" % (len(keys), "identical, bit for bit" if not diff else "DIFFER in %s" % diff)


def section_a(P, T, n, F, hop, feats, label, rounds, launches):
    S = (F - 1) * hop + n
    x = torch.empty((S + n - 1) // n, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x, 0x6D657964)
    x = x.view(-1)[:S]
    stream = torch.cuda.current_stream().cuda_stream
    ps = [("parent", RawPlan(P, n, F, feats)), ("new", RawPlan(T, n, F, feats)),
          ("parent (second plan)", RawPlan(P, n, F, feats)), ("new (second plan)", RawPlan(T, n, F, feats))]
    print("\n== A. unchanged launches: %s, %d frames" % (label, F))
    res = interleaved([(name, (lambda p=p: p.signal(x, S, hop, stream))) for name, p in ps], rounds, launches)
    report(res, F)
    med = {k: np.median(v) for k, v in res.items()}
    print("  parent against itself: %+.2f %%; new against parent: %+.2f %% (first plans), %+.2f %% (second plans)" %
          ((med["parent (second plan)"] / med["parent"] - 1) * 100, (med["new"] / med["parent"] - 1) * 100,
           (med["new (second plan)"] / med["parent (second plan)"] - 1) * 100))
    for _, p in ps[:2]:
        for t in p.out.values():
            t.fill_(float("nan"))
        p.signal(x, S, hop, stream)
    torch.cuda.synchronize()
    print("  outputs of parent and new: %s" % same_outputs(ps[0][1].out, ps[1][1].out))
    for _, p in ps:
        p.close()


def section_b(n, F, rounds, launches, ahead=None):
    stream = torch.cuda.current_stream().cuda_stream
    plan = capi.Plan(buffer_size=n)
    x = torch.empty(F, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x, 0x6D657964)
    x = x.view(-1)
    for label, feats in (("all features", capi.ALL_FEATURES), ("time-only (rms, energy, zcr)", TIME_ONLY)):
        for hop in (n, n // 4):
            S = (F - 1) * hop + n
            st = (torch.arange(F, dtype=torch.int64, device="cuda") * hop).contiguous()
            outs, o = plan.alloc_outputs(F, feats)
            outg, og = plan.alloc_outputs(F, feats)
            print("\n== B. starts = f * %d against the signal launch at hop %d, %s, N = %d, %d frames (+%.1f MiB of starts)" %
                  (hop, hop, label, n, F, F * 8 / 2 ** 20))
            # --ahead: the same launch from a build with -DMGX_GATHER_AHEAD_ALL=1 (the next start kept a frame ahead
            # at every N, not at N = 2048 alone)
            ap = RawPlan(ahead, n, F, feats) if ahead is not None else None
            extra = [("gather, start a frame ahead", lambda: ap.gather(x, S, st, stream)),
                     ("gather, start a frame ahead (again)", lambda: ap.gather(x, S, st, stream))] if ap else []
            res = interleaved([
                ("signal", lambda: plan.extract_signal_device(x.data_ptr(), S, hop, o, stream)),
                ("gather", lambda: plan.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)),
                ("signal (again)", lambda: plan.extract_signal_device(x.data_ptr(), S, hop, o, stream)),
                ("gather (again)", lambda: plan.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)),
            ] + extra, rounds, launches)
            report(res, F)
            print("  outputs of the two: %s" % same_outputs(outs, outg))
            if ap:
                print("  outputs of the build that keeps the start ahead: %s" % same_outputs(outs, ap.out))
                ap.close()
    plan.close()


def section_c(n, hop, nsig, per, rounds, launches, host):
    F = nsig * per
    L = n + (per - 1) * hop
    S = nsig * L
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.empty((S + n - 1) // n, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x, 0x6D657964)
    x = x.view(-1)[:S]
    starts, fo = capi.signals_frame_starts([L] * nsig, n, hop)
    assert starts.size == F and fo[-1] == F
    st = torch.from_numpy(starts.view(np.int64)).cuda()
    default = capi.Plan(buffer_size=n)
    nt = plan_with({"MGX_NT_MIN_MB": 0}, buffer_size=n)
    plain = plan_with({"MGX_NT_MIN_MB": 1 << 20}, buffer_size=n)
    print("\n== C. %d signals of %d samples (N = %d, hop %d: %d buffers each, %d in all; %.0f MiB of samples)" %
          (nsig, L, n, hop, per, F, S * 4 / 2 ** 20))
    for label, feats in (("all features", capi.ALL_FEATURES), ("time-only (rms, energy, zcr)", TIME_ONLY)):
        outs, o = default.alloc_outputs(F, feats)
        outg, og = default.alloc_outputs(F, feats)
        # the per-signal launches write their rows of the same arrays: an Outputs per signal, built once
        ss = 4
        per_sig = []
        for s in range(nsig):
            q = capi.Outputs()
            for k in range(capi.NUM_SCALARS):
                if o.scalars[k]:
                    q.scalars[k] = o.scalars[k] + s * per * ss
            if o.loudness_specific:
                q.loudness_specific = o.loudness_specific + s * per * capi.NUM_BARK * 4
            if o.mfcc:
                q.mfcc = o.mfcc + s * per * default.desc.num_mfcc_coeffs * 4
            per_sig.append(q)

        def signals():
            for s in range(nsig):
                default.extract_signal_device(x.data_ptr() + s * L * 4, L, hop, per_sig[s], stream)

        print(" device, %s:" % label)
        res = interleaved([
            ("%d signal launches" % nsig, signals, 2),
            ("one gather launch", lambda: default.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)),
            ("one gather launch, plain", lambda: plain.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)),
            ("one gather launch, nt", lambda: nt.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)),
        ], rounds, launches, warm=2)
        report(res, F)
        for t in list(outs.values()) + list(outg.values()):
            t.fill_(float("nan"))
        signals()
        default.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, og, stream)
        torch.cuda.synchronize()
        print("  outputs of the %d launches and of the one: %s" % (nsig, same_outputs(outs, outg)))
    if host:
        xh = x.cpu().numpy()
        feats = capi.ALL_FEATURES
        ref, ro = default._host_outputs(F, feats)
        sd = np.float32
        per_sig = []
        for s in range(nsig):
            q = capi.Outputs()
            for k in range(capi.NUM_SCALARS):
                if ro.scalars[k]:
                    q.scalars[k] = ro.scalars[k] + s * per * np.dtype(sd).itemsize
            q.loudness_specific = ro.loudness_specific + s * per * capi.NUM_BARK * 4
            q.mfcc = ro.mfcc + s * per * default.desc.num_mfcc_coeffs * 4
            per_sig.append(q)
        L_ = capi.lib()

        def host_signals():
            for s in range(nsig):
                capi.check(L_.mgx_extract_signal_host(default._h, xh.ctypes.data + s * L * 4, L, hop, ctypes.byref(per_sig[s])))

        got = {}

        def host_gather():
            got.update(default.extract_gather(xh, starts, feats))

        print(" host, all features, wall clock per corpus:")
        for name, fn in (("%d mgx_extract_signal_host calls" % nsig, host_signals), ("one mgx_extract_gather_host call", host_gather)):
            fn()  # (staging allocated)
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t) * 1e3)
            print("  %-36s median %9.1f ms  min %9.1f  max %9.1f  (%.2f M frames/s)" %
                  (name, np.median(ts), np.min(ts), np.max(ts), F / np.median(ts) / 1e3))
        diff = [k for k in ref if not np.array_equal(ref[k].view(np.uint32), got[k].view(np.uint32))]
        print("  outputs of the two routes: %d arrays %s" % (len(ref), "identical, bit for bit" if not diff else "DIFFER in %s" % diff))
    for p in (default, nt, plain):
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--sections", default="ABC")
    ap.add_argument("--ahead", default=None, help="a build of this tree with -DMGX_GATHER_AHEAD_ALL=1, timed beside the tree's in B")
    a = ap.parse_args()
    F = a.frames
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "A" in a.sections:
        P, T = load_parent(a.parent), capi.lib()
        for n, hop, feats, label in ((1024, 1024, capi.ALL_FEATURES, "N = 1024, all features (the headline)"),
                                     (2048, 2048, capi.ALL_FEATURES, "N = 2048, all features"),
                                     (512, 512, TIME_ONLY, "N = 512, time-only (rms, energy, zcr)"),
                                     (1024, 256, TIME_ONLY, "the signal launch, N = 1024 at hop 256, time-only")):
            section_a(P, T, n, F, hop, feats, label, a.rounds, a.launches)
            torch.cuda.empty_cache()
    if "B" in a.sections:
        section_b(1024, F, a.rounds, a.launches, load_parent(a.ahead) if a.ahead else None)
        torch.cuda.empty_cache()
    if "C" in a.sections:
        section_c(1024, 256, 1024, 256, a.rounds, a.launches, not a.no_host)


if __name__ == "__main__":
    main()
