#!/usr/bin/env python3
"""The measurements of profiles/mel_bands.txt on one MI355X: what the melBands output (mgx_aux_outputs.mel_bands)
costs, and that launches which do not ask for it did not move.

A. unchanged launches: the tree's library against a build of the parent revision (tools/build_rev.sh REV NAME ->
   ab/lib_NAME.so), the same feature list on both, outputs compared bit for bit.
B. what it costs: at 262,144 x 1024 and 40 bands ["melBands"] and ["mfcc", "melBands"] against ["mfcc"] (the
   parent's too); at 26 bands every feature with and without it.
C. the use case: a log-mel spectrogram of a host signal at hop N/4, mgx_extract_host_ex returning melBands only,
   against the parent's route (power spectrum out over PCIe, the filterbank and log in numpy on the host).

Every variant of a section runs in one process, in interleaved rounds of 20 launches (device events); per variant
the median, min and spread (max - min over the rounds) are printed: a difference is read against that spread.
usage: mel_bands_bench.py [--parent ab/lib_parent.so] [--rounds R] [--no-host]"""
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
    L.mgx_extract_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(capi.Outputs),
                                     ctypes.c_void_p]
    L.mgx_extract_signal_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                          ctypes.POINTER(capi.Outputs)]
    L.mgx_last_error.restype = ctypes.c_char_p
    return L


class Variant:
    """One library, one plan, one feature list over the shared frames."""

    def __init__(self, name, L, n, F, feats, mel):
        self.name, self.L, self.F, self.n = name, L, F, n
        d = capi.make_desc(buffer_size=n, num_mel_bands=mel)
        self.h = ctypes.c_void_p()
        rc = L.mgx_plan_create(ctypes.byref(d), ctypes.byref(self.h))
        assert rc == 0, (name, rc, L.mgx_last_error())
        self.layout = capi.Plan.__new__(capi.Plan)  # (alloc_outputs only: the launches go through self.L)
        self.layout.desc, self.layout.n, self.layout.scalar_dtype, self.layout._h = d, n, np.float32, None
        self.out, self.o = self.layout.alloc_outputs(F, feats)
        self.ms = []

    def launch(self, x, stream):
        aux = capi._aux(self.o)
        if aux is None:
            rc = self.L.mgx_extract_device(self.h, ctypes.c_void_p(x.data_ptr()), self.F, ctypes.byref(self.o),
                                           ctypes.c_void_p(stream))
        else:
            rc = self.L.mgx_extract_device_ex(self.h, ctypes.c_void_p(x.data_ptr()), self.F * self.n, self.n,
                                              ctypes.byref(self.o), ctypes.byref(aux), ctypes.c_void_p(stream))
        assert rc == 0, (self.name, rc, self.L.mgx_last_error())

    def close(self):
        self.L.mgx_plan_destroy(self.h)
        self.out = None


def section(title, x, variants, rounds, compare=()):
    s = torch.cuda.current_stream()
    print("\n== %s" % title)
    for _ in range(3):  # clock settle, every variant's code loaded and scratch allocated
        for v in variants:
            for _ in range(20):
                v.launch(x, s.cuda_stream)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(20):
                v.launch(x, s.cuda_stream)
            e1.record(s)
            torch.cuda.synchronize()
            v.ms.append(e0.elapsed_time(e1) / 20)
    base = np.median(variants[0].ms)
    for v in variants:
        m = np.median(v.ms)
        print("%-34s median %.4f ms  min %.4f  spread %.4f  (%+.2f %% vs %s)  %.1f M frames/s" %
              (v.name, m, np.min(v.ms), np.max(v.ms) - np.min(v.ms), (m / base - 1) * 100, variants[0].name, v.F / m / 1e3))
    for a, b in compare:
        for t in list(a.out.values()) + list(b.out.values()):
            t.fill_(float("nan"))
        a.launch(x, s.cuda_stream)
        b.launch(x, s.cuda_stream)
        torch.cuda.synchronize()
        keys = [k for k in a.out if k in b.out]
        diff = [k for k in keys if not torch.equal(a.out[k].view(torch.int32), b.out[k].view(torch.int32))]
        print("outputs of %s and %s (%d arrays): %s" % (a.name, b.name, len(keys), "identical, bit for bit" if not diff else "DIFFER in %s" % diff))
    for v in variants:
        v.close()


def host_use_case(parent, n, F, mel, reps):
    """Wall clock per call, each call ending with the log-mel rows in host memory."""
    hop = n // 4
    S = (F - 1) * hop + n
    x = np.random.default_rng(1).uniform(-1, 1, S).astype(np.float32)
    print("\n== C. log-mel spectrogram of a host signal: %d buffers of N = %d at hop %d (%d samples, %.0f MiB), %d bands" %
          (F, n, hop, S, S * 4 / 2 ** 20, mel))
    plan = capi.Plan(buffer_size=n, num_mel_bands=mel)
    new = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        got = plan.extract_signal(x, hop, ["melBands"])["melBands"]
        new.append((time.perf_counter() - t0) * 1e3)
    plan.close()
    # the parent's route: the power spectrum out (2 KB per buffer over PCIe), mfcc.js:40-65 on the host
    d = capi.make_desc(buffer_size=n, num_mel_bands=mel)
    h = ctypes.c_void_p()
    assert parent.mgx_plan_create(ctypes.byref(d), ctypes.byref(h)) == 0
    bins = capi.host_tables(buffer_size=n, num_mel_bands=mel)["mel_bins"]
    L = n // 2
    w = np.zeros((L, mel), np.float32)
    for j in range(mel):
        b0, b1, b2 = int(bins[j]), int(bins[j + 1]), int(bins[j + 2])
        for i in range(b0, min(b1, L)):
            w[i, j] = (i - b0) / (b1 - b0)
        for i in range(b1, min(b2, L)):
            w[i, j] = (b2 - i) / (b2 - b1)
    power = np.empty((F, L), np.float32)
    o = capi.Outputs()
    o.power_spectrum = power.ctypes.data
    old, fetch = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        rc = parent.mgx_extract_signal_host(h, x.ctypes.data, S, hop, ctypes.byref(o))
        t1 = time.perf_counter()
        assert rc == 0, parent.mgx_last_error()
        with np.errstate(divide="ignore"):
            ref = np.log(power @ w)  # (one float32 matrix product: the cheapest host filterbank, not the reference's order)
        old.append((time.perf_counter() - t0) * 1e3)
        fetch.append((t1 - t0) * 1e3)
    parent.mgx_plan_destroy(h)
    err = np.nanmax(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-5 * np.abs(ref).max(1, keepdims=True)))
    for name, t in (("new: mgx_extract_host_ex, melBands only", new), ("parent: power spectrum out + host filterbank", old),
                    ("  of which the parent's extract call", fetch)):
        t = t[1:]  # (the first call allocates the staging buffers)
        print("%-46s median %.1f ms  min %.1f  max %.1f per call" % (name, np.median(t), np.min(t), np.max(t)))
    print("largest relative difference between the two routes' rows: %.2e (float32 matrix product against the kernel's sums)" % err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=262144)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    P, T = load_parent(a.parent), capi.lib()
    F = a.frames
    print("device: %s; %d frames per launch; %d interleaved rounds of 20 launches" % (torch.cuda.get_device_name(0), F, a.rounds))
    for n, feats, label in ((1024, capi.ALL_FEATURES, "N = 1024, all features (the headline)"),
                            (2048, capi.ALL_FEATURES, "N = 2048, all features"), (512, TIME_ONLY, "N = 512, time-only (rms, energy, zcr)")):
        x = torch.empty(F, n, dtype=torch.float32, device="cuda")
        capi.synth_frames_device(x, 0x6D657964)
        # (parent, new, parent, new: two plans of each library, so the spread between equal builds shows beside the difference)
        vs = [Variant("parent", P, n, F, feats, 26), Variant("new", T, n, F, feats, 26),
              Variant("parent (second plan)", P, n, F, feats, 26), Variant("new (second plan)", T, n, F, feats, 26)]
        section("A. unchanged launches: %s, 26 bands" % label, x, vs, a.rounds, compare=[(vs[0], vs[1])])
        del x
    n = 1024
    x = torch.empty(F, n, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x, 0x6D657964)
    vs = [Variant("parent [mfcc]", P, n, F, ["mfcc"], 40), Variant("new [mfcc]", T, n, F, ["mfcc"], 40),
          Variant("new [melBands]", T, n, F, ["melBands"], 40), Variant("new [mfcc, melBands]", T, n, F, ["mfcc", "melBands"], 40)]
    section("B1. N = 1024, 40 bands: the mel path alone (52 B of mfcc / 160 B of melBands per frame)", x, vs, a.rounds,
            compare=[(vs[0], vs[1]), (vs[1], vs[3]), (vs[2], vs[3])])
    vs = [Variant("new all features", T, n, F, capi.ALL_FEATURES, 26), Variant("new all features + melBands", T, n, F, capi.ALL_FEATURES + ["melBands"], 26),
          Variant("parent all features", P, n, F, capi.ALL_FEATURES, 26)]
    section("B2. N = 1024, 26 bands: every feature with and without melBands (+104 B per frame)", x, vs, a.rounds,
            compare=[(vs[0], vs[1])])
    del x
    torch.cuda.empty_cache()
    if not a.no_host:
        host_use_case(P, 1024, F, 40, 3)


if __name__ == "__main__":
    main()
