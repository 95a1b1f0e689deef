#!/usr/bin/env python3
"""The measurements of profiles/chroma.txt on one MI355X: what the chroma operator (mgx_chroma_device) and the host
route (mgx_chroma_host) cost, against forming the same rows with torch (device) or numpy (host) -- what a caller has
without them --, and that the existing launches did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all).

O. the operator alone on the launch's amplitudeSpectrum rows (262,144 x 512), the library's bank at C = 12 and at
   C = 36, both norms, against torch on the device: rows.double() @ W.double().T and the max-normalisation, and a
   float32 matmul (the price of the fixed float64 order), with mgx_flux_device on the same array in the same process
   as the yardstick. torch sums in another order, so the two are compared within the definition's bound, (ceil(cols
   / 64) + 5) 2^-53 relative (every product is non-negative), plus a float32 rounding each. Bytes: the array once.
H. host, wall clock: mgx_chroma_host (per frame and pooled) against mgx_extract_gather_host of the amplitude
   spectrum + numpy (the matmul, the normalisation, the pooling), and against mgx_extract_gather_host alone.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: chroma_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections OHA] [--host-reps R]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meyda_amd import capi  # noqa: E402
import gather_bench as gb  # noqa: E402
from summary_bench import N, HOP, NSIG, PER, corpus  # noqa: E402

SR = 44100.0


def torch_chroma(r, w, norm, dtype):
    s = r.to(dtype) @ w.to(dtype).T
    if norm:
        m = s.max(dim=1, keepdim=True).values
        s = torch.where((m > 0) & m.isfinite(), s / m, s)
    return s.to(torch.float32)


def section_o(rounds, launches):
    x, starts, fo = corpus()
    F = starts.size
    stream = torch.cuda.current_stream().cuda_stream
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N)
    r = plan.extract_gather_torch(x, starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]
    torch.cuda.synchronize()
    plan.close()
    cols = r.shape[1]
    flux = torch.zeros(F, dtype=torch.float32, device="cuda")
    array = 4 * F * cols
    for C in (12, 36):
        w = torch.from_numpy(capi.chroma_weights(N, SR, num_chroma=C)).cuda()
        out = torch.zeros((F, C), dtype=torch.float32, device="cuda")
        keep = {}

        def op(norm):
            return lambda: capi.chroma_device(r.data_ptr(), F, cols, w.data_ptr(), C, norm, out.data_ptr(), stream)

        def with_torch(dtype):
            def fn():
                keep["t"] = torch_chroma(r, w, 1, dtype)
            return fn

        def flux_op():
            capi.flux_device(r.data_ptr(), F, cols, False, tb.data_ptr(), NSIG, 0, 1, flux.data_ptr(), stream)

        print("\n== O. the operator alone: C = %d, %d rows x %d columns float32 (%.1f MB), the bank %.0f KB" %
              (C, F, cols, array / 1e6, 4 * C * cols / 1024))
        variants = [("mgx_chroma_device, max", op(1)), ("mgx_chroma_device, none", op(0)), ("mgx_flux_device (the yardstick)", flux_op),
                    ("torch float64 matmul + max", with_torch(torch.float64)), ("torch float32 matmul + max", with_torch(torch.float32)),
                    ("mgx_chroma_device, max (again)", op(1)), ("mgx_flux_device (again)", flux_op)]
        res = gb.interleaved(variants, rounds, launches, warm=2)
        gb.report(res, F)
        med = {k: float(np.median(v)) for k, v in res.items()}
        for k in ("mgx_chroma_device, max", "mgx_chroma_device, none", "mgx_flux_device (the yardstick)"):
            print("  %-34s %.1f MB (the array once) in %.4f ms: %.2f TB/s" % (k, array / 1e6, med[k], array / med[k] / 1e9))
        flops = 2.0 * F * cols * C
        print("  %.2f GFLOP of float64: %.1f TFLOP/s; torch float64 takes %.1f times as long, torch float32 %.2f times" %
              (flops / 1e9, flops / med["mgx_chroma_device, max"] / 1e9, med["torch float64 matmul + max"] / med["mgx_chroma_device, max"],
               med["torch float32 matmul + max"] / med["mgx_chroma_device, max"]))
        bound = (-(-cols // 64) + 5) * 2.0 ** -53 + 2.0 ** -23
        for norm, label in ((0, "none"), (1, "max")):
            op(norm)()
            t = torch_chroma(r, w, norm, torch.float64)
            torch.cuda.synchronize()
            rel = float(((out.double() - t.double()).abs() / t.double().abs().clamp_min(1e-300)).nan_to_num(0.0).max())
            # (norm max divides two sums: twice the bound)
            lim = bound * (2 if norm else 1)
            print("  norm %-5s against torch float64: largest relative difference %.3g (bound %.3g): %s" %
                  (label, rel, lim, "inside" if rel <= lim else "OUTSIDE"))
            if not rel <= lim:
                sys.exit("chroma_bench: C = %d, norm %s differs from torch by more than the definition's bound" % (C, label))


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N)
    w = capi.chroma_weights(N, SR)
    seg = fo[:-1].astype(np.int64)
    per = np.diff(fo.astype(np.int64))
    cnt = per.astype(np.float64)[:, None]
    got = {}

    def chroma():
        got["lib"] = plan.chroma(xh, starts, fo, weights=w, summary=True)

    def gather():
        got["amp"] = plan.extract_gather(xh, starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]

    def gather_numpy():
        gather()
        s = got["amp"].astype(np.float64) @ w.astype(np.float64).T
        m = s.max(axis=1, keepdims=True)
        with np.errstate(all="ignore"):
            c = np.where((m > 0) & np.isfinite(m), s / m, s)
        mean = np.add.reduceat(c, seg) / cnt
        d = c - np.repeat(mean, per, axis=0)
        got["numpy"] = (c.astype(np.float32), np.stack([mean, np.add.reduceat(d * d, seg) / cnt, np.minimum.reduceat(c, seg),
                                                         np.maximum.reduceat(c, seg)], axis=1))

    print("\n== H. host, wall clock per corpus (%d buffers, %d clips; C = 12, per frame and pooled)" % (F, NSIG))
    variants = [("mgx_chroma_host", chroma), ("mgx_extract_gather_host(amplitudeSpectrum) + numpy", gather_numpy),
                ("mgx_extract_gather_host(amplitudeSpectrum) alone", gather)]
    chroma()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-52s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f" % (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v)))
    with np.errstate(all="ignore"):
        rows, st = got["numpy"]
        a = float(np.nan_to_num(np.abs(got["lib"]["chroma"] - rows) / (np.abs(rows) + 1e-300)).max())
        b = float(np.nan_to_num(np.abs(got["lib"]["summary"] - st) / (np.abs(st) + 1e-300)).max())
    print("  largest relative difference between the two routes: per frame %.3g, statistics %.3g" % (a, b))
    print("  bytes that cross back: %.1f MB of chroma rows and %.2f MB of summaries, against %.1f MB of spectra" %
          (4 * F * 12 / 1e6, 8 * NSIG * 4 * 12 / 1e6, 4 * F * (N // 2) / 1e6))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="OHA")
    a = ap.parse_args()
    print("command: tools/chroma_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches; corpus %d clips x %d buffers, N = %d, hop %d" %
          (torch.cuda.get_device_name(0), a.rounds, a.launches, NSIG, PER, N, HOP))
    if "O" in a.sections:
        section_o(a.rounds, a.launches)
        torch.cuda.empty_cache()
    if "H" in a.sections:
        section_h(a.host_reps)
        torch.cuda.empty_cache()
    if "A" in a.sections:
        P, T = gb.load_parent(a.parent), capi.lib()
        for rep in (1, 2):
            for n, label in ((1024, "N = 1024, all features (the headline)"), (2048, "N = 2048, all features (C5)")):
                gb.section_a(P, T, n, 262144, n, capi.ALL_FEATURES, "%s, measurement %d" % (label, rep), a.rounds, a.launches)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
