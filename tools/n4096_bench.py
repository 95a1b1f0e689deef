#!/usr/bin/env python3
"""The measurements of profiles/n4096.txt on one MI355X: what a launch costs at bufferSize 4096.

A. 131,072 x 4096 against 262,144 x 2048 (C5's shard): the same 2 GiB of samples, read as buffers of either size,
   with every feature, with melBands alone and with rms + energy + zcr alone. Beside each ratio of times the
   FFT's flops per sample (5 N log2 N per frame: 12 / 11), the FP64 roofline fraction as README defines it (those
   flops over the time, against the 78.6 TFLOP/s peak) and the persistent grid (MGX_GRID_CAP=print: workgroups
   per CU).
B. the tail pool at 4096 (MGX_POOL_PCT 15 against 0), every feature.
C. --parent LIB: the existing sizes against a build of the parent revision (tools/build_rev.sh REV NAME ->
   ab/lib_NAME.so): the headline (262,144 x 1024), C5 and N = 256, outputs compared bit for bit; the times are read
   against the parent's own spread over the rounds.

Every variant of a section runs in one process, in interleaved rounds of 20 launches timed with device events
(tools/mel_bands_bench.py's section); median, min and spread (max - min over the rounds) per variant.
usage: n4096_bench.py [--parent ab/lib_parent.so] [--rounds R] [--frames F4096]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meyda_amd import capi  # noqa: E402
from mel_bands_bench import TIME_ONLY, Variant, load_parent, section  # noqa: E402

FP64_PEAK = 78.6e12  # README "FP64 roofline"


def fft_flops(n, F):
    return 5.0 * n * math.log2(n) * F


def variant(name, L, n, F, feats, env=None):
    """A Variant whose plan is created with `env` set (the knobs mgx_plan_create reads)."""
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Variant(name, L, n, F, feats, 26)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=131072, help="buffers of 4096 (twice as many of 2048)")
    ap.add_argument("--pool", type=int, nargs="+", default=[15, 0, 10, 25, 35], help="MGX_POOL_PCT values of section B")
    ap.add_argument("--only", default="ABC", help="sections to run")
    a = ap.parse_args()
    L = capi.lib()
    F4, F2 = a.frames, 2 * a.frames
    x = torch.empty(F4 * 4096, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x.view(F4, 4096), 0x6D657964)
    print("n4096_bench: %d x 4096 and %d x 2048 over the same %.2f GiB of samples, %d rounds of 20 launches" %
          (F4, F2, x.numel() * 4 / 2.0 ** 30, a.rounds))

    print("\n#### A. 4096 against 2048 (C5's shard), the same samples")
    for title, feats in () if "A" not in a.only else (("every feature", capi.ALL_FEATURES), ("melBands alone", ["melBands"]), ("rms + energy + zcr", TIME_ONLY)):
        v2 = variant("%d x 2048" % F2, L, 2048, F2, feats, {"MGX_GRID_CAP": "print"})
        v4 = variant("%d x 4096" % F4, L, 4096, F4, feats, {"MGX_GRID_CAP": "print"})
        section("A: %s" % title, x, [v2, v4], a.rounds)
        m2, m4 = np.median(v2.ms), np.median(v4.ms)
        print("ratio of times 4096 / 2048: %.3f (medians; mins %.3f); the FFT's flops per sample grow by 12 / 11 = %.3f" %
              (m4 / m2, np.min(v4.ms) / np.min(v2.ms), 12.0 / 11.0))
        if feats is not TIME_ONLY:
            for n, F, m in ((2048, F2, m2), (4096, F4, m4)):
                r = fft_flops(n, F) / (m * 1e-3)
                print("FP64 roofline at N = %d: %.1f TFLOP/s of FFT flops = %.3f of the %.1f TFLOP/s peak" %
                      (n, r / 1e12, r / FP64_PEAK, FP64_PEAK / 1e12))
        else:
            for n, F, m in ((2048, F2, m2), (4096, F4, m4)):
                print("samples read at N = %d: %.2f TB/s" % (n, F * n * 4 / (m * 1e-3) / 1e12))

    print("\n#### B. the tail pool at 4096")
    vs = [] if "B" not in a.only else [variant("pool %d %%" % p if p else "no pool", L, 4096, F4, capi.ALL_FEATURES, {"MGX_POOL_PCT": p}) for p in a.pool]
    if vs:
        section("B: every feature, MGX_POOL_PCT %s (15: the setting, 2048's)" % ", ".join(str(p) for p in a.pool), x, vs, a.rounds,
                compare=[(vs[0], v) for v in vs[1:]])

    if a.parent and "C" in a.only:
        P = load_parent(a.parent)
        print("\n#### C. the existing sizes against the parent build (%s)" % a.parent)
        for title, n, F in (("headline, 262,144 x 1024", 1024, 262144), ("C5, 262,144 x 2048", 2048, 262144),
                            ("N = 256, 262,144 frames", 256, 262144)):
            vp, vt = Variant("parent", P, n, F, capi.ALL_FEATURES, 26), Variant("this tree", L, n, F, capi.ALL_FEATURES, 26)
            section("C: %s, every feature" % title, x[:F * n].view(F, n), [vp, vt], a.rounds, compare=[(vp, vt)])
            d = np.median(vt.ms) - np.median(vp.ms)
            print("difference of medians %+.4f ms; the parent's own spread %.4f ms, this tree's %.4f ms: %s" %
                  (d, np.max(vp.ms) - np.min(vp.ms), np.max(vt.ms) - np.min(vt.ms),
                   "inside the parent's spread" if abs(d) <= np.max(vp.ms) - np.min(vp.ms) else "OUTSIDE the parent's spread"))


if __name__ == "__main__":
    main()
