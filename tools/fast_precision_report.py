#!/usr/bin/env python3
"""What precision="fast" costs, measured: per buffer size and per kind of input (tests/fast_ref.py frames), the
worst distance of its spectrum from the exact transform beside the bar tests/test_gpu_fast.py holds it to, the
worst distance from the CPU oracle's spectrum beside the project's 1e-5, and for every scalar feature, the mfcc
and the specific loudness the worst deviation from the oracle's OWN features (the reference's values on the same
frames, not the features of the returned spectrum the tests compare with). The last table is what "fails the bar
off broadband input" means. Nothing here is asserted. Needs a GPU and the built libraries.

usage: python tools/fast_precision_report.py > profiles/fast_precision.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import fast_ref  # noqa: E402
from meyda_amd import capi  # noqa: E402
from oracle import oracle  # noqa: E402

SCALARS = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope", "spectralRolloff",
           "spectralSpread", "spectralSkewness", "spectralKurtosis", "loudness.total", "perceptualSpread",
           "perceptualSharpness"]
FEATS = SCALARS[:10] + ["loudness", "perceptualSpread", "perceptualSharpness", "mfcc", "amplitudeSpectrum", "complexSpectrum"]
KINDS = [k for k in fast_ref.KINDS if k != "silent"]


def rel_elem(g, r):
    """Largest |g - r| / |r| over the finite, non-zero reference elements (NaN, printed "-", when there is none)."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    m = np.isfinite(r) & np.isfinite(g) & (r != 0)
    return float(np.max(np.abs(g[m] - r[m]) / np.abs(r[m]))) if m.any() else float("nan")


def rel_vec(g, r):
    """Largest |g - r| / max(|r|, ||r||_inf of the frame) over the finite reference elements (the vector policy's
    scale, tests/tolerance.py check_vectors)."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    m = np.isfinite(r) & np.isfinite(g)
    norm = np.max(np.where(np.isfinite(r), np.abs(r), 0), 1, keepdims=True)
    scale = np.maximum(np.abs(r), norm)
    m &= scale > 0
    return float(np.max(np.abs(g[m] - r[m]) / scale[m])) if m.any() else float("nan")


def ratios(got, ex):
    """Per frame ||got - exact||_2 / ||exact||_2 (0 where the exact spectrum is 0)."""
    err = np.sqrt((np.abs(got - ex) ** 2).sum(1))
    norm = np.sqrt((np.abs(ex) ** 2).sum(1))
    return np.where(norm > 0, err / np.where(norm > 0, norm, 1), 0.0)


def row(name, vals):
    print("  %-22s" % name + "".join(" %-11s" % ("-" if v != v else "%.3g" % v) for v in vals))


def main():
    print("precision=\"fast\" against the exact transform, the CPU oracle's spectrum and the CPU oracle's own features: %d"
          " frames per N (tests/fast_ref.py), hanning, 44.1 kHz, 26 mel bands, float64 scalars. One column per kind of"
          " frame (the silent frame left out: its spectrum is zero on both sides); every figure the worst over the kind's"
          " frames. Scalars: |d| / |ref| over finite non-zero reference values; loudness.specific and mfcc: |d| /"
          " max(|ref|, ||ref||_inf of the frame). The tests' bar on a feature is 1e-5 (tests/tolerance.py), against the"
          " oracle's features of the RETURNED spectrum; the rows below the spectrum are against the oracle's own features"
          " and are not held to it; \"-\": the reference has no finite non-zero value there (the mfcc at N = 256, where a mel band"
          " holds no bin)." % fast_ref.F)
    for n in fast_ref.SIZES:
        x, kinds = fast_ref.frames(n), fast_ref.kinds(n)
        w = capi.host_tables(buffer_size=n)["window"]
        ex = fast_ref.exact(x, w)
        ref = oracle.extract(x)
        plan = capi.Plan(buffer_size=n, precision="fast", scalar_f64=True)
        out = plan.extract(x, FEATS)
        plan.close()
        amp = out["amplitudeSpectrum"].astype(np.float64)
        ra = ratios(amp, np.abs(ex[:, :n // 2]))
        rc = ratios(fast_ref.complex_of(out), ex)
        r = ref["amp"].astype(np.float64)
        norm = np.abs(r).max(1)
        ri = np.where(norm > 0, np.abs(amp - r).max(1) / np.where(norm > 0, norm, 1), 0.0)
        print("\nN = %d   (bar against the exact transform: %.3g; against the oracle's spectrum: 1e-05)" % (n, fast_ref.spectrum_bar(n)))
        print("  %-22s" % "" + "".join(" %-11s" % k for k in KINDS))
        sel = [kinds == k for k in KINDS]
        row("frames", [s.sum() for s in sel])
        row("amp vs exact, 2-norm", [ra[s].max() for s in sel])
        row("complex vs exact", [rc[s].max() for s in sel])
        row("amp vs oracle, inf", [ri[s].max() for s in sel])
        for j, k in enumerate(SCALARS):
            row(k, [rel_elem(out[k][s], ref["scalars"][s, j]) for s in sel])
        row("loudness.specific", [rel_vec(out["loudness.specific"][s], ref["loudness_specific"][s]) for s in sel])
        row("mfcc", [rel_vec(out["mfcc"][s], ref["mfcc"][s]) for s in sel])
        print("  worst over all frames: amplitude %.3g of the bar, complex %.3g of the bar"
              % (ra.max() / fast_ref.spectrum_bar(n), rc.max() / fast_ref.spectrum_bar(n)))


if __name__ == "__main__":
    main()
