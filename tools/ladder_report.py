#!/usr/bin/env python3
"""The record of the magnitude ladder (tests/ladder.py) on the GPU: per N the frames per regime, the share of
frames left out of the mel comparisons, the bit-exact fraction of the amplitudes and of the reference-order
MFCC coefficients, and the worst relative deviation of each output from the CPU oracle over the frames
tests/test_gpu_ladder.py compares it on. Needs a GPU and the built libraries.

usage: python tools/ladder_report.py > profiles/ladder.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ladder  # noqa: E402
from meyda_amd import capi  # noqa: E402
from oracle import oracle  # noqa: E402

SCALARS = ["rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope", "spectralRolloff",
           "spectralSpread", "spectralSkewness", "spectralKurtosis", "loudness.total", "perceptualSpread",
           "perceptualSharpness"]
FEATS = SCALARS[:10] + ["loudness", "perceptualSpread", "perceptualSharpness", "mfcc", "amplitudeSpectrum"]


def rel_elem(g, r, rows):
    """Largest |g - r| / |r| over the finite, non-zero reference elements of `rows`."""
    g, r = g[rows].astype(np.float64), r[rows].astype(np.float64)
    m = np.isfinite(r) & np.isfinite(g) & (r != 0)
    return float(np.max(np.abs(g[m] - r[m]) / np.abs(r[m]))) if m.any() else 0.0


def rel_norm(g, r, rows):
    """Largest per-frame ||g - r||_inf / ||r||_inf over the rows whose reference is finite and not all zero."""
    g, r = g[rows].astype(np.float64), r[rows].astype(np.float64)
    fin = np.isfinite(r).all(1) & np.isfinite(g).all(1)
    norm = np.abs(r[fin]).max(1)
    err = np.abs(g[fin] - r[fin]).max(1)
    return float(np.max(err[norm > 0] / norm[norm > 0])) if (norm > 0).any() else 0.0


def rel_vec(g, r, rows):
    """Largest |g - r| / max(|r|, ||r||_inf of the frame) over the finite reference elements of `rows` (the vector
    policy's scale, tests/tolerance.py check_vectors)."""
    g, r = g[rows].astype(np.float64), r[rows].astype(np.float64)
    m = np.isfinite(r) & np.isfinite(g)
    norm = np.max(np.where(np.isfinite(r), np.abs(r), 0), 1, keepdims=True)
    scale = np.maximum(np.abs(r), norm)
    m &= scale > 0
    return float(np.max(np.abs(g[m] - r[m]) / scale[m])) if m.any() else 0.0


def run(plan, n, feats):
    out = plan.extract(ladder.gpu_frames(n), feats)
    return {k: ladder.unpermute(v, n) for k, v in out.items()}


def main():
    print("magnitude ladder: %d ladder frames (5 bases x k = %d .. %d, permuted) + %d outliers per N; default plan,"
          % (ladder.NUM_LADDER, ladder.K_MIN, ladder.K_MAX, len(ladder.OUTLIER_K)))
    print("float64 scalars, against the CPU oracle. scalars and the reference-order mfcc: largest element-wise relative "
          "deviation over finite non-zero reference values (the cancelling formulas, slope / skewness / kurtosis, "
          "are held to an absolute term beside it: tests/tolerance.py); loudness.specific and mfcc: largest "
          "|d| / max(|ref|, ||ref||_inf of the frame); spectra: largest ||d||_inf / ||ref||_inf per frame. "
          "Frames whose reference spectrum holds a float32 denormal, or a NaN in bin 0 or N/4, are compared with the oracle's "
          "features of the spectrum the GPU returned (DESIGN.md §6): the second column")
    for n in ladder.SIZES:
        x = ladder.host_frames(n)
        ref = oracle.extract(x)
        lad = slice(0, ladder.NUM_LADDER)
        counts = ladder.regimes(x[lad], {"amp": ref["amp"][lad]}).sum(1)
        excl = ladder.mel_excluded(ref["amp"])
        amp64 = ref["amp"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            den = ((amp64 > 0) & (amp64 < 2.0 ** -126)).any(1)  # denormal spectra
        two = np.isnan(amp64[:, 0]) | np.isnan(amp64[:, n // 4])    # and the two bins of an overflowing frame
        every = ~den & ~two
        plan = capi.Plan(buffer_size=n, scalar_f64=True)
        out = run(plan, n, FEATS)
        plan.close()
        print("\nN = %d" % n)
        print("  frames per regime (of %d): %s" % (ladder.NUM_LADDER, ", ".join("%s: %d" % kv for kv in zip(ladder.REGIMES, counts.tolist()))))
        print("  mel_excluded share of the ladder: %.4f" % excl[lad].mean())
        a, r = out["amplitudeSpectrum"], ref["amp"]
        same = (a.view(np.uint32) == r.view(np.uint32)) | (np.isnan(a) & np.isnan(r))
        print("  compared with the reference's features: %d frames; with the oracle's features of the returned spectrum: "
              "%d with a denormal amplitude, %d with a NaN in bin 0 or N/4" % (int(every.sum()), int(den.sum()), int(two.sum())))
        err = np.abs(a[den].astype(np.float64) - amp64[den]).max(1)
        grid = np.log2(n) * 2.0 ** -149
        bar = np.maximum(1e-5 * amp64[den].max(1), grid)
        binds = bar == grid  # the norm-wise bar is finer than the float32 grid
        print("  amplitudeSpectrum: bit-exact on %.6f of the bins, %d of %d frames; worst norm-wise deviation %.3g outside the "
              "denormal spectra; inside, %.3g of the bar max(1e-5 ||ref||_inf, log2 N x 2^-149), and %g steps of 2^-149 on the "
              "%d frames where the steps are the bar" % (same.mean(), int(same.all(1).sum()), len(x), rel_norm(a, r, ~den),
                                                          (err / bar).max(), err[binds].max() / 2.0 ** -149, int(binds.sum())))
        own = oracle.features_from_amp(x[den | two], a[den | two])
        if n in (512, 1024, 2048):
            for bands in (26, 40):
                rb = oracle.extract(x, num_mel=bands)
                p = capi.Plan(buffer_size=n, num_mel_bands=bands, mfcc_reference=True)
                o = run(p, n, ["mfcc", "amplitudeSpectrum"])
                p.close()
                ok = ~excl
                g, rr = o["mfcc"][ok], rb["mfcc"][ok]
                s = (g.view(np.uint32) == rr.view(np.uint32)) | (np.isnan(g) & np.isnan(rr))
                print("  reference-order mfcc, %d bands: bit-exact on %.6f of the coefficients of the %d compared frames; "
                      "worst deviation %.3g" % (bands, s.mean(), int(ok.sum()), rel_elem(o["mfcc"], rb["mfcc"], ok)))
        sub = den | two
        allsub = np.ones(int(sub.sum()), bool)
        print("  %-20s %-12s %s" % ("", "reference", "own spectrum"))
        for j, k in enumerate(SCALARS):
            print("  %-20s %-12.3g %.3g" % (k, rel_elem(out[k][:, None], ref["scalars"][:, j:j + 1], every),
                                            rel_elem(out[k][sub][:, None], own["scalars"][:, j:j + 1], allsub)))
        print("  %-20s %-12.3g %.3g" % ("loudness.specific", rel_vec(out["loudness.specific"], ref["loudness_specific"], every),
                                        rel_vec(out["loudness.specific"][sub], own["loudness_specific"], allsub)))
        print("  %-20s %-12.3g %.3g (outside mel_excluded: %d and %d frames)"
              % ("mfcc", rel_vec(out["mfcc"], ref["mfcc"], every & ~excl), rel_vec(out["mfcc"][sub], own["mfcc"], ~excl[sub]),
                 int((every & ~excl).sum()), int((sub & ~excl).sum())))


if __name__ == "__main__":
    main()
