#!/usr/bin/env python3
"""The measurements of profiles/hpss.txt on one MI355X: what the HPSS operator (mgx_hpss_device) and the host route
(mgx_hpss_host) cost, against forming the same rows with torch (device) or scipy and numpy (host) -- what a caller
has without them --, and that the existing launches did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all). Kt = Kf = 31, SOFT2, unit margins.

O. the operator alone on the launch's amplitudeSpectrum rows (262,144 x 512): both outputs, one output, MEDIANS mode,
   with mgx_flux_device on the same array in the same process as the memory-rate yardstick. Bytes: the array once in,
   each output once. torch on the device: the windows unfolded (reflected index tables), kthvalue along the window,
   the masks in float64, in chunks of clips that fit; checked equal (the medians bit for bit on this input, which has
   neither NaN nor -0; the outputs bit for bit).
H. host, wall clock: mgx_hpss_host with harmonic chroma and percussive flux (per frame and pooled) against
   mgx_extract_gather_host of the amplitude spectrum + scipy.ndimage.median_filter per clip + the numpy masks, chroma
   and flux (where scipy imports; the filters, masks, chroma and flux of the first --scipy-clips clips only, timed apart
   and scaled to the corpus: the median filter takes minutes), and against mgx_extract_gather_host alone.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: hpss_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections OHA] [--host-reps R]"""
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
K = 31


def reflect_index(m, h, device):
    """(m, 2h + 1) reflected indices of the definition's r(u, m)."""
    u = torch.arange(m, device=device)[:, None] + torch.arange(-h, h + 1, device=device)[None, :]
    q = torch.remainder(u, 2 * m)
    return torch.where(q < m, q, 2 * m - 1 - q)


def torch_hpss(r, per, clips_per_chunk=16):
    """SOFT2 under unit margins of clips of `per` rows each, by unfolded kthvalue: (harmonic, percussive, H, P)."""
    F, cols = r.shape
    h = K // 2
    it, ic = reflect_index(per, h, r.device), reflect_index(cols, h, r.device)
    outs = [torch.empty_like(r) for _ in range(4)]
    for c0 in range(0, F // per, clips_per_chunk):
        x = r[c0 * per:(c0 + clips_per_chunk) * per].view(-1, per, cols)           # (clips, per, cols)
        H = x[:, it, :].kthvalue(h + 1, dim=2).values                               # (clips, per, K, cols) -> (clips, per, cols)
        P = x[:, :, ic].kthvalue(h + 1, dim=3).values                               # (clips, per, cols, K) -> (clips, per, cols)
        x64, hp, rp = x.double(), H.double() ** 2, P.double() ** 2
        den = hp + rp
        mh = torch.where(den == 0, torch.full_like(den, 0.5), hp / den)
        mp = torch.where(den == 0, torch.full_like(den, 0.5), rp / den)
        sl = slice(c0 * per, c0 * per + x.shape[0] * per)
        for o, v in zip(outs, ((x64 * mh).float(), (x64 * mp).float(), H, P)):
            o[sl] = v.reshape(-1, cols)
    return outs


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
    oh, op = torch.zeros_like(r), torch.zeros_like(r)
    array = 4 * F * cols
    soft, med = capi.hpss_params(), capi.hpss_params(mode="medians")
    keep = {}

    def run(params, h, p):
        return lambda: capi.hpss_device(r.data_ptr(), F, cols, tb.data_ptr(), NSIG, params, h, p, stream)

    def flux_op():
        capi.flux_device(r.data_ptr(), F, cols, False, tb.data_ptr(), NSIG, 0, 1, flux.data_ptr(), stream)

    def with_torch():
        keep["t"] = torch_hpss(r, PER)

    print("\n== O. the operator alone: Kt = Kf = %d, %d rows x %d columns float32 (%.1f MB), %d clips of %d rows" %
          (K, F, cols, array / 1e6, NSIG, PER))
    variants = [("mgx_hpss_device, soft2, both outputs", run(soft, oh.data_ptr(), op.data_ptr())),
                ("mgx_hpss_device, soft2, harmonic alone", run(soft, oh.data_ptr(), None)),
                ("mgx_hpss_device, medians, both outputs", run(med, oh.data_ptr(), op.data_ptr())),
                ("mgx_flux_device (the yardstick)", flux_op),
                ("mgx_hpss_device, soft2, both (again)", run(soft, oh.data_ptr(), op.data_ptr())),
                ("mgx_flux_device (again)", flux_op)]
    res = gb.interleaved(variants, rounds, launches, warm=2)
    gb.report(res, F)
    m = {k: float(np.median(v)) for k, v in res.items()}
    for k, nbytes in (("mgx_hpss_device, soft2, both outputs", 3 * array), ("mgx_hpss_device, soft2, harmonic alone", 2 * array),
                      ("mgx_hpss_device, medians, both outputs", 3 * array), ("mgx_flux_device (the yardstick)", array + 4 * F)):
        print("  %-40s %.1f MB in %.4f ms: %.2f TB/s" % (k, nbytes / 1e6, m[k], nbytes / m[k] / 1e9))
    print("  the operator with both outputs takes %.1f times the yardstick's time for 3 times its bytes" %
          (m["mgx_hpss_device, soft2, both outputs"] / m["mgx_flux_device (the yardstick)"]))
    # torch on the device, once (it is seconds, not a variant of the rounds), and the comparison
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with_torch()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print("  torch (unfolded kthvalue, float64 masks, 16 clips a chunk): %.1f ms, %.0f times the operator" %
          ((t1 - t0) * 1e3, (t1 - t0) * 1e3 / m["mgx_hpss_device, soft2, both outputs"]))
    th, tp, tH, tP = keep["t"]
    run(med, oh.data_ptr(), op.data_ptr())()
    torch.cuda.synchronize()
    same_med = bool(torch.equal(oh.view(torch.int32), tH.view(torch.int32)) and torch.equal(op.view(torch.int32), tP.view(torch.int32)))
    run(soft, oh.data_ptr(), op.data_ptr())()
    torch.cuda.synchronize()
    same_out = bool(torch.equal(oh.view(torch.int32), th.view(torch.int32)) and torch.equal(op.view(torch.int32), tp.view(torch.int32)))
    print("  against torch: the medians %s, the soft2 outputs %s" %
          ("equal bit for bit" if same_med else "DIFFER", "equal bit for bit" if same_out else "DIFFER"))
    if not (same_med and same_out):
        sys.exit("hpss_bench: the operator differs from torch")


def section_h(reps, scipy_clips):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N)
    w = capi.chroma_weights(N, SR)
    seg_all = fo[:-1].astype(np.int64)
    per_all = np.diff(fo.astype(np.int64))
    cnt_all = per_all.astype(np.float64)[:, None]
    got = {}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None

    def hpss():
        got["lib"] = plan.hpss(xh, starts, fo, chroma=dict(weights=w, summary=True), flux=dict(summary=True))

    def gather():
        got["amp"] = plan.extract_gather(xh, starts, ["amplitudeSpectrum"])["amplitudeSpectrum"]

    def host_statement():
        a = got["amp"][:int(fo[scipy_clips])]
        seg, per, cnt = seg_all[:scipy_clips], per_all[:scipy_clips], cnt_all[:scipy_clips]

        def pooled(c):
            mean = np.add.reduceat(c, seg) / cnt
            d = c - np.repeat(mean, per, axis=0)
            return np.stack([mean, np.add.reduceat(d * d, seg) / cnt, np.minimum.reduceat(c, seg), np.maximum.reduceat(c, seg)], axis=1)
        H, P = np.empty_like(a), np.empty_like(a)
        for s in range(scipy_clips):
            lo, hi = int(fo[s]), int(fo[s + 1])
            H[lo:hi] = ndimage.median_filter(a[lo:hi], size=(K, 1), mode="reflect")
            P[lo:hi] = ndimage.median_filter(a[lo:hi], size=(1, K), mode="reflect")
        a64, hp, rp = a.astype(np.float64), H.astype(np.float64) ** 2, P.astype(np.float64) ** 2
        den = hp + rp
        with np.errstate(all="ignore"):
            yh = (a64 * np.where(den == 0, 0.5, hp / den)).astype(np.float32)
            yp = (a64 * np.where(den == 0, 0.5, rp / den)).astype(np.float32)
            s = yh.astype(np.float64) @ w.astype(np.float64).T
            mx = s.max(axis=1, keepdims=True)
            c = np.where((mx > 0) & np.isfinite(mx), s / mx, s)
        d = np.diff(yp.astype(np.float64), axis=0, prepend=yp[:1].astype(np.float64))
        d[seg] = 0.0  # (a clip's first row has no earlier row)
        f = np.maximum(d, 0.0).sum(axis=1)
        got["numpy"] = (c.astype(np.float32), pooled(c), f.astype(np.float32), pooled(f[:, None]))

    print("\n== H. host, wall clock per corpus (%d buffers, %d clips; harmonic chroma C = 12 and percussive flux, per frame and pooled)" %
          (F, NSIG))
    variants = [("mgx_hpss_host", hpss), ("mgx_extract_gather_host(amplitudeSpectrum) alone", gather)]
    hpss()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for i in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-60s median %10.1f ms  min %10.1f  max %10.1f  (%d runs)" % (name, np.median(v), np.min(v), np.max(v), len(v)))
    if ndimage is None:
        print("  (scipy does not import: the host statement is left out)")
    else:
        t = time.perf_counter()
        host_statement()
        dt = (time.perf_counter() - t) * 1e3
        k = int(fo[scipy_clips])
        print("  scipy median filters + numpy masks, chroma, flux and pooling of the first %d clips (%d buffers): %.1f ms, once;" %
              (scipy_clips, k, dt))
        print("  scaled to the %d clips: %.1f s on top of the gather call's %.1f ms, against %.1f ms for mgx_hpss_host" %
              (NSIG, dt * NSIG / scipy_clips / 1e3, np.median(ts["mgx_extract_gather_host(amplitudeSpectrum) alone"]), np.median(ts["mgx_hpss_host"])))
        with np.errstate(all="ignore"):
            rows, st, f, fst = got["numpy"]
            a = float(np.nan_to_num(np.abs(got["lib"]["chroma"][:k] - rows) / (np.abs(rows) + 1e-300)).max())
            b = float(np.nan_to_num(np.abs(got["lib"]["flux"][:k] - f) / (np.abs(f) + 1e-300)).max())
        print("  largest relative difference between the two routes on those rows: chroma rows %.3g, flux %.3g (sums in another order)" % (a, b))
    print("  bytes that cross back: %.1f MB of chroma rows, %.1f MB of flux and %.2f MB of summaries, against %.1f MB of spectra each way" %
          (4 * F * 12 / 1e6, 4 * F / 1e6, 8 * NSIG * 4 * 13 / 1e6, 4 * F * (N // 2) / 1e6))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--scipy-clips", type=int, default=32)
    ap.add_argument("--sections", default="OHA")
    a = ap.parse_args()
    print("command: tools/hpss_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches; corpus %d clips x %d buffers, N = %d, hop %d" %
          (torch.cuda.get_device_name(0), a.rounds, a.launches, NSIG, PER, N, HOP))
    if "O" in a.sections:
        section_o(a.rounds, a.launches)
        torch.cuda.empty_cache()
    if "H" in a.sections:
        section_h(a.host_reps, min(a.scipy_clips, NSIG))
        torch.cuda.empty_cache()
    if "A" in a.sections:
        P, T = gb.load_parent(a.parent), capi.lib()
        for rep in (1, 2):
            for n, label in ((1024, "N = 1024, all features (the headline)"), (2048, "N = 2048, all features (C5)")):
                gb.section_a(P, T, n, 262144, n, capi.ALL_FEATURES, "%s, measurement %d" % (label, rep), a.rounds, a.launches)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
