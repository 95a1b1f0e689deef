#!/usr/bin/env python3
"""The measurements of profiles/flux.txt on one MI355X: what the flux operator (mgx_flux_device) and flux through
the summaries (mgx_summarize_flux_*) cost, against forming the same column with torch (device) or numpy (host) --
what a caller has without them --, and that the launches which ask for no flux did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all).

O. the operator alone on the launch's amplitudeSpectrum (512 columns) and melBands (40 columns) rows, the three
   modes at lag 1 and the rectified mode at lag 8, against torch on the device: the earlier row's index clamped per
   clip (computed once, outside the timing), the difference with its equality rule and the term in float64, torch's
   own sum over the columns. torch sums in another order, so the two are compared within the definition's bound,
   (ceil(cols / 64) + 5) 2^-53 relative to the sum (all terms are non-negative), plus a float32 rounding each.
   Bytes moved: the array once plus the flux column (what an ideal pass reads and writes).
D. device summaries with flux: mgx_summarize_flux_device (every scalar, loudness, mfcc, melBands and their deltas
   pooled, and the rectified flux of amplitudeSpectrum and melBands pooled) against mgx_summarize_deltas_device
   with the same fields and no flux: what flux adds, the spectrum's rows kept in the workspace included.
H. host, wall clock: mgx_summarize_flux_host (the flux of amplitudeSpectrum and melBands per frame and pooled)
   against mgx_extract_gather_host of those two fields + numpy flux and pooling of the rows that crossed back.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: flux_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections ODHA] [--host-reps R]"""
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

NM = 40
FEATS = capi.ALL_FEATURES + ["melBands"]
FLUX = [dict(feature="amplitudeSpectrum", mode="rectified", lag=1), dict(feature="melBands", mode="rectified", lag=1)]


def earlier_rows(fo, F, lag):
    """The row max(t - lag, a) of every row t, a its signal's first row: an (F,) int64 array."""
    fo = fo.astype(np.int64)
    a = np.repeat(fo[:-1], np.diff(fo))
    return np.maximum(np.arange(F) - lag, a)


def torch_flux(x, prev, mode):
    r = x.to(torch.float64)
    p = r.index_select(0, prev)
    d = torch.where(r == p, torch.zeros_like(r), r - p)
    if mode == 0:
        e = torch.where((d > 0) | d.isnan(), d, torch.zeros_like(d))
    elif mode == 1:
        e = d.abs()
    else:
        e = d * d
    s = e.sum(dim=1)
    return (s.sqrt() if mode == 2 else s).to(x.dtype)


def numpy_flux(x, prev, mode):
    r = x.astype(np.float64)
    p = r[prev]
    with np.errstate(all="ignore"):
        d = np.where(r == p, 0.0, r - p)
        e = np.where((d > 0) | np.isnan(d), d, 0.0) if mode == 0 else np.abs(d) if mode == 1 else d * d
        s = e.sum(axis=1)
        return (np.sqrt(s) if mode == 2 else s).astype(x.dtype)


def section_o(rounds, launches):
    x, starts, fo = corpus()
    F = starts.size
    stream = torch.cuda.current_stream().cuda_stream
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    rows = plan.extract_gather_torch(x, starts, ["amplitudeSpectrum", "melBands"])
    torch.cuda.synchronize()
    plan.close()
    for name, r in rows.items():
        w = r.shape[1]
        out = torch.zeros(F, dtype=torch.float32, device="cuda")
        prev = {lag: torch.from_numpy(earlier_rows(fo, F, lag)).cuda() for lag in (1, 8)}
        got = {}
        cases = [("rectified, lag 1", 0, 1), ("l1, lag 1", 1, 1), ("l2, lag 1", 2, 1), ("rectified, lag 8", 0, 8)]

        def op(mode, lag):
            return lambda: capi.flux_device(r.data_ptr(), F, w, False, tb.data_ptr(), NSIG, mode, lag, out.data_ptr(), stream)

        def with_torch():
            got["t"] = torch_flux(r, prev[1], 0)

        print("\n== O. the operator alone: %s, %d rows x %d columns float32 (%.1f MB)" % (name, F, w, 4 * F * w / 1e6))
        variants = [("mgx_flux_device, " + label, op(mode, lag)) for label, mode, lag in cases]
        variants += [("torch, clamped index, rectified, lag 1", with_torch), ("mgx_flux_device, rectified, lag 1 (again)", op(0, 1))]
        res = gb.interleaved(variants, rounds, launches, warm=2)
        gb.report(res, F)
        med = {k: float(np.median(v)) for k, v in res.items()}
        moved = 4 * F * w + 4 * F  # the array once and the flux column
        for label, _, _ in cases:
            print("  %-18s %.1f MB (the array once + the column) in %.4f ms: %.2f TB/s" %
                  (label, moved / 1e6, med["mgx_flux_device, " + label], moved / med["mgx_flux_device, " + label] / 1e9))
        print("  torch takes %.1f times as long" % (med["torch, clamped index, rectified, lag 1"] / med["mgx_flux_device, rectified, lag 1"]))
        bound = (-(-w // 64) + 5) * 2.0 ** -53 + 2.0 ** -23
        for label, mode, lag in cases:
            op(mode, lag)()
            t = torch_flux(r, prev[lag], mode)
            torch.cuda.synchronize()
            # (in float64, where the floor of the denominator is not 0: two zeros differ by 0)
            rel = float(((out.double() - t.double()).abs() / t.double().abs().clamp_min(1e-300)).nan_to_num(0.0).max())
            print("  %-18s against torch: largest relative difference %.3g (bound %.3g): %s" %
                  (label, rel, bound, "inside" if rel <= bound else "OUTSIDE"))
            if not rel <= bound:
                sys.exit("flux_bench: %s, %s differs from torch by more than the definition's bound" % (name, label))


def section_d(rounds, launches):
    x, starts, fo = corpus()
    F, S = starts.size, x.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    st = torch.from_numpy(starts.view(np.int64)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    alloc = lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    _, none = plan.alloc_outputs(0, [])
    _, so = plan._summary_outputs(NSIG, FEATS, alloc)
    _, _, ds = plan._delta_summaries(NSIG, FEATS, (2, 2), alloc)
    reqs, _ = plan._flux_requests(F, NSIG, FLUX, alloc, lambda shape: torch.zeros(shape, dtype=torch.float32, device="cuda"))
    mel_only, _ = plan._flux_requests(F, NSIG, FLUX[1:], alloc, None)
    nb_delta = plan.summarize_deltas_workspace_bytes(none, so, ds, F, NSIG)
    nb_flux = plan.summarize_flux_workspace_bytes(none, so, ds, reqs, len(FLUX), F, NSIG)
    nb_mel = plan.summarize_flux_workspace_bytes(none, so, ds, mel_only, 1, F, NSIG)
    ws = torch.empty(max(nb_delta, nb_flux), dtype=torch.uint8, device="cuda")
    print("\n== D. device summaries: %d clips x %d buffers, N = %d, hop %d; workspace %.1f MB with the flux of amplitudeSpectrum "
          "and melBands, %.1f MB with melBands' alone (the deltas call's: %.1f MB)" % (NSIG, PER, N, HOP, nb_flux / 1e6, nb_mel / 1e6, nb_delta / 1e6))

    def deltas():
        plan.summarize_deltas_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ds, ws.data_ptr(), nb_delta, stream)

    def flux():
        plan.summarize_flux_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ds, reqs, len(FLUX), ws.data_ptr(),
                                   nb_flux, stream)

    def flux_mel():
        plan.summarize_flux_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ds, mel_only, 1, ws.data_ptr(), nb_mel,
                                   stream)

    res = gb.interleaved([("mgx_summarize_deltas_device", deltas), ("mgx_summarize_flux_device, amplitude + melBands", flux),
                          ("mgx_summarize_flux_device, melBands (rows shared)", flux_mel), ("mgx_summarize_deltas_device (again)", deltas),
                          ("mgx_summarize_flux_device, amplitude + melBands (again)", flux)], rounds, launches, warm=2)
    gb.report(res, F)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("  added by the two fluxes, their pooling and the spectrum's rows: %.4f ms; by melBands' flux alone: %.4f ms" %
          (med["mgx_summarize_flux_device, amplitude + melBands"] - med["mgx_summarize_deltas_device"],
           med["mgx_summarize_flux_device, melBands (rows shared)"] - med["mgx_summarize_deltas_device"]))
    plan.close()


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    prev = earlier_rows(fo, F, 1)
    seg = fo[:-1].astype(np.int64)
    cnt = np.diff(fo.astype(np.int64)).astype(np.float64)
    reqs = [dict(q, per_frame=True) for q in FLUX]
    got = {}

    def flux():
        got["flux"] = plan.summarize_gather(xh, starts, fo, [], flux=reqs)[2]

    def pool(r):
        mean = np.add.reduceat(r, seg) / cnt
        d = r - np.repeat(mean, np.diff(fo.astype(np.int64)))
        return np.stack([mean, np.add.reduceat(d * d, seg) / cnt, np.minimum.reduceat(r, seg), np.maximum.reduceat(r, seg)], axis=1)

    def gather_numpy():
        rows = plan.extract_gather(xh, starts, [q["feature"] for q in FLUX])
        got["numpy"] = []
        for q in FLUX:
            col = numpy_flux(rows[q["feature"]], prev, 0)
            got["numpy"].append((col, pool(col.astype(np.float64))))

    print("\n== H. host, wall clock per corpus (%d buffers; the flux of amplitudeSpectrum, %d columns, and melBands, %d)" % (F, N // 2, NM))
    variants = [("mgx_summarize_flux_host", flux), ("mgx_extract_gather_host + numpy flux and pooling", gather_numpy)]
    flux()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-52s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f" % (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v)))
    worst = [0.0, 0.0]
    with np.errstate(all="ignore"):
        for r, (col, st) in zip(got["flux"], got["numpy"]):
            worst[0] = max(worst[0], float(np.nan_to_num(np.abs(r["per_frame"] - col) / (np.abs(col) + 1e-300)).max()))
            worst[1] = max(worst[1], float(np.nan_to_num(np.abs(r["summary"] - st) / (np.abs(st) + 1e-300)).max()))
    print("  largest relative difference between the two routes: per frame %.3g, statistics %.3g" % tuple(worst))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="ODHA")
    a = ap.parse_args()
    print("command: tools/flux_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "O" in a.sections:
        section_o(a.rounds, a.launches)
        torch.cuda.empty_cache()
    if "D" in a.sections:
        section_d(a.rounds, a.launches)
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
