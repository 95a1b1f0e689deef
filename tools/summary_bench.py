#!/usr/bin/env python3
"""The measurements of profiles/summaries.txt on one MI355X: what the per-signal summaries (mgx_summarize_*) cost
beside the gather launch they follow, against pooling the per-frame rows with torch (device) or numpy (host), and
that the launches which make no summary did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all), every feature with both spectra (4,296 bytes of per-frame records a buffer, 1.1 GB in all).

D. device: the gather launch alone; mgx_summarize_device with no per-frame field requested (the records go to the
   workspace); the gather launch followed by the same four statistics with torch on its outputs (the clips are of
   equal length here, so torch reduces a (1024, 256, w) view: the case that favours it).
H. host, wall clock: mgx_summarize_host (only the summaries cross back); mgx_extract_gather_host alone (every
   record crosses back); that call followed by np.add.reduceat-style pooling of its rows.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: summary_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections DHA] [--host-reps R]"""
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

N, HOP, NSIG, PER = 1024, 256, 1024, 256


def corpus():
    L = N + (PER - 1) * HOP
    S = NSIG * L
    x = torch.empty((S + N - 1) // N, N, dtype=torch.float32, device="cuda")
    capi.synth_frames_device(x, 0x6D657964)
    starts, fo = capi.signals_frame_starts([L] * NSIG, N, HOP)
    assert starts.size == NSIG * PER
    return x.view(-1)[:S], starts, fo


def section_d(feats, rounds, launches):
    x, starts, fo = corpus()
    F, S = starts.size, x.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    st = torch.from_numpy(starts.view(np.int64)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N)
    rows, o = plan.alloc_outputs(F, feats)
    _, none = plan.alloc_outputs(0, [])
    summ, so = plan._summary_outputs(NSIG, feats, lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda"))
    nbytes = plan.summary_workspace_bytes(none, so, F, NSIG)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rec = sum(v[0].numel() * v.element_size() for v in rows.values())
    print("\n== D. device: %d clips x %d buffers, N = %d, hop %d; %d bytes of records a buffer, %.2f GB in all; workspace %.2f GB "
          "(%.1f MB beyond the records)" % (NSIG, PER, N, HOP, rec, rec * F / 1e9, nbytes / 1e9, (nbytes - rec * F) / 1e6))

    def gather():
        plan.extract_gather_device(x.data_ptr(), S, st.data_ptr(), F, o, stream)

    def summarize():
        plan.summarize_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ws.data_ptr(), nbytes, stream)

    tstat = {}

    def gather_torch():
        gather()
        for k, v in rows.items():
            r = v.view(NSIG, PER, -1).to(torch.float64)
            tstat[k] = torch.stack([r.mean(dim=1), r.var(dim=1, unbiased=False), r.amin(dim=1), r.amax(dim=1)], dim=1)

    res = gb.interleaved([("gather launch alone", gather), ("mgx_summarize_device", summarize),
                          ("gather launch + torch statistics", gather_torch), ("gather launch alone (again)", gather),
                          ("mgx_summarize_device (again)", summarize)], rounds, launches, warm=2)
    gb.report(res, F)
    med = {k: float(np.median(v)) for k, v in res.items()}
    add_s, add_t = med["mgx_summarize_device"] - med["gather launch alone"], med["gather launch + torch statistics"] - med["gather launch alone"]
    print("  added by the summary kernels: %.4f ms (%.2f TB/s over the records read once); added by torch: %.4f ms" %
          (add_s, rec * F / add_s / 1e9 if add_s > 0 else float("nan"), add_t))
    summarize()
    gather_torch()
    torch.cuda.synchronize()
    worst = 0.0
    for k in summ:
        a, b = summ[k], tstat[k]
        worst = max(worst, float(((a - b).abs() / (b.abs() + 1e-300)).nan_to_num(0.0).max()))
    print("  largest relative difference between the two routes' statistics: %.3g" % worst)
    plan.close()


def section_h(feats, reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N)
    got = {}

    def summarize():
        got["summary"] = plan.summarize_gather(xh, starts, fo, feats)[0]

    def gather():
        got["rows"] = plan.extract_gather(xh, starts, feats)

    def gather_numpy():
        gather()
        idx = fo[:-1].astype(np.int64)
        cnt = np.diff(fo.astype(np.int64)).astype(np.float64)
        out = {}
        for k, v in got["rows"].items():
            r = v.reshape(F, -1).astype(np.float64)
            mean = np.add.reduceat(r, idx, axis=0) / cnt[:, None]
            d = r - np.repeat(mean, np.diff(fo.astype(np.int64)), axis=0)
            out[k] = np.stack([mean, np.add.reduceat(d * d, idx, axis=0) / cnt[:, None], np.minimum.reduceat(r, idx, axis=0),
                               np.maximum.reduceat(r, idx, axis=0)], axis=1)
        got["numpy"] = out

    print("\n== H. host, wall clock per corpus (%d buffers; the records are %.2f GB, the summaries %.1f MB)" %
          (F, sum(4 * w for w in (13, 24, 13, N // 2, N // 2)) * F / 1e9, 32 * (13 + 24 + 13 + N) * NSIG / 1e6))
    variants = [("mgx_summarize_host", summarize), ("mgx_extract_gather_host alone", gather),
                ("mgx_extract_gather_host + numpy reduceat", gather_numpy)]
    for _, fn in variants[:2]:
        fn()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-42s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f" % (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v)))
    worst = 0.0
    with np.errstate(all="ignore"):
        for k, a in got["summary"].items():
            b = got["numpy"][k]
            worst = max(worst, float(np.nan_to_num(np.abs(a - b) / (np.abs(b) + 1e-300)).max()))
    print("  largest relative difference between the two routes' statistics: %.3g" % worst)
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="DHA")
    a = ap.parse_args()
    feats = capi.ALL_FEATURES + ["amplitudeSpectrum", "powerSpectrum"]
    print("command: tools/summary_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "D" in a.sections:
        section_d(feats, a.rounds, a.launches)
        torch.cuda.empty_cache()
    if "H" in a.sections:
        section_h(feats, a.host_reps)
        torch.cuda.empty_cache()
    if "A" in a.sections:
        P, T = gb.load_parent(a.parent), capi.lib()
        for n, label in ((1024, "N = 1024, all features (the headline)"), (2048, "N = 2048, all features (C5)")):
            gb.section_a(P, T, n, 262144, n, capi.ALL_FEATURES, label, a.rounds, a.launches)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
