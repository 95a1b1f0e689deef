#!/usr/bin/env python3
"""The measurements of profiles/onsets.txt on one MI355X: what the peak picker (mgx_peaks_device) and the onsets host
call (mgx_onsets_host) cost against what a caller has without them, and that the launches which pick no peaks did
not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all); the envelope is the rectified flux of its melBands rows at lag 1 (a 1 MB column).

P. the picker alone on that column, as 1,024 signals and as one signal of 262,144 rows, against
   - the candidate stage written with torch on the device (the clamped indices computed once, outside the timing;
     one gather, compare and addition per window offset in float64, in the definition's order) followed by the copy
     of the candidate mask and the greedy step on the host, and
   - tests/peaks_ref.py in numpy on the host, the copy of the column included.
   All three give integers and are compared for equality.
H. host, wall clock: mgx_onsets_host against mgx_summarize_flux_host with per_frame + the numpy picker.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: onset_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections PHA] [--host-reps R]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meyda_amd import capi  # noqa: E402
import gather_bench as gb  # noqa: E402
import peaks_ref  # noqa: E402
from summary_bench import N, HOP, NSIG, PER, corpus  # noqa: E402

NM = 40
REQ = dict(feature="melBands", mode="rectified", lag=1)
PARAMS = dict(pre_max=3, post_max=3, pre_avg=10, post_avg=10, delta=0.05, wait=4)


def torch_candidates(e, a, last, p):
    """The candidate stage on the device: e (F,) float64, a / last the first and last row of every row's signal."""
    t = torch.arange(e.shape[0], device=e.device)
    at = lambda k: e.index_select(0, torch.minimum(torch.maximum(t + k, a), last))
    top = torch.ones_like(e, dtype=torch.bool)
    for k in range(-p["pre_max"], p["post_max"] + 1):
        top &= ~(at(k) > e)
    m = torch.zeros_like(e)
    for k in range(-p["pre_avg"], p["post_avg"] + 1):
        m = m + at(k)
    return top & (e >= m / float(p["pre_avg"] + p["post_avg"] + 1) + p["delta"])


def host_greedy(cand, fo, wait):
    rows = np.nonzero(cand)[0]
    cut = np.searchsorted(rows, fo.astype(np.int64))
    out = []
    for s in range(len(fo) - 1):
        out += peaks_ref.greedy(rows[cut[s]:cut[s + 1]], wait)
    return np.array(out, np.uint64)


def section_p(rounds, launches):
    x, starts, fo = corpus()
    F = starts.size
    stream = torch.cuda.current_stream().cuda_stream
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    _, _, fres = plan.summarize_gather_torch(x, starts, fo, [], (), flux=[dict(REQ, per_frame=True, summary=False)])
    env = fres[0]["per_frame"]
    torch.cuda.synchronize()
    plan.close()
    print("\n== P. the picker alone: %d rows of melBands rectified flux (%.1f MB), %s" % (F, 4 * F / 1e6, PARAMS))
    nbytes = capi.peaks_workspace_bytes(F, NSIG)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    pp = capi.peak_params(**PARAMS)
    for label, table in (("%d signals of %d rows" % (NSIG, PER), fo), ("one signal of %d rows" % F, np.array([0, F], np.uint64))):
        S = table.size - 1
        tb = torch.from_numpy(table.view(np.int64)).cuda()
        mask = torch.zeros(F, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
        peaks = torch.zeros(F, dtype=torch.int64, device="cuda")
        o = capi.PeakOutputs()
        o.struct_size = ctypes.sizeof(capi.PeakOutputs)
        o.mask, o.peak_offsets, o.peaks, o.capacity = mask.data_ptr(), offs.data_ptr(), peaks.data_ptr(), F
        ti = table.astype(np.int64)
        a = torch.from_numpy(np.repeat(ti[:-1], np.diff(ti))).cuda()
        last = torch.from_numpy(np.repeat(ti[1:] - 1, np.diff(ti))).cuda()
        got = {}

        def op():
            capi.peaks_device(env.data_ptr(), F, False, tb.data_ptr(), S, pp, o, ws.data_ptr(), nbytes, stream)

        def with_torch():
            cand = torch_candidates(env.double(), a, last, PARAMS).cpu().numpy()
            got["torch"] = host_greedy(cand, table, PARAMS["wait"])

        def with_numpy():
            got["numpy"] = peaks_ref.peaks(env.cpu().numpy(), table, **PARAMS)

        print("  -- %s (workspace %.1f KB)" % (label, nbytes / 1e3))
        res = gb.interleaved([("mgx_peaks_device", op), ("torch candidates + host greedy", with_torch, 1),
                              ("numpy peaks_ref, column copied", with_numpy, 1), ("mgx_peaks_device (again)", op)], rounds, launches, warm=2)
        gb.report(res, F)
        med = {k: float(np.median(v)) for k, v in res.items()}
        print("  torch + host greedy takes %.0f times as long, numpy %.0f times" %
              (med["torch candidates + host greedy"] / med["mgx_peaks_device"], med["numpy peaks_ref, column copied"] / med["mgx_peaks_device"]))
        op()
        torch.cuda.synchronize()
        total = int(offs[-1])
        mine = peaks[:total].cpu().numpy().view(np.uint64)
        same = np.array_equal(mine, got["numpy"][2]) and np.array_equal(mine, got["torch"]) and \
            np.array_equal(offs.cpu().numpy().view(np.uint64), got["numpy"][1]) and np.array_equal(mask.cpu().numpy(), got["numpy"][0])
        print("  %d peaks; the three routes: %s" % (total, "identical" if same else "DIFFER"))
        if not same:
            sys.exit("onset_bench: the picker differs from its definition")


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    got = {}

    def onsets():
        got["onsets"] = plan.onsets(xh, starts, fo, capacity=F, **REQ, **PARAMS)

    def flux_numpy():
        col = plan.summarize_gather(xh, starts, fo, [], flux=[dict(REQ, per_frame=True, summary=False)])[2][0]["per_frame"]
        got["numpy"] = peaks_ref.peaks(col, fo, **PARAMS)

    print("\n== H. host, wall clock per corpus (%d buffers of %d clips; the rectified flux of melBands, %d columns, and its peaks)" % (F, NSIG, NM))
    variants = [("mgx_onsets_host", onsets), ("mgx_summarize_flux_host (per_frame) + numpy picker", flux_numpy)]
    onsets()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-52s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f" % (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v)))
    same = np.array_equal(got["onsets"]["peaks"], got["numpy"][2]) and np.array_equal(got["onsets"]["peak_offsets"], got["numpy"][1])
    print("  %d peaks; the two routes: %s" % (got["numpy"][2].size, "identical" if same else "DIFFER"))
    plan.close()
    if not same:
        sys.exit("onset_bench: the host call differs from the picker on the flux call's column")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="PHA")
    a = ap.parse_args()
    print("command: tools/onset_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "P" in a.sections:
        section_p(a.rounds, a.launches)
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
