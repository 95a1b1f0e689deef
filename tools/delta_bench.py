#!/usr/bin/env python3
"""The measurements of profiles/deltas.txt on one MI355X: what the delta operator (mgx_delta_device) and the delta
summaries (mgx_summarize_deltas_*) cost, against forming the same rows with torch (device) or numpy (host) -- what
a caller has without them --, and that the launches which ask for no delta did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip,
262,144 in all). W = 2, both orders.

O. the operator alone on the launch's mfcc (13 columns) and melBands (40 columns) rows: mgx_delta_device with both
   outputs (two passes) and with delta2 alone (one pass, the delta rows recomputed), against torch on the device:
   row indices clamped per clip (computed once, outside the timing), the weighted differences in float64, rounded
   to float32 after each order. Bytes moved: the rows read once and each output written once per pass.
D. device summaries of every scalar, loudness, mfcc and melBands with their deltas: mgx_summarize_deltas_device,
   against mgx_summarize_device alone (what the deltas add) and against mgx_summarize_device with the rows
   requested per frame + the torch deltas of O + torch statistics of both orders.
H. host, wall clock: mgx_summarize_deltas_host against mgx_summarize_host alone (what the deltas add) and against
   mgx_extract_gather_host + numpy deltas and pooling of the rows that crossed back.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of
   the parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: delta_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections ODHA] [--host-reps R]"""
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

W = 2
D = W * (W + 1) * (2 * W + 1) // 3
NM = 40
FEATS = capi.ALL_FEATURES + ["melBands"]


def clamped_indices(fo, F, device):
    """Per n = 1..W the rows t + n and t - n limited to the row's own signal: W pairs of (F,) int64 arrays (numpy,
    or CUDA tensors with `device`)."""
    fo = fo.astype(np.int64)
    counts, t = np.diff(fo), np.arange(F)
    a, last = np.repeat(fo[:-1], counts), np.repeat(fo[1:] - 1, counts)
    idx = [(np.minimum(t + n, last), np.maximum(t - n, a)) for n in range(1, W + 1)]
    return [(torch.from_numpy(u).cuda(), torch.from_numpy(m).cuda()) for u, m in idx] if device else idx


def torch_delta(x, idx):
    """One order of the definition on a (F, w) tensor: float64 sums in ascending n, one division, the rows' type."""
    r = x.to(torch.float64)
    acc = torch.zeros_like(r)
    for n, (up, um) in enumerate(idx, 1):
        acc += n * (r.index_select(0, up) - r.index_select(0, um))
    return (acc / D).to(x.dtype)


def numpy_delta(x, idx):
    r = x.astype(np.float64)
    acc = np.zeros_like(r)
    for n, (up, um) in enumerate(idx, 1):
        acc += n * (r[up] - r[um])
    return (acc / D).astype(x.dtype)


def section_o(rounds, launches):
    x, starts, fo = corpus()
    F, S = starts.size, x.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    rows = plan.extract_gather_torch(x, starts, ["mfcc", "melBands"])
    torch.cuda.synchronize()
    plan.close()
    idx = clamped_indices(fo, F, True)
    for name, r in rows.items():
        w = r.shape[1]
        d1, d2, alone = torch.empty_like(r), torch.empty_like(r), torch.empty_like(r)
        got = {}

        def both():
            capi.delta_device(r.data_ptr(), F, w, False, tb.data_ptr(), NSIG, W, d1.data_ptr(), d2.data_ptr(), stream)

        def second_alone():
            capi.delta_device(r.data_ptr(), F, w, False, tb.data_ptr(), NSIG, W, None, alone.data_ptr(), stream)

        def with_torch():
            got["d1"] = torch_delta(r, idx)
            got["d2"] = torch_delta(got["d1"], idx)

        print("\n== O. the operator alone: %s, %d rows x %d columns float32 (%.1f MB), W = %d, both orders" %
              (name, F, w, 4 * F * w / 1e6, W))
        res = gb.interleaved([("mgx_delta_device, delta + delta2", both), ("mgx_delta_device, delta2 alone", second_alone),
                              ("torch, clamped indices", with_torch), ("mgx_delta_device, delta + delta2 (again)", both)],
                             rounds, launches, warm=2)
        gb.report(res, F)
        med = {k: float(np.median(v)) for k, v in res.items()}
        moved = 4 * F * w * 4  # two passes, each a read and a write of the array
        print("  two passes move %.1f MB (each a read and a write of the array): %.2f TB/s; torch takes %.1f times as long" %
              (moved / 1e6, moved / med["mgx_delta_device, delta + delta2"] / 1e9,
               med["torch, clamped indices"] / med["mgx_delta_device, delta + delta2"]))
        both()
        second_alone()
        with_torch()
        torch.cuda.synchronize()
        print("  delta2 alone against the two passes: %s; torch against them: delta %s, delta2 %s" %
              ("identical, bit for bit" if torch.equal(alone.view(torch.int32), d2.view(torch.int32)) else "DIFFERS",
               "identical" if torch.equal(got["d1"].view(torch.int32), d1.view(torch.int32)) else
               "largest difference %.3g" % float((got["d1"] - d1).abs().nan_to_num(0.0).max()),
               "identical" if torch.equal(got["d2"].view(torch.int32), d2.view(torch.int32)) else
               "largest difference %.3g" % float((got["d2"] - d2).abs().nan_to_num(0.0).max())))


def torch_stats(v):
    r = v.view(NSIG, PER, -1).to(torch.float64)
    return torch.stack([r.mean(dim=1), r.var(dim=1, unbiased=False), r.amin(dim=1), r.amax(dim=1)], dim=1)


def section_d(rounds, launches):
    x, starts, fo = corpus()
    F, S = starts.size, x.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    st = torch.from_numpy(starts.view(np.int64)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    alloc = lambda shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    rows, o = plan.alloc_outputs(F, FEATS)
    _, none = plan.alloc_outputs(0, [])
    summ, so = plan._summary_outputs(NSIG, FEATS, alloc)
    d1, d2, ds = plan._delta_summaries(NSIG, FEATS, (W, 2), alloc)
    nb_plain = plan.summary_workspace_bytes(none, so, F, NSIG)
    nb_rows = plan.summary_workspace_bytes(o, so, F, NSIG)
    nb_delta = plan.summarize_deltas_workspace_bytes(none, so, ds, F, NSIG)
    ws = torch.empty(max(nb_plain, nb_rows, nb_delta), dtype=torch.uint8, device="cuda")
    idx = clamped_indices(fo, F, True)
    cols = sum(v[0].numel() for v in rows.values())
    print("\n== D. device summaries: %d clips x %d buffers, N = %d, hop %d; %d delta'd columns a buffer; workspace %.1f MB "
          "(the summary call's: %.1f MB)" % (NSIG, PER, N, HOP, cols, nb_delta / 1e6, nb_plain / 1e6))

    def plain():
        plan.summarize_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ws.data_ptr(), nb_plain, stream)

    def deltas():
        plan.summarize_deltas_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, none, so, ds, ws.data_ptr(), nb_delta,
                                     stream)

    tstat = [{}, {}]

    def plain_torch():
        plan.summarize_device(x.data_ptr(), S, st.data_ptr(), F, tb.data_ptr(), NSIG, o, so, ws.data_ptr(), nb_rows, stream)
        for k, v in rows.items():
            a = torch_delta(v.view(F, -1), idx)
            b = torch_delta(a, idx)
            tstat[0][k], tstat[1][k] = torch_stats(a), torch_stats(b)

    res = gb.interleaved([("mgx_summarize_device", plain), ("mgx_summarize_deltas_device", deltas),
                          ("mgx_summarize_device + torch", plain_torch), ("mgx_summarize_device (again)", plain),
                          ("mgx_summarize_deltas_device (again)", deltas)], rounds, launches, warm=2)
    gb.report(res, F)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("  added by the deltas and their pooling: %.4f ms; added by torch deltas and statistics: %.4f ms" %
          (med["mgx_summarize_deltas_device"] - med["mgx_summarize_device"],
           med["mgx_summarize_device + torch"] - med["mgx_summarize_device"]))
    deltas()
    plain_torch()
    torch.cuda.synchronize()
    worst = 0.0
    for got, want in ((d1, tstat[0]), (d2, tstat[1])):
        for k in got:
            worst = max(worst, float(((got[k] - want[k]).abs() / (want[k].abs() + 1e-300)).nan_to_num(0.0).max()))
    print("  largest relative difference between the two routes' delta statistics: %.3g" % worst)
    plan.close()


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    idx = clamped_indices(fo, F, False)
    seg = fo[:-1].astype(np.int64)
    cnt = np.diff(fo.astype(np.int64)).astype(np.float64)
    got = {}

    def deltas():
        got["deltas"] = plan.summarize_gather(xh, starts, fo, FEATS, deltas=(W, 2))

    def plain():
        got["plain"] = plan.summarize_gather(xh, starts, fo, FEATS)

    def pool(r):
        mean = np.add.reduceat(r, seg, axis=0) / cnt[:, None]
        d = r - np.repeat(mean, np.diff(fo.astype(np.int64)), axis=0)
        return np.stack([mean, np.add.reduceat(d * d, seg, axis=0) / cnt[:, None], np.minimum.reduceat(r, seg, axis=0),
                         np.maximum.reduceat(r, seg, axis=0)], axis=1)

    def gather_numpy():
        rows = plan.extract_gather(xh, starts, FEATS)
        out = ({}, {}, {})
        for k, v in rows.items():
            v = v.reshape(F, -1)
            a = numpy_delta(v, idx)
            b = numpy_delta(a, idx)
            for o, r in zip(out, (v, a, b)):
                o[k] = pool(r.astype(np.float64))
        got["numpy"] = out

    print("\n== H. host, wall clock per corpus (%d buffers, %d delta'd columns a buffer)" % (F, 13 + 24 + 13 + NM))
    variants = [("mgx_summarize_host", plain), ("mgx_summarize_deltas_host", deltas),
                ("mgx_extract_gather_host + numpy deltas and pooling", gather_numpy)]
    for _, fn in variants[:2]:
        fn()  # (staging allocated)
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-52s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f" % (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v)))
    worst = 0.0
    with np.errstate(all="ignore"):
        for order in (1, 2):
            for k, a in got["deltas"][order + 1].items():
                b = got["numpy"][order][k]
                worst = max(worst, float(np.nan_to_num(np.abs(a - b) / (np.abs(b) + 1e-300)).max()))
    base_same = all(np.array_equal(got["deltas"][0][k].view(np.uint64), got["plain"][0][k].view(np.uint64)) for k in got["plain"][0])
    print("  largest relative difference between the two routes' delta statistics: %.3g; base summaries beside the deltas: %s" %
          (worst, "identical, bit for bit" if base_same else "DIFFER"))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="ODHA")
    a = ap.parse_args()
    print("command: tools/delta_bench.py %s" % " ".join(sys.argv[1:]))
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
        for n, label in ((1024, "N = 1024, all features (the headline)"), (2048, "N = 2048, all features (C5)")):
            gb.section_a(P, T, n, 262144, n, capi.ALL_FEATURES, label, a.rounds, a.launches)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
