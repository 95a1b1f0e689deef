#!/usr/bin/env python3
"""The measurements of profiles/beats.txt on one MI355X: what the beat tracker (mgx_beats_device) and the host route
(mgx_beats_host) cost, against the numpy statement of the same definition on the host (tests/beat_ref.py) -- what a
caller has without them: the column copied back and a loop per clip --, and that the existing launches did not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip, 262,144
in all); the envelope is the rectified flux of melBands (40 bands), the periods are the lags of mgx_tempo_device at
W = L = 384, the tables those of max_period 383.

O. the operator alone, the corpus as 1,024 clips (each at its own lag) and as one signal of 262,144 rows (at the median
   lag), with the steps of the recurrence's serial chain (n / lo(p) per signal); against the numpy statement on the
   host with the column copied back, whose beats are compared.
H. host, wall clock: mgx_beats_host against mgx_tempo_host alone, and against that call plus the flux column copied
   back and the numpy statement.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of the
   parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: beat_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections OHA] [--host-reps R]"""
import argparse
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
import beat_ref  # noqa: E402
import gather_bench as gb  # noqa: E402
from summary_bench import N, HOP, NSIG, PER, corpus  # noqa: E402
from tempo_bench import NM, REQ, W, L, RATE, envelope  # noqa: E402

P = L - 1


def section_o(rounds, launches):
    env, fo = envelope()
    F = env.shape[0]
    tables = capi.beat_tables(P)
    gauss, penalty = (torch.from_numpy(t).cuda() for t in tables)
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    h = torch.from_numpy(capi.tempogram_window(W)).cuda()
    pr = torch.from_numpy(capi.tempo_prior(RATE, L)).cuda()
    lag = capi.tempo_torch(env, h, pr, tb, summary=False)["lag"]
    torch.cuda.synchronize()
    lags = lag.cpu().numpy().astype(np.uint32)
    med = int(np.median(lags[lags > 0]))
    one = torch.full((1,), med, dtype=torch.int32, device="cuda")
    ws = torch.empty(capi.beats_workspace_bytes(F, NSIG), dtype=torch.uint8, device="cuda")
    print("\n== O. the operator alone: %d rows; lags of mgx_tempo_device: %d clips with one, median %d; workspace %.1f MB (%.1f bytes a row)" %
          (F, int((lags > 0).sum()), med, ws.numel() / 1e6, ws.numel() / F))
    cases = (("%d clips of %d rows" % (NSIG, PER), tb, lag, fo, lags), ("one signal of %d rows at p = %d" % (F, med), None, one, None, [med]))
    for label, table, period, hfo, hper in cases:
        got = {}

        def op():
            got["d"] = capi.beats_torch(env, period, gauss, penalty, table, max_period=P, workspace=ws)
        print("  -- %s" % label)
        res = gb.interleaved([("mgx_beats_device", op)], rounds, launches, warm=2)
        gb.report(res, F)
        steps = [-(-(int(hfo[s + 1]) - int(hfo[s])) // beat_ref.lo(int(p))) for s, p in enumerate(hper) if p] if hfo is not None else \
            [-(-F // beat_ref.lo(med))]
        ms = float(np.median(res["mgx_beats_device"]))
        print("  the recurrence's chain: %d steps in the longest signal (%d in all): at most %.2f us a step" %
              (max(steps), sum(steps), 1e3 * ms / max(steps)))
        t = time.perf_counter()
        back = env.cpu().numpy()
        ref = beat_ref.beats_ref(back, hper, hfo, P, *tables)
        host_ms = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        off = got["d"]["peak_offsets"].cpu().numpy().astype(np.uint64)
        rows = got["d"]["peaks"].cpu().numpy()[:int(off[-1])].astype(np.uint64)
        same = np.array_equal(off, ref["peak_offsets"]) and np.array_equal(rows, ref["peaks"])
        print("  the numpy statement on the host, column copied back: %.1f ms (%.0f times the operator); %d beats, %s" %
              (host_ms, host_ms / ms, rows.size, "identical" if same else "DIFFER"))
        if not same:
            sys.exit("beat_bench: the operator differs from its definition")


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    tables = capi.beat_tables(P)
    got = {}

    def beats():
        got["lib"] = plan.beats(xh, starts, fo, RATE, win_length=W, tables=tables, capacity=F, **REQ)

    def tempo():
        return plan.tempo(xh, starts, fo, RATE, win_length=W, **REQ)

    def tempo_statement():
        t = plan.tempo(xh, starts, fo, RATE, win_length=W, envelope=True, **REQ)
        got["statement"] = beat_ref.beats_ref(t["envelope"], t["lag"], fo, P, *tables)

    print("\n== H. host, wall clock per corpus (%d buffers of %d clips; the rectified flux of melBands, W = L = %d, lags and beats)" %
          (F, NSIG, W))
    variants = [("mgx_beats_host", beats, reps), ("mgx_tempo_host alone", tempo, reps),
                ("mgx_tempo_host (envelope) + the numpy statement", tempo_statement, reps)]
    beats()  # (staging allocated)
    ts = {name: [] for name, _, _ in variants}
    for r in range(reps):
        for name, fn, k in variants:
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-52s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f  (%d)" %
              (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v), len(v)))
    lib, st = got["lib"], got["statement"]
    same = np.array_equal(lib["peak_offsets"], st["peak_offsets"]) and np.array_equal(lib["beats"], st["peaks"])
    print("  beats: the library and the numpy statement %s (%d beats in %d clips)" %
          ("identical" if same else "DIFFER", lib["beats"].size, NSIG))
    print("  bytes that cross: %.2f MB of tables up, %.2f MB of lags, counts and beats back, against %.1f MB of envelope" %
          ((tables[0].nbytes + tables[1].nbytes) / 1e6, (4 * NSIG + 8 * (NSIG + 1) + 8 * lib["beats"].size) / 1e6, 4 * F / 1e6))
    plan.close()
    if not same:
        sys.exit("beat_bench: the host route differs from the definition")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="OHA")
    a = ap.parse_args()
    print("command: tools/beat_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "O" in a.sections:
        section_o(a.rounds, a.launches)
        torch.cuda.empty_cache()
    if "H" in a.sections:
        section_h(a.host_reps)
        torch.cuda.empty_cache()
    if "A" in a.sections:
        Pl, T = gb.load_parent(a.parent), capi.lib()
        for rep in (1, 2):
            for n, label in ((1024, "N = 1024, all features (the headline)"), (2048, "N = 2048, all features (C5)")):
                gb.section_a(Pl, T, n, 262144, n, capi.ALL_FEATURES, "%s, measurement %d" % (label, rep), a.rounds, a.launches)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
