#!/usr/bin/env python3
"""The measurements of profiles/tempo.txt on one MI355X: what the tempogram operator (mgx_tempogram_device), the
tempogram -> pooling -> pick call (mgx_tempo_device) and the host route (mgx_tempo_host) cost, against forming the
same rows with torch (device) or numpy (host) -- what a caller has without them --, and that the existing launches did
not move.

The corpus is tools/gather_bench.py's: 1,024 clips of 66,304 samples, N = 1024, hop 256 (256 buffers a clip, 262,144
in all); the envelope is the rectified flux of melBands (40 bands), W = L = 384, norm lag0.

T. the operator alone, the corpus as 1,024 clips and as one signal of 262,144 rows, with the achieved FP64 rate: the
   FMAs the definition needs (F (W L - L (L - 1) / 2)) and the FMAs the kernel issues (F roundup(W, K) 64 K: every
   lane walks the whole window), against the 78.6 TFLOP/s vector peak. Against torch on the device for the one
   signal: the windowed frames' rfft at length 2 W, |.|^2, irfft, divided by lag 0, in float64 and in float32, 65,536
   rows at a time. torch sums in another order: the largest difference of the normalised rows is printed.
D. mgx_tempo_device with and without the tempogram output (the second passes 65,536 rows at a time through the
   workspace), and the bytes of both workspaces; the two routes' bits are compared.
H. host, wall clock: mgx_tempo_host against mgx_summarize_flux_host with per_frame plus numpy: the statement of
   tests/tempo_ref.py (one pass: it is the definition, not a fast route) and the FFT autocorrelation librosa uses, each
   with the pooling and the pick.
A. unchanged launches: the headline (N = 1024) and C5 (N = 2048) launches of the tree's library against a build of the
   parent revision (tools/build_rev.sh REV NAME -> ab/lib_NAME.so), as tools/gather_bench.py section A, twice.

Variants of a section run in one process in interleaved rounds; per variant the median, min and spread (max - min
over the rounds) are printed: a difference is read against that spread.
usage: tempo_bench.py [--parent ab/lib_parent.so] [--rounds R] [--launches K] [--sections TDHA] [--host-reps R]"""
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
import gather_bench as gb  # noqa: E402
import tempo_ref  # noqa: E402
from summary_bench import N, HOP, NSIG, PER, corpus  # noqa: E402

NM = 40
REQ = dict(feature="melBands", mode="rectified", lag=1)
W = L = 384
RATE = 44100.0 / HOP
PEAK = 78.6e12
CHUNK = 65536


def envelope():
    x, starts, fo = corpus()
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    _, _, fres = plan.summarize_gather_torch(x, starts, fo, [], (), flux=[dict(REQ, per_frame=True, summary=False)])
    env = fres[0]["per_frame"]
    torch.cuda.synchronize()
    plan.close()
    return env, fo


def torch_tempogram(env, h, dtype, out):
    """One signal: zero padding at both ends, the windowed frames' power spectrum at length 2 W back to the lags."""
    F = env.shape[0]
    pad = torch.zeros(F + W, dtype=dtype, device=env.device)
    pad[W // 2:W // 2 + F] = env.to(dtype)
    frames = pad.unfold(0, W, 1)
    hw = h.to(dtype)
    for r0 in range(0, F, CHUNK):
        y = frames[r0:r0 + CHUNK] * hw
        s = torch.fft.irfft(torch.fft.rfft(y, n=2 * W).abs().square(), n=2 * W)[:, :L]
        s0 = s[:, :1]
        out[r0:r0 + CHUNK] = torch.where((s0 > 0) & s0.isfinite(), s / s0, s).to(torch.float32)


def section_t(rounds, launches):
    env, fo = envelope()
    F = env.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    h = torch.from_numpy(capi.tempogram_window(W)).cuda()
    out = torch.zeros((F, L), dtype=torch.float32, device="cuda")
    tout = torch.zeros((F, L), dtype=torch.float32, device="cuda")
    K = next(k for k in (1, 2, 3, 4, 6, 8, 12, 16) if 64 * k >= L)
    need = F * (W * L - L * (L - 1) // 2)
    issued = F * (-(-W // K) * K) * 64 * K
    print("\n== T. the operator alone: %d rows, W = L = %d, norm lag0; %.2f G FMAs by the definition, %.2f G issued (K = %d)" %
          (F, W, need / 1e9, issued / 1e9, K))
    tables = (("%d clips of %d rows" % (NSIG, PER), torch.from_numpy(fo.view(np.int64)).cuda(), NSIG), ("one signal of %d rows" % F, None, 0))
    for label, tb, S in tables:
        def op():
            capi.tempogram_device(env.data_ptr(), F, False, None if tb is None else tb.data_ptr(), S, h.data_ptr(), W, L, 1,
                                  out.data_ptr(), stream)
        variants = [("mgx_tempogram_device", op)]
        if tb is None:
            variants += [("torch rfft, float64", lambda: torch_tempogram(env, h, torch.float64, tout), 1),
                         ("torch rfft, float32", lambda: torch_tempogram(env, h, torch.float32, tout), 1),
                         ("mgx_tempogram_device (again)", op)]
        print("  -- %s" % label)
        res = gb.interleaved(variants, rounds, launches, warm=2)
        gb.report(res, F)
        ms = float(np.median(res["mgx_tempogram_device"]))
        print("  %.4f ms: %.2f TFLOP/s of the definition's FMAs (%.1f %% of the %.1f TFLOP/s FP64 peak), %.2f TFLOP/s issued (%.1f %%); "
              "%.1f MB written: %.2f TB/s" % (ms, 2 * need / ms / 1e9, 200 * need / ms / 1e9 / PEAK * 1e12, PEAK / 1e12,
                                             2 * issued / ms / 1e9, 200 * issued / ms / 1e9 / PEAK * 1e12, 4 * F * L / 1e6, 4 * F * L / ms / 1e9))
        if tb is None:
            op()
            for dtype in (torch.float64, torch.float32):
                torch_tempogram(env, h, dtype, tout)
                torch.cuda.synchronize()
                print("  against torch %s: largest difference of the normalised rows %.3g; torch takes %.1f times as long" %
                      (str(dtype).split(".")[1], float((out - tout).abs().max()),
                       np.median(res["torch rfft, %s" % str(dtype).split(".")[1]]) / ms))
            rows = tempo_ref.tempogram_ref(env[:2000].cpu().numpy(), h.cpu().numpy(), L, tempo_ref.NORM_LAG0, [0, F])
            same = np.array_equal(out[:1800].cpu().numpy().view(np.uint32), rows[:1800].view(np.uint32))
            print("  the first 1,800 rows against the numpy statement: %s" % ("identical, bit for bit" if same else "DIFFER"))
            if not same:
                sys.exit("tempo_bench: the operator differs from its definition")


def section_d(rounds, launches):
    env, fo = envelope()
    F = env.shape[0]
    h = torch.from_numpy(capi.tempogram_window(W)).cuda()
    p = torch.from_numpy(capi.tempo_prior(RATE, L)).cuda()
    tb = torch.from_numpy(fo.view(np.int64)).cuda()
    tp = capi.tempo_params(W, L)
    rows = torch.zeros((F, L), dtype=torch.float32, device="cuda")
    ws = {keep: torch.empty(capi.tempo_workspace_bytes(F, NSIG, tp, keep), dtype=torch.uint8, device="cuda") for keep in (True, False)}
    got = {}

    def call(keep):
        def fn():
            got[keep] = capi.tempo_torch(env, h, p, tb, tempogram=rows if keep else None, workspace=ws[keep])
        return fn
    print("\n== D. mgx_tempo_device: tempogram -> pooling -> pick, %d rows in %d clips; workspace %.1f MB with the tempogram output "
          "(%.1f MB, the caller's), %.1f MB without" % (F, NSIG, ws[True].numel() / 1e6, 4 * F * L / 1e6, ws[False].numel() / 1e6))
    res = gb.interleaved([("with the tempogram output", call(True)), ("without (4 passes of 65,536 rows)", call(False)),
                          ("with the tempogram output (again)", call(True))], rounds, launches, warm=2)
    gb.report(res, F)
    torch.cuda.synchronize()
    same = all(torch.equal(got[True][k].view(torch.int32), got[False][k].view(torch.int32)) for k in ("summary", "lag"))
    lag = got[True]["lag"].cpu().numpy()
    print("  the two routes: %s; lags picked: %d clips with a tempo, median lag %d (%.1f bpm)" %
          ("identical, bit for bit" if same else "DIFFER", int((lag > 0).sum()), int(np.median(lag)), 60 * RATE / max(float(np.median(lag)), 1)))
    if not same:
        sys.exit("tempo_bench: the two routes of mgx_tempo_device differ")


def numpy_fft_rows(col, fo, h):
    """The FFT autocorrelation of librosa.feature.tempogram per clip, float64."""
    out = np.zeros((col.size, L), np.float32)
    h64 = h.astype(np.float64)
    for s in range(len(fo) - 1):
        a, b = int(fo[s]), int(fo[s + 1])
        if b <= a:
            continue
        pad = np.zeros(b - a + W, np.float64)
        pad[W // 2:W // 2 + b - a] = col[a:b]
        y = np.lib.stride_tricks.sliding_window_view(pad, W)[:b - a] * h64
        ac = np.fft.irfft(np.abs(np.fft.rfft(y, n=2 * W, axis=1)) ** 2, n=2 * W, axis=1)[:, :L]
        s0 = ac[:, :1]
        with np.errstate(all="ignore"):
            out[a:b] = np.where((s0 > 0) & np.isfinite(s0), ac / s0, ac)
    return out


def pooled_pick(rows, fo, p):
    seg = fo[:-1].astype(np.int64)
    cnt = np.diff(fo.astype(np.int64)).astype(np.float64)[:, None]
    mean = np.add.reduceat(rows.astype(np.float64), seg) / cnt
    return mean, tempo_ref.pick_ref(mean, p)


def section_h(reps):
    x, starts, fo = corpus()
    xh = x.cpu().numpy()
    F = starts.size
    plan = capi.Plan(buffer_size=N, num_mel_bands=NM)
    h, p = capi.tempogram_window(W), capi.tempo_prior(RATE, L)
    got = {}

    def tempo():
        got["lib"] = plan.tempo(xh, starts, fo, RATE, mean=True, win_length=W, **REQ)

    def flux():
        return plan.summarize_gather(xh, starts, fo, [], flux=[dict(REQ, per_frame=True, summary=False)])[2][0]["per_frame"]

    def flux_fft():
        got["fft"] = pooled_pick(numpy_fft_rows(flux(), fo, h), fo, p)

    def flux_statement():
        got["statement"] = pooled_pick(tempo_ref.tempogram_ref(flux(), h, L, tempo_ref.NORM_LAG0, fo), fo, p)

    print("\n== H. host, wall clock per corpus (%d buffers of %d clips; the rectified flux of melBands, W = L = %d, mean row and lag)" %
          (F, NSIG, W))
    variants = [("mgx_tempo_host", tempo, reps), ("mgx_summarize_flux_host (per_frame) + numpy FFT autocorrelation", flux_fft, reps),
                ("mgx_summarize_flux_host (per_frame) alone", flux, reps),
                ("mgx_summarize_flux_host (per_frame) + the numpy statement", flux_statement, 1)]
    tempo()  # (staging allocated)
    ts = {name: [] for name, _, _ in variants}
    for r in range(reps):
        for name, fn, k in variants:
            if r >= k:
                continue
            t = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t) * 1e3)
    for name, v in ts.items():
        print("  %-66s median %9.1f ms  min %9.1f  max %9.1f  spread %7.1f  (%d)" %
              (name, np.median(v), np.min(v), np.max(v), np.max(v) - np.min(v), len(v)))
    lib = got["lib"]
    st_mean, st_lag = got["statement"]
    ff_mean, ff_lag = got["fft"]
    print("  lags: the library and the numpy statement %s (%d of %d differ); the library and the FFT route differ in %d of %d; the mean rows: "
          "largest difference %.3g (statement), %.3g (FFT)" %
          ("identical" if np.array_equal(lib["lag"], st_lag) else "DIFFER", int((lib["lag"] != st_lag).sum()), NSIG,
           int((lib["lag"] != ff_lag).sum()), NSIG, float(np.abs(lib["summary"][:, 0] - st_mean).max()),
           float(np.abs(lib["summary"][:, 0] - ff_mean).max())))
    print("  bytes that cross back: %.2f MB of summaries and lags, against %.1f MB of envelope and %.1f MB of tempogram rows" %
          ((8 * NSIG * 4 * L + 4 * NSIG) / 1e6, 4 * F / 1e6, 4 * F * L / 1e6))
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sections", default="TDHA")
    a = ap.parse_args()
    print("command: tools/tempo_bench.py %s" % " ".join(sys.argv[1:]))
    print("device: %s; %d interleaved rounds of %d launches" % (torch.cuda.get_device_name(0), a.rounds, a.launches))
    if "T" in a.sections:
        section_t(a.rounds, a.launches)
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
