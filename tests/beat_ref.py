"""The beat tracker of include/meyda_gpu.h (mgx_beat_tables, mgx_beats_device) restated in numpy, twice: signal_ref
vectorises every step over rows (the recurrence over the lo(p) rows of a step), signal_loop is plain loops over
Python floats (IEEE doubles; the float32 roundings through numpy scalars). Both return, for one signal's rows, the
local score, the cumulative score and the beat rows relative to the signal's first row; beats_ref assembles a whole
array with its table as the device call sees it."""
import math

import numpy as np

MAX_PERIOD = 1023  # MGX_BEAT_MAX_PERIOD


def lo(p):
    """np.round(p / 2) as integers: half of p, ties to even, at least 1."""
    h = p // 2
    if p & 1:
        h += h & 1
    return max(1, h)


def tables(P, tightness=100.0):
    """(gauss, penalty) of mgx_beat_tables: (P + 1)(P + 2) / 2 float32 and (P + 1)^2 float64."""
    gauss = np.zeros((P + 1) * (P + 2) // 2, np.float32)
    penalty = np.full((P + 1) ** 2, -np.inf, np.float64)
    gauss[0] = 1.0
    for p in range(1, P + 1):
        k = np.arange(p + 1, dtype=np.float64)
        gauss[p * (p + 1) // 2:p * (p + 1) // 2 + p + 1] = np.exp(-0.5 * (32.0 * k / p) ** 2).astype(np.float32)
        d = np.arange(lo(p), 2 * p + 1, dtype=np.float64)
        penalty[p * p + lo(p):p * p + 2 * p + 1] = -tightness * np.log(d / p) ** 2
    return gauss, penalty


def _fold(parts):
    """P[l] += P[l + h] for l < h, h = 32, 16, .., 1, on 64 partials; returns P[0]."""
    parts = parts.copy()
    h = 32
    while h >= 1:
        parts[:h] = parts[:h] + parts[h:2 * h]
        h //= 2
    return parts[0]


def _sum64(v):
    """The 64 partials of v (float64) in ascending order, folded."""
    n = v.size
    pad = np.zeros((n + 63) // 64 * 64, np.float64)
    pad[:n] = v
    parts = np.zeros(64, np.float64)
    for row in pad.reshape(-1, 64):  # (a row at a time: sequential per partial; the padding adds +0 to a sum that is never -0)
        parts = parts + row
    return _fold(parts)


def scale_ref(x):
    """sd of step 1 for a signal's rows x (n >= 2), float64."""
    x = x.astype(np.float64)
    n = x.size
    with np.errstate(all="ignore"):
        mean = _sum64(x) / n
        e = x - mean
        return np.sqrt(_sum64(e * e) / (n - 1))


def _nothing(n):
    return np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(0, np.int64)


def _median(v):
    v = np.sort(v)
    m = v.size
    return v[(m - 1) // 2] if m & 1 else (v[m // 2 - 1] + v[m // 2]) * 0.5


def signal_ref(x, p, P, gauss, penalty, trim=1):
    """(local_score, cum_score, beats) of one signal's rows x at period p; a signal that stops before step 3 has +0 in
    both scores."""
    n = x.size
    p = int(p)
    if n < 2 or p == 0 or p > P:
        return _nothing(n)
    with np.errstate(all="ignore"):
        sd = scale_ref(x)
        if not (sd > 0 and np.isfinite(sd)):
            return _nothing(n)
        xn = (x.astype(np.float64) / sd).astype(np.float32)
        g = gauss[p * (p + 1) // 2:p * (p + 1) // 2 + p + 1].astype(np.float64)
        pad = np.zeros(n + 2 * p, np.float64)
        pad[p:p + n] = xn
        ls = np.zeros(n, np.float64)
        for k in range(-p, p + 1):
            ls = ls + g[abs(k)] * pad[p + k:p + k + n]
        lsmax = -np.inf
        finite = ls[~np.isnan(ls)]
        if finite.size and finite.max() > lsmax:
            lsmax = finite.max()
        thr = 0.01 * lsmax
        below = ls < thr
        t0 = n if below.all() else int(np.argmin(below))
        # the recurrence, lo(p) rows at a time: candidates d = 2p .. lo(p) descending along the last axis
        l, ds = lo(p), np.arange(2 * p, lo(p) - 1, -1)
        pen = penalty[p * p + ds]
        Cp = np.zeros(n + 2 * p, np.float64)  # Cp[2p + u] = C(u)
        arg = np.zeros(n, np.int64)
        for t in range(0, n, l):
            rows = np.arange(t, min(t + l, n))
            c = pen[None, :] + Cp[2 * p + rows[:, None] - ds[None, :]]
            c = np.where(np.isnan(c), -np.inf, c)
            j = np.argmax(c, axis=1)  # the first of equal maxima: the larger d
            best = c[np.arange(rows.size), j]
            arg[rows] = np.where(best > -np.inf, ds[j], 0)
            Cp[2 * p + rows] = ls[rows] + best
        C = Cp[2 * p:]
        rows = np.arange(n)
        back = np.where((rows >= t0) & (arg > 0) & (rows - arg >= 0), rows - arg, -1)
        M = np.zeros(n, bool)
        M[1:n - 1] = (C[1:n - 1] > C[:n - 2]) & (C[1:n - 1] >= C[2:])
        M[n - 1] = C[n - 1] > C[n - 2]
        if not M.any():
            return ls, C, np.zeros(0, np.int64)
        med = _median(C[M])
        ok = M & (2.0 * C > med)
        if not ok.any():
            return ls, C, np.zeros(0, np.int64)
        chain = [int(np.flatnonzero(ok).max())]
        while back[chain[-1]] >= 0:
            chain.append(int(back[chain[-1]]))
        chain = np.array(chain, np.int64)  # descending rows
        v = ls[chain]
        later = np.concatenate([[0.0], v[:-1]])
        earlier = np.concatenate([v[1:], [0.0]])
        s = (0.5 * earlier + v) + 0.5 * later
        thr = 0.0
        if trim:
            R = 0.0
            for q in s * s:
                R = R + q
            thr = 0.5 * np.sqrt(R / chain.size)
        valid = chain[s > thr]
        if valid.size == 0:
            return ls, C, np.zeros(0, np.int64)
        beats = chain[(chain >= valid.min()) & (chain <= valid.max())][::-1]
    return ls, C, beats


def signal_loop(x, p, P, gauss, penalty, trim=1):
    """signal_ref as plain loops."""
    n = int(x.size)
    p = int(p)
    if n < 2 or p == 0 or p > P:
        return _nothing(n)
    xs = [float(v) for v in x]

    def sum64(vals):
        parts = [0.0] * 64
        for i, v in enumerate(vals):
            parts[i % 64] += v
        h = 32
        while h >= 1:
            for q in range(h):
                parts[q] += parts[q + h]
            h //= 2
        return parts[0]

    mean = sum64(xs) / n
    es = [v - mean for v in xs]
    Q = sum64([e * e for e in es])
    q = Q / (n - 1)
    sd = math.sqrt(q)  # (q is a sum of squares over a count: not negative, or NaN)
    if not (sd > 0 and math.isfinite(sd)):
        return _nothing(n)
    with np.errstate(all="ignore"):
        xn = [float(np.float32(np.float64(v) / np.float64(sd))) for v in xs]
    g = [float(gauss[p * (p + 1) // 2 + k]) for k in range(p + 1)]
    ls = []
    for t in range(n):
        acc = 0.0
        for k in range(-p, p + 1):
            u = t + k
            acc += g[abs(k)] * (xn[u] if 0 <= u < n else 0.0)
        ls.append(acc)
    lsmax = -math.inf
    for v in ls:
        if v > lsmax:
            lsmax = v
    thr = 0.01 * lsmax
    t0 = n
    for t in range(n):
        if not ls[t] < thr:
            t0 = t
            break
    l = lo(p)
    C, back = [], []
    for t in range(n):
        best, arg = -math.inf, None
        for d in range(2 * p, l - 1, -1):
            c = float(penalty[p * p + d]) + (C[t - d] if t - d >= 0 else 0.0)
            if c > best:
                best, arg = c, d
        C.append(ls[t] + best)
        back.append(t - arg if t >= t0 and arg is not None and t - arg >= 0 else None)
    v = []
    marks = []
    for t in range(1, n):
        m = C[t] > C[t - 1] and (t == n - 1 or C[t] >= C[t + 1])
        if m:
            marks.append(t)
            v.append(C[t])
    out_ls, out_C = np.array(ls, np.float64), np.array(C, np.float64)
    none = np.zeros(0, np.int64)
    if not v:
        return out_ls, out_C, none
    v.sort()
    m = len(v)
    med = v[(m - 1) // 2] if m & 1 else (v[m // 2 - 1] + v[m // 2]) * 0.5
    tail = None
    for t in marks:
        if 2.0 * C[t] > med:
            tail = t
    if tail is None:
        return out_ls, out_C, none
    chain = [tail]
    while back[chain[-1]] is not None:
        chain.append(back[chain[-1]])
    K = len(chain)
    s = []
    for i in range(K):  # i - 1 is the later neighbour, i + 1 the earlier one
        early = ls[chain[i + 1]] if i + 1 < K else 0.0
        late = ls[chain[i - 1]] if i >= 1 else 0.0
        s.append((0.5 * early + ls[chain[i]]) + 0.5 * late)
    thr = 0.0
    if trim:
        R = 0.0
        for q in s:
            R += q * q
        thr = 0.5 * math.sqrt(R / K)
    valid = [chain[i] for i in range(K) if s[i] > thr]
    if not valid:
        return out_ls, out_C, none
    low, high = min(valid), max(valid)
    return out_ls, out_C, np.array(sorted(r for r in chain if low <= r <= high), np.int64)


def beats_ref(x, period, fo, P, gauss, penalty, trim=1, fill=0.0, mask_fill=0, one=signal_ref):
    """The whole call on host arrays: x (F,), period (S,), fo (S + 1,) or None for one signal. Returns a dict with
    local_score and cum_score ((F,) float64, `fill` in rows of no signal), mask ((F,) uint8, `mask_fill` there),
    peak_offsets ((S + 1,) uint64) and peaks (uint64 rows of the whole array, ascending)."""
    F = x.size
    fo = np.array([0, F], np.uint64) if fo is None else np.minimum(np.asarray(fo, np.uint64), np.uint64(F))
    S = fo.size - 1
    ls = np.full(F, fill, np.float64)
    C = np.full(F, fill, np.float64)
    mask = np.full(F, mask_fill, np.uint8)
    offs, rows = [0], []
    for s in range(S):
        a, b = int(fo[s]), int(fo[s + 1])
        l, c, beats = one(x[a:b], period[s], P, gauss, penalty, trim)
        ls[a:b], C[a:b], mask[a:b] = l, c, 0
        mask[a + beats] = 1
        rows.extend(int(a + r) for r in beats)
        offs.append(len(rows))
    return {"local_score": ls, "cum_score": C, "mask": mask, "peak_offsets": np.array(offs, np.uint64),
            "peaks": np.array(rows, np.uint64)}
