"""The numpy statements of the tempo definitions of include/meyda_gpu.h: the tempogram, the window, the prior and
the pick. Every device route is compared with these, the tempogram and the pick for equal bits."""
import numpy as np

NORM_NONE, NORM_LAG0 = 0, 1


def window_ref(W):
    """The periodic Hann window: float64, one rounding to float32."""
    j = np.arange(W, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * j / np.float64(W))).astype(np.float32)


def prior_ref(frame_rate, L, start_bpm=120.0, std_octaves=1.0, max_bpm=320.0):
    """librosa's log-normal prior over the lags, without its constant factor; float64."""
    p = np.zeros(L, np.float64)
    l = np.arange(1, L, dtype=np.float64)
    bpm = 60.0 * np.float64(frame_rate) / l
    z = (np.log2(bpm) - np.log2(np.float64(start_bpm))) / np.float64(std_octaves)
    v = np.exp(-0.5 * (z * z))
    if max_bpm > 0:
        v = np.where(bpm > max_bpm, 0.0, v)
    p[1:] = v
    return p


def _signals(F, frame_offsets):
    if frame_offsets is None:
        return [(0, F)]
    t = np.minimum(np.asarray(frame_offsets, dtype=np.uint64).astype(np.int64), F)
    return [(int(t[s]), int(t[s + 1])) for s in range(t.size - 1)]


def windowed_ref(x, h, frame_offsets=None):
    """y of step 1 for every row: (F, W) float32, and the mask of the rows that belong to a signal."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float32)
    F, W = x.shape[0], h.shape[0]
    y = np.zeros((F, W), np.float32)
    owned = np.zeros(F, bool)
    j = np.arange(W)
    with np.errstate(all="ignore"):
        for a, b in _signals(F, frame_offsets):
            if b <= a:
                continue
            owned[a:b] = True
            u = np.arange(a, b)[:, None] - W // 2 + j[None, :]
            inside = (u >= a) & (u < b)
            xs = np.where(inside, x[np.clip(u, 0, F - 1)].astype(np.float64), 0.0)
            y[a:b] = (h.astype(np.float64)[None, :] * xs).astype(np.float32)
    return y, owned


def sums_ref(x, h, L, frame_offsets=None):
    """S of step 2 for every row: (F, L) float64, and the mask of the rows that belong to a signal."""
    y, owned = windowed_ref(x, h, frame_offsets)
    F, W = y.shape
    y64 = y.astype(np.float64)
    S = np.zeros((F, L), np.float64)
    with np.errstate(all="ignore"):
        for j in range(W):
            n = min(L, W - j)
            # the product of two float32 values is exact in float64; the addition rounds once
            S[:, :n] += y64[:, j:j + 1] * y64[:, j:j + n]
    return S, owned


def finish_ref(S, owned, norm=NORM_LAG0, fill=0.0):
    """Steps 3 to 5 on the sums: (F, L) float32, `fill` in the rows of no signal."""
    S = S.copy()
    with np.errstate(all="ignore"):
        if norm == NORM_LAG0:
            s0 = S[:, 0]
            ok = (s0 > 0) & np.isfinite(s0)
            S[ok] = S[ok] / s0[ok, None]
        out = S.astype(np.float32)
    out[~owned] = fill
    return out


def tempogram_ref(x, h, L, norm=NORM_LAG0, frame_offsets=None, fill=0.0):
    """The tempogram: (F, L) float32, `fill` in the rows of no signal."""
    S, owned = sums_ref(x, h, L, frame_offsets)
    return finish_ref(S, owned, norm, fill)


def tempogram_loops(x, h, L, norm=NORM_LAG0, frame_offsets=None, fill=0.0):
    """The same, written from the definition as a loop per row and per lag (slow: for small cases)."""
    x = np.asarray(x)
    h = np.asarray(h, dtype=np.float32)
    F, W = x.shape[0], h.shape[0]
    out = np.full((F, L), fill, np.float32)
    with np.errstate(all="ignore"):
        for a, b in _signals(F, frame_offsets):
            for t in range(a, b):
                y = np.zeros(W, np.float32)
                for j in range(W):
                    u = t - W // 2 + j
                    xv = np.float64(x[u]) if a <= u < b else np.float64(0.0)
                    y[j] = np.float32(np.float64(h[j]) * xv)
                S = np.zeros(L, np.float64)
                for l in range(L):
                    acc = np.float64(0.0)
                    for j in range(W - l):
                        acc = acc + np.float64(y[j]) * np.float64(y[j + l])
                    S[l] = acc
                if norm == NORM_LAG0 and S[0] > 0 and np.isfinite(S[0]):
                    S = S / S[0]
                out[t] = S.astype(np.float32)
    return out


def pick_ref(mean, prior, gain=1e6):
    """The lag of every mean row ((S, L) float64): the lowest l whose score is greater than every score before it,
    from a best of +0; a NaN never wins; 0: none."""
    mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
    prior = np.asarray(prior, dtype=np.float64)
    with np.errstate(all="ignore"):
        gm = np.float64(gain) * mean
        one = 1.0 + gm
        score = one * prior[None, :]
    score = np.where(score > 0, score, 0.0)  # (a NaN compares false)
    lag = np.argmax(score, axis=1)           # (the first maximum)
    return np.where(score[np.arange(score.shape[0]), lag] > 0, lag, 0).astype(np.uint32)


def pick_loop(mean, prior, gain=1e6):
    """The pick of one mean row as the definition's scan."""
    best, at = 0.0, 0
    with np.errstate(all="ignore"):
        for l in range(len(mean)):
            s = (np.float64(1.0) + np.float64(gain) * np.float64(mean[l])) * np.float64(prior[l])
            if s > best:
                best, at = s, l
    return at
