"""The two definitions of the chroma section of include/meyda_gpu.h in numpy: the filter bank of mgx_chroma_weights
(librosa.filters.chroma, float64 throughout, one rounding to float32 that keeps a positive value positive) and the operator of mgx_chroma_device, bit for
bit: exact float64 products, 64 partials added over the columns in ascending blocks of 64, the halvings at 32 .. 1,
the maximum scanned in ascending order, one correctly rounded division and one rounding to float32. numpy's float64
additions, multiplications and divisions are IEEE and never fused."""
import numpy as np

NONE, MAX = 0, 1
NORMS = {"none": NONE, "max": MAX}
MAX_BINS = 36


def weights(n, sample_rate, num_chroma=12, a440=440.0, center_octave=5.0, octave_width=2.0, base_c=True):
    """The C x n/2 float32 table."""
    C, K = int(num_chroma), n // 2
    k = np.arange(1, K + 1, dtype=np.float64)
    fb = np.empty(K + 1)
    fb[1:] = C * np.log2((k * float(sample_rate) / n) / (a440 / 16.0))
    fb[0] = fb[1] - 1.5 * C
    bw = np.maximum(fb[1:] - fb[:-1], 1.0)  # k < K
    h = np.round(C / 2.0)  # ties to even
    c = np.arange(C, dtype=np.float64)[:, None]
    d = np.mod(fb[None, :K] - c + h, float(C)) - h
    w = np.exp(-0.5 * (2.0 * d / bw[None, :]) ** 2)
    w = w / np.sqrt(np.sum(w * w, axis=0, keepdims=True))
    if octave_width > 0:
        w = w * np.exp(-0.5 * ((fb[None, :K] / C - center_octave) / octave_width) ** 2)
    if base_c:
        w = np.roll(w, -3 * (C // 12), axis=0)
    w32 = w.astype(np.float32)
    # a positive value below the smallest float32 takes that value, not +0: the table is strictly positive
    w32[(w > 0) & (w32 == 0)] = np.float32(1e-45)
    return np.ascontiguousarray(w32)


def ordered_sums(rows, w):
    """S(t, c) in float64: rows F x cols, w C x cols, any float type whose values float64 holds."""
    x = np.asarray(rows, np.float64)
    w = np.asarray(w, np.float64)
    F, cols = x.shape
    C = w.shape[0]
    blocks = (cols + 63) // 64
    xp = np.zeros((F, blocks * 64))
    xp[:, :cols] = x
    wp = np.zeros((C, blocks * 64))
    wp[:, :cols] = w
    S = np.empty((F, C))
    step = max(1, (1 << 22) // (C * 64))  # rows at a time: the partials of a pass stay near 32 MB
    with np.errstate(all="ignore"):
        for f0 in range(0, F, step):
            xs = xp[f0:f0 + step]
            P = np.zeros((xs.shape[0], C, 64))
            for b in range(blocks):
                prod = xs[:, None, b * 64:(b + 1) * 64] * wp[None, :, b * 64:(b + 1) * 64]
                if (b + 1) * 64 > cols:
                    prod[:, :, cols - b * 64:] = 0.0  # a column that does not exist adds nothing (not 0 x Inf)
                P = P + prod
            for h in (32, 16, 8, 4, 2, 1):
                P = P[:, :, :h] + P[:, :, h:2 * h]
            S[f0:f0 + step] = P[:, :, 0]
    return S


def normalise(S):
    """MGX_CHROMA_NORM_MAX over float64 sums S (F x C)."""
    S = np.array(S, np.float64)
    m = np.full(S.shape[0], -np.inf)
    with np.errstate(all="ignore"):
        for c in range(S.shape[1]):
            m = np.where(S[:, c] > m, S[:, c], m)
        ok = (m > 0) & np.isfinite(m)
        S[ok] = S[ok] / m[ok, None]
    return S


def chroma(rows, w, norm=MAX):
    """The F x C float32 chroma rows."""
    norm = NORMS.get(norm, norm)
    S = ordered_sums(rows, w)
    if norm == MAX:
        S = normalise(S)
    with np.errstate(all="ignore"):
        return S.astype(np.float32)
