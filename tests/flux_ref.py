"""The definition of the spectral flux (include/meyda_gpu.h, mgx_flux_device) in numpy, bit for bit: the difference
with its equality rule, the term of each mode, the 64 partials added over the columns in ascending blocks of 64, the
halvings at 32 .. 1, and one rounding to the rows' element type. numpy's float64 additions and multiplications are
IEEE and never fused, so the sum S is the definition's; for the L2 mode numpy's sqrt is the correctly rounded one."""
import numpy as np

RECTIFIED, L1, L2 = 0, 1, 2
MODES = {"rectified": RECTIFIED, "l1": L1, "l2": L2}


def terms(xt, xp, mode):
    """The terms e(c) of rows xt against the earlier rows xp (float64 arrays of one shape)."""
    with np.errstate(all="ignore"):
        d = np.where(xt == xp, 0.0, xt - xp)
        if mode == RECTIFIED:
            return np.where((d > 0) | np.isnan(d), d, 0.0)
        if mode == L1:
            return np.abs(d)
        return d * d


def ordered_sum(e):
    """S of every row of e (rows x cols, float64) in the definition's order."""
    rows, cols = e.shape
    blocks = (cols + 63) // 64
    pad = np.zeros((rows, blocks * 64))
    pad[:, :cols] = e
    pad = pad.reshape(rows, blocks, 64)
    with np.errstate(all="ignore"):
        P = np.zeros((rows, 64))
        for k in range(blocks):
            P = P + pad[:, k, :]
        for h in (32, 16, 8, 4, 2, 1):
            P = P[:, :h] + P[:, h:2 * h]
    return P[:, 0]


def signal_rows(F, fo):
    """For every row its signal's first row, -1 for a row that belongs to no signal. fo: the table (entries limited
    to F, non-decreasing), or None for one signal [0, F)."""
    first = np.full(F, -1, np.int64)
    if fo is None:
        first[:] = 0
        return first
    fo = np.minimum(np.asarray(fo, np.uint64), np.uint64(F)).astype(np.int64)
    for s in range(len(fo) - 1):
        first[fo[s]:fo[s + 1]] = fo[s]
    return first


def sums(rows, fo=None, mode=RECTIFIED, lag=1):
    """(S, written): the float64 sum S of every row and the rows that belong to a signal."""
    x = np.asarray(rows)
    x = x.reshape(x.shape[0], -1).astype(np.float64)
    F = x.shape[0]
    first = signal_rows(F, fo)
    written = first >= 0
    t = np.nonzero(written)[0]
    p = np.maximum(t - lag, first[t])
    S = np.zeros(F)
    if t.size:
        S[t] = ordered_sum(terms(x[t], x[p], mode))
    return S, written


def flux(rows, fo=None, mode=RECTIFIED, lag=1, fill=0.0):
    """The flux column of `rows` in their element type; rows that belong to no signal hold `fill`."""
    mode = MODES.get(mode, mode)
    S, written = sums(rows, fo, mode, lag)
    with np.errstate(all="ignore"):
        v = np.sqrt(S) if mode == L2 else S
        out = np.full(S.shape, fill, np.asarray(rows).dtype)
        out[written] = v[written].astype(out.dtype)
    return out
