"""The definition of the peak picker (include/meyda_gpu.h, mgx_peaks_device) in numpy: the moving maximum and the
moving mean vectorised over the rows with a Python loop over the window's offsets -- so the mean's additions come
in the definition's order, t - pre_avg first, each rounded to float64 --, one division, one addition of delta, and
the greedy minimum distance as a loop over each signal's candidates. Every output is an integer."""
import numpy as np

PARAMS = ("pre_max", "post_max", "pre_avg", "post_avg", "delta", "wait")


def table(F, fo):
    """The signals' [a, b) as int64 arrays: the table's entries limited to F, or one signal [0, F) for None."""
    if fo is None:
        return np.array([0], np.int64), np.array([F], np.int64)
    fo = np.minimum(np.asarray(fo, np.uint64), np.uint64(F)).astype(np.int64)
    return fo[:-1], fo[1:]


def candidates(x, a, b, pre_max=0, post_max=0, pre_avg=0, post_avg=0, delta=0.0):
    """The candidates among rows [a, b) of x (float64), as a boolean array of b - a entries."""
    t = np.arange(a, b)
    at = lambda k: x[np.clip(t + k, a, b - 1)]
    with np.errstate(all="ignore"):
        xt = x[t]
        top = np.ones(b - a, bool)
        for k in range(-pre_max, post_max + 1):
            top &= ~(at(k) > xt)
        m = np.zeros(b - a)
        for k in range(-pre_avg, post_avg + 1):
            m = m + at(k)
        m = m / np.float64(pre_avg + post_avg + 1)
        m = m + np.float64(delta)
        return top & (xt >= m)


def greedy(rows, wait):
    """Of the ascending candidate rows, the first, and every later one more than `wait` behind the last one kept."""
    kept = []
    for t in rows:
        if not kept or t - kept[-1] > wait:
            kept.append(int(t))
    return kept


def peaks(envelope, fo=None, pre_max=0, post_max=0, pre_avg=0, post_avg=0, delta=0.0, wait=0, fill=0):
    """(mask, peak_offsets, peaks): mask uint8 with `fill` in rows that belong to no signal (the rows the operator
    does not write), peak_offsets uint64 of S + 1 entries, peaks uint64, ascending."""
    x = np.asarray(envelope).astype(np.float64).ravel()
    F = x.size
    mask = np.full(F, fill, np.uint8)
    offsets, out = [0], []
    for a, b in zip(*table(F, fo)):
        if b > a:
            mask[a:b] = 0
            c = candidates(x, int(a), int(b), pre_max, post_max, pre_avg, post_avg, delta)
            kept = greedy(a + np.nonzero(c)[0], wait)
            mask[kept] = 1
            out += kept
        offsets.append(len(out))
    return mask, np.array(offsets, np.uint64), np.array(out, np.uint64)
