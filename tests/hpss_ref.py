"""The definition of HPSS (include/meyda_gpu.h, section "HPSS") stated in numpy, twice: vectorised (order keys, a
table of reflected indices, a stable argsort) and as plain loops over Python lists. tests/test_hpss_host.py holds
the two against each other and against scipy; the GPU tests hold the library against the vectorised one."""
import numpy as np

MEDIANS, SOFT1, SOFT2, HARD = 0, 1, 2, 3
MODES = {"medians": MEDIANS, "soft1": SOFT1, "soft2": SOFT2, "hard": HARD}


def keys(x):
    """The order-preserving key of every float32: all bits of a negative value flipped, the sign bit of a
    non-negative one set; unsigned comparison of keys is the IEEE total order of the values."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def reflect(u, m):
    """r(u, m): q = u mod 2m in [0, 2m); q if q < m, else 2m - 1 - q."""
    q = np.mod(np.asarray(u, dtype=np.int64), 2 * m)
    return np.where(q < m, q, 2 * m - 1 - q)


def median_axis0(x, K):
    """The median of the K reflected neighbours along axis 0 of a 2-D float32 array, by key order: an element of
    the window, bit for bit."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    m, h = x.shape[0], K // 2
    if m == 0:
        return x.copy()
    idx = reflect(np.arange(m)[:, None] + np.arange(-h, h + 1)[None, :], m)  # (m, K)
    win = x.view(np.uint32)[idx]                                              # (m, K, cols)
    order = np.argsort(keys(win.view(np.float32)), axis=1, kind="stable")
    pick = np.take_along_axis(win, order[:, h:h + 1, :], axis=1)[:, 0, :]
    return np.ascontiguousarray(pick).view(np.float32)


def medians(x, offsets, kt, kf):
    """H and P of the definition for an (F, cols) float32 array and a non-decreasing table of F-limited offsets
    (None: one signal, every row). Rows of no signal are 0 in both."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F = x.shape[0]
    offsets = [0, F] if offsets is None else [min(int(o), F) for o in offsets]
    H, P = np.zeros_like(x), np.zeros_like(x)
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b > a:
            H[a:b] = median_axis0(x[a:b], kt)
            P[a:b] = median_axis0(np.ascontiguousarray(x[a:b].T), kf).T
    return H, P


def mask_outputs(x, H, P, mode, mh=1.0, mp=1.0):
    """The two outputs of a mode from the elements and the two medians: float64 throughout, one rounding to
    float32."""
    if mode == MEDIANS:
        return H.copy(), P.copy()
    mh, mp = np.float32(mh), np.float32(mp)
    with np.errstate(invalid="ignore"):  # (the conversion of a signalling NaN)
        x64, aH, aP = x.astype(np.float64), np.abs(H.astype(np.float64)), np.abs(P.astype(np.float64))
    zero = np.float64(0.5) if (mh == 1 and mp == 1) else np.float64(0.0)

    def one(A, other, margin):
        R = other * np.float64(margin)
        with np.errstate(all="ignore"):
            if mode == HARD:
                return np.where(A > R, x, np.float32(0.0)).astype(np.float32)
            hp, rp = (A * A, R * R) if mode == SOFT2 else (A, R)
            den = hp + rp
            mask = np.where(den == 0.0, zero, hp / np.where(den == 0.0, 1.0, den))
            return (x64 * mask).astype(np.float32)
    return one(aH, aP, mh), one(aP, aH, mp)


def hpss(x, offsets=None, kt=31, kf=31, mode=SOFT2, mh=1.0, mp=1.0):
    """(harmonic, percussive) of the definition; rows of no signal are 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, P = medians(x, offsets, kt, kf)
    yh, yp = mask_outputs(x, H, P, MODES.get(mode, mode), mh, mp)
    F = x.shape[0]
    offs = [0, F] if offsets is None else [min(int(o), F) for o in offsets]
    member = np.zeros(F, bool)
    for a, b in zip(offs[:-1], offs[1:]):
        member[a:b] = True
    yh[~member] = 0
    yp[~member] = 0
    return yh, yp


# ---- the same as plain loops ----

def _key1(bits):
    return (~bits) & 0xFFFFFFFF if bits & 0x80000000 else bits | 0x80000000


def _reflect1(u, m):
    q = u % (2 * m)
    return q if q < m else 2 * m - 1 - q


def _median1(window):
    """The middle of the window's bit patterns sorted by key."""
    return sorted(window, key=_key1)[len(window) // 2]


def medians_loops(x, offsets, kt, kf):
    x = np.ascontiguousarray(x, dtype=np.float32)
    F, cols = x.shape
    bits = x.view(np.uint32).tolist()
    offsets = [0, F] if offsets is None else [min(int(o), F) for o in offsets]
    H = [[0] * cols for _ in range(F)]
    P = [[0] * cols for _ in range(F)]
    ht, hf = kt // 2, kf // 2
    for a, b in zip(offsets[:-1], offsets[1:]):
        n = b - a
        for t in range(a, b):
            for k in range(cols):
                H[t][k] = _median1([bits[a + _reflect1(t - a + j, n)][k] for j in range(-ht, ht + 1)])
                P[t][k] = _median1([bits[t][_reflect1(k + j, cols)] for j in range(-hf, hf + 1)])
    return (np.array(H, np.uint32).reshape(F, cols).view(np.float32), np.array(P, np.uint32).reshape(F, cols).view(np.float32))


def mask_loops(x, H, P, mode, mh=1.0, mp=1.0):
    """Element by element in numpy float64 scalars (each operation rounded once)."""
    F, cols = x.shape
    yh, yp = np.zeros((F, cols), np.float32), np.zeros((F, cols), np.float32)
    if mode == MEDIANS:
        return H.copy(), P.copy()
    mh, mp = np.float64(np.float32(mh)), np.float64(np.float32(mp))
    zero = np.float64(0.5) if (mh == 1 and mp == 1) else np.float64(0.0)

    def one(xv, own, other, margin):
        A, R = abs(np.float64(own)), abs(np.float64(other)) * margin
        if mode == HARD:
            return xv if A > R else np.float32(0.0)
        hp, rp = (A * A, R * R) if mode == SOFT2 else (A, R)
        den = hp + rp
        mask = zero if den == 0.0 else hp / den
        return np.float32(np.float64(xv) * mask)
    with np.errstate(all="ignore"):
        for t in range(F):
            for k in range(cols):
                yh[t, k] = one(x[t, k], H[t, k], P[t, k], mh)
                yp[t, k] = one(x[t, k], P[t, k], H[t, k], mp)
    return yh, yp


def same_bits(got, want, what, payload=False):
    """Equality of bits over every element; a NaN for a NaN unless `payload` (MEDIANS: the output is a copied
    element, payload and all; a computed NaN's payload is not part of the definition)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    diff = g != w
    if not payload:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, "NaNs differ", np.argwhere(np.isnan(got) != nan)[:4])
        diff &= ~nan
    bad = np.argwhere(diff)
    assert bad.size == 0, (what, len(bad), bad[:4], [(hex(g[tuple(i)]), hex(w[tuple(i)])) for i in bad[:4]])
