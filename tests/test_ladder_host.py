"""Conditions on the magnitude ladder (tests/ladder.py) from the CPU oracle alone: what keeps the GPU tests of
tests/test_gpu_ladder.py from going vacuous. They are conditions, not measurements: if a base changes, the
shares are measured again here and the caps stay.

Measured with the bases as they stand (N = 256 / 512 / 1024 / 2048 / 4096): mel_excluded share 0.085 / 0.090 /
0.095 / 0.101 / 0.104; the smallest regime (a non-finite amplitude) holds 5 / 6 / 7 / 8 / 10 frames.
"""
import numpy as np
import pytest

import ladder


@pytest.fixture(scope="module", params=ladder.SIZES)
def case(request, oracle_mod):
    n = request.param
    x = ladder.ladder(n)
    ref = oracle_mod.extract(x)
    return n, x, ref


def test_shapes_and_order():
    n = 256
    x = ladder.ladder(n)
    assert x.shape == (1385, n) and x.dtype == np.float32
    assert ladder.NUM_LADDER == 1385 == 86 * 16 + 9 == 346 * 4 + 1  # the last group and batch are ragged
    b = ladder.bases(n)
    for k, base in ((-149, 0), (0, 3), (127, 4), (-126, 1)):
        assert np.array_equal(x[ladder.frame_index(k, base)], np.ldexp(b[base], k).astype(np.float32))
    assert np.array_equal(x[ladder.frame_index(0, 2)], b[2])
    p = ladder.PERM(n)
    assert np.array_equal(np.sort(p), np.arange(1385))
    assert np.array_equal(p, np.random.default_rng(n).permutation(1385))
    g = ladder.gpu_frames(n)
    assert g.shape == (1385 + 18, n)
    assert np.array_equal(ladder.unpermute(g, n).view(np.uint32), ladder.host_frames(n).view(np.uint32))
    o = ladder.outliers(n)
    for i, k in enumerate(ladder.OUTLIER_K):
        assert o[i, (37 * i + 11) % n] == (1.0 if i % 2 == 0 else -1.0) * 2.0 ** k
        assert (np.abs(np.delete(o[i], (37 * i + 11) % n)) <= 1).all()


def test_inputs_are_finite(case):
    n, x, _ = case
    assert np.isfinite(x).all()
    assert np.isfinite(ladder.outliers(n)).all()
    assert np.isfinite(ladder.bases(n)).all() and (np.abs(ladder.bases(n)) < 2).all()


def test_masked_share_is_capped(case):
    n, _, ref = case
    share = ladder.mel_excluded(ref["amp"]).mean()
    print("N=%d: mel_excluded share %.4f" % (n, share))
    assert share <= 0.125, share


def test_every_regime_is_populated(case):
    n, x, ref = case
    counts = ladder.regimes(x, ref).sum(1)
    print("N=%d: %s" % (n, dict(zip(ladder.REGIMES, counts.tolist()))))
    assert (counts >= 5).all(), dict(zip(ladder.REGIMES, counts.tolist()))


def test_both_sides_of_every_threshold_for_the_unit_base(case):
    """Base 4 is +-2^k: it is tame (every lane partial <= 2^100) for k <= 50 - log2(n / 64) / 2 and not above,
    and each regime of regimes() has a frame of it on either side."""
    n, x, ref = case
    rows = [ladder.frame_index(k, 4) for k in range(ladder.K_MIN, ladder.K_MAX + 1)]
    tame = ladder.tame(x[rows])
    kt = int(np.floor(50 - np.log2(n // 64) / 2))
    assert {256: 49, 512: 48, 1024: 48, 2048: 47, 4096: 47}[n] == kt
    ks = np.arange(ladder.K_MIN, ladder.K_MAX + 1)
    assert tame[ks <= kt].all() and not tame[ks > kt].any()
    r = ladder.regimes(x[rows], {"amp": ref["amp"][rows]})
    part = ladder.lane_partials(x[rows]).astype(np.float64)
    a = ref["amp"][rows].astype(np.float64)
    with np.errstate(all="ignore"):
        amax = a.max(1)
    sides = {
        "partial 2^-100": (part < 2.0 ** -100).any(1),
        "partial 2^100": r[1],
        "|X| 2^-40": amax < 2.0 ** -40,
        "|X| 2^60": amax > 2.0 ** 60,
        "|X| 2^64": amax >= 2.0 ** 64,
        "denormal |X|": r[6],
        "denormal power": r[7],
    }
    for name, m in sides.items():
        assert m.any() and (~m).any(), (n, name)
    if n == 4096:  # the one size at which +-2^127 overflows the spectrum (|X| up to sqrt(N) / 2 of it)
        assert r[5].any() and (~r[5]).any()
