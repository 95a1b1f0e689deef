"""Conditions on tests/fast_ref.py from the CPU alone: what keeps tests/test_gpu_fast.py from going vacuous. The
exact statement and its scale are right (the oracle's own spectrum meets it with a tenth of the bar to spare), an
honest float32 transform meets it with half to spare, three wrong transforms do not, and the inputs leave no
frame out of any comparison.

Measured with the inputs as they stand (N = 256 / 512 / 1024 / 2048 / 4096), worst ratio to the bar: the oracle's
amplitudes 0.025 / 0.022 / 0.032 / 0.031 / 0.019, fast_ref.fft32 0.082 / 0.069 / 0.074 / 0.064 / 0.069.
"""
import numpy as np
import pytest

import fast_ref
import ladder


@pytest.fixture(scope="module", params=fast_ref.SIZES)
def case(request, oracle_mod):
    n = request.param
    x = fast_ref.frames(n)
    w = fast_ref.window(n)
    ref = oracle_mod.extract(x, want_complex=True)
    return n, x, w, fast_ref.exact(x, w), ref


def test_shape_and_kinds():
    for n in (256, 4096):
        x, k = fast_ref.frames(n), fast_ref.kinds(n)
        assert x.shape == (67, n) and x.dtype == np.float32 and fast_ref.F == 67 == 4 * 16 + 3
        assert sorted(set(k)) == sorted(fast_ref.KINDS)
        assert np.isfinite(x).all() and (np.abs(x) < 2).all()
        assert np.array_equal(fast_ref.frames(n), fast_ref.frames(n, 7000 + n))
        assert not np.array_equal(fast_ref.frames(n), fast_ref.frames(n, 1))
        for b in ladder.bases(n):
            assert (x == b).all(1).any()
    assert [round(fast_ref.spectrum_bar(n) * 1e7) for n in (256, 4096)] == [35, 51]


def test_the_window_is_the_plans(case):
    """fast_ref.window is the oracle's table; the library's host table (no GPU needed) is the same bits."""
    n, _, w, _, _ = case
    from meyda_amd import capi
    for name in ("hanning", "hamming"):
        t = capi.host_tables(buffer_size=n, window=name)["window"]
        assert np.array_equal(t.view(np.uint32), fast_ref.window(n, name).view(np.uint32)), (n, name)


def test_the_oracle_meets_the_exact_statement(case):
    n, x, w, ex, ref = case
    bad, worst = fast_ref.check_exact(ref["amp"], ex)
    bad_c, worst_c = fast_ref.check_exact(fast_ref.complex_of(ref), ex)
    print("N=%d: the oracle against the exact transform, worst ratio to the bar: amplitude %.4f, complex %.4f"
          % (n, worst, worst_c))
    assert not bad and not bad_c
    assert worst < 0.1 and worst_c < 0.1, (worst, worst_c)
    # (a tenth of the bar is 3.5e-7 .. 5.1e-7 in relative 2-norm: a wrong scale, 1 / N for 1 / sqrt N, is far off)
    a, e = ref["amp"].astype(np.float64), np.abs(ex[:, :n // 2])
    live = ~fast_ref.silent_rows(x, w)
    rel = np.sqrt(((a - e) ** 2).sum(1))[live] / np.sqrt((e ** 2).sum(1))[live]
    print("N=%d: the oracle's amplitudes, worst relative 2-norm distance from |X|: %.3g" % (n, rel.max()))


def test_an_honest_float32_transform_meets_it(case):
    n, x, w, ex, _ = case
    got = fast_ref.fft32(fast_ref.windowed(x, w))
    bad, worst = fast_ref.check_exact(got, ex)
    amp = np.abs(got[:, :n // 2]).astype(np.float32)
    bad_a, worst_a = fast_ref.check_exact(amp, ex)
    print("N=%d: a plain float32 radix-2 transform, worst ratio to the bar: complex %.4f, amplitude %.4f" % (n, worst, worst_a))
    assert not bad and not bad_a
    assert worst < 0.5 and worst_a < 0.5, (worst, worst_a)


@pytest.mark.parametrize("name,kw,least", [("one twiddle of the last stage negated", dict(negate_last=True), 20),
                                           ("every twiddle rounded to 12 bits", dict(twiddle_bits=12), 60),
                                           ("a stage without its 1/sqrt 2", dict(unscaled_stage=3), 64)])
def test_the_checker_rejects_wrong_transforms(case, name, kw, least):
    """`least`: the frames that must fail, of the 64 that are not silent. A coarse table and a missing scale spoil
    every frame with more than one nonzero sample; one wrong twiddle spoils those with energy in its two bins."""
    n, x, w, ex, _ = case
    got = fast_ref.fft32(fast_ref.windowed(x, w), **kw)
    for what, g in (("complex", got), ("amplitude", np.abs(got[:, :n // 2]).astype(np.float32))):
        bad, worst = fast_ref.check_exact(g, ex)
        print("N=%d, %s, %s: %d frames rejected, worst ratio %.3g" % (n, name, what, len(bad), worst))
        assert len(bad) >= least and worst > 10.0, (n, name, what, len(bad), worst)
        assert not set(bad) & set(np.nonzero(fast_ref.silent_rows(x, w))[0].tolist())


def test_the_checker_rejects_what_is_not_a_number(case):
    n, x, w, ex, ref = case
    a = ref["amp"].copy()
    a[3, 5] = np.nan
    a[11, 0] = np.inf
    s = int(np.nonzero(fast_ref.kinds(n) == "silent")[0][0])
    a[s, 1] = 1e-30
    bad, worst = fast_ref.check_exact(a, ex)
    assert bad == sorted({3, 11, s}) and worst == np.inf


def test_no_frame_is_left_out(case):
    """No nonzero exact bin has a denormal float32 square, nor has the oracle's spectrum one (ladder.mel_excluded):
    the mel comparisons then cover every frame. Every frame that is not silent once windowed has ||X||_2 > 0; under
    the hanning window the silent ones are the silent frame and the impulses at samples 0 and N - 1, where the
    window is 0, and under hamming the silent frame alone."""
    n, x, w, ex, ref = case
    a = np.abs(ex[:, :n // 2]).astype(np.float32)
    p = a * a
    assert not ((a > 0) & (p < np.float32(2.0 ** -126))).any()
    assert not ladder.mel_excluded(ref["amp"]).any()
    sil = fast_ref.silent_rows(x, w)
    k = fast_ref.kinds(n)
    assert sorted(k[sil]) == ["impulse", "impulse", "silent"]
    assert (np.sqrt((np.abs(ex) ** 2).sum(1))[~sil] > 0).all() and not ex[sil].any()
    ham = fast_ref.window(n, "hamming")
    assert list(k[fast_ref.silent_rows(x, ham)]) == ["silent"]
    assert (np.abs(fast_ref.exact(x, ham)).max(1)[k != "silent"] > 0).all()
    # the frames that get a non-finite sample in tests/test_gpu_fast.py are ordinary ones
    assert not sil[[9, 22, 41]].any()


@pytest.mark.parametrize("n", fast_ref.SIZES)
def test_scale_frames_have_no_small_bins(n):
    """The condition of the scale test: every nonzero exact bin of fast_ref.spread_frames(n) is at least 2^-10 of
    the frame's largest (so at 2^-40 no bin's square is below 2^-126 and at 2^40 none overflows: see
    tests/test_gpu_fast.py), and no bin is exactly zero."""
    x = fast_ref.spread_frames(n)
    assert x.shape == (10, n)
    e = np.abs(fast_ref.exact(x, fast_ref.window(n)))
    assert (e > 0).all()
    ratio = e.min(1) / e.max(1)
    print("N=%d: smallest bin / largest, worst frame: 2^%.2f" % (n, np.log2(ratio.min())))
    assert (ratio >= 2.0 ** -10).all(), np.log2(ratio.min())
    assert e.max() < 2.0 ** 6  # |X| <= sqrt(N) / 2 of a sample below 2
