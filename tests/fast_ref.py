"""What precision="fast" (MGX_PRECISION_FAST, float32 butterflies) promises, stated without the kernel: a helper
module shared by tests/test_fast_host.py, tests/test_gpu_fast.py and tools/fast_precision_report.py. No GPU.

The spectrum. Let xw = float32(x * w) be the windowed frame (the reference's single rounding; w the plan's window
table) and X = fft(float64(xw)) / sqrt(N): jsfft scales each of its log2 N stages by 1 / sqrt(2). A radix-2 FFT in
float32 whose twiddles are rounded to float32 obeys, per frame,

    ||X^ - X||_2 <= log2(N) eta ||X||_2,   eta = u + gamma_4 (sqrt(2) + u) < 7 u,   u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 24.2). The window product is already in xw;
the amplitude's float32 sum of squares and sqrtf add at most 2 u per bin. The bar for amplitudeSpectrum (N / 2
bins) and for complexSpectrum (N bins, both parts together as complex numbers) is therefore

    ||got - exact||_2 <= (7 log2 N + 2) 2^-24 ||exact||_2   per frame:

3.5e-6 at N = 256, 5.1e-6 at N = 4096. An honest float32 radix-2 transform (fft32 below) sits near 3e-7, a tenth
of it; a wrong twiddle, a coarse table or a missing stage scale sits orders of magnitude above it
(tests/test_fast_host.py shows all three).

The inputs. frames(n) is 67 rows -- four groups of 16 and a batch of 3, so full groups, a partial batch and every
wave's lane roles occur -- of every kind of frame a caller has: see KINDS. Under the hanning window the two
impulses at the frame's ends are silent once windowed (w[0] = w[N - 1] = 0); under hamming they are not.
"""
import functools

import numpy as np

import ladder

U = 2.0 ** -24
SIZES = [256, 512, 1024, 2048, 4096]
F = 67
SR = 44100.0
SEED = 0x6D657964
KINDS = ["base", "noise", "tone", "pcm16", "steep", "impulse", "dc", "alternating", "silent"]
# frames per kind: 5 + 14 + 16 + 12 + 14 + 3 + 1 + 1 + 1 = 67
_COUNTS = {"noise": 14, "tone": 16, "pcm16": 12, "steep": 14}


def spectrum_bar(n):
    """(7 log2 N + 2) u: the relative 2-norm bar of the module docstring."""
    return (7.0 * np.log2(n) + 2.0) * U


def window(n, name="hanning"):
    """The reference's window table (windowing.js), from the CPU oracle."""
    from oracle import oracle
    return oracle.tables(n)["hann" if name == "hanning" else "hamming"]


def windowed(x, w):
    """float32(x * w): the exact product rounded once, which is a float32 multiply."""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32) * np.asarray(w, np.float32)[None, :]


def exact(x, w):
    """X = fft(float64(xw)) / sqrt(N), all N bins, complex128, with jsfft's sign of the exponent (e^{+2 pi i jk / N}:
    the conjugate of numpy's forward transform, which for a real frame changes the imaginary parts' sign only)."""
    xw = windowed(x, w).astype(np.float64)
    return np.conj(np.fft.fft(xw, axis=1)) / np.sqrt(xw.shape[1])


def check_exact(got, ex):
    """got: an amplitude spectrum (F x N/2, real) or a complex spectrum (F x N, complex); ex: exact() of the same
    frames. Returns (bad frames, worst ||got - exact||_2 / (bar ||exact||_2)). A frame whose exact spectrum is zero
    must be zero; anything that is not a number is bad."""
    got = np.asarray(got)
    n = ex.shape[1]
    if np.iscomplexobj(got):
        assert got.shape == ex.shape, (got.shape, ex.shape)
        g, e = got.astype(np.complex128), ex
    else:
        assert got.shape == (ex.shape[0], n // 2), (got.shape, ex.shape)
        g, e = got.astype(np.float64), np.abs(ex[:, :n // 2])
    with np.errstate(all="ignore"):
        err = np.sqrt((np.abs(g - e) ** 2).sum(1))
        norm = np.sqrt((np.abs(e) ** 2).sum(1))
        ratio = np.where(norm > 0, err / (spectrum_bar(n) * np.where(norm > 0, norm, 1.0)), np.where(err == 0, 0.0, np.inf))
    bad = np.nonzero(~(ratio <= 1.0))[0].tolist()
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if len(ratio) else 0.0
    return bad, worst


def complex_of(out):
    """The complex spectrum of a GPU result (complexSpectrum.real / .imag) or of the oracle (complex_re / _im)."""
    if "complexSpectrum.real" in out:
        return out["complexSpectrum.real"].astype(np.float64) + 1j * out["complexSpectrum.imag"].astype(np.float64)
    return out["complex_re"].astype(np.float64) + 1j * out["complex_im"].astype(np.float64)


# ---------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def _build(n, seed):
    from oracle import oracle
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    rows, kinds = [], []

    def add(kind, x):
        rows.append(np.asarray(x, np.float64).astype(np.float32))
        kinds.append(kind)

    for b in ladder.bases(n):
        add("base", b)
    for x in oracle.synth_frames(SEED, seed, _COUNTS["noise"], n):
        add("noise", x)
    # off-bin tones, 30 Hz .. 0.45 sr in equal ratios, amplitudes 0.01 .. 0.9 likewise (the loud ones not all high)
    nt = _COUNTS["tone"]
    freqs = 30.0 * (0.45 * SR / 30.0) ** (np.arange(nt) / (nt - 1))
    amps = (0.01 * 90.0 ** (np.arange(nt) / (nt - 1)))[rng.permutation(nt)]
    for f, a, ph in zip(freqs, amps, rng.uniform(0, 2 * np.pi, nt)):
        add("tone", a * np.sin(2 * np.pi * f * t / SR + ph))
    # int16 PCM: a tone in noise at a level, quantised to 1 / 32768
    for i in range(_COUNTS["pcm16"]):
        f, lvl = rng.uniform(100.0, 0.4 * SR), 10.0 ** rng.uniform(-3, -0.1)
        y = lvl * (0.7 * np.sin(2 * np.pi * f * t / SR) + 0.3 * rng.uniform(-1, 1, n))
        add("pcm16", np.round(y * 32768.0) / 32768.0)
    # twice-integrated noise: a spectrum falling by 12 dB per octave
    for i in range(_COUNTS["steep"]):
        y = rng.standard_normal(n)
        y = np.cumsum(np.cumsum(y - y.mean()))
        add("steep", 0.9 * y / np.abs(y).max())
    for at in (0, n - 1, n // 2):
        y = np.zeros(n)
        y[at] = 1.0
        add("impulse", y)
    add("dc", np.full(n, 0.5))
    add("alternating", np.where(t % 2 == 0, 1.0, -1.0))
    add("silent", np.zeros(n))
    assert len(rows) == F
    p = rng.permutation(F)
    x = np.stack(rows)[p]
    k = np.array(kinds)[p]
    x.setflags(write=False)
    k.setflags(write=False)
    return x, k


def frames(n, seed=None):
    """The F = 67 frames at buffer size n, in a seeded permutation (read-only, built once)."""
    return _build(n, 7000 + n if seed is None else seed)[0]


def kinds(n, seed=None):
    """The kind (an entry of KINDS) of every row of frames(n, seed)."""
    return _build(n, 7000 + n if seed is None else seed)[1]


def silent_rows(x, w):
    """Rows whose windowed frame is zero in every sample."""
    return ~windowed(x, w).any(1)


def spread_frames(n):
    """The frames of the scale test (tests/test_gpu_fast.py): the noise and +-1 bases and 8 oracle-noise frames,
    whose nonzero exact bins all lie within 2^-10 of the frame's largest (tests/test_fast_host.py)."""
    from oracle import oracle
    b = ladder.bases(n)
    x = np.concatenate([b[[0, 4]], oracle.synth_frames(SEED, 9000 + n, 8, n)])
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------- a plain float32 transform
def _round_bits(v, bits):
    m, e = np.frexp(v)
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)


def fft32(xw, negate_last=False, twiddle_bits=None, unscaled_stage=None):
    """A plain decimation-in-time radix-2 FFT of the rows of xw in float32 arithmetic, each stage scaled by
    float32(1 / sqrt 2), the twiddles computed in double and rounded to float32: honest float32, no relation to
    the kernel's network. Returns complex128 (F x N) holding the float32 results.

    The three defects tests/test_fast_host.py must see rejected: negate_last negates one twiddle of the last
    stage, twiddle_bits rounds every twiddle to that many mantissa bits, unscaled_stage leaves one stage without
    its 1 / sqrt 2."""
    x = np.asarray(xw, np.float32)
    nf, n = x.shape
    m = int(np.log2(n))
    assert 1 << m == n
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for b in range(m):
        rev |= ((idx >> b) & 1) << (m - 1 - b)
    re, im = x[:, rev].copy(), np.zeros((nf, n), np.float32)
    s = np.float32(np.sqrt(0.5))
    for q in range(m):
        h = 1 << q
        ang = 2.0 * np.pi * np.arange(h) / (2 * h)  # (jsfft's sign: exact())
        c, sn = np.cos(ang), np.sin(ang)
        if twiddle_bits is not None:
            c, sn = _round_bits(c, twiddle_bits), _round_bits(sn, twiddle_bits)
        if negate_last and q == m - 1:
            c[h // 3], sn[h // 3] = -c[h // 3], -sn[h // 3]
        c, sn = c.astype(np.float32), sn.astype(np.float32)
        re, im = re.reshape(nf, -1, 2, h), im.reshape(nf, -1, 2, h)
        ar, ai, br, bi = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
        tr = br * c - bi * sn
        ti = br * sn + bi * c
        k = np.float32(1.0) if q == unscaled_stage else s
        re = np.stack([(ar + tr) * k, (ar - tr) * k], 2).reshape(nf, n)
        im = np.stack([(ai + ti) * k, (ai - ti) * k], 2).reshape(nf, n)
        assert re.dtype == np.float32 and im.dtype == np.float32
    return re.astype(np.float64) + 1j * im.astype(np.float64)
