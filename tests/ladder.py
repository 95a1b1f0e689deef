"""The magnitude ladder: five base frames at every power-of-two scale a float32 holds, so that every range
branch of the frame kernel (kernels.hip frame_phase1 and phase 2: the f64 energy redo, the tame / two-form
butterflies, the rsq amplitude or slot_amp, the paired log, the non-finite band sums, the float32 stores of
f64 scalars) is crossed at its threshold and not only visited well inside it. A helper module: the inputs and
the masks, built once per N and shared by tests/test_ladder_host.py, tests/test_oracle_golden.py and
tests/test_gpu_ladder.py. Every mask comes from the input and the CPU oracle alone, never from a GPU result.

`python tests/ladder.py` writes tests/golden/ladder/bases.f32, the input of `tools/gen_golden.js --ladder`.
"""
import functools
import os

import numpy as np

K_MIN, K_MAX = -149, 127
NUM_BASES = 5
NUM_LADDER = (K_MAX - K_MIN + 1) * NUM_BASES  # 1,385 = 86 groups of 16 + 9 = 346 batches of 4 + 1
OUTLIER_K = [44, 45, 46, 47, 48, 49, 50, 51, 52, 59, 60, 61, 63, 64, 65, 100, 126, 127]
SIZES = [256, 512, 1024, 2048, 4096]
# the fixture that pins the oracle to the reference on the ladder (tools/gen_golden.js --ladder)
GOLDEN_N = 512
GOLDEN_KS = list(range(K_MIN, K_MAX + 1, 4))  # 70 scales, 350 frames
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ladder")
# one-frame calls (tests/test_gpu_ladder.py g): bases 0 and 4 on both sides of every threshold
ONE_FRAME_K = [-149, -127, -126, -101, -100, -51, -50, -41, -40, -39, 0, 47, 48, 49, 50, 51, 59, 60, 61, 63, 64,
               65, 100, 126, 127]
ONE_FRAME_BASES = [0, 4]

REGIMES = ["partial<2^-100", "partial>2^100", "min|X|<2^-40<=max", "max|X| in (2^60,2^64)", "max|X|>=2^64 finite",
           "non-finite |X|", "denormal |X|", "denormal power"]


@functools.lru_cache(maxsize=None)
def bases(n):
    """Five float32 frames: noise, an off-bin tone, a bin-centred tone (exact-zero and near-zero bins beside a
    large one), an impulse, and +-1 (exact powers of two after scaling).

    The tones are louder than the 0.8 sin(..) they began as: with those, only 2 ladder frames at N = 256 and 4
    at N = 512 and 1024 reach a non-finite amplitude (the tones at k = 127, and 126), below the 5 that
    tests/test_ladder_host.py asks of every regime. Every sample has to stay below 2 (the frame at k = 127
    is finite), and a tone's largest |X| is sqrt(N) / 4 of its amplitude, so a tone alone overflows on two
    rungs at N = 256. The off-bin tone is therefore doubled (an exact scaling: the same frames one rung up) and
    the bin-centred tone stands on a DC offset of 1.1, whose bin 0 is sqrt(N) / 2 of it: three rungs.
    Non-finite frames: 5 / 6 / 7 / 8 / 10 at N = 256 .. 4096; mel_excluded shares 0.085 / 0.090 / 0.095 /
    0.101 / 0.104 (CPU oracle)."""
    rng = np.random.default_rng(4000 + n)
    t = np.arange(n)
    noise = rng.uniform(-1, 1, n)
    off_bin = 1.6 * np.sin(2 * np.pi * (n / 16 + 0.37) * t / n)
    on_bin = 0.8 * np.sin(2 * np.pi * (n / 8) * t / n) + 1.1
    impulse = np.zeros(n)
    impulse[5] = 1.0
    signs = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    b = np.stack([noise, off_bin, on_bin, impulse, signs]).astype(np.float32)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def ladder(n):
    """np.ldexp(base, k) for k = -149 .. 127 and every base, k-major: frame 5 (k + 149) + b. Each an exact
    scaling (a result below 2^-149 rounds once, to a denormal or zero)."""
    b = bases(n)
    k = np.arange(K_MIN, K_MAX + 1, dtype=np.int32)
    x = np.ldexp(b[None, :, :], k[:, None, None]).astype(np.float32).reshape(NUM_LADDER, n)
    x.setflags(write=False)
    return x


def frame_index(k, base):
    return NUM_BASES * (k - K_MIN) + base


@functools.lru_cache(maxsize=None)
def PERM(n):
    """The order every GPU run takes the ladder in: the 4 frames of a wave's batch and the 16 of a group then
    belong to different regimes."""
    p = np.random.default_rng(n).permutation(NUM_LADDER)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def outliers(n):
    """18 noise frames with one sample at +-2^k: one lane trips the ballot in an otherwise ordinary frame."""
    x = np.random.default_rng(4100 + n).uniform(-1, 1, (len(OUTLIER_K), n)).astype(np.float32)
    for i, k in enumerate(OUTLIER_K):
        x[i, (37 * i + 11) % n] = np.float32(np.ldexp(1.0 if i % 2 == 0 else -1.0, k))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def gpu_frames(n):
    """The 1,385 + 18 frames of a GPU run: the permuted ladder, then the outliers."""
    x = np.concatenate([ladder(n)[PERM(n)], outliers(n)])
    x.setflags(write=False)
    return x


def unpermute(a, n):
    """Rows of a GPU result over gpu_frames(n), back in ladder order (the outliers stay last)."""
    a = np.asarray(a)
    out = np.empty_like(a)
    out[PERM(n)] = a[:NUM_LADDER]
    out[NUM_LADDER:] = a[NUM_LADDER:]
    return out


@functools.lru_cache(maxsize=None)
def host_frames(n):
    """gpu_frames(n) un-permuted: the ladder in k-major order, then the outliers (what the oracle runs on)."""
    x = np.concatenate([ladder(n), outliers(n)])
    x.setflags(write=False)
    return x


def mel_excluded(ref_amp):
    """Frames whose float32 power a * a has an element in (0, 2^-126): denormal powers leave the reference's own
    mel sums a few significant bits (tests/test_gpu_edge.py edge_frames), so their mfcc and melBands values
    are no parity target. From the oracle's amplitudes alone."""
    a = np.asarray(ref_amp, np.float32)
    with np.errstate(all="ignore"):
        p = a * a
    return ((p > 0) & (p < np.float32(2.0 ** -126))).any(1)


def lane_partials(x):
    """Lane l's float32 sum of squares: lane l of chunk c holds sample 64 c + l, n / 64 samples per lane."""
    x = np.asarray(x, np.float32)
    F, n = x.shape
    ch = x.reshape(F, n // 64, 64)
    e = np.zeros((F, 64), np.float32)
    with np.errstate(all="ignore"):
        for c in range(n // 64):
            e = (ch[:, c].astype(np.float64) * ch[:, c].astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    return e


def regimes(x, ref):
    """Per-frame booleans, one row per name of REGIMES, from the input and the oracle's amplitudes only."""
    a = np.asarray(ref["amp"], np.float32).astype(np.float64)
    e = lane_partials(x).astype(np.float64)
    fin = np.isfinite(a).all(1)
    with np.errstate(all="ignore"):
        amax, amin = a.max(1), a.min(1)
        p = (a.astype(np.float32) * a.astype(np.float32))
    tiny = np.float32(2.0 ** -126)
    return np.stack([
        (e < 2.0 ** -100).any(1),
        (e > 2.0 ** 100).any(1),
        fin & (amin < 2.0 ** -40) & (amax >= 2.0 ** -40),
        fin & (amax > 2.0 ** 60) & (amax < 2.0 ** 64),
        fin & (amax >= 2.0 ** 64),
        ~fin,
        ((a > 0) & (a < float(tiny))).any(1),
        ((p > 0) & (p < tiny)).any(1),
    ])


def tame(x):
    """kernels.hip frame_phase1: every lane partial <= 2^100 (and none NaN)."""
    return (lane_partials(x).astype(np.float64) <= 2.0 ** 100).all(1)


def golden_frames():
    """The 350 frames of the committed ladder fixture: float32(base * 2^k) for GOLDEN_KS, k-major."""
    return ladder(GOLDEN_N).reshape(-1, NUM_BASES, GOLDEN_N)[[k - K_MIN for k in GOLDEN_KS]].reshape(-1, GOLDEN_N)


def load_golden():
    """The reference's outputs on golden_frames() (tests/golden/ladder/, made by tools/gen_golden.js --ladder)."""
    import json
    with open(os.path.join(GOLDEN_DIR, "manifest.json")) as f:
        m = json.load(f)
    F = m["frames"]
    g = {"manifest": m, "F": F}
    dt = {".f32": np.float32, ".f64": np.float64}
    for key, rel in m["files"].items():
        g[key] = np.fromfile(os.path.join(GOLDEN_DIR, rel), dtype=dt[os.path.splitext(rel)[1]])
    g["bases"] = g["bases"].reshape(NUM_BASES, GOLDEN_N)
    for key in ("amp", "scalars", "loudness_specific", "mfcc"):
        g[key] = g[key].reshape(F, -1)
    return g


if __name__ == "__main__":
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    bases(GOLDEN_N).tofile(os.path.join(GOLDEN_DIR, "bases.f32"))
    print("wrote %s" % os.path.join(GOLDEN_DIR, "bases.f32"))
