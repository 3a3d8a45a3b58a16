"""Referee of the intensity augmentation (include/micformer_intensity.h): numpy, float64 by default; `dtype=np.float32` runs the
same formulas in float32 (the fp32 gate of tests/test_intensity_cpu.py).  The blur is written out as explicit reflect + weights
(`blur`), which test_intensity_cpu.py holds to scipy.ndimage.gaussian_filter; the noise comes from the same integer hash in
uint64 and Box-Muller in `dtype`.  Also the cases the GPU tests run (shapes, parameter rows, inputs) and their tolerance E."""
import functools

import numpy as np

SLOTS = 8
MASK64 = (1 << 64) - 1
MUTATIONS = ("drop_tap", "nearest", "ddof1", "no_clip", "invert_once", "blur_first")

# The fp32 gate (tests/test_intensity_cpu.py::test_fp32_gate measures it on the cases below): the worst |float32 referee - float64
# referee| / (channel max - min) is MEASURED_FP32; the GPU tolerance is E = 4 x that (headroom for a different summation order).
MEASURED_FP32 = 4.3e-7
E = 4.0 * MEASURED_FP32


# ---- blur -------------------------------------------------------------------------------------------------------------------

def reflect(i, n):
    """scipy's "reflect" (d c b a | a b c d | d c b a), period 2 n, for any integer array i."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def weights(sigma):
    """-> (radius, float64 weights of -radius..radius), as scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5))."""
    r = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (float(sigma) * float(sigma)))
    return r, w / w.sum()


def blur(x, sigma, dtype=np.float64, mutate=None):
    """gaussian_filter(x, sigma, mode="reflect", truncate=4.0) of a 3-D array, axis by axis, tap by tap in `dtype`."""
    r, w = weights(sigma)
    if mutate == "drop_tap" and r > 0:
        w = w.copy()
        w[0] = w[-1] = 0.0
    w = w.astype(dtype)
    out = x.astype(dtype)
    for axis in range(3):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for j, k in enumerate(range(-r, r + 1)):
            i = np.arange(n) + k
            i = np.clip(i, 0, n - 1) if mutate == "nearest" else reflect(i, n)
            acc = acc + w[j] * np.take(out, i, axis=axis)
        out = acc
    return out


# ---- noise ------------------------------------------------------------------------------------------------------------------

def mix64(z):
    z = (np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def words(seed, c, n):
    """h(i) = mix64(mix64(seed ^ mix64(c)) + i) for i < n, uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(int(seed) & MASK64) ^ mix64(np.uint64(c)))
        return mix64(key + np.arange(n, dtype=np.uint64))


def uniforms(h, dtype=np.float64):
    k1, k2 = (h >> np.uint64(40)).astype(np.int64), (h & np.uint64(0xFFFFFF)).astype(np.int64)
    s = dtype(1.0 / 16777216.0)
    return (k1.astype(dtype) + dtype(0.5)) * s, (k2.astype(dtype) + dtype(0.5)) * s


def normal(h, dtype=np.float64):
    """sqrt(-2 ln u1) cos(2 pi u2); ln u1 through the exact complement above k = 2^23 (csrc/intensity_coords.h log_uniform_hi;
    in float64 both branches are the same number)."""
    k1 = (h >> np.uint64(40)).astype(np.int64)
    u1, u2 = uniforms(h, dtype)
    comp = ((16777215 - k1).astype(dtype) + dtype(0.5)) * dtype(1.0 / 16777216.0)
    ln = np.where(k1 < (1 << 23), np.log(np.where(k1 < (1 << 23), u1, dtype(0.5))), np.log1p(-np.where(k1 < (1 << 23), dtype(0.5), comp)))
    return np.sqrt(dtype(-2.0) * ln) * np.cos(dtype(np.float32(6.2831855) if dtype is np.float32 else 2.0 * np.pi) * u2)


# ---- the chain --------------------------------------------------------------------------------------------------------------

def channel(x, row, seed, c, dtype=np.float64, mutate=None):
    """One (sample, channel): x [D, H, W], row = the 8 parameters -> (output in `dtype`, the 8 float64 statistics)."""
    sigma, noise_std, brightness, contrast, gamma, mode, retain = (float(v) for v in row[:7])
    x = x.astype(dtype)
    stats = np.zeros(SLOTS)
    if mutate == "blur_first" and sigma > 0:
        x = blur(x, sigma, dtype)
    if noise_std > 0:
        x = x + dtype(noise_std) * normal(words(seed, c, x.size), dtype).reshape(x.shape)
    if sigma > 0 and mutate != "blur_first":
        x = blur(x, sigma, dtype, mutate)
    stats[:3] = x.mean(dtype=np.float64), x.min(), x.max()
    x = x * dtype(brightness) if brightness != 1 else x
    if contrast != 1:
        mn, lo, hi = x.mean(dtype=dtype), x.min(), x.max()
        x = (x - mn) * dtype(contrast) + mn
        if mutate != "no_clip":
            x = np.clip(x, lo, hi)
    if mode in (1, 2):
        ddof = 1 if mutate == "ddof1" else 0        # of s0 alone: in both standard deviations the factor would cancel
        if mode == 2:
            x = -x
        if retain:
            m0, s0 = x.mean(dtype=dtype), x.std(dtype=dtype, ddof=ddof)
            stats[3:5] = x.mean(dtype=np.float64), x.std(dtype=np.float64, ddof=ddof)
        lo = x.min()
        rng = x.max() - lo
        x = np.power((x - lo) / (rng + dtype(1e-7)), dtype(gamma)) * rng + lo
        if retain:
            stats[5:7] = x.mean(dtype=np.float64), x.std(dtype=np.float64)
            x = (x - x.mean(dtype=dtype)) / (x.std(dtype=dtype) + dtype(1e-8)) * s0 + m0
        if mode == 2 and mutate != "invert_once":
            x = -x
    assert x.dtype == dtype
    return x, stats


def augment(image, params, seeds, dtype=np.float64, mutate=None):
    """image [B, C, D, H, W], params [B, C, 8], seeds [B] -> (output [B, C, D, H, W] in `dtype`, stats float64 [B, C, 8])."""
    out = np.empty(image.shape, dtype)
    stats = np.zeros(image.shape[:2] + (SLOTS,))
    for b in range(image.shape[0]):
        for c in range(image.shape[1]):
            out[b, c], stats[b, c] = channel(image[b, c], params[b, c], seeds[b], c, dtype, mutate)
    return out, stats


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------

SHAPES = ((5, 9, 70), (33, 34, 35), (64, 64, 64))
KINDS = ("zscore", "minmax")
B, C = 3, 2
#          sigma noise bright contrast gamma mode retain 0
ROWS = {
    "steps": [(0.0, 0.08, 1.0, 1.0, 1.0, 0, 0, 0),       # noise alone
              (0.1, 0.0, 1.0, 1.0, 1.0, 0, 0, 0),        # blur alone, the smallest sigma (radius 0)
              (2.0, 0.0, 1.0, 1.0, 1.0, 0, 0, 0),        # blur alone, the largest (radius 8)
              (0.0, 0.0, 1.2, 1.0, 1.0, 0, 0, 0),        # brightness alone
              (0.0, 0.0, 1.0, 0.8, 1.0, 0, 0, 0),        # contrast below 1
              (0.0, 0.0, 1.0, 1.2, 1.0, 0, 0, 0)],       # contrast above 1: the clip acts
    "gamma": [(0.0, 0.0, 1.0, 1.0, 0.7, 1, 1, 0),        # plain, retain_stats
              (0.0, 0.0, 1.0, 1.0, 1.5, 2, 1, 0),        # inverted, retain_stats
              (0.0, 0.0, 1.0, 1.0, 1.5, 1, 0, 0),        # plain, no retain_stats
              (0.0, 0.0, 1.0, 1.0, 0.7, 2, 0, 0),        # inverted, no retain_stats
              (0.8, 0.05, 0.9, 1.15, 1.3, 2, 1, 0),      # every step together
              (0.0, 0.0, 1.0, 1.0, 1.0, 0, 0, 0)],       # every step off
}
SEEDS = np.array([0x1234_5678_9ABC_DEF0, -7, 3], np.int64)


def rows(name):
    return np.array(ROWS[name], np.float32).reshape(B, C, SLOTS)


def volume(shape, kind, seed=0):
    """[B, C, D, H, W] float32: z-score-like (normal, a smooth offset) or min-max-like (in [0, 1]) data inside an ellipsoid, an
    exact zero background outside, as the loader's normalisations leave it."""
    g = np.random.default_rng(9100 + seed + 17 * KINDS.index(kind) + sum(shape))
    x = g.standard_normal((B, C) + tuple(shape)) if kind == "zscore" else g.random((B, C) + tuple(shape))
    grid = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")
    if kind == "zscore":
        x = x + 0.5 * grid[2]
    x = x * (sum(a * a for a in grid) <= 1.6)
    return x.astype(np.float32)


def cases():
    return [(shape, kind, name) for shape in SHAPES for kind in KINDS for name in ROWS]


@functools.lru_cache(maxsize=None)
def reference(shape, kind, name, half=False):
    """-> (input float32 (rounded to float16 first with `half`), params, seeds, referee output float64, stats).  Computed once;
    do not modify."""
    x = volume(shape, kind)
    if half:
        x = x.astype(np.float16).astype(np.float32)
    out, stats = augment(x, rows(name), SEEDS)
    for a in (x, out, stats):
        a.setflags(write=False)
    return x, rows(name), SEEDS, out, stats


def span(out):
    """channel max - min of a referee output [B, C, D, H, W] -> [B, C, 1, 1, 1]"""
    return (out.max(axis=(2, 3, 4)) - out.min(axis=(2, 3, 4)))[:, :, None, None, None]
