"""Referee of the low-resolution simulation (include/micformer_lowres.h): numpy, float64 by default; `dtype=np.float32` runs the
same formulas in float32 (the fp32 gate of tests/test_lowres_cpu.py).  Written out the way the definition reads: the integer
nearest gather, the cubic B-spline prefilter of the edge-extended signal in the kernels' own start scheme (closed-form sums of the
constant extension at both ends, the coefficients of the extension kept two entries out) and explicit taps with the four B-spline
weights.  test_lowres_cpu.py holds it to scipy.ndimage.zoom.  Also the cases the GPU tests run and their tolerance E."""
import functools

import numpy as np

POLE = np.sqrt(3.0) - 2.0
EXT = 2                                           # coefficients kept beyond either end of an axis
MUTATIONS = ("ties_down", "floor_gather", "align_corners", "no_prefilter", "keys", "trilinear", "reflect", "prefilter_two_axes")

# The fp32 gate (tests/test_lowres_cpu.py::test_fp32_gate measures it on the cases below): the worst |float32 referee - float64
# referee| / (channel max - min of the input) is MEASURED_FP32; the GPU tolerance is E = 4 x that.
MEASURED_FP32 = 6.0e-7
E = 4.0 * MEASURED_FP32


# ---- indices and weights ------------------------------------------------------------------------------------------------------

def clamp_target(t, n):
    return min(max(int(t), 1), int(n))


def gather_index(n, t, mutate=None):
    """The source index of every low-resolution position o < t of an axis of extent n."""
    o = np.arange(t, dtype=np.int64)
    if mutate == "ties_down":
        g = ((2 * o + 1) * n - 1) // (2 * t)
    elif mutate == "floor_gather":
        g = (o * n) // t
    else:
        g = ((2 * o + 1) * n) // (2 * t)
    return np.minimum(g, n - 1)


def is_tie(n, t):
    return ((2 * np.arange(t, dtype=np.int64) + 1) * n) % (2 * t) == 0


def taps(n, t, dtype=np.float64, mutate=None):
    """-> (floor(s) [n], fraction [n] in `dtype`) of s = (o + 1/2) t / n - 1/2 for every output o < n; the fraction is the exact
    remainder over 2 n, rounded once."""
    o = np.arange(n, dtype=np.int64)
    if mutate == "align_corners":
        s = o.astype(np.float64) * ((t - 1) / (n - 1) if n > 1 else 0.0)
        fl = np.floor(s).astype(np.int64)
        return fl, (s - fl).astype(dtype)
    num, den = (2 * o + 1) * t - n, 2 * n
    fl = num // den                                       # (numpy's // floors)
    return fl, ((num - fl * den).astype(dtype) / dtype(den)).astype(dtype)


def bspline_weights(f):
    g = 1 - f
    six = f.dtype.type(6)
    return [g * g * g / six, (4 - 6 * f * f + 3 * f * f * f) / six, (4 - 6 * g * g + 3 * g * g * g) / six, f * f * f / six]


def keys_weights(f):
    a = f.dtype.type(-0.5)

    def k(x):
        x = np.abs(x)
        return np.where(x <= 1, (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1, a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a)
    return [k(f + 1), k(f), k(1 - f), k(2 - f)]


def linear_weights(f):
    return [np.zeros_like(f), 1 - f, f, np.zeros_like(f)]


# ---- the prefilter ------------------------------------------------------------------------------------------------------------

def prefilter(a, axis, dtype=np.float64):
    """The cubic B-spline coefficients of `a` along `axis`, `a` extended by its edge values to infinity; returned with EXT
    coefficients of the extension on either side (length t + 2 EXT along `axis`):
      causal      p[0] = 6 / (1 - z) s[0] (the sum over the constant extension), p[k] = 6 s[k] + z p[k - 1]
      anticausal  c[t - 1] = s[t - 1] - z / (1 - z^2) (p[t - 1] - 6 / (1 - z) s[t - 1]), c[k] = z (c[k + 1] - p[k])
      extension   c[-j] = s[0] + (c[0] - s[0]) z^j, c[t - 1 + j] = s[t - 1] + (c[t - 1] - s[t - 1]) z^j"""
    s = np.moveaxis(a.astype(dtype), axis, 0)
    t = s.shape[0]
    z = dtype(POLE)
    first, last = dtype(6.0 / (1.0 - POLE)), dtype(-POLE / (1.0 - POLE * POLE))
    p = np.empty_like(s)
    p[0] = first * s[0]
    for k in range(1, t):
        p[k] = dtype(6) * s[k] + z * p[k - 1]
    c = np.empty((t + 2 * EXT,) + s.shape[1:], dtype)
    c[EXT + t - 1] = s[t - 1] + last * (p[t - 1] - first * s[t - 1])
    for k in range(t - 2, -1, -1):
        c[EXT + k] = z * (c[EXT + k + 1] - p[k])
    for j in range(1, EXT + 1):
        zj = dtype(POLE ** j)
        c[EXT - j] = s[0] + (c[EXT] - s[0]) * zj
        c[EXT + t - 1 + j] = s[t - 1] + (c[EXT + t - 1] - s[t - 1]) * zj
    assert c.dtype == dtype
    return np.moveaxis(c, 0, axis)


def edge_extend(a, axis, dtype=np.float64):
    """`a` with EXT copies of its edge values on either side of `axis`: what stands in the prefilter's place in a mutation."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (EXT, EXT)
    return np.pad(a.astype(dtype), pad, mode="edge")


def prefilter_reflect(a, axis, dtype=np.float64):
    """The prefilter of `a` extended by reflection (d c b a | a b c d | d c b a) instead of by its edge values."""
    far = 32                                              # z^30 = 7e-18
    pad = [(0, 0)] * a.ndim
    pad[axis] = (far, far)
    c = prefilter(np.pad(a.astype(dtype), pad, mode="symmetric"), axis, dtype)
    return np.take(c, np.arange(far, far + a.shape[axis] + 2 * EXT), axis=axis)


# ---- one channel --------------------------------------------------------------------------------------------------------------

def downsample(x, target, mutate=None):
    n = x.shape
    t = [clamp_target(target[a], n[a]) for a in range(3)]
    low = x
    for a in range(3):
        low = np.take(low, gather_index(n[a], t[a], mutate), axis=a)
    return low


def upsample(low, n, dtype=np.float64, mutate=None):
    """`low` [td, th, tw] -> [n] by cubic B-spline interpolation: prefilter along W, H, D, then four taps along D, H, W (the kernels' order)."""
    c = low.astype(dtype)
    for a in (2, 1, 0):
        if mutate in ("no_prefilter", "keys", "trilinear") or (mutate == "prefilter_two_axes" and a == 0):
            c = edge_extend(c, a, dtype)
        elif mutate == "reflect":
            c = prefilter_reflect(c, a, dtype)
        else:
            c = prefilter(c, a, dtype)
    weights = {"keys": keys_weights, "trilinear": linear_weights}.get(mutate, bspline_weights)
    for a in (0, 1, 2):
        fl, f = taps(n[a], low.shape[a], dtype, mutate)
        w = weights(f)
        shape = [1, 1, 1]
        shape[a] = n[a]
        acc = None
        for j in range(4):
            term = w[j].astype(dtype).reshape(shape) * np.take(c, fl - 1 + j + EXT, axis=a)
            acc = term if acc is None else acc + term
        c = acc
    assert c.dtype == dtype and c.shape == tuple(n)
    return c


def channel(x, target, dtype=np.float64, mutate=None):
    """One (sample, channel): x [D, H, W], target (td, th, tw) -> the output in `dtype`; the input itself where the step is off."""
    n = x.shape
    if all(clamp_target(target[a], n[a]) == n[a] for a in range(3)):
        return x.astype(dtype)
    return upsample(downsample(x, target, mutate), n, dtype, mutate)


def simulate(image, target, dtype=np.float64, mutate=None):
    """image [B, C, D, H, W], target [B, C, 3] -> output [B, C, D, H, W] in `dtype`."""
    out = np.empty(image.shape, dtype)
    for b in range(image.shape[0]):
        for c in range(image.shape[1]):
            out[b, c] = channel(image[b, c], target[b, c], dtype, mutate)
    return out


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------

SHAPES = ((5, 9, 70), (33, 34, 35), (64, 64, 64))
KINDS = ("zscore", "minmax")
B, C = 3, 2
# per shape, two sets of B x C targets (d, h, w): exact halves (every position a tie), t = 1 on an axis, t = n on one or two axes
# (ignore_axes), t = n - 1, odd ratios such as 35 -> 23, one channel off
TARGETS = {
    (5, 9, 70): {
        "a": [(1, 9, 35), (3, 5, 70), (5, 9, 69), (2, 1, 47), (5, 9, 70), (4, 8, 1)],
        "b": [(5, 4, 35), (3, 9, 53), (5, 9, 70), (1, 1, 1), (4, 9, 70), (2, 6, 64)],
    },
    (33, 34, 35): {
        "a": [(33, 17, 23), (16, 17, 17), (32, 33, 34), (33, 34, 35), (1, 34, 35), (21, 19, 23)],
        "b": [(17, 34, 18), (33, 34, 23), (33, 34, 35), (25, 1, 30), (19, 23, 1), (32, 34, 35)],
    },
    (64, 64, 64): {
        "a": [(32, 32, 32), (64, 64, 32), (63, 63, 63), (47, 33, 55), (64, 64, 64), (1, 40, 64)],
        "b": [(48, 48, 48), (64, 37, 64), (64, 64, 64), (32, 64, 1), (35, 23, 41), (33, 63, 32)],
    },
}
NAMES = ("a", "b")


def targets(shape, name):
    return np.array(TARGETS[tuple(shape)][name], np.int32).reshape(B, C, 3)


def volume(shape, kind, seed=0):
    """[B, C, D, H, W] float32: z-score-like (normal, a smooth offset) or min-max-like (in [0, 1]) data inside an ellipsoid, an
    exact zero background outside, as the loader's normalisations leave it (the inputs of intensity_ref.volume)."""
    g = np.random.default_rng(9300 + seed + 17 * KINDS.index(kind) + sum(shape))
    x = g.standard_normal((B, C) + tuple(shape)) if kind == "zscore" else g.random((B, C) + tuple(shape))
    grid = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing="ij")
    if kind == "zscore":
        x = x + 0.5 * grid[2]
    x = x * (sum(a * a for a in grid) <= 1.6)
    return x.astype(np.float32)


def cases():
    return [(shape, kind, name) for shape in SHAPES for kind in KINDS for name in NAMES]


@functools.lru_cache(maxsize=None)
def reference(shape, kind, name, half=False):
    """-> (input float32 (rounded to float16 first with `half`), targets, referee output float64).  Computed once; do not modify."""
    x = volume(shape, kind)
    if half:
        x = x.astype(np.float16).astype(np.float32)
    t = targets(shape, name)
    out = simulate(x, t)
    for a in (x, t, out):
        a.setflags(write=False)
    return x, t, out


def is_off(shape, target):
    """[B, C] bool: the channels whose clamped target equals the shape."""
    return np.array([[all(clamp_target(target[b, c, a], shape[a]) == shape[a] for a in range(3)) for c in range(target.shape[1])]
                     for b in range(target.shape[0])])


def span(x):
    """channel max - min of an input [B, C, D, H, W] -> [B, C, 1, 1, 1]"""
    return (x.max(axis=(2, 3, 4)) - x.min(axis=(2, 3, 4)))[:, :, None, None, None]
