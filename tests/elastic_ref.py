"""CPU referee of the loader's elastic resample (micformer_amd/elastic.py, csrc/volume_elastic.hip): a float64 restatement of the
semantics of include/micformer_elastic.h.  For output voxel (z, y, x) of (D, H, W)

    n = ((2x+1)/W - 1, (2y+1)/H - 1, (2z+1)/D - 1),   u = the field at control position p = o (g - 1) / (out - 1) per axis,
    s = theta . (n + u, 1),   i = ((s + 1) * extent - 1) / 2   per axis of the array

and from i on the rules of tests/affine_ref.py (image: trilinear over the 8 taps, each normalised first; label: round-half-even and
the value lookup; "zeros" / "border"; a non-finite s gives 0 / class 0).  The field: float32 [3, gd, gh, gw], components (x, y, z),
normalised output units, corner control points on the centres of the first and last voxel.  "linear": the 2 taps k, k + 1 per axis
with weights (1 - t, t); "cubic": the 4 taps k - 1 ... k + 2 (clamped to the grid) with the uniform cubic B-spline's weights.  A
non-finite control value reaches every voxel whose taps include it, whatever its weight (0 * NaN = NaN in the kernel's sum).
tests/test_elastic_cpu.py holds this file to F.interpolate, scipy.ndimage.map_coordinates and F.grid_sample.

Bounds of the GPU tests: the affine tests' with EPS = 2^-19 (the affine arithmetic's extent * 2^-20, plus the rounding of n + u and
the roundings of u, a value <= 0.25, through a map with row sums <= 1.5)."""
import functools

import numpy as np

import affine_ref as A
import loader_ref as R
import normalise_ref as N

EPS = 2.0 ** -19
SIZE, BATCH = A.SIZE, A.BATCH
MODES = ("linear", "cubic")
AMPLITUDE = 0.12
MAX_EXCLUDED = 2e-3
# name -> (samples of affine_ref.case(), control grid, maps: "one" [n, 3, 4] | "two" [n, 2, 3, 4] | None)
CASES = {"nine": (tuple(range(9)), (5, 4, 6), "one"),          # a second chunk of 8
         "dense": ((0, 1), SIZE, "two"),                       # one vector per output voxel, a map per modality
         "minimal": ((2, 3), (2, 2, 2), None)}                 # the smallest grid, no map


def axis_taps(out, g, mode):
    """-> (address int64 [out, T] in [0, g), weight float64 [out, T]) of the T = 2 | 4 taps of every output voxel of one axis."""
    o = np.arange(out, dtype=np.int64)
    if out > 1:
        k, t = (o * (g - 1)) // (out - 1), ((o * (g - 1)) % (out - 1)) / float(out - 1)
    else:
        k, t = np.zeros(1, np.int64), np.zeros(1)
    if mode == "linear":
        first, w = k, [1.0 - t, t]
    elif mode == "cubic":
        first = k - 1
        w = [(1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0, (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0,
             t ** 3 / 6.0]
    else:
        raise ValueError(mode)
    address = np.stack([np.clip(first + j, 0, g - 1) for j in range(len(w))], 1)
    return address, np.stack(w, 1)


def _axis_matrices(out, g, mode):
    """The taps of an axis as dense [out, g] matrices: the weights (summed where two taps clamp onto one point) and membership."""
    address, weight = axis_taps(out, g, mode)
    m, member = np.zeros((out, g)), np.zeros((out, g))
    rows = np.repeat(np.arange(out), address.shape[1])
    np.add.at(m, (rows, address.ravel()), weight.ravel())
    member[rows, address.ravel()] = 1.0
    return m, member


def displacement(field, size, mode, optimize=False):
    """field float32 [3, gd, gh, gw] -> u float64 [3, D, H, W] in (x, y, z) order; NaN where a tap is non-finite.  optimize: let
    einsum contract axis by axis (another summation order in the last bits; what a 128^3 output needs to finish in seconds)."""
    f = np.asarray(field, np.float32).astype(np.float64)
    mats = [_axis_matrices(o, g, mode) for o, g in zip(size, f.shape[1:])]
    bad = ~np.isfinite(f)
    u = np.einsum("zd,yh,xw,cdhw->czyx", mats[0][0], mats[1][0], mats[2][0], np.where(bad, 0.0, f), optimize=optimize)
    if bad.any():
        tainted = np.einsum("zd,yh,xw,cdhw->czyx", mats[0][1], mats[1][1], mats[2][1], bad.astype(np.float64)) > 0
        u[tainted] = np.nan
    return u


def indices(theta, u, size, shape):
    """theta [3, 4] | None, u [3, D, H, W] -> (float64 [3, D, H, W] source index on the z, y, x axes of an array of `shape`,
    bool [D, H, W] all three finite); a non-finite index is reported as 0."""
    D, H, W = size
    th = (A.IDENTITY if theta is None else np.asarray(theta, np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nz = ((2.0 * np.arange(D) + 1.0) / D - 1.0)[:, None, None] + u[2]
        ny = ((2.0 * np.arange(H) + 1.0) / H - 1.0)[None, :, None] + u[1]
        nx = ((2.0 * np.arange(W) + 1.0) / W - 1.0)[None, None, :] + u[0]
        sx, sy, sz = (th[r, 0] * nx + th[r, 1] * ny + th[r, 2] * nz + th[r, 3] for r in range(3))
        ok = np.isfinite(sx) & np.isfinite(sy) & np.isfinite(sz)
        i = np.stack([((s + 1.0) * e - 1.0) / 2.0 for s, e in zip((sz, sy, sx), shape)])
    i[:, ~ok] = 0.0
    return i, ok


def sample_image(norm, i, ok, padding_mode):
    """affine_ref.sample_image from the index on.  norm: the normalised float32 array; (i, ok) from indices().
    -> dict(value, spread, tapmax, outside, index)."""
    norm64 = np.asarray(norm, np.float64)
    shape, size = norm64.shape, i.shape[1:]
    ax = []
    for a in range(3):
        c = np.clip(i[a], 0.0, shape[a] - 1.0) if padding_mode == "border" else np.clip(i[a], -1.0, float(shape[a]))
        k0 = np.floor(c).astype(np.int64)
        w1 = c - k0
        ax.append(((k0, 1.0 - w1), (k0 + 1, w1)))
    value, tapmax, outside = np.zeros(size), np.zeros(size), np.zeros(size, bool)
    lo, hi = np.full(size, np.inf), np.full(size, -np.inf)
    for kz, wz in ax[0]:
        for ky, wy in ax[1]:
            for kx, wx in ax[2]:
                if padding_mode == "border":                          # (k0 + 1 == extent only with weight 0)
                    inside = np.ones(size, bool)
                else:
                    inside = (kz >= 0) & (kz < shape[0]) & (ky >= 0) & (ky < shape[1]) & (kx >= 0) & (kx < shape[2])
                t = np.where(inside, norm64[np.clip(kz, 0, shape[0] - 1), np.clip(ky, 0, shape[1] - 1), np.clip(kx, 0, shape[2] - 1)],
                             0.0)
                with np.errstate(invalid="ignore"):
                    value += t * (wz * wy * wx)
                    lo, hi, tapmax = np.minimum(lo, t), np.maximum(hi, t), np.maximum(tapmax, np.abs(t))
                outside |= ~inside
    spread = hi - lo
    for arr in (value, spread, tapmax):
        arr[~ok] = 0.0
    return dict(value=value, spread=spread, tapmax=tapmax, outside=outside & ok, index=i)


def error_term(ref, shape):
    """The part of the bound that is the resample's own (no float16 spacing): what decides whether `value != 0` is ambiguous."""
    return ref["spread"] * (EPS * sum(shape)) + 8.0 * 2.0 ** -23 * ref["tapmax"]


def image_bound(ref, shape):
    """The element bound for one plane: u16(ref) + S * (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap|."""
    with np.errstate(invalid="ignore", over="ignore"):
        u16 = np.spacing(np.abs(ref["value"]).astype(np.float16)).astype(np.float64)
    return u16 + error_term(ref, shape)


def sample_label(label, i, ok, padding_mode, label_values=R.MMWHS_LABEL_VALUES):
    """affine_ref.sample_label from the index on -> dict(cls uint8 [D, H, W], sure bool: every axis further than extent * EPS from
    a rounding boundary k + 0.5)."""
    label = np.asarray(label)
    shape = label.shape
    inside, sure, k = ok.copy(), np.ones(ok.shape, bool), []
    for a in range(3):
        r = np.rint(i[a])                                             # round half to even
        sure &= np.abs(i[a] - np.floor(i[a]) - 0.5) > shape[a] * EPS
        if padding_mode == "border":
            r = np.clip(r, 0, shape[a] - 1)
        else:
            inside &= (r >= 0) & (r <= shape[a] - 1)
        k.append(np.clip(r, 0, shape[a] - 1).astype(np.int64))
    val = np.where(inside, label[k[0], k[1], k[2]], 0)
    cls = np.where(val == 0, 0, 255).astype(np.uint8)
    for j, v in enumerate(label_values):
        cls[val == v] = j + 1
    return dict(cls=cls, sure=sure | ~ok)                             # a non-finite coordinate is class 0 without a doubt


def load_pair(ct, mr, lab, field, mode, theta, size, padding_mode, normalisation="minmax", percentiles=(1, 99), stats=None):
    """field [3, gd, gh, gw]; theta None, [3, 4] or [2, 3, 4].  stats: float64 [2, 2] to feed the normalisers (default: the
    referee's own).  -> dict(planes [ref of CT, ref of MR], label | None, crop int32 [3, 2], u)."""
    u = displacement(field, size, mode)
    theta = None if theta is None else np.asarray(theta, np.float32)
    tc, tm = (theta, theta) if theta is None or theta.ndim == 2 else (theta[0], theta[1])
    modes = (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)
    planes = []
    for c, (vol, nmode, th) in enumerate(((ct, modes[0], tc), (mr, modes[1], tm))):
        st = None if stats is None or nmode == "minmax" else stats[c]
        planes.append(sample_image(N.normalise(vol, nmode, percentiles, st), *indices(th, u, size, np.shape(vol)), padding_mode))
    label = None if lab is None else sample_label(lab, *indices(tc, u, size, np.shape(lab)), padding_mode)
    return dict(planes=planes, label=label, crop=A.crop_indexes(np.stack([p["value"] for p in planes])), u=u)


# ---- the shared cases of the tests ------------------------------------------------------------------------------------------------
# The seed of every sample's field, chosen on the CPU so that the referee alone meets the conditions test_elastic_cpu.py asserts of
# it.  One seed per sample and not per case: under "zeros" a sample has a voxel whose `!= 0` is in doubt (a tap just inside the array's
# face with a weight below the coordinate bound) in about three draws of four, so nine samples in two interpolation modes have none
# in about one draw of 10^5, while each sample alone is found in a few tries.
SEEDS = {"nine": (8311, 8312, 8317, 8332, 8337, 8342, 8347, 8349, 8363), "dense": (8316, 8320), "minimal": (8303, 8308)}


@functools.lru_cache(maxsize=None)
def case(name, seeds=None):
    """-> (samples: triples of numpy arrays, maps float32 [n, 3, 4] | [n, 2, 3, 4] | None, fields float32 [n, 3, gd, gh, gw]);
    cached, never written to."""
    which, grid, layout = CASES[name]
    samples, maps = A.case()
    fields = np.stack([np.random.default_rng(seed).uniform(-AMPLITUDE, AMPLITUDE, (3,) + tuple(grid)).astype(np.float32)
                       for seed in (SEEDS[name] if seeds is None else seeds)])
    fields.setflags(write=False)
    if layout == "one":
        theta = np.stack([maps[b] for b in which])
    elif layout == "two":
        theta = np.stack([np.stack([maps[b], maps[BATCH - 1 - b]]) for b in which])
    else:
        theta = None
    if theta is not None:
        theta.setflags(write=False)
    return tuple(samples[b] for b in which), theta, fields


@functools.lru_cache(maxsize=None)
def case_reference(name, mode, padding_mode, seeds=None):
    """The min-max referee of every sample of case(name): a tuple of load_pair results; cached, shared by the tests."""
    samples, theta, fields = case(name, seeds)
    return tuple(load_pair(*s, fields[b], mode, None if theta is None else theta[b], SIZE, padding_mode) for b, s in enumerate(samples))
