"""CPU referee of the loader's affine resample (micformer_amd/affine.py, csrc/volume_affine.hip): a float64 restatement of the
semantics of include/micformer_affine.h, F.affine_grid + F.grid_sample(align_corners=False).  For output voxel (z, y, x) of (D, H, W)

    n = ((2x+1)/W - 1, (2y+1)/H - 1, (2z+1)/D - 1),   s = theta . (n, 1),   i = ((s + 1) * extent - 1) / 2   per axis of the array

image: trilinear over the 8 taps around i, each tap normalised (in float32, as the kernel does) before it is weighted; "zeros": a tap
outside the array counts 0; "border": i is clamped to [0, extent - 1] first.  label: round-half-even of i, the raw label 0 outside
the array ("zeros") or the index clamped ("border"), then the loader's value lookup.  A non-finite s gives 0 / class 0.
tests/test_affine_cpu.py holds this file to torch's own operators.

Bounds of the GPU tests (the issue's, restated): EPS = 2^-20, eps_axis = extent * EPS voxels for a coordinate; an image element may be
off by u16(ref) + S * (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap| with S the spread (max - min) of its 8 taps and u16 the
float16 spacing at |ref|; a label voxel is compared where its float64 index is further than eps_axis from every k + 0.5."""
import functools

import numpy as np

import loader_ref as R
import normalise_ref as N

EPS = 2.0 ** -20
CT_SHAPE, MR_SHAPE, SIZE, BATCH = (37, 45, 29), (41, 33, 47), (24, 20, 28), 9
VALUES = np.array((0,) + R.MMWHS_LABEL_VALUES + (421, -3), np.int32)
MAX_EXCLUDED = 2e-3
IDENTITY = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
# np.flip(mr, 0).transpose(1, 0, 2) as a map: the re-oriented array R[a, b, c] = mr[d - 1 - b, a, c], so sx = nx, sy = nz, sz = -ny
MR_REORIENT = np.float32([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0]])


def source_coords(theta, size):
    """theta [3, 4] -> normalised source coordinates (sx, sy, sz), float64 [D, H, W] each."""
    D, H, W = size
    th = np.asarray(theta, np.float32).astype(np.float64)
    nz = ((2.0 * np.arange(D) + 1.0) / D - 1.0)[:, None, None]
    ny = ((2.0 * np.arange(H) + 1.0) / H - 1.0)[None, :, None]
    nx = ((2.0 * np.arange(W) + 1.0) / W - 1.0)[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(np.broadcast_to(th[r, 0] * nx + th[r, 1] * ny + th[r, 2] * nz + th[r, 3], (D, H, W)) for r in range(3))


def indices(theta, size, shape):
    """-> (float64 [3, D, H, W] source index on the z, y, x axes of an array of `shape`, bool [D, H, W] all three finite);
    a non-finite index is reported as 0."""
    sx, sy, sz = source_coords(theta, size)
    ok = np.isfinite(sx) & np.isfinite(sy) & np.isfinite(sz)
    with np.errstate(invalid="ignore", over="ignore"):
        i = np.stack([((s + 1.0) * e - 1.0) / 2.0 for s, e in zip((sz, sy, sx), shape)])
    i[:, ~ok] = 0.0
    return i, ok


def sample_image(norm, theta, size, padding_mode):
    """norm: the normalised float32 array.  -> dict(value float64, spread S, tapmax max|tap| (both counting 0 for a tap outside),
    outside bool (some tap outside the array), index float64 [3, D, H, W])."""
    norm64 = np.asarray(norm, np.float64)
    shape = norm64.shape
    i, ok = indices(theta, size, shape)
    ax = []
    for a in range(3):
        c = np.clip(i[a], 0.0, shape[a] - 1.0) if padding_mode == "border" else np.clip(i[a], -1.0, float(shape[a]))
        k0 = np.floor(c).astype(np.int64)
        w1 = c - k0
        ax.append(((k0, 1.0 - w1), (k0 + 1, w1)))
    value = np.zeros(size)
    lo, hi = np.full(size, np.inf), np.full(size, -np.inf)
    tapmax = np.zeros(size)
    outside = np.zeros(size, bool)
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
    value[~ok] = 0.0
    spread = hi - lo
    spread[~ok] = 0.0
    tapmax[~ok] = 0.0
    return dict(value=value, spread=spread, tapmax=tapmax, outside=outside, index=i)


def image_bound(ref, shape):
    """The issue's element bound for one plane: u16(ref) + S * (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap|."""
    with np.errstate(invalid="ignore", over="ignore"):
        u16 = np.spacing(np.abs(ref["value"]).astype(np.float16)).astype(np.float64)
    return u16 + ref["spread"] * (EPS * sum(shape)) + 8.0 * 2.0 ** -23 * ref["tapmax"]


def error_term(ref, shape):
    """The part of the bound that is the resample's own (no float16 spacing): what decides whether `value != 0` is ambiguous."""
    return ref["spread"] * (EPS * sum(shape)) + 8.0 * 2.0 ** -23 * ref["tapmax"]


def sample_label(label, theta, size, padding_mode, label_values=R.MMWHS_LABEL_VALUES):
    """-> dict(cls uint8 [D, H, W], sure bool: every axis further than extent * EPS from a rounding boundary k + 0.5)."""
    label = np.asarray(label)
    shape = label.shape
    i, ok = indices(theta, size, shape)
    inside = ok.copy()
    sure = np.ones(size, bool)
    k = []
    for a in range(3):
        r = np.rint(i[a])                                             # round half to even
        frac = np.abs(i[a] - np.floor(i[a]) - 0.5)                    # distance to the nearest k + 0.5
        sure &= frac > shape[a] * EPS
        if padding_mode == "border":
            r = np.clip(r, 0, shape[a] - 1)
        else:
            inside &= (r >= 0) & (r <= shape[a] - 1)
        k.append(np.clip(r, 0, shape[a] - 1).astype(np.int64))
    val = np.where(inside, label[k[0], k[1], k[2]], 0)
    cls = np.where(val == 0, 0, 255).astype(np.uint8)
    for j, v in enumerate(label_values):
        cls[val == v] = j + 1
    sure |= ~ok                                                       # a non-finite coordinate is class 0 without a doubt
    return dict(cls=cls, sure=sure)


def crop_indexes(values):
    """The loader's rule on the (2, D, H, W) resampled values: extents of the voxels where either channel != 0."""
    with np.errstate(invalid="ignore"):
        idx = np.nonzero((values[0] != 0) | (values[1] != 0))
    if idx[0].size == 0:
        return np.zeros((3, 2), np.int32)
    return np.array([[max(0, int(a.min()) - 1), int(a.max()) + 1] for a in idx], np.int32)


def load_pair(ct, mr, lab, theta, size, padding_mode, normalisation="minmax", percentiles=(1, 99), stats=None):
    """theta [3, 4] or [2, 3, 4].  stats: float64 [2, 2] to feed the normalisers (default: the referee's own).
    -> dict(planes [ref of CT, ref of MR] from sample_image, label from sample_label | None, crop int32 [3, 2])."""
    theta = np.asarray(theta, np.float32)
    tc, tm = (theta, theta) if theta.ndim == 2 else (theta[0], theta[1])
    modes = (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)
    planes = []
    for c, (vol, mode, th) in enumerate(((ct, modes[0], tc), (mr, modes[1], tm))):
        st = None if stats is None or mode == "minmax" else stats[c]
        planes.append(sample_image(N.normalise(vol, mode, percentiles, st), th, size, padding_mode))
    label = None if lab is None else sample_label(lab, tc, size, padding_mode)
    return dict(planes=planes, label=label, crop=crop_indexes(np.stack([p["value"] for p in planes])))


# ---- the shared case of the tests: nine samples at the smallest shapes that exercise everything, a different map each -----------
def rotation(a_d, a_h, a_w):
    cd, sd, ch, sh, cw, sw = np.cos(a_d), np.sin(a_d), np.cos(a_h), np.sin(a_h), np.cos(a_w), np.sin(a_w)
    r_d = np.array([[cd, -sd, 0], [sd, cd, 0], [0, 0, 1.0]])
    r_h = np.array([[ch, 0, sh], [0, 1.0, 0], [-sh, 0, ch]])
    r_w = np.array([[1.0, 0, 0], [0, cw, -sw], [0, sw, cw]])
    return r_d @ r_h @ r_w


def draw_maps(g, count):
    """Rotations up to 0.4 rad, factors 0.8 ... 1.25, shifts +-0.15 normalised -> float32 [count, 3, 4]."""
    out = np.zeros((count, 3, 4), np.float32)
    for b in range(count):
        out[b, :, :3] = rotation(*g.uniform(-0.4, 0.4, 3)) @ np.diag(g.uniform(0.8, 1.25, 3))
        out[b, :, 3] = g.uniform(-0.15, 0.15, 3)
    return out


def raw_sample(g):
    ct = g.integers(-400, 2000, size=CT_SHAPE, dtype=np.int16)
    ct[g.random(CT_SHAPE) < 0.05] = 0
    mr = g.random(MR_SHAPE, dtype=np.float32) * np.float32(1500.0) - np.float32(200.0)
    mr[g.random(MR_SHAPE) < 0.05] = 0
    lab = VALUES[g.integers(0, len(VALUES), size=CT_SHAPE)].astype(np.int16)
    return ct, mr, lab


SEED = 7122            # chosen on the CPU: no voxel whose `!= 0` is in doubt, label exclusions under the cap (test_affine_cpu.py asserts both)


@functools.lru_cache(maxsize=None)
def case(seed=SEED):
    """-> (samples: BATCH triples of numpy arrays, maps float32 [BATCH, 3, 4]); cached, never written to."""
    g = np.random.default_rng(seed)
    samples = tuple(raw_sample(g) for _ in range(BATCH))
    maps = draw_maps(g, BATCH)
    for s in samples:
        for a in s:
            a.setflags(write=False)
    maps.setflags(write=False)
    return samples, maps


@functools.lru_cache(maxsize=None)
def case_reference(padding_mode, seed=SEED):
    """The min-max referee of every sample of case(seed): a tuple of load_pair results; cached, shared by the tests."""
    samples, maps = case(seed)
    return tuple(load_pair(*s, maps[b], SIZE, padding_mode) for b, s in enumerate(samples))
