"""CPU referee of the patch sampler's crop through a map (micformer_amd/patch_warp.py, csrc/volume_patch_warp.hip): a float64
restatement of include/micformer_patch_warp.h.  The origin o and `picked` are patches_ref.locate's, unchanged.  For patch voxel
(z, y, x) of (Pd, Ph, Pw) on a scan of extent L per axis

    n = ((2x+1)/Pw - 1, (2y+1)/Ph - 1, (2z+1)/Pd - 1),   u = the field on the PATCH grid (elastic_ref.displacement; 0 without one),
    s = theta . (n + u, 1),   i = o + ((s + 1) P - 1) / 2   per axis

and from i on affine_ref.sample_image's form (elastic_ref.sample_image: trilinear over the 8 taps, each normalised in float32 first;
"zeros": a tap outside the scan counts 0; "border": i clamped to [0, L - 1]) and sample_label's with the patch sampler's own outside
rule: round half to even, pad_class wherever the rounded index lies outside the scan, in BOTH padding modes.  A non-finite s gives
image 0 and pad_class.  tests/test_patch_warp_cpu.py holds this file to F.grid_sample.

Bounds of the GPU tests (the header's): EPS = 2^-20, eps_axis = P EPS + (L + P) 2^-24 for a map, 2 P EPS + (L + P) 2^-24 with a field
(|u| <= 0.25, row sums <= 1.5); an image element may be off by u16(ref) + S (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap|; a label
voxel is compared where its float64 index is further than eps_axis from every k + 0.5.  `exact=True` (maps whose arithmetic is
exact in float32: the identity and translations by multiples of half a voxel on power-of-two patches) compares every label voxel.

`mutate` switches ONE deliberate mistake on, for the tests that show the comparison catches it:
  "o+half"       o + 1/2 instead of o                      "theta_T"      the map's 3 x 3 block transposed
  "zyx"          the coordinate fed to the map as (z, y, x) "half_up"      round half up instead of half to even
  "class0"       class 0 instead of pad_class outside       "field_after"  the field added after the map
"""
import functools

import numpy as np

import affine_ref as A
import elastic_ref as E
import loader_ref as R
import normalise_ref as N
import patches_ref as P

EPS = 2.0 ** -20
MAX_EXCLUDED = A.MAX_EXCLUDED
MR_REORIENT = A.MR_REORIENT


def eps_axes(patch_size, shape, field):
    """-> the coordinate bound per axis (z, y, x), in voxels."""
    return tuple((2.0 if field else 1.0) * p * EPS + (l + p) * 2.0 ** -24 for p, l in zip(patch_size, shape))


def indices(theta, u, patch_size, origin, mutate=None):
    """theta [3, 4] | None; u float64 [3, Pd, Ph, Pw] in (x, y, z) order | None -> (float64 [3, Pd, Ph, Pw] scan index on the z, y, x
    axes, bool all three coordinates finite); a non-finite index is reported as 0."""
    Pd, Ph, Pw = patch_size
    th = (A.IDENTITY if theta is None else np.asarray(theta, np.float32)).astype(np.float64)
    if mutate == "theta_T":
        th = th.copy()
        th[:, :3] = th[:, :3].T
    u = np.zeros((3,) + tuple(patch_size)) if u is None else u
    nz = np.broadcast_to(((2.0 * np.arange(Pd) + 1.0) / Pd - 1.0)[:, None, None], patch_size)
    ny = np.broadcast_to(((2.0 * np.arange(Ph) + 1.0) / Ph - 1.0)[None, :, None], patch_size)
    nx = np.broadcast_to(((2.0 * np.arange(Pw) + 1.0) / Pw - 1.0)[None, None, :], patch_size)
    if mutate == "zyx":
        nx, nz = nz, nx
    with np.errstate(invalid="ignore", over="ignore"):
        if mutate == "field_after":
            sx, sy, sz = (th[r, 0] * nx + th[r, 1] * ny + th[r, 2] * nz + th[r, 3] + u[r] for r in range(3))
        else:
            px, py, pz = nx + u[0], ny + u[1], nz + u[2]
            sx, sy, sz = (th[r, 0] * px + th[r, 1] * py + th[r, 2] * pz + th[r, 3] for r in range(3))
        ok = np.isfinite(sx) & np.isfinite(sy) & np.isfinite(sz)
        shift = 0.5 if mutate == "o+half" else 0.0
        i = np.stack([o + shift + ((s + 1.0) * p - 1.0) / 2.0 for o, s, p in zip(origin, (sz, sy, sx), patch_size)])
    i[:, ~ok] = 0.0
    return i, ok


def sample_label(cmap, i, ok, pad_class, eps, mutate=None):
    """cmap: the scan's class map.  eps: per-axis bounds, or None (every voxel is compared).
    -> dict(cls uint8, sure bool)."""
    shape = cmap.shape
    inside, sure, k = ok.copy(), np.ones(ok.shape, bool), []
    for a in range(3):
        r = np.floor(i[a] + 0.5) if mutate == "half_up" else np.rint(i[a])
        if eps is not None:
            sure &= np.abs(i[a] - np.floor(i[a]) - 0.5) > eps[a]
        inside &= (r >= 0) & (r <= shape[a] - 1)
        k.append(np.clip(r, 0, shape[a] - 1).astype(np.int64))
    cls = np.where(inside, cmap[k[0], k[1], k[2]], 0 if mutate == "class0" else pad_class).astype(np.uint8)
    return dict(cls=cls, sure=sure | ~ok)


def image_bound(ref, eps):
    """u16(ref) + S * (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap|: affine_ref.image_bound's form with this file's eps."""
    with np.errstate(invalid="ignore", over="ignore"):
        u16 = np.spacing(np.abs(ref["value"]).astype(np.float16)).astype(np.float64)
    return u16 + ref["spread"] * sum(eps) + 8.0 * 2.0 ** -23 * ref["tapmax"]


def sample(ct, mr, label, draw, patch_size, theta=None, field=None, mode="linear", padding_mode="zeros", pad_class=0, clamp="both",
           normalisation="minmax", percentiles=(1, 99), stats=None, normalised=None, cmap=None, exact=False, mutate=None):
    """numpy arrays of one shape; theta None, [3, 4] or [2, 3, 4]; field None or float32 [3, gd, gh, gw].  stats: float64 [2, 2] to
    feed the normalisers (default: the referee's own).
    -> dict(planes [ref of CT, ref of MR] (elastic_ref.sample_image's), label dict(cls, sure) | None, origin, picked, eps)."""
    modes = (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)
    if cmap is None and label is not None:
        cmap = P.full_class_map(label)
    origin, picked = P.locate(cmap, ct.shape, draw, patch_size, clamp)
    if normalised is None:
        normalised = tuple(N.normalise(v, m, percentiles, None if stats is None or m == "minmax" else stats[c])
                           for c, (v, m) in enumerate(zip((ct, mr), modes)))
    u = None if field is None else E.displacement(field, patch_size, mode)
    theta = None if theta is None else np.asarray(theta, np.float32)
    tc, tm = (theta, theta) if theta is None or theta.ndim == 2 else (theta[0], theta[1])
    eps = eps_axes(patch_size, ct.shape, field is not None)
    ic, okc = indices(tc, u, patch_size, origin, mutate)
    im, okm = indices(tm, u, patch_size, origin, mutate)
    planes = [E.sample_image(normalised[0], ic, okc, padding_mode), E.sample_image(normalised[1], im, okm, padding_mode)]
    lab = None if cmap is None else sample_label(cmap, ic, okc, pad_class, None if exact else eps, mutate)
    return dict(planes=planes, label=lab, origin=np.array(origin, np.int32), picked=np.array(picked, np.int32), eps=eps)


def compare(got, want):
    """got: dict(image float16 [2, ...], label uint8 | None, origin, picked) of one sample; want: sample()'s.
    -> (the names of what differs, dict(worst image error / bound, failing image elements, excluded share of the label))."""
    bad, info = [], dict(worst=0.0, failing=0, excluded=0.0)
    for name in ("origin", "picked"):
        if not np.array_equal(np.asarray(got[name]), want[name]):
            bad.append(name)
    for c, ref in enumerate(want["planes"]):
        g = np.asarray(got["image"][c]).astype(np.float64)
        err, bound = np.abs(g - ref["value"]), image_bound(ref, want["eps"])
        ok = err <= bound                                             # (False for a NaN on either side)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        info["worst"] = max(info["worst"], float(np.nanmax(ratio)) if np.isfinite(ratio).any() else 0.0)
        info["failing"] += int((~ok).sum())
        if not ok.all() and "image" not in bad:
            bad.append("image")
    if (got["label"] is None) != (want["label"] is None):
        bad.append("label")
    elif want["label"] is not None:
        sure, cls = want["label"]["sure"], want["label"]["cls"]
        info["excluded"] = 1.0 - float(sure.mean())
        if (sure & (np.asarray(got["label"]) != cls)).any():
            bad.append("label")
    return bad, info


def as_got(ref):
    """A referee result in the form the kernel returns: what a faultless implementation would hand to compare()."""
    return dict(image=np.stack([p["value"] for p in ref["planes"]]).astype(np.float16),
                label=None if ref["label"] is None else ref["label"]["cls"], origin=ref["origin"], picked=ref["picked"])


# ---- the shared cases of the tests ------------------------------------------------------------------------------------------------
SCAN_SHAPE, BATCH = (37, 45, 29), 9
PATCHES = ((24, 20, 28), (9, 11, 13))              # x runs of 4; one voxel per thread
POW2_PATCHES = ((8, 16, 16), (16, 16, 32))         # x runs of 8; the arithmetic of the identity is exact
POW2_SCANS = ((20, 30, 40), (5, 30, 40))           # the second is shorter than either patch in d: negative origins
VALUES = np.array((0, 0) + R.MMWHS_LABEL_VALUES + (421, -3), np.int32)
FIELD_AMPLITUDE = 0.12                             # |u| <= 0.25 with room for the cubic's sum of weights (1)
SEED = 9511


def image(g, shape, dtype):
    if dtype == np.int16:
        v = g.integers(-400, 2000, size=shape, dtype=np.int16)
    else:
        v = g.random(shape, dtype=np.float32) * np.float32(1500.0) - np.float32(200.0)
    v[g.random(shape) < 0.05] = 0
    return v


def generic_maps(g, count, patch_size, rotate=0.26, scale=0.15, shift=3.0):
    """Rotations up to `rotate` rad about each axis, factors 1 +- scale, shifts of +- `shift` patch voxels, conjugated into normalised
    patch coordinates as affine.draw_affine does (so the rotation is rigid on the patch grid) -> float32 [count, 3, 4]."""
    Pd, Ph, Pw = patch_size
    n = np.array([Pw, Ph, Pd], np.float64) / 2.0
    out = np.zeros((count, 3, 4), np.float32)
    for b in range(count):
        a = A.rotation(*g.uniform(-rotate, rotate, 3)) @ np.diag(1.0 + g.uniform(-scale, scale, 3))
        out[b, :, :3] = a * n[None, :] / n[:, None]
        out[b, :, 3] = g.uniform(-shift, shift, 3) / n
    return out


def compose(theta, fixed):
    """theta [3, 4] applied after the fixed map [3, 4] (affine.draw_affine's per_modality rule): s = theta . (fixed . (n, 1), 1)."""
    t, f = np.asarray(theta, np.float64), np.asarray(fixed, np.float64)
    out = np.zeros((3, 4))
    out[:, :3] = t[:, :3] @ f[:, :3]
    out[:, 3] = t[:, :3] @ f[:, 3] + t[:, 3]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def nine(seed=SEED):
    """-> (samples: BATCH (ct, mr, label) triples on SCAN_SHAPE -- CT int16 with MR float32 and the reverse, label int16 and int32 --,
    draws float32 [BATCH, 6] with the forced tail of draw_patches and one more); cached, never written to."""
    g = np.random.default_rng(seed)
    samples = []
    for b in range(BATCH):
        ct = image(g, SCAN_SHAPE, np.int16 if b % 2 == 0 else np.float32)
        mr = image(g, SCAN_SHAPE, np.float32 if b % 2 == 0 else np.int16)
        lab = VALUES[g.integers(0, len(VALUES), size=SCAN_SHAPE)].astype(np.int16 if b % 3 else np.int32)
        samples.append((ct, mr, lab))
    draws = np.concatenate([P.forced_column(BATCH, 1 / 3)[:, None], g.random((BATCH, 5), dtype=np.float32)], axis=1)
    draws[4, 0] = 1.0
    for s in samples:
        for a in s:
            a.setflags(write=False)
    draws.setflags(write=False)
    return tuple(samples), draws


@functools.lru_cache(maxsize=None)
def nine_maps(patch_size, seed=SEED):
    maps = generic_maps(np.random.default_rng(seed + 1 + sum(patch_size)), BATCH, patch_size)
    maps.setflags(write=False)
    return maps


@functools.lru_cache(maxsize=None)
def nine_fields(grid, seed=SEED):
    """float32 [BATCH, 3, gd, gh, gw], uniform in +-FIELD_AMPLITUDE."""
    g = np.random.default_rng(seed + 100 + sum(grid))
    f = g.uniform(-FIELD_AMPLITUDE, FIELD_AMPLITUDE, (BATCH, 3) + tuple(grid)).astype(np.float32)
    f.setflags(write=False)
    return f


# name -> (patch, which samples of nine(), maps: "one" | "two" (MR_REORIENT composed for MR) | None, field grid | None | "dense",
#          field interpolation): every warped case the GPU tests hold to the referee
CASES = {
    "maps-4": (PATCHES[0], tuple(range(9)), "one", None, "linear"),
    "maps-1": (PATCHES[1], tuple(range(9)), "one", None, "linear"),
    "per-modality": (PATCHES[0], (0, 1, 2), "two", None, "linear"),
    "cubic": (PATCHES[0], tuple(range(9)), "one", (5, 5, 5), "cubic"),
    "linear": (PATCHES[1], (0, 1, 2), "one", (5, 5, 5), "linear"),
    "cubic-no-map": (POW2_PATCHES[0], (3, 4), None, (5, 5, 5), "cubic"),
    "dense": (PATCHES[1], (5, 6), "one", "dense", "linear"),
    "dense-no-map": (POW2_PATCHES[1], (7, 8), None, "dense", "linear"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (patch, samples, draws [n, 6], theta [n, 3, 4] | [n, 2, 3, 4] | None, fields [n, 3, gd, gh, gw] | None, interpolation)."""
    patch, which, layout, grid, mode = CASES[name]
    samples, draws = nine()
    which = list(which)
    theta = None
    if layout is not None:
        theta = nine_maps(patch)[which]
        if layout == "two":
            theta = np.stack([np.stack([t, compose(t, MR_REORIENT)]) for t in theta])
        theta.setflags(write=False)
    fields = None
    if grid is not None:
        fields = nine_fields(patch if grid == "dense" else grid)[which]
    return patch, tuple(samples[b] for b in which), draws[which], theta, fields, mode


@functools.lru_cache(maxsize=None)
def case_reference(name, padding_mode, pad_class=255):
    """The min-max referee of every sample of case(name): a tuple of sample() results; cached, shared by the tests."""
    patch, samples, draws, theta, fields, mode = case(name)
    return tuple(sample(*s, draws[b], patch, theta=None if theta is None else theta[b], field=None if fields is None else fields[b],
                        mode=mode, padding_mode=padding_mode, pad_class=pad_class) for b, s in enumerate(samples))


@functools.lru_cache(maxsize=None)
def extremes():
    """Six samples on PATCHES[1] (odd extents: the centre voxel's n is exactly 0), every one with a map and a linear (5, 5, 5) field:
    0 and 5 ordinary; 1 a NaN map entry (s_x is NaN everywhere); 2 a +inf offset (s_y is +inf everywhere); 3 a 1e30 entry on s_z and
    a zero field (finite and far outside everywhere but on the centre plane, where n_z = 0); 4 a NaN control point inside the grid.
    -> (patch, samples, draws, theta float32 [6, 3, 4], fields float32 [6, 3, 5, 5, 5])."""
    patch = PATCHES[1]
    samples, draws = nine()
    theta = nine_maps(patch)[:6].copy()
    fields = nine_fields((5, 5, 5))[:6].copy()
    theta[1, 0, 0] = np.nan
    theta[2, 1, 3] = np.inf
    theta[3, 2, 2] = 1e30
    fields[3] = 0.0
    fields[4, 1, 2, 2, 2] = np.nan
    theta.setflags(write=False)
    fields.setflags(write=False)
    return patch, samples[:6], draws[:6], theta, fields


@functools.lru_cache(maxsize=None)
def extremes_reference(padding_mode, pad_class=255):
    patch, samples, draws, theta, fields = extremes()
    return tuple(sample(*s, draws[b], patch, theta=theta[b], field=fields[b], mode="linear", padding_mode=padding_mode,
                        pad_class=pad_class) for b, s in enumerate(samples))
