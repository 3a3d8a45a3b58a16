"""CPU referee of the patch sampler (micformer_amd/patches.py, csrc/volume_patches.hip), written from the rule stated in
include/micformer_patches.h -- nnU-Net's DataLoader3D.generate_train_batch restated; parity with nnU-Net itself is unpinned
(batchgenerators is not a dependency).  Picks go through np.flatnonzero(class_map == c)[r], the image is a crop / np.pad of
normalise_ref.normalise(vol, mode), the label a crop / pad of the looked-up class map.

`mutate` switches ONE deliberate mistake on, for the tests that show the comparison catches it:
  "rank+1"       the pick at rank r + 1 (cyclic)          "lb_floor"     lb = -floor(need / 2)
  "pad_side"     the padding put on the wrong side        "label_edge"   the label replicated outside the scan in "border" mode
  "no_upper"     the upper clamp dropped under clamp="both"
"""
import numpy as np

import loader_ref as R
import normalise_ref as N

SEGMENT = 2048
RANDOM_PICK = (0, -1, -1, -1)


def full_class_map(label, label_values=R.MMWHS_LABEL_VALUES):
    """raw label volume -> uint8 class map on the scan's own grid: 0 for 0, k for label_values[k - 1], 255 elsewhere."""
    label = np.asarray(label)
    out = np.full(label.shape, 255, np.uint8)
    out[label == 0] = 0
    for k, v in enumerate(label_values):
        out[label == v] = k + 1
    return out


def class_counts(label, label_values=R.MMWHS_LABEL_VALUES):
    """-> int64 [K + 2]: np.bincount of the class map, "other" (255) moved to slot K + 1."""
    counts = np.bincount(full_class_map(label, label_values).ravel(), minlength=256)
    k = len(label_values)
    return np.concatenate([counts[:k + 1], counts[255:]])


def bounds(L, P, mutate=None):
    need = max(P - L, 0)
    lb = -(need // 2) if mutate == "lb_floor" else -((need + 1) // 2)
    ub = L + need // 2 + need % 2 - P
    return lb, ub


def draw_index(u, n):
    """min(int64(double(u) * double(n)), n - 1); 0 for u < 0 or NaN, n - 1 for u >= 1."""
    u = np.float32(u)
    if not u >= 0:
        return 0
    if u >= 1:
        return n - 1
    return min(int(np.float64(u) * np.float64(n)), n - 1)


def locate(cmap, shape, draw, patch_size, clamp="both", mutate=None):
    """cmap: the scan's class map or None; draw: six floats.  -> (origin [3], picked [4]) as Python ints."""
    force, u_class, u_voxel = draw[0], draw[1], draw[2]
    if cmap is not None and np.float32(force) >= 0.5:
        counts = np.bincount(cmap.ravel(), minlength=256)[:255]
        present = [c for c in range(1, 255) if counts[c]]
        if present:
            c = present[draw_index(u_class, len(present))]
            where = np.flatnonzero(cmap.ravel() == c)
            r = draw_index(u_voxel, len(where))
            if mutate == "rank+1":
                r = (r + 1) % len(where)
            v = np.unravel_index(where[r], shape)
            origin = []
            for ax in range(3):
                lb, ub = bounds(shape[ax], patch_size[ax], mutate)
                o = max(int(v[ax]) - patch_size[ax] // 2, lb)
                if clamp == "both" and mutate != "no_upper":
                    o = min(o, ub)
                origin.append(o)
            return origin, [c] + [int(i) for i in v]
    origin = []
    for ax in range(3):
        lb, ub = bounds(shape[ax], patch_size[ax], mutate)
        origin.append(lb + draw_index(draw[3 + ax], ub - lb + 1))
    return origin, list(RANDOM_PICK)


def crop(vol, origin, patch_size, mode, value=0, mutate=None):
    """The window [origin, origin + patch_size) of vol: a slice of what lies inside, np.pad for the rest ("constant" with `value`,
    or "edge")."""
    sl, pads = [], []
    for o, P, L in zip(origin, patch_size, vol.shape):
        lo, hi = max(o, 0), min(o + P, L)
        assert lo < hi, "the window misses the scan"
        sl.append(slice(lo, hi))
        pads.append((o + P - hi, lo - o) if mutate == "pad_side" else (lo - o, o + P - hi))
    inner = vol[tuple(sl)]
    return np.pad(inner, pads, mode="edge") if mode == "edge" else np.pad(inner, pads, mode="constant", constant_values=value)


def sample(ct, mr, label, draw, patch_size, label_values=R.MMWHS_LABEL_VALUES, normalisation="minmax", percentiles=(1, 99),
           padding_mode="zeros", pad_class=0, clamp="both", mutate=None, normalised=None, cmap=None):
    """numpy arrays of one shape -> dict(image float32 [2, Pd, Ph, Pw] BEFORE the float16 rounding, label uint8 | None, origin,
    picked).  normalised: the (ct, mr) float32 volumes, cmap: the scan's class map, where the caller has them already."""
    modes = (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)
    if cmap is None and label is not None:
        cmap = full_class_map(label, label_values)
    origin, picked = locate(cmap, ct.shape, draw, patch_size, clamp, mutate)
    if normalised is None:
        normalised = (N.normalise(ct, modes[0], percentiles), N.normalise(mr, modes[1], percentiles))
    how = "edge" if padding_mode == "border" else "constant"
    image = np.stack([crop(v, origin, patch_size, how, 0, mutate) for v in normalised])
    lab = None
    if cmap is not None:
        lab = crop(cmap, origin, patch_size, "edge" if (mutate == "label_edge" and padding_mode == "border") else "constant",
                   pad_class, mutate)
    return dict(image=image, label=lab, origin=np.array(origin, np.int32), picked=np.array(picked, np.int32))


def forced_column(B, p):
    """draw_patches' column 0: nnU-Net's `not j < round(B * (1 - p))`."""
    return np.array([0.0 if j < round(B * (1 - p)) else 1.0 for j in range(B)], np.float32)


def compare(got, want):
    """got: dict(image float16, label, origin, picked) of one sample; want: sample()'s.  -> the names of what differs: origin,
    picked and label exactly, the image by normalise_ref.close (0 failing elements, share <= MAX_SHARE)."""
    bad = []
    for name in ("origin", "picked"):
        if not np.array_equal(np.asarray(got[name]), want[name]):
            bad.append(name)
    if (got["label"] is None) != (want["label"] is None) or (want["label"] is not None and not np.array_equal(got["label"], want["label"])):
        bad.append("label")
    fails, share, _ = N.close(got["image"], want["image"])
    if fails or share > N.MAX_SHARE:
        bad.append("image")
    return bad


def steer(r, n):
    """The u_voxel (or u_class) that selects index r of n: (r + 0.5) / n, checked."""
    u = np.float32((r + 0.5) / n)
    assert draw_index(u, n) == r, (r, n)
    return float(u)
