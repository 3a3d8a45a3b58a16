"""Referee of the connected components (micformer_amd/postprocess.py): scipy.ndimage.label once per class on the host, and the
scenes the tests run on.  Everything is an integer: the device results must EQUAL these, there is no tolerance.

Rules as include/micformer_components.h states them.  scipy numbers the components of a binary mask in the order of their first
voxel (checked against a flood fill in tests/test_components_cpu.py), so a component's root is ndimage.minimum of the linear
index over it, its canonical label root + 1, and "the largest, lowest root on a tie" is argmax of bincount over scipy's labels."""
import numpy as np
from scipy import ndimage

MMWHS_LABEL_VALUES = (205, 420, 500, 550, 600, 820, 850)
_RANK = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return ndimage.generate_binary_structure(3, _RANK[connectivity])


def class_values(K, label_values):
    """The value of class 1..K-1 in the volume."""
    return list(range(1, K)) if label_values is None else [int(v) for v in label_values]


def per_class(vol, K, label_values=None, connectivity=26):
    """Yields (class k, scipy labels of the class's mask, roots [n], sizes [n])."""
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    values = class_values(K, label_values)
    assert len(values) == K - 1
    for k, value in enumerate(values, start=1):
        lab, n = ndimage.label(vol == value, structure(connectivity))
        if n == 0:
            yield k, lab, np.zeros(0, np.int64), np.zeros(0, np.int64)
            continue
        roots = np.asarray(ndimage.minimum(lin, lab, np.arange(1, n + 1))).astype(np.int64).reshape(n)
        sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
        yield k, lab, roots, sizes


def components(vol, K, label_values=None, connectivity=26):
    """-> (labels int32: root + 1, 0 off-component; sizes int32: the voxel's component's size, 0 off-component)."""
    labels = np.zeros(vol.shape, np.int32)
    sizes = np.zeros(vol.shape, np.int32)
    for _, lab, roots, counts in per_class(vol, K, label_values, connectivity):
        on = lab > 0
        labels[on] = (roots[lab[on] - 1] + 1).astype(np.int32)
        sizes[on] = counts[lab[on] - 1].astype(np.int32)
    return labels, sizes


def keep_largest(vol, K, label_values=None, connectivity=26, classes=None):
    out = vol.copy()
    for k, lab, roots, counts in per_class(vol, K, label_values, connectivity):
        if (classes is not None and k not in classes) or len(counts) == 0:
            continue
        assert np.all(np.diff(roots) > 0)                 # scipy's numbering ascends with the first voxel
        out[(lab > 0) & (lab != int(np.argmax(counts)) + 1)] = 0
    return out


def remove_small(vol, min_size, K, label_values=None, connectivity=26, classes=None):
    out = vol.copy()
    for k, lab, roots, counts in per_class(vol, K, label_values, connectivity):
        if (classes is not None and k not in classes) or len(counts) == 0:
            continue
        small = np.concatenate([[False], counts < min_size])
        out[small[lab]] = 0
    return out


def brute_force_components(vol, K, label_values=None, connectivity=26):
    """Flood fill in pure Python, for tiny volumes: the check of the referee itself."""
    d, h, w = vol.shape
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < abs(dz) + abs(dy) + abs(dx) <= _RANK[connectivity]]
    values = set(class_values(K, label_values))
    labels = np.zeros(vol.shape, np.int32)
    sizes = np.zeros(vol.shape, np.int32)
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if labels[z, y, x] or int(vol[z, y, x]) not in values:
                    continue
                root = (z * h + y) * w + x                   # raster order: the first voxel met is the smallest index
                stack, seen = [(z, y, x)], {(z, y, x)}
                while stack:
                    cz, cy, cx = stack.pop()
                    for dz, dy, dx in offs:
                        n = (cz + dz, cy + dy, cx + dx)
                        if 0 <= n[0] < d and 0 <= n[1] < h and 0 <= n[2] < w and n not in seen and vol[n] == vol[z, y, x]:
                            seen.add(n)
                            stack.append(n)
                for v in seen:
                    labels[v] = root + 1
                    sizes[v] = len(seen)
    return labels, sizes


# ---- scenes (class maps, uint8) ----------------------------------------------------------------------------------------------------

def to_values(cmap, label_values, dtype):
    """A class map -> the label volume that holds label_values (dtype int16 / int32)."""
    table = np.array((0,) + tuple(label_values), dtype=dtype)
    return table[cmap]


def binary_noise(shape, density, seed=0):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def class_noise(shape, K=8, seed=0):
    return np.random.default_rng(seed).integers(0, K, size=shape).astype(np.uint8)


def blobs(shape, K=8, seed=0, sigma=2.5):
    """Smooth blobs: gaussian-filtered noise thresholded into K classes of about equal share."""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma, mode="nearest")
    edges = np.quantile(f, np.linspace(0, 1, K + 1)[1:-1])
    return np.digitize(f, edges).astype(np.uint8)


def blobs_with_islands(shape, K=8, seed=0, islands=12, sigma=2.5):
    """The blobs plus planted islands: small boxes of another class dropped at random places."""
    g = np.random.default_rng(seed + 1000)
    vol = blobs(shape, K, seed, sigma)
    for _ in range(islands):
        size = [int(min(g.integers(1, 4), s)) for s in shape]
        at = [int(g.integers(0, s - e + 1)) for s, e in zip(shape, size)]
        vol[at[0]:at[0] + size[0], at[1]:at[1] + size[1], at[2]:at[2] + size[2]] = g.integers(1, K)
    return vol


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def snake(shape):
    """A one-voxel-wide path along every other row of every other plane, linked at alternating ends: ONE component (for every
    connectivity) that crosses every tile face many times."""
    d, h, w = shape
    vol = np.zeros(shape, np.uint8)
    at_end = False                                        # which end of the current row the path arrived at
    rows = [(z, y) for zi, z in enumerate(range(0, d, 2)) for y in (range(0, h, 2) if zi % 2 == 0 else reversed(range(0, h, 2)))]
    for i, (z, y) in enumerate(rows):
        vol[z, y, :] = 1
        if i + 1 < len(rows):
            nz, ny = rows[i + 1]
            x = 0 if at_end else w - 1                    # leave this row at the end opposite to the one it was entered at
            vol[min(z, nz):max(z, nz) + 1, min(y, ny):max(y, ny) + 1, x] = 1
            at_end = not at_end
    return vol
