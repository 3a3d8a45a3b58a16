"""CPU referee of the loader's z-score and percentile-clip normalisations (micformer_amd/normalise.py, csrc/volume_normalise.hip):
the reference's zscore_normalise and irm_min_max_preprocess (dataset/image_utils.py) restated on numpy.  The statistics are taken in
float64 (x[x != 0].mean() / .std(), np.percentile(x[x > 0], ...)), rounded to float32 once, and the element map runs in float32;
resize, class map and crop_indexes are loader_ref's.

Edge rules: z-score of an all-zero volume is all zeros; of a constant non-zero value NaN at the non-zero voxels and 0 at the zeros;
percentile with high == low, or with no positive voxel (the reference raises there), is NaN everywhere.  Deviation from the
reference: zscore_normalise writes into its input array, which truncates the result for an int16 array; here every volume is
z-scored as float32.

Closeness of an image to this referee (close()): the fp16-step measure of the loader tests alone is wrong for z-scores, whose values
near 0 have fp16 steps far below a float32 rounding of the largest value; an element therefore passes within ONE fp16 step OR
within A = 2^-20 * max(1, max |referee|), and at most MAX_SHARE of the elements may differ and be more than A away."""
import numpy as np

import loader_ref as R

MODES = ("minmax", "zscore", "percentile")
MAX_SHARE = 1e-3


def stats(vol, mode, percentiles=(1, 99)):
    """-> the normaliser's two float64 statistics: (min, max), (mean, std) or (low, high); NaN where there is no voxel to take
    them from."""
    vol = np.asarray(vol)
    x = vol.astype(np.float64)
    if mode == "minmax":
        return np.array([x.min(), x.max()])
    if mode == "zscore":
        sel = x[x != 0]
        return np.array([sel.mean(), sel.std()]) if sel.size else np.array([np.nan, np.nan])
    if mode == "percentile":
        sel = x[x > 0]
        return np.percentile(sel, list(percentiles)) if sel.size else np.array([np.nan, np.nan])
    raise ValueError(mode)


def normalise(vol, mode, percentiles=(1, 99), st=None):
    """-> float32 array.  st: stats(vol, mode, percentiles) where the caller has them already."""
    if mode == "minmax":
        return R.normalize(vol)
    a, b = (np.float32(s) for s in (stats(vol, mode, percentiles) if st is None else st))
    x = np.asarray(vol).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "zscore":
            out = np.zeros_like(x)
            nz = x != 0
            out[nz] = (x[nz] - a) / b
            return out
        if np.isnan(a):
            return np.full_like(x, np.nan)
        return (np.minimum(np.maximum(x, a), b) - a) / (b - a)


def _pair(normalisation):
    return (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)


def load_pair(ct, mr, ct_label=None, size=(128, 128, 128), label_values=R.MMWHS_LABEL_VALUES, normalisation="minmax",
              percentiles=(1, 99)):
    """numpy arrays -> (image float32 [2, D, H, W] BEFORE the float16 rounding, class map uint8 [D, H, W] | None, crop_indexes
    int32 [3, 2], stats float64 [2, 2])."""
    m = _pair(normalisation)
    st = np.stack([stats(ct, m[0], percentiles), stats(mr, m[1], percentiles)])
    image = np.stack([R.resize_image(normalise(ct, m[0], percentiles, st[0]), size),
                      R.resize_image(normalise(mr, m[1], percentiles, st[1]), size)])
    lab = None if ct_label is None else R.class_map(ct_label, size, label_values)
    return image, lab, R.crop_indexes(image), st


def close(got16, want32):
    """got16: float16 array; want32: the referee's float32 array of the same shape.  -> (number of failing elements, share of
    elements that differ and are more than A away, A).  An element fails when it is more than one fp16 step AND more than A away
    (NaN against NaN passes, NaN against a number fails)."""
    got16 = np.asarray(got16, np.float16)
    want32 = np.asarray(want32, np.float32)
    want16 = want32.astype(np.float16)
    finite = np.isfinite(want32)
    A = 2.0 ** -20 * max(1.0, float(np.abs(want32[finite]).max()) if finite.any() else 1.0)
    steps = R.fp16_steps(got16, want16)
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(got16.astype(np.float64) - want16.astype(np.float64)) <= A)      # (true where either is NaN)
    far &= ~(np.isnan(got16) & np.isnan(want32))
    fails = int(((steps > 1) & far).sum())
    share = float(((steps != 0) & far).mean())
    return fails, share, A


def ulps(a, b):
    """Distance of two float64 values in units in the last place (0 where both are NaN)."""
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) and np.isnan(b):
        return 0
    if np.isnan(a) or np.isnan(b):
        return 1 << 62

    def order(x):
        u = int(np.array(x, np.float64).view(np.int64))
        return u if u >= 0 else -(u & 0x7FFFFFFFFFFFFFFF)
    return abs(order(a) - order(b))
