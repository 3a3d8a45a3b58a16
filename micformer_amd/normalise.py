"""The volume loader's choice of intensity normalisation per channel: the binding of include/micformer_normalise.h (kernels:
csrc/volume_normalise.hip) and the checks of the three keywords that loader.load_batch / load_pair and restore.segment_pair take.

    image, label_map, crop = loader.load_pair(ct, mr, lab, normalisation=("minmax", "percentile"), percentiles=(1, 99))
    image, label_map, crop, stats = loader.load_pair(ct, mr, lab, normalisation="zscore", return_stats=True)   # stats float64 [2, 2]

  * "minmax"      (x - min) / (max - min) over the whole volume: image_utils.normalize, what the loader has always done.
  * "zscore"      x != 0 ? (x - mean) / std : 0 with mean and population std over the voxels != 0: image_utils.zscore_normalise.
  * "percentile"  (clip(x, low, high) - low) / (high - low) with low, high = np.percentile(x[x > 0], percentiles):
                  image_utils.irm_min_max_preprocess.
One name applies to both channels, a (ct, mr) pair gives each its own.  `stats` holds per channel (min, max), (mean, std) or
(low, high) in float64.  Edge rules: z-score of an all-zero volume is all zeros, of a constant non-zero value NaN at the non-zero
voxels; percentile with high == low or with no positive voxel is NaN everywhere.  One deliberate deviation: the reference's
zscore_normalise writes its result back into the input array, which truncates it to integers for an int16 array; here an int16
volume is z-scored as if converted to float32 first.  The entry points are bound from this module's table (SIGNATURES below),
which is apart from every other header's.  Rules: DESIGN.md "Volume loader".
"""
from . import _lib

MINMAX, ZSCORE, PERCENTILE = 0, 1, 2          # MICF_NORM_*
MODES = {"minmax": MINMAX, "zscore": ZSCORE, "percentile": PERCENTILE}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_volume_loader_norm_workspace": "i",
    "micf_volume_loader_norm": "piiiipiiiddplppppp",
}
INT64_RETURNS = frozenset(("micf_volume_loader_norm_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="volume normalisation")


def modes(normalisation):
    """One name or a (ct, mr) pair of names -> (ct mode, mr mode); touches no device."""
    rule = f"normalisation must be one of {sorted(MODES)} or a (ct, mr) pair of them"
    if isinstance(normalisation, str):
        names = (normalisation, normalisation)
    elif isinstance(normalisation, (tuple, list)):
        if len(normalisation) != 2:
            raise ValueError(f"{rule}, got {len(normalisation)} entries")
        names = tuple(normalisation)
    else:
        raise TypeError(f"{rule}, got {type(normalisation).__name__}")
    for name in names:
        if not isinstance(name, str):
            raise TypeError(f"{rule}, got {type(name).__name__}")
        if name not in MODES:
            raise ValueError(f"{rule}, got {name!r}")
    return MODES[names[0]], MODES[names[1]]


def percentile_pair(percentiles):
    """(low, high) with 0 <= low < high <= 100 -> two floats; touches no device."""
    rule = "percentiles must be (low, high) with 0 <= low < high <= 100"
    if isinstance(percentiles, str) or not hasattr(percentiles, "__len__"):
        raise TypeError(f"{rule}, got {percentiles!r}")
    if len(percentiles) != 2:
        raise ValueError(f"{rule}, got {len(percentiles)} entries")
    try:
        low, high = (float(p) for p in percentiles)
    except (TypeError, ValueError):
        raise TypeError(f"{rule}, got {percentiles!r}") from None
    if not 0.0 <= low < high <= 100.0:
        raise ValueError(f"{rule}, got {tuple(percentiles)!r}")
    return low, high


__all__ = ["MODES", "SIGNATURES", "modes", "percentile_pair"]
