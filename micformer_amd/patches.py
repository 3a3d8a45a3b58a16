"""On-device patch sampler: native-resolution crops of a registered CT / MR pair and its CT label, a share of every batch centred
on a foreground voxel -- the sampling rule of nnU-Net's DataLoader3D.generate_train_batch (dataset_loading.py:297-412), on the HIP
kernels of csrc/volume_patches.hip.

    from micformer_amd import patches
    samples = [(ct, mr, lab), ...]                       # loader.load_batch's device tensors; the three arrays of a sample share one shape
    idx = patches.index_scans(samples)                   # once per resident scan: statistics, class counts, per-segment class counts
    draws = patches.draw_patches(len(samples), generator=g, device="cuda")                     # float32 [B, 6]
    image, label_map, origins, picked = patches.sample_patches(samples, idx, draws, patch_size=(128, 128, 128))
    draws.copy_(patches.draw_patches(len(samples), generator=g))                               # a graph captured with out= reads the new draws

Parity with nnU-Net is UNPINNED: batchgenerators is not a dependency and nnU-Net's loader is not run by any test here.  The rule
is stated in include/micformer_patches.h and in DESIGN.md "Patch sampler", and a numpy referee written from that statement
(tests/patches_ref.py) is the judge.  Per sample, with L the scan extent on an axis and P the patch extent:
  * bounds: need = max(P - L, 0), lb = -ceil(need / 2), ub = L + need // 2 + need % 2 - P (for odd need lb = ub - 1, as nnU-Net's
    `- need // 2` gives).
  * draws[b] = (force, u_class, u_voxel, u_z, u_y, u_x); an index from u and a count n is min(int64(double(u) * double(n)), n - 1),
    0 for u < 0 or NaN, n - 1 for u >= 1.
  * force >= 0.5, a label and at least one voxel of a class 1..K: the j-th present class (ascending), the r-th voxel of that class
    in flat scan order, exactly; origin = v - P // 2 per axis, clamped to [lb, ub] (clamp="both") or below only (clamp="lower", as
    the bundled nnU-Net v1 code does: the window may run past the far end and is padded there).
  * otherwise -- a forced sample without foreground included, nnU-Net's fallback -- origin = lb + index(u_axis, ub - lb + 1).
  * image: fp16_rn(normalise(x)) inside the scan with the loader's per-element function and whole-volume statistics for each
    `normalisation=` mode, no interpolation; outside 0.0 ("zeros") or the nearest scan voxel ("border", numpy's "edge").
  * label: the loader's class of the raw value inside, `pad_class` outside in both padding modes (nnU-Net's -1 is 255 here).
One deliberate difference: the voxel is drawn uniformly from ALL voxels of the class; nnU-Net draws from at most 10 000 locations
per class that its preprocessing sampled beforehand.

Nothing here synchronises with the host or runs an ATen compute op (allocation only); the launches go to the current stream and
sample_patches can be captured by torch.cuda.graph when `out` is given.  Everything that crosses threads is an integer: outputs
are bit-identical from run to run and independent of the other samples of the batch.  The entry points are declared in
include/micformer_patches.h; _lib.bind binds them from this module's table (SIGNATURES below), which is apart from every other
header's.
"""
import ctypes

import torch

from . import _args, _lib, loader, normalise

MMWHS_LABEL_VALUES = loader.MMWHS_LABEL_VALUES
SEGMENT = 2048                                # MICF_PATCH_SEGMENT: voxels per segment of the index (csrc/patches_coords.h says why)
PADDING_MODES = {"zeros": 0, "border": 1}     # MICF_PATCH_PAD_*
CLAMPS = {"both": 0, "lower": 1}              # MICF_PATCH_CLAMP_*
_COUNTS_OFFSET, _STAT_OFFSET, _CHANNEL_BYTES = 256, 96, 112

# name -> argument signature (as _lib.SIGNATURES); the two queries return int64 (INT64_RETURNS), the others int
SIGNATURES = {
    "micf_patch_index_bytes": "lii",
    "micf_patch_index_workspace": "i",
    "micf_patch_index": "pipiiiddplppp",
    "micf_patch_sample": "pipppipiiiiiippppp",
}
INT64_RETURNS = frozenset(("micf_patch_index_bytes", "micf_patch_index_workspace"))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="patch sampler")


class PatchIndex:
    """The index of one resident scan.  .stats: float64 [2, 2], per channel (min, max), (mean, std) or (low, high) -- what
    loader.load_batch(..., return_stats=True) returns; .class_counts: int32 [K + 2], the voxels of class 0, 1..K and "other" (255).
    Both are views of .buffer (uint8, device)."""

    def __init__(self, buffer, shape, dtypes, label_values, modes, percentiles):
        self.buffer, self.shape, self.dtypes = buffer, shape, dtypes
        self.label_values, self.modes, self.percentiles = label_values, modes, percentiles
        k = len(label_values)
        self.stats = buffer[:2 * _CHANNEL_BYTES].view(torch.float64).view(2, _CHANNEL_BYTES // 8)[:, _STAT_OFFSET // 8:_STAT_OFFSET // 8 + 2]
        self.class_counts = buffer[_COUNTS_OFFSET:_COUNTS_OFFSET + 4 * (k + 2)].view(torch.int32)

    @property
    def has_label(self):
        return self.dtypes[2] is not None


def _describe(samples, what):
    """-> (LoaderSample array, device, has_label, per-sample (shape, dtypes)); load_batch's checks plus the equal shapes."""
    samples = list(samples)
    if not samples:
        raise ValueError(f"{what} needs at least one sample")
    items = (loader.LoaderSample * len(samples))()
    device, has_label, meta = None, None, []
    for b, smp in enumerate(samples):
        if not isinstance(smp, (tuple, list)) or len(smp) != 3:
            raise ValueError(f"sample {b} must be a (ct, mr, ct_label | None) triple")
        ct, mr, lab = smp
        loader._typed(ct, f"sample {b}: ct", loader._IMAGE_DTYPES)
        loader._typed(mr, f"sample {b}: mr", loader._IMAGE_DTYPES)
        if lab is not None:
            loader._typed(lab, f"sample {b}: ct_label", loader._LABEL_DTYPES)
        it = items[b]
        it.ct, shape, it.ct_dtype = loader._volume(ct, f"sample {b}: ct", loader._IMAGE_DTYPES, device)
        it.ct_shape[:] = shape
        device = ct.device
        it.mr, mr_shape, it.mr_dtype = loader._volume(mr, f"sample {b}: mr", loader._IMAGE_DTYPES, device)
        it.mr_shape[:] = mr_shape
        if has_label is None:
            has_label = lab is not None
        elif has_label != (lab is not None):
            raise ValueError("either every sample of a batch has a ct_label or none has")
        lab_shape = shape
        if lab is not None:
            it.label, lab_shape, it.label_dtype = loader._volume(lab, f"sample {b}: ct_label", loader._LABEL_DTYPES, device)
            it.label_shape[:] = lab_shape
        if mr_shape != shape or lab_shape != shape:
            raise ValueError(f"sample {b}: ct, mr and ct_label must have the same shape (a patch of a registered pair has one "
                             f"origin), got {shape}, {mr_shape}" + ("" if lab is None else f", {lab_shape}"))
        meta.append((shape, (ct.dtype, mr.dtype, None if lab is None else lab.dtype)))
    return items, device, has_label, meta


def _index_arrays(indexes):
    ptrs = (ctypes.c_void_p * len(indexes))(*[i.buffer.data_ptr() for i in indexes])
    sizes = (ctypes.c_int64 * len(indexes))(*[i.buffer.numel() for i in indexes])
    return ptrs, sizes


def index_scans(samples, label_values=MMWHS_LABEL_VALUES, normalisation="minmax", percentiles=(1, 99)):
    """samples: sequence of (ct, mr, ct_label | None) as loader.load_batch takes them, the arrays of a sample of one shape.
    -> [PatchIndex per scan].  The statistics are exactly load_batch(..., normalisation=, percentiles=, return_stats=True)'s; the
    counts are exact (LDS histograms and integer atomics)."""
    vals, nvals = loader._label_values(label_values)
    modes = normalise.modes(normalisation)
    p_low, p_high = normalise.percentile_pair(percentiles)
    items, device, has_label, meta = _describe(samples, "index_scans")
    B = len(meta)
    indexes = []
    for shape, dtypes in meta:
        nbytes = _lib.query_bytes("micf_patch_index_bytes", shape[0] * shape[1] * shape[2], nvals, int(has_label))
        indexes.append(PatchIndex(torch.empty(nbytes, dtype=torch.uint8, device=device), shape, dtypes,
                                  tuple(vals[i] for i in range(nvals)), modes, (p_low, p_high)))
    ws_bytes = _lib.query_bytes("micf_patch_index_workspace", B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    ptrs, sizes = _index_arrays(indexes)
    _lib.call_on(device, "micf_patch_index", ctypes.addressof(items), B, ctypes.addressof(vals), nvals, modes[0], modes[1], p_low,
                 p_high, ws.data_ptr(), ws_bytes, ctypes.addressof(ptrs), ctypes.addressof(sizes))
    return indexes


def draw_patches(B, oversample_foreground_percent=1 / 3, generator=None, device=None):
    """-> float32 [B, 6]: (force, u_class, u_voxel, u_z, u_y, u_x) per sample.  force is 1.0 for the batch positions j with
    `not j < round(B * (1 - oversample_foreground_percent))` (nnU-Net's deterministic tail of the batch, Python's round), else 0.0;
    the other columns are uniform in [0, 1).  A caller may fill column 0 by any rule.  Drawn on the generator's device (the CPU
    without one), then moved to `device`."""
    if isinstance(B, bool) or not isinstance(B, int):
        raise TypeError(f"B must be an integer, got {type(B).__name__}")
    if B < 1:
        raise ValueError(f"B must be at least 1, got {B}")
    p = float(oversample_foreground_percent)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"oversample_foreground_percent must lie in [0, 1], got {oversample_foreground_percent!r}")
    where = generator.device if generator is not None else "cpu"
    draws = torch.rand((B, 6), generator=generator, dtype=torch.float32, device=where)
    first_forced = round(B * (1 - p))
    draws[:, 0] = torch.tensor([0.0 if j < first_forced else 1.0 for j in range(B)], dtype=torch.float32, device=where)
    return draws if device is None else draws.to(device)


def _mode(value, table, what):
    if not isinstance(value, str):
        raise TypeError(f"{what} must be one of {sorted(table)}, got {type(value).__name__}")
    if value not in table:
        raise ValueError(f"{what} must be one of {sorted(table)}, got {value!r}")
    return table[value]


def _typed_pad_class(pad_class):
    if isinstance(pad_class, bool) or not isinstance(pad_class, int):
        raise TypeError(f"pad_class must be an integer, got {type(pad_class).__name__}")


def _typed_draws(draws):
    if not isinstance(draws, torch.Tensor) or draws.dtype != torch.float32:
        raise TypeError("draws must be a float32 tensor")


def _typed(padding_mode, pad_class, clamp, draws):
    """The TypeError half of sample_patches' keyword checks, for a caller (patch_warp) that raises every TypeError of its own
    keywords before the first ValueError."""
    for value, table, what in ((padding_mode, PADDING_MODES, "padding_mode"), (clamp, CLAMPS, "clamp")):
        if not isinstance(value, str):
            _mode(value, table, what)
    _typed_pad_class(pad_class)
    _typed_draws(draws)


def _prepare(samples, indexes, draws, patch_size, padding_mode, pad_class, clamp, out, what="sample_patches"):
    """Every check of sample_patches and the allocation of its outputs.  -> (the leading arguments of micf_patch_sample up to
    `picked`, in order; the four outputs; device; B; what must stay alive until the call returns)."""
    Pd, Ph, Pw = _args.triple(patch_size, "patch_size")
    pad = _mode(padding_mode, PADDING_MODES, "padding_mode")
    clamp_mode = _mode(clamp, CLAMPS, "clamp")
    _typed_pad_class(pad_class)
    if not 0 <= pad_class <= 255:
        raise ValueError(f"pad_class must lie in 0..255, got {pad_class}")
    _typed_draws(draws)
    items, device, has_label, meta = _describe(samples, what)
    B = len(meta)
    indexes = list(indexes)
    if len(indexes) != B:
        raise ValueError(f"{B} samples but {len(indexes)} indexes")
    for b, (idx, (shape, dtypes)) in enumerate(zip(indexes, meta)):
        if not isinstance(idx, PatchIndex):
            raise TypeError(f"index {b} must be a PatchIndex")
        if idx.shape != shape or idx.dtypes != dtypes or idx.buffer.device != device:
            raise ValueError(f"index {b} was built for a scan of shape {idx.shape} and dtypes {idx.dtypes}, sample {b} has {shape} "
                             f"and {dtypes}")
        if (idx.label_values, idx.modes, idx.percentiles) != (indexes[0].label_values, indexes[0].modes, indexes[0].percentiles):
            raise ValueError(f"index {b} was built with other label values or another normalisation than index 0")
    if tuple(draws.shape) != (B, 6):
        raise ValueError(f"draws must have shape [{B}, 6], got {list(draws.shape)}")
    if not draws.is_cuda or draws.device != device:
        raise ValueError(f"draws must be a CUDA (ROCm) tensor on {device}")
    if not draws.is_contiguous():
        raise ValueError("draws must be contiguous")
    if out is None:
        image = torch.empty((B, 2, Pd, Ph, Pw), dtype=torch.float16, device=device)
        label_map = torch.empty((B, Pd, Ph, Pw), dtype=torch.uint8, device=device) if has_label else None
        origins = torch.empty((B, 3), dtype=torch.int32, device=device)
        picked = torch.empty((B, 4), dtype=torch.int32, device=device)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("out must be an (image, label_map | None, origins, picked) tuple")
        image = _args.out_tensor(out[0], "out image", (B, 2, Pd, Ph, Pw), torch.float16, device)
        if has_label != (out[1] is not None):
            raise ValueError("out label_map must be given exactly when the samples have labels")
        label_map = _args.out_tensor(out[1], "out label_map", (B, Pd, Ph, Pw), torch.uint8, device) if has_label else None
        origins = _args.out_tensor(out[2], "out origins", (B, 3), torch.int32, device)
        picked = _args.out_tensor(out[3], "out picked", (B, 4), torch.int32, device)
    vals = _args.int32_array(list(indexes[0].label_values))
    ptrs, sizes = _index_arrays(indexes)
    args = (ctypes.addressof(items), B, ctypes.addressof(ptrs), ctypes.addressof(sizes), ctypes.addressof(vals),
            len(indexes[0].label_values), draws.data_ptr(), Pd, Ph, Pw, pad, pad_class, clamp_mode, image.data_ptr(),
            None if label_map is None else label_map.data_ptr(), origins.data_ptr(), picked.data_ptr())
    return args, (image, label_map, origins, picked), device, B, (items, ptrs, sizes, vals)


def sample_patches(samples, indexes, draws, patch_size=(128, 128, 128), padding_mode="zeros", pad_class=0, clamp="both", out=None,
                   affine=None, displacement=None, field_interpolation="linear"):
    """indexes: index_scans' result for these samples.  Each index is checked against its sample by shape, dtypes and device;
    label values, normalisation and percentiles, which a sample does not carry, are checked for agreement across the batch's
    indexes (ValueError either way);
    draws: float32 CUDA [B, 6], read on the device.  out: optional preallocated (image, label_map | None, origins, picked).
    affine / displacement / field_interpolation: with a map or a field the patch is cut through it, rotate / zoom / elastic
    deformation of the patch in the crop pass itself (patch_warp.sample_warped_patches, which this call then is); with both None
    the launches are the plain crop's.
    -> (image fp16 [B, 2, Pd, Ph, Pw], label_map uint8 [B, Pd, Ph, Pw] | None, origins int32 [B, 3], picked int32 [B, 4])."""
    if affine is not None or displacement is not None:
        from . import patch_warp
        return patch_warp.sample_warped_patches(samples, indexes, draws, patch_size=patch_size, affine=affine,
                                                displacement=displacement, field_interpolation=field_interpolation,
                                                padding_mode=padding_mode, pad_class=pad_class, clamp=clamp, out=out)
    args, outputs, device, _, keep = _prepare(samples, indexes, draws, patch_size, padding_mode, pad_class, clamp, out)
    _lib.call_on(device, "micf_patch_sample", *args)
    del keep
    return outputs


def sample_batch(samples, draws, patch_size=(128, 128, 128), label_values=MMWHS_LABEL_VALUES, normalisation="minmax",
                 percentiles=(1, 99), padding_mode="zeros", pad_class=0, clamp="both", out=None, affine=None, displacement=None,
                 field_interpolation="linear"):
    """index_scans + sample_patches in one call: the same results bit for bit (for scans that do not stay resident)."""
    samples = list(samples)
    indexes = index_scans(samples, label_values=label_values, normalisation=normalisation, percentiles=percentiles)
    return sample_patches(samples, indexes, draws, patch_size=patch_size, padding_mode=padding_mode, pad_class=pad_class,
                          clamp=clamp, out=out, affine=affine, displacement=displacement, field_interpolation=field_interpolation)


__all__ = ["index_scans", "draw_patches", "sample_patches", "sample_batch", "PatchIndex", "SEGMENT", "MMWHS_LABEL_VALUES",
           "SIGNATURES"]
