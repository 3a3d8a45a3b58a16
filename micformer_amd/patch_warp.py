"""Rotate, zoom and elastic warps of a patch, in the patch sampler's crop pass: the binding of include/micformer_patch_warp.h
(kernel: csrc/volume_patch_warp.hip).  The patch is cut THROUGH the map, straight from the raw resident scan: one interpolation of
the image, one rounding of the label, nothing intermediate written, and a rotated patch's corners read the scan wherever it has data
instead of the zeros a second F.grid_sample over a finished patch would put there.

    from micformer_amd import affine, elastic, patches, patch_warp
    idx = patches.index_scans(samples)
    draws = patches.draw_patches(len(samples), device="cuda")
    theta = affine.draw_affine(len(samples), size=patch_size, device="cuda")                 # [B, 3, 4], normalised PATCH coordinates
    field = elastic.draw_elastic(len(samples), size=patch_size, device="cuda")               # [B, 3, 7, 7, 7]
    image, label_map, origins, picked = patch_warp.sample_warped_patches(samples, idx, draws, patch_size, affine=theta,
                                                                         displacement=field, field_interpolation="cubic")

(patches.sample_patches(..., affine=theta, displacement=field) is the same call.)  The origin and `picked` come from the draws
exactly as in patches.sample_patches: a forced patch is still centred on its drawn foreground voxel, and the warp turns about the
patch centre.  theta is F.affine_grid's map in normalised patch coordinates, so affine.draw_affine(B, size=patch_size) and
elastic.draw_elastic(B, size=patch_size) are the draw functions as they stand and a rotation is rigid on the patch grid.  [B, 2, 3, 4]
gives map 0 to CT and its label and map 1 to MR; the field is applied before the map.  image: trilinear over the 8 taps, each
normalised first with the index's statistics, fp16 round-to-nearest; "zeros": a tap outside the scan counts 0, "border": the index
is clamped into the scan.  label: nearest (half to even); pad_class wherever the rounded index lies outside the scan, in both
padding modes.  With the identity map and power-of-two patch extents the result is patches.sample_patches' bit for bit; with a
zero field it is the map-only call's.  Rules and bounds: include/micformer_patch_warp.h, DESIGN.md "Patch sampler".

Nothing here synchronises with the host or runs an ATen compute op; with `out=` the call can be captured by torch.cuda.graph, and a
replay reads new `draws`, `affine` and `displacement` from the same tensors.  Outputs are bit-identical from run to run and
independent of the other samples of the batch.
"""
from . import _lib, affine as _affine, elastic as _elastic, patches

# name -> argument signature (as _lib.SIGNATURES); apart from every other module's table
SIGNATURES = {
    "micf_patch_sample_warped": "pipppipiiiiiipppppipiiiip",
}
INT64_RETURNS = frozenset()

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="patch warp")


def sample_warped_patches(samples, indexes, draws, patch_size, affine=None, displacement=None, field_interpolation="linear",
                          padding_mode="zeros", pad_class=0, clamp="both", out=None):
    """patches.sample_patches' arguments and results, the patch cut through `affine` (float32 CUDA [B, 3, 4] or [B, 2, 3, 4], None =
    the identity) and `displacement` (float32 CUDA [B, 3, gd, gh, gw] with 2..512 points per axis, None = no field;
    field_interpolation "linear" | "cubic").  Every TypeError of the keywords is raised before the first ValueError; nothing is
    launched before every check has passed.
    -> (image fp16 [B, 2, Pd, Ph, Pw], label_map uint8 [B, Pd, Ph, Pw] | None, origins int32 [B, 3], picked int32 [B, 4])."""
    if affine is not None:
        _affine.typed(affine)
    if displacement is not None:
        _elastic.typed(displacement)
    if not isinstance(field_interpolation, str):
        _elastic.interpolation(field_interpolation)                  # (raises the TypeError)
    patches._typed(padding_mode, pad_class, clamp, draws)
    interpolation = _elastic.interpolation(field_interpolation)
    args, outputs, device, B, keep = patches._prepare(samples, indexes, draws, patch_size, padding_mode, pad_class, clamp, out,
                                                      what="sample_warped_patches")
    per_modality = 0 if affine is None else _affine.maps(affine, B)
    gd, gh, gw = (0, 0, 0) if displacement is None else _elastic.fields(displacement, B)
    for t, name in ((affine, "affine"), (displacement, "displacement")):
        if t is not None and t.device != device:
            raise ValueError(f"{name} must be on {device}, got {t.device}")
    _lib.call_on(device, "micf_patch_sample_warped", *args, None if affine is None else affine.data_ptr(), per_modality,
                 None if displacement is None else displacement.data_ptr(), gd, gh, gw, interpolation)
    del keep
    return outputs


def sample_warped_batch(samples, draws, patch_size, label_values=patches.MMWHS_LABEL_VALUES, normalisation="minmax",
                        percentiles=(1, 99), affine=None, displacement=None, field_interpolation="linear", padding_mode="zeros",
                        pad_class=0, clamp="both", out=None):
    """patches.index_scans + sample_warped_patches in one call: the same results bit for bit (for scans that do not stay resident)."""
    samples = list(samples)
    indexes = patches.index_scans(samples, label_values=label_values, normalisation=normalisation, percentiles=percentiles)
    return sample_warped_patches(samples, indexes, draws, patch_size, affine=affine, displacement=displacement,
                                 field_interpolation=field_interpolation, padding_mode=padding_mode, pad_class=pad_class, clamp=clamp,
                                 out=out)


__all__ = ["SIGNATURES", "sample_warped_patches", "sample_warped_batch"]
