"""Elastic deformation for the volume loader's resample pass: the binding of include/micformer_elastic.h (kernel:
csrc/volume_elastic.hip), the checks of the two keywords `displacement=` / `field_interpolation=` that loader.load_batch / load_pair
take, and the host-side draw of random control-grid fields.

    field = elastic.draw_elastic(len(samples), device="cuda")                     # [B, 3, 7, 7, 7] float32, one field per sample
    image, label_map, crop = loader.load_batch(samples, displacement=field, field_interpolation="cubic", affine=theta)

A field is [B, 3, gd, gh, gw]: per control point a vector in (x, y, z) order (x along W, as F.grid_sample's last dimension), in
normalised OUTPUT coordinates (2 = the whole axis), on a control grid whose corner points sit on the centres of the first and last
output voxel of each axis (align_corners=True with respect to the output grid).  The loader interpolates it at every output voxel,
u, and samples the raw volumes at s = theta . (n + u, 1) -- theta the `affine=` map, or the identity -- once, in the pass that reads
the raw scan: the image is interpolated once and the label rounded once.  The deformation lives in the output frame and comes before
the map, so with a [B, 2, 3, 4] map CT, label and MR see the same deformation and then each its own map.  "linear" interpolates the
control values trilinearly (with the grid equal to `size` the field is one vector per voxel, a registration network's output);
"cubic" is the uniform cubic B-spline, which approximates them and is C2: what makes a coarse random grid an elastic deformation
without kinks.  The tensor is read on the device when the kernel runs: a graph captured with `out=` picks up new draws after
`field.copy_(...)`.  Rules: include/micformer_elastic.h, DESIGN.md "Volume loader".
"""
import torch

from . import _args, _lib
from .affine import _three

FIELD_LINEAR, FIELD_CUBIC = 0, 1              # MICF_FIELD_*
FIELD_INTERPOLATIONS = {"linear": FIELD_LINEAR, "cubic": FIELD_CUBIC}
MAX_GRID = 512                                # of one axis of the control grid

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_volume_loader_elastic_workspace": "i",
    "micf_volume_loader_elastic": "piiiipiiiddplpppppiipiiiip",
}
INT64_RETURNS = frozenset(("micf_volume_loader_elastic_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="elastic deformation")


def interpolation(field_interpolation):
    """"linear" | "cubic" -> MICF_FIELD_*; touches no device."""
    rule = f"field_interpolation must be one of {sorted(FIELD_INTERPOLATIONS)}"
    if not isinstance(field_interpolation, str):
        raise TypeError(f"{rule}, got {type(field_interpolation).__name__}")
    if field_interpolation not in FIELD_INTERPOLATIONS:
        raise ValueError(f"{rule}, got {field_interpolation!r}")
    return FIELD_INTERPOLATIONS[field_interpolation]


def typed(displacement):
    """The TypeError half of the checks of `displacement` (a float32 tensor), so that a caller can raise every TypeError of its
    keywords before the first ValueError."""
    if not isinstance(displacement, torch.Tensor):
        raise TypeError(f"displacement must be a float32 tensor, got {type(displacement).__name__}")
    if displacement.dtype != torch.float32:
        raise TypeError(f"displacement must be a float32 tensor, got {displacement.dtype}")


def fields(displacement, batch):
    """The ValueError half: a CUDA, contiguous [batch, 3, gd, gh, gw] tensor with every grid extent in 2..512 -> (gd, gh, gw).
    Looks at the tensor's metadata only."""
    shape = tuple(displacement.shape)
    if len(shape) != 5 or shape[1] != 3:
        raise ValueError(f"displacement must have shape [B, 3, gd, gh, gw], got {list(shape)}")
    if min(shape[2:]) < 2 or max(shape[2:]) > MAX_GRID:
        raise ValueError(f"displacement needs a control grid of 2..{MAX_GRID} points per axis, got {list(shape[2:])}")
    if shape[0] != batch:
        raise ValueError(f"displacement holds fields for {shape[0]} samples, the batch has {batch}")
    if not displacement.is_cuda:
        raise ValueError("micformer_amd.loader runs on the GPU: displacement must be a CUDA (ROCm) tensor")
    if not displacement.is_contiguous():
        raise ValueError("displacement must be contiguous")
    return shape[2:]


def draw_elastic(batch, size=(128, 128, 128), grid=(7, 7, 7), magnitude=5.0, prob=1.0, locked_borders=True, generator=None,
                 device="cpu"):
    """Random control-grid displacement fields for a batch, drawn on the host from `generator` (as affine.draw_affine):
    -> [B, 3, gd, gh, gw] float32 on `device`, components in (x, y, z) order, in normalised coordinates of `size`.

    Per sample, with probability `prob` (the zero field otherwise): every control vector uniform in +-magnitude OUTPUT VOXELS per
    axis (`magnitude` a number or a (d, h, w) triple), i.e. +-2 magnitude / extent normalised.  locked_borders: the outermost layer
    of control points is zero, so under "linear" the faces of the output grid stay where they are (under "cubic" they move by the
    little the next layer contributes); a grid axis of 2 points is then all border.  Meant for field_interpolation="cubic".

    magnitude must stay below half the control spacing (extent - 1) / (g - 1) voxels on every axis: beyond it two neighbouring
    control points could swap places and the deformation fold.  That bound alone does not exclude folding for every draw; freedom
    from folding (a positive Jacobian determinant of n -> n + u(n) everywhere) is tested at the defaults only.

    Parity with MONAI's Rand3DElasticd, TorchIO's RandomElasticDeformation or batchgenerators is unpinned: none of them was
    available to compare against, so the distribution above (uniform per control point, no smoothing kernel) is this function's
    own; only the control-grid-plus-B-spline construction is TorchIO's."""
    if isinstance(batch, bool) or not isinstance(batch, int):
        raise TypeError(f"batch must be an integer, got {type(batch).__name__}")
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}")
    D, H, W = _args.triple(size, "size")
    gd, gh, gw = _args.triple(grid, "grid", max_extent=MAX_GRID)
    if min(gd, gh, gw) < 2:
        raise ValueError(f"grid must have at least 2 points per axis, got {grid!r}")
    mag = _three(magnitude, "magnitude")                                          # (d, h, w)
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"prob must lie in [0, 1], got {prob!r}")
    for m, extent, g, axis in zip(mag, (D, H, W), (gd, gh, gw), "dhw"):
        spacing = (extent - 1) / (g - 1)
        if m > 0.0 and m >= spacing / 2.0:
            raise ValueError(f"magnitude {m:g} on axis {axis} must stay below half the control spacing ({spacing:g} voxels): "
                             "neighbouring control points could swap")
    apply = torch.rand(batch, generator=generator, dtype=torch.float64) < prob
    sym = 2.0 * torch.rand(batch, 3, gd, gh, gw, generator=generator, dtype=torch.float64) - 1.0
    scale = torch.tensor([2.0 * mag[2] / W, 2.0 * mag[1] / H, 2.0 * mag[0] / D], dtype=torch.float64)      # (x, y, z)
    keep = apply[:, None, None, None, None].expand(batch, 3, gd, gh, gw).clone()
    if locked_borders:
        inner = torch.zeros(gd, gh, gw, dtype=torch.bool)
        inner[1:-1, 1:-1, 1:-1] = True
        keep &= inner
    field = torch.where(keep, sym * scale[None, :, None, None, None], torch.zeros((), dtype=torch.float64))
    return field.to(torch.float32).contiguous().to(device)


__all__ = ["FIELD_INTERPOLATIONS", "SIGNATURES", "draw_elastic", "fields", "interpolation", "typed"]
