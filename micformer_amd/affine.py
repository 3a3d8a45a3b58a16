"""Affine maps for the volume loader's resample pass: the binding of include/micformer_affine.h (kernels: csrc/volume_affine.hip),
the checks of the two keywords `affine=` / `padding_mode=` that loader.load_batch / load_pair take, and the host-side draw of random
rotate / zoom / translate maps.

    theta = affine.draw_affine(len(samples), device="cuda")                       # [B, 3, 4] float32, one map per sample
    image, label_map, crop = loader.load_batch(samples, affine=theta, padding_mode="border")

A map is F.affine_grid's theta: it acts on the normalised OUTPUT coordinate n = (x, y, z) in [-1, 1]^3 (x along W) and gives the
normalised SOURCE coordinate, s = theta . (n, 1); nothing is inverted.  The loader samples the raw volumes there
(F.grid_sample(align_corners=False): image trilinear, label nearest), once, in the pass that reads the raw scan.  Because the map
lives in normalised coordinates, one map serves the CT, MR and label arrays of a sample whatever their shapes.  [B, 3, 4] is one
map per sample for CT, MR and label; [B, 2, 3, 4] gives index 0 to CT and its label and index 1 to MR (a re-orientation or a
registration of one modality).  The tensor is read on the device when the kernels run: a graph captured with `out=` picks up new
draws after `theta.copy_(...)`.  Rules: include/micformer_affine.h, DESIGN.md "Volume loader".
"""
import math

import torch

from . import _args, _lib

PAD_ZEROS, PAD_BORDER = 0, 1                  # MICF_PAD_*
PADDING_MODES = {"zeros": PAD_ZEROS, "border": PAD_BORDER}

# name -> argument signature (as _lib.SIGNATURES); the workspace query returns int64 (INT64_RETURNS), the other int
SIGNATURES = {
    "micf_volume_loader_affine_workspace": "i",
    "micf_volume_loader_affine": "piiiipiiiddplpppppiip",
}
INT64_RETURNS = frozenset(("micf_volume_loader_affine_workspace",))

lib = _lib.bind(SIGNATURES, INT64_RETURNS, feature="affine augmentation")


def padding(padding_mode):
    """"zeros" | "border" -> MICF_PAD_*; touches no device."""
    rule = f"padding_mode must be one of {sorted(PADDING_MODES)}"
    if not isinstance(padding_mode, str):
        raise TypeError(f"{rule}, got {type(padding_mode).__name__}")
    if padding_mode not in PADDING_MODES:
        raise ValueError(f"{rule}, got {padding_mode!r}")
    return PADDING_MODES[padding_mode]


def typed(affine):
    """The TypeError half of the checks of `affine` (a float32 tensor), so that a caller can raise every TypeError of its
    keywords before the first ValueError."""
    if not isinstance(affine, torch.Tensor):
        raise TypeError(f"affine must be a float32 tensor, got {type(affine).__name__}")
    if affine.dtype != torch.float32:
        raise TypeError(f"affine must be a float32 tensor, got {affine.dtype}")


def maps(affine, batch):
    """The ValueError half: a CUDA, contiguous [batch, 3, 4] or [batch, 2, 3, 4] tensor -> per_modality (0 / 1).  Looks at the
    tensor's metadata only."""
    shape = tuple(affine.shape)
    if shape[-2:] != (3, 4) or len(shape) not in (3, 4) or (len(shape) == 4 and shape[1] != 2):
        raise ValueError(f"affine must have shape [B, 3, 4] or [B, 2, 3, 4], got {list(shape)}")
    if shape[0] != batch:
        raise ValueError(f"affine holds maps for {shape[0]} samples, the batch has {batch}")
    if not affine.is_cuda:
        raise ValueError("micformer_amd.loader runs on the GPU: affine must be a CUDA (ROCm) tensor")
    if not affine.is_contiguous():
        raise ValueError("affine must be contiguous")
    return int(len(shape) == 4)


def _rotation(a_d, a_h, a_w):
    """R_d . R_h . R_w in (x, y, z) order (x along W): rotations about the D, H and W axes."""
    cd, sd, ch, sh, cw, sw = math.cos(a_d), math.sin(a_d), math.cos(a_h), math.sin(a_h), math.cos(a_w), math.sin(a_w)
    r_d = torch.tensor([[cd, -sd, 0.0], [sd, cd, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    r_h = torch.tensor([[ch, 0.0, sh], [0.0, 1.0, 0.0], [-sh, 0.0, ch]], dtype=torch.float64)
    r_w = torch.tensor([[1.0, 0.0, 0.0], [0.0, cw, -sw], [0.0, sw, cw]], dtype=torch.float64)
    return r_d @ r_h @ r_w


def _three(value, what):
    """A number (for all three axes) or a (d, h, w) triple of numbers >= 0 -> three floats."""
    try:
        vals = [float(value)] * 3 if not hasattr(value, "__len__") else [float(v) for v in value]
    except (TypeError, ValueError):
        raise TypeError(f"{what} must be a number or a (d, h, w) triple of numbers, got {value!r}") from None
    if len(vals) != 3 or not all(math.isfinite(v) and v >= 0.0 for v in vals):
        raise ValueError(f"{what} must be a finite number >= 0 or a (d, h, w) triple of them, got {value!r}")
    return vals


def draw_affine(batch, size=(128, 128, 128), rotate=(0.26, 0.26, 0.26), scale=0.15, translate=(8, 8, 8), prob=1.0,
                per_modality=None, generator=None, device="cpu"):
    """Random rotate / zoom / translate maps for a batch, drawn on the host from `generator` (as data.draw_augmentation):
    -> [B, 3, 4] float32 on `device`, or [B, 2, 3, 4] when `per_modality` is given.

    Per sample, with probability `prob` (the identity otherwise): angles a_d, a_h, a_w uniform in +-rotate (radians, about the D, H
    and W axes), factors 1 + U(-scale, scale) per axis, shifts uniform in +-translate (output voxels); each of the three a number
    or a (d, h, w) triple.  The matrix acts on output coordinates and gives source coordinates (MONAI's grid convention, nothing is
    inverted): a factor above 1 shows more of the scan, which therefore looks smaller.  In output voxel space, (x, y, z) order,
    A = R_d . R_h . R_w . diag(factors) and t is the shift; the returned map is that pair conjugated into normalised coordinates,
    theta[:, :3] = N^-1 A N and theta[:, 3] = N^-1 t with N = diag(W, H, D) / 2 of `size`, so a rotation is rigid on the output grid
    whatever `size` is (on a non-cubic grid the 3 x 3 block is orthonormal only after the conjugation is undone).

    per_modality: an optional fixed [2, 3, 4] map in normalised coordinates (index 0 CT and its label, index 1 MR): the MR
    re-orientation of MMWHS_noCrop or a precomputed registration.  It is composed after the draw and applied FIRST to the output
    coordinate: s = theta . (P_m . (n, 1), 1), i.e. block theta_A . P_A and offset theta_A . P_t + theta_t.

    Parity with MONAI's RandAffined is unpinned: MONAI was not available to compare against, so the distributions above and the
    order R_d . R_h . R_w are this function's own and only the grid convention is MONAI's."""
    if isinstance(batch, bool) or not isinstance(batch, int):
        raise TypeError(f"batch must be an integer, got {type(batch).__name__}")
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}")
    D, H, W = _args.triple(size, "size")
    rot, fac, shift = _three(rotate, "rotate"), _three(scale, "scale"), _three(translate, "translate")
    if not 0.0 <= float(prob) <= 1.0:
        raise ValueError(f"prob must lie in [0, 1], got {prob!r}")
    if any(f >= 1.0 for f in fac):
        raise ValueError(f"scale must stay below 1 (the factors are 1 + U(-scale, scale)), got {scale!r}")
    if per_modality is not None:
        per_modality = torch.as_tensor(per_modality, dtype=torch.float64, device="cpu")
        if tuple(per_modality.shape) != (2, 3, 4):
            raise ValueError(f"per_modality must have shape [2, 3, 4], got {list(per_modality.shape)}")
    u = torch.rand(batch, 10, generator=generator, dtype=torch.float64)          # [apply, 3 angles, 3 factors, 3 shifts], (d, h, w) each
    n = torch.tensor([W, H, D], dtype=torch.float64) / 2.0
    theta = torch.zeros(batch, 3, 4, dtype=torch.float64)
    for b in range(batch):
        a, t = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        if float(u[b, 0]) < prob:
            sym = (2.0 * u[b, 1:] - 1.0).tolist()
            ang = [sym[i] * rot[i] for i in range(3)]
            f_d, f_h, f_w = (1.0 + sym[3 + i] * fac[i] for i in range(3))
            t_d, t_h, t_w = (sym[6 + i] * shift[i] for i in range(3))
            a = _rotation(*ang) @ torch.diag(torch.tensor([f_w, f_h, f_d], dtype=torch.float64))
            t = torch.tensor([t_w, t_h, t_d], dtype=torch.float64)
        theta[b, :, :3] = a * n[None, :] / n[:, None]                            # N^-1 A N
        theta[b, :, 3] = t / n
    if per_modality is not None:
        pa, pt = per_modality[:, :, :3], per_modality[:, :, 3]                   # [2, 3, 3], [2, 3]
        both = torch.zeros(batch, 2, 3, 4, dtype=torch.float64)
        both[:, :, :, :3] = torch.einsum("bij,mjk->bmik", theta[:, :, :3], pa)
        both[:, :, :, 3] = torch.einsum("bij,mj->bmi", theta[:, :, :3], pt) + theta[:, None, :, 3]
        theta = both
    return theta.to(torch.float32).to(device)


__all__ = ["PADDING_MODES", "SIGNATURES", "draw_affine", "maps", "padding", "typed"]
