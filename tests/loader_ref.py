"""CPU referee of the volume loader (micformer_amd/loader.py): the reference's MMWHS_noCrop_Augment.__getitem__ arithmetic between
"the raw arrays are in memory" and the sample (MMWHS.py:308-405, image_utils.py:48-55), restated on numpy / torch-CPU.
F.interpolate on the CPU IS the reference's resize operator; the rest is written out from the formulas.

Deviations from the reference, both deliberate (see the loader's docstring): int16 volumes are normalised with int32 arithmetic (no
int16 wrap), and the label is a uint8 class map with 255 where none of the reference's planes is set."""
import numpy as np
import torch
import torch.nn.functional as F

MMWHS_LABEL_VALUES = (205, 420, 500, 550, 600, 820, 850)


def normalize(vol):
    """image_utils.normalize -> float32 array.  Integer input: the two integers are exact in float32 and the divide is one
    correctly rounded float32 divide (equal to the reference's float64 divide followed by torch.Tensor(...))."""
    vol = np.asarray(vol)
    with np.errstate(invalid="ignore", divide="ignore"):
        if vol.dtype.kind == "i":
            v = vol.astype(np.int32)
            mn, mx = int(v.min()), int(v.max())
            return (v - mn).astype(np.float32) / np.float32(mx - mn)
        if vol.dtype != np.float32:
            raise TypeError(f"image volumes are int16 / int32 / float32 here, got {vol.dtype}")
        mn, mx = vol.min(), vol.max()
        return (vol - mn) / (mx - mn)


def resize_image(norm, size):
    """float32 (d, h, w) -> float32 `size`, MMWHS.py:332."""
    t = torch.from_numpy(np.ascontiguousarray(norm))[None, None]
    return F.interpolate(t, size=tuple(size), mode="trilinear")[0, 0].numpy()


def class_map(label, size, label_values=MMWHS_LABEL_VALUES):
    """label_to_one_hot + F.interpolate(mode="nearest") + "which plane is set" -> uint8 `size` (255: none)."""
    label = np.asarray(label)
    out = np.full(tuple(size), 255, np.uint8)
    for k, plane in enumerate([label == 0] + [label == v for v in label_values]):      # (plane by plane: 8x less memory)
        plane = torch.from_numpy(plane.astype(np.float32))[None, None]
        out[F.interpolate(plane, size=tuple(size), mode="nearest")[0, 0].numpy() != 0] = k
    return out


def crop_indexes(image):
    """MMWHS.py:380-383 on the float32 (2, D, H, W) image; (0, 0) per axis where the reference would raise (all zero)."""
    idx = np.nonzero(np.sum(image, axis=0) != 0)
    if idx[0].size == 0:
        return np.zeros((3, 2), np.int32)
    return np.array([[max(0, int(a.min()) - 1), int(a.max()) + 1] for a in idx], np.int32)


def load_pair(ct, mr, ct_label=None, size=(128, 128, 128), label_values=MMWHS_LABEL_VALUES):
    """numpy arrays -> (image float16 [2, D, H, W], class map uint8 [D, H, W] | None, crop_indexes int32 [3, 2])."""
    image = np.stack([resize_image(normalize(ct), size), resize_image(normalize(mr), size)])
    lab = None if ct_label is None else class_map(ct_label, size, label_values)
    return image.astype(np.float16), lab, crop_indexes(image)


def brute_force_trilinear(norm, size):
    """float64 restatement of the trilinear resize (tap indices and weights from the float32 formulas, the sum in float64)."""
    norm = np.asarray(norm, np.float64)

    def axis(n_in, n_out):
        o = np.arange(n_out, dtype=np.float32)
        scale = np.float32(n_in) / np.float32(n_out)
        s = np.maximum(scale * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0))
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = (s - i0.astype(np.float32)).astype(np.float64)
        return i0, i1, 1.0 - l1, l1

    z0, z1, lz0, lz1 = axis(norm.shape[0], size[0])
    y0, y1, ly0, ly1 = axis(norm.shape[1], size[1])
    x0, x1, lx0, lx1 = axis(norm.shape[2], size[2])
    out = np.zeros(tuple(size), np.float64)
    for zi, lz in ((z0, lz0), (z1, lz1)):
        for yi, ly in ((y0, ly0), (y1, ly1)):
            for xi, lx in ((x0, lx0), (x1, lx1)):
                out += norm[zi[:, None, None], yi[None, :, None], xi[None, None, :]] * (
                    lz[:, None, None] * ly[None, :, None] * lx[None, None, :])
    return out


def fp16_steps(a, b):
    """Distance of two float16 arrays in units of float16 steps (0 where both are NaN)."""
    def order(x):
        u = np.asarray(x, np.float16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    a, b = np.asarray(a, np.float16), np.asarray(b, np.float16)
    d = np.abs(order(a) - order(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) != np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 20, d))


# ---- the f11 fixture's raw arrays (tests/golden/make_golden_loader.py stores only the expected outputs) ------------------------
F11_SEED = 1111
F11_CT_SHAPE, F11_MR_SHAPE = (40, 56, 48), (33, 61, 52)


def f11_inputs(seed=F11_SEED):
    """-> dict(ct int16, ct_label int16, mr float32, mr_label int16): different shapes and dtypes on purpose, a zero margin of
    about an eighth of every axis in both images (so crop_indexes is not the full box), labels with the seven MM-WHS values, 0 and
    the stray value 421."""
    g = np.random.default_rng(seed)

    def margin(shape):
        return tuple(slice(max(1, n // 8), n - max(1, n // 7)) for n in shape)

    ct = np.full(F11_CT_SHAPE, -1000, np.int16)                       # the margin holds the minimum: 0 after normalisation
    box = margin(F11_CT_SHAPE)
    ct[box] = g.integers(-999, 2001, size=ct[box].shape, dtype=np.int16)
    mr = np.zeros(F11_MR_SHAPE, np.float32)
    box = margin(F11_MR_SHAPE)
    mr[box] = (g.random(mr[box].shape, dtype=np.float32) * np.float32(1500.0) + np.float32(1.0))
    values = np.array((0,) + MMWHS_LABEL_VALUES + (421,), np.int16)
    ct_label = values[g.integers(0, len(values), size=F11_CT_SHAPE)]
    mr_label = values[g.integers(0, len(values), size=F11_MR_SHAPE)]
    return dict(ct=ct, ct_label=ct_label, mr=mr, mr_label=mr_label)
