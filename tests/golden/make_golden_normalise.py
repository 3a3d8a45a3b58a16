#!/usr/bin/env python
"""Generate tests/golden/f12_normalise.npz by running the REAL reference functions on the seeded synthetic arrays of
tests/loader_ref.py::f11_inputs:
  * zscore:      MMWHS_noCrop_Augment(normalisation="zscore").__getitem__ (dataset/MMWHS.py -> image_utils.zscore_normalise), with
                 the CT handed over as float32: zscore_normalise writes into its input array, which truncates the z-scores of an
                 int16 array to integers, and the loader does not reproduce that;
  * percentile:  image_utils.irm_min_max_preprocess on each raw array, then the resize of MMWHS.py:332
                 (F.interpolate(torch.Tensor(value)[None, None], size, mode="trilinear")), float16 as __getitem__ stores it, and the
                 crop_indexes rule of MMWHS.py:380-383.

Runs ONLY where a checkout of the reference is present (read-only): MICFORMER_REFERENCE names its MicFormer/ directory.  Nothing of
the reference is copied into this repository: the fixture holds expected OUTPUTS only -- per mode the float16 image at a lattice
and crop_indexes, the class map, and the two statistics of each channel as numpy gives them on the reference's own arrays.  The
import shims are make_golden_loader.py's.

usage: MICFORMER_REFERENCE=<reference>/MicFormer python tests/golden/make_golden_normalise.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
STRIDE = 4                    # (two modes at the loader fixture's stride 3 would make this file larger than f11_loader.npz)
SIZE = (128, 128, 128)

import loader_ref  # noqa: E402
import make_golden_loader  # noqa: E402
import normalise_ref  # noqa: E402


def class_map(planes):
    assert planes.sum(0).max() <= 1
    cmap = np.full(planes.shape[1:], 255, np.uint8)
    for k in range(8):
        cmap[planes[k]] = k
    return cmap


def never_cancels(image):
    """The loader's crop rule is "either channel non-zero", the reference's "the sum is non-zero": the same unless CT + MR cancel."""
    assert not ((image.astype(np.float32).sum(0) == 0) & ((image[0] != 0) | (image[1] != 0))).any()


def main():
    M = make_golden_loader.import_reference()
    from dataset import image_utils
    arrays = loader_ref.f11_inputs()
    lat = (slice(None),) + (slice(None, None, STRIDE),) * 3

    # ---- z-score: the dataset class itself
    files = {"ct_1_image": arrays["ct"].astype(np.float32), "ct_1_label": arrays["ct_label"], "mr_1_image": arrays["mr"],
             "mr_1_label": arrays["mr_label"]}
    M.MMWHS_noCrop_Augment.load_nii = staticmethod(lambda path: files[str(path)].copy())
    item = M.MMWHS_noCrop_Augment(["ct_1_image"], training=False, normalisation="zscore")[0]
    z_image = item["image"].numpy()
    assert z_image.dtype == np.float16 and z_image.shape == (2,) + SIZE
    z32 = np.stack([F.interpolate(torch.Tensor(image_utils.zscore_normalise(files[k].copy()))[None, None], size=SIZE,
                                  mode="trilinear")[0, 0].numpy() for k in ("ct_1_image", "mr_1_image")])
    assert np.array_equal(torch.from_numpy(z32).to(torch.float16).numpy().view(np.uint16), z_image.view(np.uint16))
    never_cancels(z32)                                                # (on the float32 image, where __getitem__ takes the crop)
    cmap = class_map(item["label"].numpy())
    z_crop = np.array(item["crop_indexes"], np.int32)
    z_stats = np.array([[a[a != 0].astype(np.float64).mean(), a[a != 0].astype(np.float64).std()]
                        for a in (arrays["ct"], arrays["mr"])])

    # ---- percentile: the function + the dataset's resize and crop lines
    p32 = np.stack([F.interpolate(torch.Tensor(image_utils.irm_min_max_preprocess(arrays[k].copy()))[None, None], size=SIZE,
                                  mode="trilinear")[0, 0].numpy() for k in ("ct", "mr")])
    p_image = torch.from_numpy(p32).to(torch.float16).numpy()
    never_cancels(p32)
    idx = np.nonzero(np.sum(p32, axis=0) != 0)
    p_crop = np.array([[max(0, int(a.min()) - 1), int(a.max()) + 1] for a in idx], np.int32)
    p_stats = np.array([np.percentile(a[a > 0].astype(np.float64), [1, 99]) for a in (arrays["ct"], arrays["mr"])])

    out = os.path.join(HERE, "f12_normalise.npz")
    np.savez_compressed(out, zscore_lattice=z_image[lat], zscore_crop=z_crop, zscore_stats=z_stats, percentile_lattice=p_image[lat],
                        percentile_crop=p_crop, percentile_stats=p_stats, class_map=cmap, stride=np.int32(STRIDE),
                        seed=np.int32(loader_ref.F11_SEED), size=np.int32(SIZE))
    # the referee must restate the reference: report how close it is on this host
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")
    for mode, image, crop, st in (("zscore", z_image, z_crop, z_stats), ("percentile", p_image, p_crop, p_stats)):
        r_img, r_map, r_crop, r_st = normalise_ref.load_pair(arrays["ct"], arrays["mr"], arrays["ct_label"], normalisation=mode)
        fails, share, A = normalise_ref.close(image, r_img)
        bits = bool((r_img.astype(np.float16).view(np.uint16) == image.view(np.uint16)).all())
        print(f"{mode}: crop_indexes {crop.tolist()}; referee: {fails} failing elements, share {share:.2e} (A = {A:.2e}), "
              f"bit-equal {bits}, class map equal {bool((r_map == cmap).all())}, crop equal {bool((r_crop == crop).all())}, "
              f"stats equal {bool((r_st == st).all())}")


if __name__ == "__main__":
    main()
