#!/usr/bin/env python
"""Generate tests/golden/f11_loader.npz by running the REAL reference loader, MMWHS_noCrop_Augment.__getitem__ (dataset/MMWHS.py),
on the seeded synthetic arrays of tests/loader_ref.py::f11_inputs.

Runs ONLY where a checkout of the reference is present (read-only): MICFORMER_REFERENCE names its MicFormer/ directory.  Nothing of
the reference is copied into this repository: the fixture holds expected OUTPUTS only -- the float16 image at a stride-3 lattice,
the class map derived from the 8 bool label planes (255 where none is set), crop_indexes, the seed and the shapes.

The reference module imports two things that are absent here and that this arithmetic never touches: SimpleITK (only load_nii
reads files with it: replaced by a dict lookup) and, through dataset/__init__.py, yacs (skipped by importing dataset.MMWHS under
a bare package object whose __path__ is the reference's dataset/ directory).

usage: MICFORMER_REFERENCE=<reference>/MicFormer python tests/golden/make_golden_loader.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("MICFORMER_REFERENCE")
STRIDE = 3

import loader_ref  # noqa: E402


def import_reference():
    if not REF or not os.path.isfile(os.path.join(REF, "dataset", "MMWHS.py")):
        raise SystemExit("set MICFORMER_REFERENCE to the reference's MicFormer/ directory (it holds dataset/MMWHS.py)")
    sys.modules.setdefault("SimpleITK", types.ModuleType("SimpleITK"))
    pkg = types.ModuleType("dataset")
    pkg.__path__ = [os.path.join(REF, "dataset")]
    sys.modules["dataset"] = pkg
    import dataset.MMWHS as M
    return M


def main():
    M = import_reference()
    arrays = loader_ref.f11_inputs()
    files = {"ct_1_image": arrays["ct"], "ct_1_label": arrays["ct_label"], "mr_1_image": arrays["mr"],
             "mr_1_label": arrays["mr_label"]}
    M.MMWHS_noCrop_Augment.load_nii = staticmethod(lambda path: files[str(path)].copy())
    ds = M.MMWHS_noCrop_Augment(["ct_1_image"], training=False)
    item = ds[0]
    image = item["image"].numpy()                                     # float16 (2, 128, 128, 128)
    planes = item["label"].numpy()                                    # bool (8, 128, 128, 128)
    assert image.dtype == np.float16 and image.shape == (2, 128, 128, 128) and planes.shape == (8, 128, 128, 128)
    assert planes.sum(0).max() <= 1
    cmap = np.full(planes.shape[1:], 255, np.uint8)
    for k in range(8):
        cmap[planes[k]] = k
    crop = np.array(item["crop_indexes"], np.int32)
    out = os.path.join(HERE, "f11_loader.npz")
    np.savez_compressed(out, image_lattice=image[:, ::STRIDE, ::STRIDE, ::STRIDE], stride=np.int32(STRIDE), class_map=cmap,
                        crop_indexes=crop, seed=np.int32(loader_ref.F11_SEED), ct_shape=np.int32(loader_ref.F11_CT_SHAPE),
                        mr_shape=np.int32(loader_ref.F11_MR_SHAPE), size=np.int32((128, 128, 128)))
    # the referee must restate the reference: report how close it is on this host
    r_img, r_map, r_crop = loader_ref.load_pair(arrays["ct"], arrays["mr"], arrays["ct_label"])
    print(f"wrote {out} ({os.path.getsize(out)} bytes); crop_indexes {crop.tolist()}; 255 voxels {int((cmap == 255).sum())}; "
          f"referee: image bit-equal {bool((r_img.view(np.uint16) == image.view(np.uint16)).all())}, "
          f"class map equal {bool((r_map == cmap).all())}, crop equal {bool((r_crop == crop).all())}")


if __name__ == "__main__":
    main()
