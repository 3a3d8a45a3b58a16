"""CPU checks of the volume loader: the referee (tests/loader_ref.py) against the golden fixture made by the real reference loader and
against a float64 brute force, the ctypes struct and constants against include/micformer_loader.h (tests/test_abi.py has the
entry points), argument errors caught before any launch, and the compiled device code's scratch use."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_header
import loader_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_loader.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "f11_loader.npz")


# ---- the referee ----------------------------------------------------------------------------------------------------------------

def test_referee_matches_the_reference_loader_fixture():
    g = np.load(GOLDEN)
    assert int(g["seed"]) == R.F11_SEED and tuple(g["ct_shape"]) == R.F11_CT_SHAPE and tuple(g["mr_shape"]) == R.F11_MR_SHAPE
    a = R.f11_inputs(int(g["seed"]))
    image, cmap, crop = R.load_pair(a["ct"], a["mr"], a["ct_label"], size=tuple(int(s) for s in g["size"]))
    st = int(g["stride"])
    assert np.array_equal(cmap, g["class_map"])
    assert (cmap == 255).any() and set(np.unique(cmap)) == set(range(8)) | {255}
    assert np.array_equal(crop, g["crop_indexes"])
    assert not np.array_equal(crop, [[0, 128]] * 3)                  # the zero margins make the box smaller than the volume
    steps = R.fp16_steps(image[:, ::st, ::st, ::st], g["image_lattice"])
    print(f"referee vs fixture: {int((steps != 0).sum())} of {steps.size} stored points differ, max {int(steps.max())} fp16 step(s)")
    assert steps.max() <= 1


@pytest.mark.parametrize("src,size", [((9, 14, 11), (16, 16, 16)), ((23, 17, 31), (8, 12, 10)), ((1, 20, 7), (5, 20, 13))])
def test_referee_resize_matches_float64_brute_force(src, size):
    g = np.random.default_rng(sum(src))
    norm = R.normalize(g.integers(-500, 1500, size=src, dtype=np.int16))
    got = R.resize_image(norm, size).astype(np.float16)
    want = R.brute_force_trilinear(norm, size).astype(np.float16)
    steps = R.fp16_steps(got, want)
    print(f"{src} -> {size}: share differing {float((steps != 0).mean()):.2e}, max {int(steps.max())} step(s)")
    assert steps.max() <= 1


def test_referee_normalize_rules():
    v = np.array([[[-32768, 0, 32767]]], np.int16)                   # range 65535: int32 arithmetic, no int16 wrap
    assert np.array_equal(R.normalize(v), (np.float32([0, 32768, 65535]) / np.float32(65535)).reshape(1, 1, 3))
    assert np.isnan(R.normalize(np.full((2, 2, 2), 7, np.int16))).all()
    assert np.isnan(R.normalize(np.full((2, 2, 2), 0.5, np.float32))).all()
    f = np.float32([[[0.25, 1.5, -3.0]]])
    assert np.array_equal(R.normalize(f), (f - np.float32(-3.0)) / np.float32(4.5))


def test_referee_class_map_and_crop_rules():
    lab = np.array([[[0, 205, 421], [850, -7, 600]]], np.int16)
    assert np.array_equal(R.class_map(lab, (1, 2, 3)), np.uint8([[[0, 1, 255], [7, 255, 5]]]))
    assert np.array_equal(R.class_map(lab, (1, 2, 3), label_values=(421, 850)), np.uint8([[[0, 255, 1], [2, 255, 255]]]))
    img = np.zeros((2, 6, 7, 8), np.float32)
    assert np.array_equal(R.crop_indexes(img), np.zeros((3, 2), np.int32))
    img[0, 2, 3, 0] = 1.0
    img[1, 4, 3, 5] = 0.5
    assert np.array_equal(R.crop_indexes(img), [[1, 5], [2, 4], [0, 6]])


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_sample_struct_matches_the_header():
    from micformer_amd import loader
    names = []
    for decl in abi_header.struct_decls(HEADER, "micf_loader_sample"):
        if decl.startswith("const void*"):
            names += [(n.strip(), ctypes.c_void_p) for n in decl[len("const void*"):].split(",")]
        else:
            assert decl.startswith("int32_t"), decl
            for n in decl[len("int32_t"):].split(","):
                n = n.strip()
                names.append((n[:-3], ctypes.c_int32 * 3) if n.endswith("[3]") else (n, ctypes.c_int32))
    assert [(n, t) for n, t in loader.LoaderSample._fields_] == names
    assert ctypes.sizeof(loader.LoaderSample) == 3 * 8 + 12 * 4
    consts = abi_header.defines(HEADER, "MICF_LOADER_")
    assert (consts["MICF_LOADER_I16"], consts["MICF_LOADER_F32"], consts["MICF_LOADER_I32"]) == (
        loader.DTYPE_I16, loader.DTYPE_F32, loader.DTYPE_I32)
    assert consts["MICF_LOADER_MAX_LABEL_VALUES"] == loader.MAX_LABEL_VALUES


def _sample(loader, **kw):
    s = loader.LoaderSample()
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    s.ct, s.mr, s.label = fake, fake, fake
    s.ct_shape[:] = (8, 8, 8)
    s.mr_shape[:] = (9, 7, 8)
    s.label_shape[:] = (8, 8, 8)
    s.ct_dtype, s.mr_dtype, s.label_dtype = loader.DTYPE_I16, loader.DTYPE_F32, loader.DTYPE_I32
    for k, v in kw.items():
        if k.endswith("_shape"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.loader import lib
    a = lib.micf_volume_loader_workspace(1)
    assert a == lib.micf_volume_loader_workspace(1) and a >= 40 and a % 256 == 0
    assert lib.micf_volume_loader_workspace(100) >= 4000
    assert lib.micf_volume_loader_workspace(0) == -1
    assert lib.micf_volume_loader_workspace(-3) == -1


def test_bad_arguments_return_codes_before_any_launch():
    """The calls micf_volume_loader rejects and the code each returns; micf_volume_loader_norm and micf_volume_loader_affine, given
    valid normaliser / `stats` / affine arguments next to them and their own workspace size, return the same codes."""
    from micformer_amd import affine, loader, normalise
    fake = 1 << 20
    _rejected_calls(loader, loader.lib.micf_volume_loader, loader.lib.micf_volume_loader_workspace(1), (), ())
    norm = (normalise.ZSCORE, normalise.PERCENTILE, 1.0, 99.0)
    _rejected_calls(loader, normalise.lib.micf_volume_loader_norm, normalise.lib.micf_volume_loader_norm_workspace(1), norm, (None,))
    _rejected_calls(loader, affine.lib.micf_volume_loader_affine, affine.lib.micf_volume_loader_affine_workspace(1), norm,
                    (None, fake, 0, affine.padding("zeros")))


def _rejected_calls(loader, fn, ws, norm, tail):
    """fn(<the common head>, *norm, <workspace and outputs>, *tail, stream) for every rejected call of the table."""
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)

    def call(sample=None, B=1, size=(16, 16, 16), values=vals, nvals=7, workspace=fake, ws_bytes=ws, image=fake, label_map=fake,
             crop=fake, samples_ptr=True):
        s = sample if sample is not None else _sample(loader)
        return fn(ctypes.addressof(s) if samples_ptr else None, B, *size, None if values is None else ctypes.addressof(values),
                  nvals, *norm, workspace, ws_bytes, image, label_map, crop, *tail, None)

    assert call(samples_ptr=False) == EINVAL
    assert call(B=0) == EINVAL
    assert call(size=(16, 0, 16)) == EINVAL
    assert call(workspace=None) == EINVAL
    assert call(workspace=fake + 64) == EINVAL                        # workspace alignment
    assert call(ws_bytes=ws - 1) == EINVAL
    assert call(image=None) == EINVAL
    assert call(crop=None) == EINVAL
    assert call(label_map=None) == EINVAL                             # the sample has a label, the call no label_map
    assert call(_sample(loader, label=None)) == EINVAL                # ... and the other way round
    assert call(_sample(loader, ct=None)) == EINVAL
    assert call(_sample(loader, mr=None)) == EINVAL
    assert call(_sample(loader, mr=fake + 2)) == EINVAL               # float32 needs 4-byte alignment
    assert call(_sample(loader, ct_shape=(8, 0, 8))) == EINVAL
    assert call(values=None) == EINVAL
    assert call(nvals=-1) == EINVAL
    assert call(values=(ctypes.c_int32 * 255)(*range(1, 256)), nvals=255) == EINVAL
    assert call(values=(ctypes.c_int32 * 3)(5, 0, 7), nvals=3) == EINVAL          # zero
    assert call(values=(ctypes.c_int32 * 3)(5, 7, 5), nvals=3) == EINVAL          # duplicate
    assert call(_sample(loader, ct_dtype=loader.DTYPE_I32)) == EUNSUP             # int32 is a label dtype only
    assert call(_sample(loader, label_dtype=loader.DTYPE_F32)) == EUNSUP
    assert call(_sample(loader, mr_dtype=7)) == EUNSUP
    assert call(_sample(loader, mr_shape=(8, 2049, 8))) == EUNSUP                 # extent > 2048
    assert call(_sample(loader, ct_shape=(2048, 1024, 1024))) == EUNSUP           # 2^31 voxels
    assert call(size=(512, 512, 513)) == EUNSUP                                   # more than 512^3 target voxels


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import loader
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    with pytest.raises(ValueError, match="CUDA"):
        loader.load_pair(ct, ct)                                       # CPU tensors
    with pytest.raises(TypeError):
        loader.load_pair(ct.double(), ct)
    with pytest.raises(TypeError):
        loader.load_pair(ct, ct, ct.float())                           # float label
    with pytest.raises(TypeError):
        loader.load_pair(ct.numpy(), ct)
    with pytest.raises(ValueError):
        loader.load_batch([])
    with pytest.raises(ValueError):
        loader.load_batch([(ct, ct)])
    for bad in [(0, 205), (205, 205), range(1, 300), "ab", (2 ** 40,)]:
        with pytest.raises(ValueError):
            loader.load_pair(ct, ct, label_values=bad)
    for bad in [(128, 128), (128, 0, 128), None]:
        with pytest.raises(ValueError):
            loader.load_pair(ct, ct, size=bad)


# ---- the device code ----------------------------------------------------------------------------------------------------------

def test_volume_loader_device_code_uses_no_scratch():
    sizes, asm, flags = abi_header.device_asm("volume_loader.hip")
    assert not any("fast-math" in f or "-Ofast" in f for f in flags)     # the normalisation needs the IEEE divide
    assert len(sizes) == 4 and all(v == 0 for v in sizes.values()), sizes
    assert "v_div_fixup_f32" in asm and "v_div_fmas_f32" in asm          # the correctly rounded fp32 divide sequence
