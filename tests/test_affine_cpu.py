"""CPU checks of the loader's affine resample: the float64 referee (tests/affine_ref.py) against F.affine_grid + F.grid_sample, the
seeds of the GPU tests against the conditions those tests rely on, include/micformer_affine.h against the ctypes table of
micformer_amd/affine.py and the built library, argument errors caught before any launch, draw_affine, the compiled device code's
scratch use, and the host program tests/affine_index_main.cpp (csrc/affine_coords.h under the address and undefined-behaviour
sanitizers: a stand-alone program, nothing is preloaded)."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_header
import affine_ref as A
import loader_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_affine.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "restore", "postprocess", "surface")


# ---- the referee ----------------------------------------------------------------------------------------------------------------

def _torch_sample(vol, theta, size, mode, padding_mode):
    t = torch.from_numpy(np.ascontiguousarray(vol, np.float32))[None, None]
    grid = F.affine_grid(torch.from_numpy(np.asarray(theta, np.float32))[None], (1, 1) + tuple(size), align_corners=False)
    return F.grid_sample(t, grid, mode=mode, padding_mode=padding_mode, align_corners=False)[0, 0].numpy()


@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
def test_referee_matches_grid_sample(padding_mode):
    g = np.random.default_rng(7001)
    vol = g.random(A.CT_SHAPE, dtype=np.float32)
    lab = g.integers(1, 9, size=A.CT_SHAPE).astype(np.float32)        # (no 0: outside the array is told from inside)
    theta = A.draw_maps(g, 1)[0]
    ref = A.sample_image(vol, theta, A.SIZE, padding_mode)
    got = _torch_sample(vol, theta, A.SIZE, "bilinear", padding_mode)
    err = float(np.abs(got - ref["value"]).max())
    outside = float(ref["outside"].mean())
    print(f"{padding_mode}: trilinear referee vs grid_sample: max |diff| {err:.2e}; voxels with a tap outside: {outside:.1%}")
    assert err <= 1e-5                                                # fp32 grid + fp32 sums of values in [0, 1)
    if padding_mode == "zeros":
        assert outside >= 0.10
    # nearest: torch's fp32 coordinate may round the other way within eps of k + 0.5; compare where the referee is sure
    i, ok = A.indices(theta, A.SIZE, A.CT_SHAPE)
    near = np.rint(i)
    sure = np.ones(A.SIZE, bool)
    inside = ok.copy()
    for a in range(3):
        sure &= np.abs(i[a] - np.floor(i[a]) - 0.5) > A.CT_SHAPE[a] * A.EPS
        if padding_mode == "border":
            near[a] = np.clip(near[a], 0, A.CT_SHAPE[a] - 1)
        else:
            inside &= (near[a] >= 0) & (near[a] <= A.CT_SHAPE[a] - 1)
    k = [np.clip(near[a], 0, A.CT_SHAPE[a] - 1).astype(np.int64) for a in range(3)]
    want = np.where(inside, lab[k[0], k[1], k[2]], 0.0)
    got = _torch_sample(lab, theta, A.SIZE, "nearest", padding_mode)
    assert sure.mean() >= 1 - A.MAX_EXCLUDED
    assert np.array_equal(got[sure], want[sure])
    # ... and sample_label is that rule followed by the loader's lookup
    raw = A.VALUES[g.integers(0, len(A.VALUES), size=A.CT_SHAPE)].astype(np.int16)
    sl = A.sample_label(raw, theta, A.SIZE, padding_mode)
    via = _torch_sample(raw.astype(np.float32), theta, A.SIZE, "nearest", padding_mode)
    cls = np.where(via == 0, 0, 255).astype(np.uint8)
    for j, v in enumerate(R.MMWHS_LABEL_VALUES):
        cls[via == v] = j + 1
    assert np.array_equal(sl["cls"][sl["sure"]], cls[sl["sure"]]) and np.array_equal(sl["sure"], sure)


def test_referee_edge_rules():
    vol = np.arange(1, 25, dtype=np.float32).reshape(2, 3, 4)
    lab = np.full((2, 3, 4), 205, np.int16)
    for bad in (np.nan, np.inf, -np.inf):
        theta = A.IDENTITY.copy()
        theta[1, 3] = bad
        for pad in ("zeros", "border"):
            assert not A.sample_image(vol, theta, (3, 3, 3), pad)["value"].any()
            sl = A.sample_label(lab, theta, (3, 3, 3), pad)
            assert not sl["cls"].any() and sl["sure"].all()
    far = A.IDENTITY.copy()
    far[0, 3] = 1e30
    assert not A.sample_image(vol, far, (3, 3, 3), "zeros")["value"].any()
    assert np.array_equal(A.sample_image(vol, far, (2, 3, 4), "border")["value"], np.broadcast_to(vol[:, :, 3:], (2, 3, 4)))
    same = A.sample_image(vol, A.IDENTITY, (2, 3, 4), "border")           # identity at the array's own size: the array
    assert np.array_equal(same["value"], vol) and not same["outside"].any()
    assert np.array_equal(A.sample_label(lab, A.IDENTITY, (2, 3, 4), "zeros")["cls"], np.ones((2, 3, 4), np.uint8))
    # the re-orientation map is np.flip(axis 0).transpose(1, 0, 2)
    re = np.ascontiguousarray(np.flip(vol, 0).transpose(1, 0, 2))
    assert np.array_equal(A.sample_image(vol, A.MR_REORIENT, re.shape, "border")["value"], re)


def test_fp32_coordinates_meet_the_bound():
    """The kernel's evaluation order (csrc/affine_coords.h) restated in numpy float32 (fused multiply-adds emulated in float64,
    rounded once) against float64: within extent * 2^-20 on the case's maps."""
    samples, maps = A.case()
    worst = 0.0
    for theta in maps:
        for shape in (A.CT_SHAPE, A.MR_SHAPE):
            i64, _ = A.indices(theta, A.SIZE, shape)
            f = np.float32
            n = [(f(2 * np.arange(e) + 1) / f(e) - f(1)).astype(np.float32) for e in A.SIZE]          # z, y, x
            nz, ny, nx = n[0][:, None, None], n[1][None, :, None], n[2][None, None, :]

            def fma(a, b, c):
                return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)
            for a, row in ((2, 0), (1, 1), (0, 2)):                                                    # axis x <- row 0 ...
                r = theta[row]
                s = fma(r[0], nx, fma(r[1], ny, fma(r[2], nz, r[3])))
                i32 = fma(s + f(1), f(shape[a]), f(-1)) * f(0.5)
                worst = max(worst, float(np.abs(i32.astype(np.float64) - i64[a]).max() / (shape[a] * A.EPS)))
    print(f"fp32 coordinate error: at most {worst:.3f} eps_axis")
    assert worst <= 1.0


@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
def test_the_seed_of_the_gpu_tests_meets_their_conditions(padding_mode):
    samples, maps = A.case()
    refs = A.case_reference(padding_mode)
    excluded = float(np.mean([1.0 - r["label"]["sure"].mean() for r in refs]))
    worst = max(float(1.0 - r["label"]["sure"].mean()) for r in refs)
    print(f"{padding_mode}: label voxels excluded: mean {excluded:.2e}, worst sample {worst:.2e}")
    assert worst <= A.MAX_EXCLUDED
    for b, r in enumerate(refs):                                      # crop_indexes: no voxel whose `!= 0` is in doubt
        for c, (p, shape) in enumerate(zip(r["planes"], (A.CT_SHAPE, A.MR_SHAPE))):
            v = np.abs(p["value"])
            assert not ((v > 0) & (v <= A.error_term(p, shape))).any(), (b, c)
    if padding_mode == "zeros":
        share = float(np.mean([p["outside"].mean() for r in refs for p in r["planes"]]))
        print(f"zeros: voxels with a tap outside the array: {share:.1%}")
        assert share >= 0.10
        assert any(not np.array_equal(r["crop"], [[0, s] for s in A.SIZE]) for r in refs)     # some crop box is not the full grid


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, affine
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(affine.SIGNATURES) == {"micf_volume_loader_affine_workspace", "micf_volume_loader_affine"}
    assert affine.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert affine.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {affine.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in affine.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert set(affine.INT64_RETURNS) <= set(d)
    norm = abi_header.parse_header("micformer_normalise.h")["micf_volume_loader_norm"][1]
    assert d["micf_volume_loader_affine"][1] == norm[:-1] + "pii" + norm[-1]      # the normaliser's arguments, then the three
    assert abi_header.defines(HEADER, "MICF_PAD_") == {"MICF_PAD_ZEROS": affine.PAD_ZEROS, "MICF_PAD_BORDER": affine.PAD_BORDER}
    assert affine.PADDING_MODES == {"zeros": 0, "border": 1}
    assert '#include "micformer_normalise.h"' in open(os.path.join(abi_header.INCLUDE, HEADER)).read()
    build = abi_header.build_module()
    assert "volume_affine.hip" in build.SOURCES


def test_table_is_disjoint_from_the_others():
    from micformer_amd import affine
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(affine.SIGNATURES) & set(other), module


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.affine import lib
    a = lib.micf_volume_loader_affine_workspace(1)
    assert a == lib.micf_volume_loader_affine_workspace(1) and a > 0 and a % 256 == 0
    assert a == lib.micf_volume_loader_norm_workspace(1) and lib.micf_volume_loader_affine_workspace(9) >= 9 * (a - 256)
    assert lib.micf_volume_loader_affine_workspace(0) == -1 and lib.micf_volume_loader_affine_workspace(-2) == -1


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


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd import affine, loader
    lib = affine.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)
    ws = lib.micf_volume_loader_affine_workspace(1)

    def call(sample=None, B=1, size=(16, 16, 16), values=vals, nvals=7, modes=(0, 0), p=(1.0, 99.0), workspace=fake, ws_bytes=ws,
             image=fake, label_map=fake, crop=fake, stats=None, theta=fake, per_modality=0, pad=0):
        s = sample if sample is not None else _sample(loader)
        return lib.micf_volume_loader_affine(ctypes.addressof(s), B, *size, None if values is None else ctypes.addressof(values),
                                             nvals, modes[0], modes[1], p[0], p[1], workspace, ws_bytes, image, label_map, crop,
                                             stats, theta, per_modality, pad, None)

    assert call(theta=None) == EINVAL
    assert call(theta=fake + 2) == EINVAL                             # float32 alignment
    for pad in (-1, 2, 7):
        assert call(pad=pad) == EINVAL
    for flag in (-1, 2, 24):
        assert call(per_modality=flag) == EINVAL
    # ... the normaliser's checks
    for modes in [(3, 0), (0, -1), (7, 7)]:
        assert call(modes=modes) == EINVAL
    for p in [(-0.5, 99.0), (50.0, 50.0), (float("nan"), 99.0)]:
        assert call(p=p) == EINVAL
    assert call(stats=fake + 4) == EINVAL
    # ... and the loader's
    assert call(B=0) == EINVAL
    assert call(size=(16, 0, 16)) == EINVAL
    assert call(workspace=None) == EINVAL
    assert call(workspace=fake + 64) == EINVAL
    assert call(ws_bytes=ws - 1) == EINVAL
    assert call(image=None) == EINVAL
    assert call(crop=None) == EINVAL
    assert call(label_map=None) == EINVAL
    assert call(_sample(loader, label=None)) == EINVAL
    assert call(_sample(loader, ct=None)) == EINVAL
    assert call(_sample(loader, ct_shape=(8, 0, 8))) == EINVAL
    assert call(values=(ctypes.c_int32 * 3)(5, 7, 5), nvals=3) == EINVAL
    assert call(_sample(loader, ct_dtype=loader.DTYPE_I32)) == EUNSUP
    assert call(_sample(loader, mr_shape=(8, 2049, 8))) == EUNSUP
    assert call(size=(512, 512, 513)) == EUNSUP


def test_python_front_end_rejects_before_the_device():
    """Every argument error of the two keywords, raised with CPU tensors in hand: the keyword checks come before the first look at
    a sample's device (a correct call with CPU tensors fails later, on that check)."""
    from micformer_amd import affine, loader
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    ok = torch.zeros(1, 3, 4)
    for bad in [np.zeros((1, 3, 4), np.float32), [[0.0] * 4] * 3, 1.0, torch.zeros(1, 3, 4, dtype=torch.float64),
                torch.zeros(1, 3, 4, dtype=torch.float16), torch.zeros(1, 3, 4, dtype=torch.int32)]:
        with pytest.raises(TypeError, match="affine"):
            loader.load_batch([(ct, ct, None)], affine=bad)
        with pytest.raises(TypeError, match="affine"):
            loader.load_pair(ct, ct, affine=bad)
        with pytest.raises(TypeError, match="affine"):               # TypeError before ValueError
            loader.load_batch([(ct, ct, None)], affine=bad, padding_mode="reflect")
    for bad in [None, 0, ("zeros",), b"zeros"]:
        with pytest.raises(TypeError, match="padding_mode"):
            loader.load_batch([(ct, ct, None)], affine=ok, padding_mode=bad)
    for bad in ["reflection", "reflect", "ZEROS", ""]:
        with pytest.raises(ValueError, match="padding_mode"):
            loader.load_batch([(ct, ct, None)], affine=ok, padding_mode=bad)
        with pytest.raises(ValueError, match="padding_mode"):
            loader.load_pair(ct, ct, affine=ok[0], padding_mode=bad)
    for bad in [torch.zeros(3, 4), torch.zeros(1, 4, 3), torch.zeros(1, 3, 3, 4), torch.zeros(1, 1, 3, 4), torch.zeros(1, 2, 2, 3, 4),
                torch.zeros(12)]:
        with pytest.raises(ValueError, match="affine must have shape"):
            loader.load_batch([(ct, ct, None)], affine=bad)
    for bad in [torch.zeros(1, 3, 4), torch.zeros(4), torch.zeros(2, 2, 3, 4), torch.zeros(3, 3)]:
        with pytest.raises(ValueError, match="affine"):
            loader.load_pair(ct, ct, affine=bad)
    for bad in [torch.zeros(2, 3, 4), torch.zeros(3, 2, 3, 4)]:       # B mismatch
        with pytest.raises(ValueError, match="affine holds maps for"):
            loader.load_batch([(ct, ct, None)], affine=bad)
    with pytest.raises(ValueError, match="affine must be a CUDA"):    # device
        loader.load_batch([(ct, ct, None)], affine=ok)
    with pytest.raises(ValueError, match="affine must be a CUDA"):
        loader.load_pair(ct, ct, affine=torch.zeros(2, 3, 4), padding_mode="border")
    # padding_mode is read only with affine; without it today's path goes on to the device check
    with pytest.raises(ValueError, match="CUDA"):
        loader.load_pair(ct, ct, padding_mode="anything")
    assert affine.padding("zeros") == 0 and affine.padding("border") == 1
    import inspect

    from micformer_amd import restore
    assert "affine" not in inspect.signature(restore.segment_pair).parameters      # inference is not augmented
    for fn in (loader.load_batch, loader.load_pair):
        assert list(inspect.signature(fn).parameters)[-2:] == ["affine", "padding_mode"]


def test_contiguity_is_checked():
    from micformer_amd import affine

    class Fake:                                                       # the metadata of a non-contiguous device tensor
        shape, is_cuda = (2, 3, 4), True

        @staticmethod
        def is_contiguous():
            return False
    with pytest.raises(ValueError, match="contiguous"):
        affine.maps(Fake, 2)
    Fake.is_contiguous = staticmethod(lambda: True)
    assert affine.maps(Fake, 2) == 0
    Fake.shape = (2, 2, 3, 4)
    assert affine.maps(Fake, 2) == 1


# ---- draw_affine ------------------------------------------------------------------------------------------------------------

def test_draw_affine():
    from micformer_amd.affine import draw_affine
    a = draw_affine(5, generator=torch.Generator().manual_seed(3))
    b = draw_affine(5, generator=torch.Generator().manual_seed(3))
    c = draw_affine(5, generator=torch.Generator().manual_seed(4))
    assert a.dtype == torch.float32 and tuple(a.shape) == (5, 3, 4) and a.device.type == "cpu" and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len({tuple(m.flatten().tolist()) for m in a}) == 5         # a different map per sample
    eye = torch.from_numpy(A.IDENTITY)
    assert torch.equal(draw_affine(4, prob=0.0, generator=torch.Generator().manual_seed(1)), eye.expand(4, 3, 4))
    some = draw_affine(64, prob=0.5, generator=torch.Generator().manual_seed(2))
    n_id = sum(bool(torch.equal(m, eye)) for m in some)
    assert 12 <= n_id <= 52
    # ranges: shifts within +-translate voxels = +-2 t / extent normalised; factors within 1 +- scale (cubic grid: column norms)
    wide = draw_affine(200, size=(64, 64, 64), rotate=0.3, scale=0.15, translate=(8, 4, 2), generator=torch.Generator().manual_seed(5))
    assert (wide[:, 0, 3].abs() <= 2 * 2 / 64 + 1e-6).all() and (wide[:, 1, 3].abs() <= 2 * 4 / 64 + 1e-6).all()
    assert (wide[:, 2, 3].abs() <= 2 * 8 / 64 + 1e-6).all() and wide[:, 2, 3].abs().max() > 2 * 4 / 64
    norms = wide[:, :, :3].double().norm(dim=1)
    assert (norms >= 0.85 - 1e-6).all() and (norms <= 1.15 + 1e-6).all() and norms.max() > 1.1 and norms.min() < 0.9
    # rigid: scale = translate = 0 on a cubic grid gives orthonormal blocks of determinant 1
    rigid = draw_affine(6, size=(32, 32, 32), scale=0, translate=0, generator=torch.Generator().manual_seed(6))[:, :, :3].double()
    assert torch.allclose(rigid @ rigid.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(6, 3, 3), atol=1e-6)
    assert torch.allclose(torch.linalg.det(rigid), torch.ones(6, dtype=torch.float64), atol=1e-6)
    assert not torch.allclose(rigid, torch.eye(3, dtype=torch.float64).expand(6, 3, 3), atol=1e-3)
    assert not draw_affine(6, scale=0, translate=0, generator=torch.Generator().manual_seed(6))[:, :, 3].any()
    # a non-cubic grid: orthonormal only after the conjugation by N = diag(W, H, D) / 2 is undone
    size = (24, 20, 28)
    skew = draw_affine(6, size=size, scale=0, translate=0, generator=torch.Generator().manual_seed(6))[:, :, :3].double()
    assert not torch.allclose(skew @ skew.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(6, 3, 3), atol=1e-3)
    n = torch.tensor([size[2], size[1], size[0]], dtype=torch.float64) / 2
    back = torch.diag(n) @ skew @ torch.diag(1 / n)
    assert torch.allclose(back @ back.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(6, 3, 3), atol=1e-6)
    assert torch.allclose(back, rigid, atol=1e-6)                     # the same draws, the same rotation in voxel space
    # per_modality: composed after the draw, applied first to the output coordinate
    pm = np.stack([A.IDENTITY, A.MR_REORIENT])
    pm[1, :, 3] = (0.1, -0.2, 0.05)
    base = draw_affine(3, generator=torch.Generator().manual_seed(7)).double()
    both = draw_affine(3, per_modality=pm, generator=torch.Generator().manual_seed(7)).double()
    assert tuple(both.shape) == (3, 2, 3, 4) and torch.allclose(both[:, 0], base, atol=1e-6)
    p = torch.from_numpy(pm[1]).double()
    nvec = torch.tensor([0.3, -0.7, 0.2, 1.0], dtype=torch.float64)
    for b in range(3):
        inner = torch.cat([p @ nvec, torch.ones(1, dtype=torch.float64)])
        assert torch.allclose(both[b, 1] @ nvec, base[b] @ inner, atol=1e-5)
    assert "unpinned" in draw_affine.__doc__ and "MONAI" in draw_affine.__doc__
    with pytest.raises(ValueError):
        draw_affine(0)
    with pytest.raises(ValueError):
        draw_affine(2, prob=1.5)
    with pytest.raises(ValueError):
        draw_affine(2, rotate=(0.1, 0.2))
    with pytest.raises(ValueError):
        draw_affine(2, per_modality=np.zeros((3, 4)))
    with pytest.raises(TypeError):
        draw_affine(2.0)
    with pytest.raises(TypeError):
        draw_affine(2, translate="far")


# ---- the device code and the host program -------------------------------------------------------------------------------------------

def test_volume_affine_device_code_uses_no_scratch():
    sizes, asm, flags = abi_header.device_asm("volume_affine.hip")
    assert not any("fast-math" in f or "-Ofast" in f for f in flags)     # the normalisers need the IEEE divide
    assert sum("affine_resample_kernel" in k for k in sizes) == 1 and all(v == 0 for v in sizes.values()), sizes
    assert "v_div_fixup_f32" in asm and "v_fma_f32" in asm
    assert "global_atomic_add_f32" not in asm and "global_atomic_add_f64" not in asm       # integer maxima and counts only


def test_coordinate_functions_keep_every_index_in_range(tmp_path):
    """tests/affine_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "affine_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "affine_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every index in range" in r.stdout
