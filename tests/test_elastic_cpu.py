"""CPU checks of the loader's elastic resample: the float64 referee (tests/elastic_ref.py) against F.interpolate,
scipy.ndimage.map_coordinates and F.grid_sample, the kernel's fp32 coordinate order against the bound the GPU tests use, the seed of
the GPU tests against the conditions those tests rely on, include/micformer_elastic.h against the ctypes table of
micformer_amd/elastic.py and the built library, argument errors caught before any launch, draw_elastic, the compiled device code's
scratch use, and the host program tests/elastic_index_main.cpp (csrc/elastic_coords.h under the address and undefined-behaviour
sanitizers: a stand-alone program, nothing is preloaded)."""
import ctypes
import importlib
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_header
import affine_ref as A
import elastic_ref as E
import loader_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_elastic.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "restore", "postprocess", "surface")
GRIDS = ((5, 4, 6), E.SIZE, (2, 2, 2), (7, 7, 7))


# ---- the referee ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS, ids=str)
def test_linear_field_is_f_interpolate_with_aligned_corners(grid):
    field = np.random.default_rng(8101).uniform(-0.12, 0.12, (3,) + grid).astype(np.float32)
    want = F.interpolate(torch.from_numpy(field.astype(np.float64))[None], size=E.SIZE, mode="trilinear", align_corners=True)[0].numpy()
    err = float(np.abs(E.displacement(field, E.SIZE, "linear") - want).max())
    print(f"grid {grid}: linear u vs F.interpolate: max |diff| {err:.2e}")
    assert err <= 1e-12
    if grid == E.SIZE:                                                # one vector per output voxel
        assert np.array_equal(E.displacement(field, E.SIZE, "linear"), field.astype(np.float64))


@pytest.mark.parametrize("grid", GRIDS, ids=str)
def test_cubic_field_is_map_coordinates_without_prefilter(grid):
    ndimage = pytest.importorskip("scipy.ndimage")
    field = np.random.default_rng(8102).uniform(-0.12, 0.12, (3,) + grid).astype(np.float32)
    p = np.meshgrid(*[np.arange(o) * (g - 1) / (o - 1) for o, g in zip(E.SIZE, grid)], indexing="ij")
    want = np.stack([ndimage.map_coordinates(field[c].astype(np.float64), p, order=3, mode="nearest", prefilter=False) for c in range(3)])
    got = E.displacement(field, E.SIZE, "cubic")
    err = float(np.abs(got - want).max())
    print(f"grid {grid}: cubic u vs map_coordinates: max |diff| {err:.2e}")
    assert err <= 1e-12
    if min(grid) > 2:                                                 # approximates the control values, does not interpolate them
        assert np.abs(got[:, ::E.SIZE[0] - 1, ::E.SIZE[1] - 1, ::E.SIZE[2] - 1] - field[:, ::grid[0] - 1, ::grid[1] - 1, ::grid[2] - 1]).max() > 1e-3


def test_single_voxel_axes_sit_on_the_first_control_point():
    field = np.random.default_rng(8103).uniform(-0.12, 0.12, (3, 3, 4, 2)).astype(np.float32)
    u = E.displacement(field, (1, 1, 1), "linear")
    assert np.array_equal(u[:, 0, 0, 0], field[:, 0, 0, 0].astype(np.float64))


def _torch_sample(vol, u, theta, size, mode, padding_mode):
    """F.grid_sample on a torch-built grid: the identity affine_grid plus u, then theta; all in float64."""
    t = torch.from_numpy(np.ascontiguousarray(vol, np.float64))[None, None]
    eye = torch.from_numpy(A.IDENTITY.astype(np.float64))[None]
    grid = F.affine_grid(eye, (1, 1) + tuple(size), align_corners=False) + torch.from_numpy(u).permute(1, 2, 3, 0)[None]
    th = torch.from_numpy((A.IDENTITY if theta is None else np.asarray(theta, np.float32)).astype(np.float64))
    grid = grid @ th[:, :3].T + th[:, 3]
    return F.grid_sample(t, grid, mode=mode, padding_mode=padding_mode, align_corners=False)[0, 0].numpy()


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
def test_referee_matches_grid_sample(padding_mode, mode):
    g = np.random.default_rng(8104)
    vol = g.random(A.CT_SHAPE, dtype=np.float32)
    theta = A.draw_maps(g, 1)[0]
    field = g.uniform(-0.12, 0.12, (3, 5, 4, 6)).astype(np.float32)
    u = E.displacement(field, E.SIZE, mode)
    for th in (theta, None):
        i, ok = E.indices(th, u, E.SIZE, A.CT_SHAPE)
        assert ok.all()
        ref = E.sample_image(vol, i, ok, padding_mode)
        err = float(np.abs(_torch_sample(vol, u, th, E.SIZE, "bilinear", padding_mode) - ref["value"]).max())
        print(f"{padding_mode} {mode} map {th is not None}: trilinear referee vs grid_sample: max |diff| {err:.2e}; "
              f"voxels with a tap outside: {float(ref['outside'].mean()):.1%}")
        assert err <= 1e-9                                            # float64 on both sides
        raw = A.VALUES[g.integers(0, len(A.VALUES), size=A.CT_SHAPE)].astype(np.int16)
        sl = E.sample_label(raw, i, ok, padding_mode)
        via = _torch_sample(raw, u, th, E.SIZE, "nearest", padding_mode)
        cls = np.where(via == 0, 0, 255).astype(np.uint8)
        for j, v in enumerate(R.MMWHS_LABEL_VALUES):
            cls[via == v] = j + 1
        assert sl["sure"].mean() >= 1 - E.MAX_EXCLUDED
        assert np.array_equal(sl["cls"][sl["sure"]], cls[sl["sure"]])
    # a zero field is affine_ref's referee
    zero = E.displacement(np.zeros_like(field), E.SIZE, mode)
    i, ok = E.indices(theta, zero, E.SIZE, A.CT_SHAPE)
    assert np.array_equal(E.sample_image(vol, i, ok, padding_mode)["value"], A.sample_image(vol, theta, E.SIZE, padding_mode)["value"])


def test_referee_non_finite_control_points_reach_their_taps_only():
    field = np.zeros((3, 5, 4, 6), np.float32)
    field[1, 2, 1, 3] = np.nan
    for mode, reach in (("linear", 1), ("cubic", 2)):
        u = E.displacement(field, E.SIZE, mode)
        bad = np.isnan(u)
        assert bad[1].any() and not bad[0].any() and not bad[2].any() and not bad[1].all()
        z = np.nonzero(bad[1].any(axis=(1, 2)))[0]
        lo, hi = (2 - reach) * (E.SIZE[0] - 1) / 4, (2 + reach) * (E.SIZE[0] - 1) / 4
        assert z.min() >= lo - 1e-9 and z.max() <= hi + 1e-9 and len(z) >= (hi - lo) - 2       # the planes of its 2 | 4 cells
        i, ok = E.indices(None, u, E.SIZE, A.CT_SHAPE)
        assert np.array_equal(~ok, bad[1])
        vol = np.ones(A.CT_SHAPE, np.float32)
        assert not E.sample_image(vol, i, ok, "border")["value"][~ok].any() and E.sample_image(vol, i, ok, "border")["value"][ok].all()


# ---- the coordinate bound -----------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def _fp32_axis(out, g, mode):
    """csrc/elastic_coords.h's control_cell + linear_taps / cubic_taps in float32 -> (address [out, T], weight float32 [out, T])."""
    f = np.float32
    o = np.arange(out, dtype=np.int64)
    k = (o * (g - 1)) // (out - 1)
    t = ((o * (g - 1)) % (out - 1)).astype(np.float32) / f(out - 1)
    if mode == "linear":
        first, w = k, [f(1) - t, t]
    else:
        u, sixth = f(1) - t, f(1) / f(6)
        first = k - 1
        w = [u * u * u * sixth, _fma(t * t, _fma(f(0.5), t, f(-1)), f(2) / f(3)),
             _fma(t, _fma(t, _fma(f(-0.5), t, f(0.5)), f(0.5)), sixth), t * t * t * sixth]
    assert all(x.dtype == np.float32 for x in w)
    return np.stack([np.clip(first + j, 0, g - 1) for j in range(len(w))], 1), np.stack(w, 1)


def _fp32_displacement(field, size, mode):
    """micf_elastic::interpolate's order: x innermost, one fused multiply-add per tap, per finished row and per finished plane."""
    (az, wz), (ay, wy), (ax, wx) = (_fp32_axis(o, g, mode) for o, g in zip(size, field.shape[1:]))
    out = []
    for c in range(3):
        acc = np.zeros(size, np.float32)
        for jz in range(az.shape[1]):
            plane = np.zeros(size, np.float32)
            for jy in range(ay.shape[1]):
                r = np.zeros(size, np.float32)
                for jx in range(ax.shape[1]):
                    r = _fma(wx[None, None, :, jx], field[c][az[:, jz][:, None, None], ay[:, jy][None, :, None], ax[:, jx][None, None, :]], r)
                plane = _fma(wy[None, :, None, jy], r, plane)
            acc = _fma(wz[:, None, None, jz], plane, acc)
        out.append(acc)
    return out                                                        # x, y, z


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_fp32_coordinates_meet_the_bound(name, mode):
    """The kernel's evaluation order (csrc/elastic_coords.h, then csrc/affine_coords.h) restated in numpy float32 (fused
    multiply-adds emulated in float64, rounded once) against float64: within extent * 2^-19 on the cases of the GPU tests."""
    samples, theta, fields = E.case(name)
    f = np.float32
    worst = 0.0
    n = [(f(2 * np.arange(e) + 1) / f(e) - f(1)).astype(np.float32) for e in E.SIZE]                  # z, y, x
    for b in range(len(samples)):
        assert np.abs(fields[b]).max() <= 0.25
        ux, uy, uz = _fp32_displacement(fields[b], E.SIZE, mode)
        nz, ny, nx = n[0][:, None, None] + uz, n[1][None, :, None] + uy, n[2][None, None, :] + ux
        assert nx.dtype == np.float32
        u64 = E.displacement(fields[b], E.SIZE, mode)
        th = A.IDENTITY if theta is None else theta[b]
        for t, shape in ((th, A.CT_SHAPE), (th, A.MR_SHAPE)) if th.ndim == 2 else ((th[0], A.CT_SHAPE), (th[1], A.MR_SHAPE)):
            i64, _ = E.indices(t, u64, E.SIZE, shape)
            for a, row in ((2, 0), (1, 1), (0, 2)):                                                    # axis x <- row 0 ...
                r = t[row]
                s = _fma(r[0], nx, _fma(r[1], ny, _fma(r[2], nz, r[3])))
                i32 = _fma(s + f(1), f(shape[a]), f(-1)) * f(0.5)
                worst = max(worst, float(np.abs(i32.astype(np.float64) - i64[a]).max() / (shape[a] * E.EPS)))
    print(f"{name} {mode}: fp32 coordinate error: at most {worst:.3f} eps_axis (eps_axis = extent * 2^-19)")
    assert worst <= 1.0


# ---- the seed of the GPU tests -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
def test_the_seed_of_the_gpu_tests_meets_their_conditions(padding_mode, mode):
    shares = []
    for name in sorted(E.CASES):
        refs = E.case_reference(name, mode, padding_mode)
        worst = max(float(1.0 - r["label"]["sure"].mean()) for r in refs)
        print(f"{name} {padding_mode} {mode}: label voxels excluded, worst sample: {worst:.2e}")
        assert worst <= E.MAX_EXCLUDED
        for b, r in enumerate(refs):                                  # crop_indexes: no voxel whose `!= 0` is in doubt
            for c, (p, shape) in enumerate(zip(r["planes"], (A.CT_SHAPE, A.MR_SHAPE))):
                v = np.abs(p["value"])
                assert not ((v > 0) & (v <= E.error_term(p, shape))).any(), (name, b, c)
        if name == "nine":
            shares = [p["outside"].mean() for r in refs for p in r["planes"]]
            assert len(np.unique(np.concatenate([r["label"]["cls"].ravel() for r in refs]))) == 9     # 0, the seven classes, 255
    if padding_mode == "zeros":
        print(f"zeros {mode}: voxels of the batch of nine with a tap outside the array: {float(np.mean(shares)):.1%}")
        assert np.mean(shares) >= 0.10


def test_the_cases_cover_both_chunks_and_both_map_layouts():
    nine, dense, minimal = (E.case(n) for n in ("nine", "dense", "minimal"))
    assert len(nine[0]) == 9 and nine[1].shape == (9, 3, 4) and nine[2].shape == (9, 3, 5, 4, 6)
    assert dense[1].shape == (2, 2, 3, 4) and dense[2].shape == (2, 3) + E.SIZE and not np.array_equal(dense[1][:, 0], dense[1][:, 1])
    assert minimal[1] is None and minimal[2].shape == (2, 3, 2, 2, 2)
    for _, _, fields in (nine, dense, minimal):
        assert fields.dtype == np.float32 and 0.1 < np.abs(fields).max() <= E.AMPLITUDE


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, elastic
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(elastic.SIGNATURES) == {"micf_volume_loader_elastic_workspace", "micf_volume_loader_elastic"}
    assert elastic.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert elastic.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {elastic.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in elastic.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert set(elastic.INT64_RETURNS) <= set(d)
    aff = abi_header.parse_header("micformer_affine.h")["micf_volume_loader_affine"][1]
    assert d["micf_volume_loader_elastic"][1] == aff[:-1] + "piiii" + aff[-1]         # the affine entry's arguments, then the five
    assert abi_header.defines(HEADER, "MICF_FIELD_") == {"MICF_FIELD_LINEAR": elastic.FIELD_LINEAR, "MICF_FIELD_CUBIC": elastic.FIELD_CUBIC}
    assert elastic.FIELD_INTERPOLATIONS == {"linear": 0, "cubic": 1}
    assert '#include "micformer_affine.h"' in open(os.path.join(abi_header.INCLUDE, HEADER)).read()
    assert "volume_elastic.hip" in abi_header.build_module().SOURCES


def test_table_is_disjoint_from_the_others():
    from micformer_amd import elastic
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(elastic.SIGNATURES) & set(other), module


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.elastic import lib
    a = lib.micf_volume_loader_elastic_workspace(1)
    assert a == lib.micf_volume_loader_elastic_workspace(1) and a > 0 and a % 256 == 0
    assert a == lib.micf_volume_loader_affine_workspace(1)
    assert lib.micf_volume_loader_elastic_workspace(9) == lib.micf_volume_loader_affine_workspace(9)
    assert lib.micf_volume_loader_elastic_workspace(0) == -1 and lib.micf_volume_loader_elastic_workspace(-2) == -1


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
    from micformer_amd import elastic, loader
    lib = elastic.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)
    ws = lib.micf_volume_loader_elastic_workspace(1)

    def call(sample=None, B=1, size=(16, 16, 16), values=vals, nvals=7, modes=(0, 0), p=(1.0, 99.0), workspace=fake, ws_bytes=ws,
             image=fake, label_map=fake, crop=fake, stats=None, theta=fake, per_modality=0, pad=0, field=fake, grid=(7, 7, 7), interp=0):
        s = sample if sample is not None else _sample(loader)
        return lib.micf_volume_loader_elastic(ctypes.addressof(s), B, *size, None if values is None else ctypes.addressof(values),
                                              nvals, modes[0], modes[1], p[0], p[1], workspace, ws_bytes, image, label_map, crop,
                                              stats, theta, per_modality, pad, field, *grid, interp, None)

    assert call(field=None) == EINVAL
    assert call(field=fake + 2) == EINVAL                             # float32 alignment
    for grid in [(1, 7, 7), (7, 0, 7), (7, 7, -3), (1, 600, 7)]:      # (EINVAL before EUNSUPPORTED)
        assert call(grid=grid) == EINVAL
    for interp in (-1, 2, 3):
        assert call(interp=interp) == EINVAL
    for grid in [(513, 7, 7), (7, 7, 2048), (2, 1 << 20, 2)]:
        assert call(grid=grid) == EUNSUP
        assert call(grid=grid, theta=None) == EUNSUP
    assert call(grid=(513, 7, 7), B=0) == EINVAL
    # ... the affine entry's checks, where a map is given
    assert call(theta=fake + 2) == EINVAL
    for pad in (-1, 2, 7):
        assert call(pad=pad) == EINVAL
        assert call(pad=pad, theta=None) == EINVAL
    for flag in (-1, 2, 24):
        assert call(per_modality=flag) == EINVAL
    for modes in [(3, 0), (0, -1), (7, 7)]:
        assert call(modes=modes) == EINVAL
    for p in [(-0.5, 99.0), (50.0, 50.0), (float("nan"), 99.0)]:
        assert call(p=p) == EINVAL
    assert call(stats=fake + 4) == EINVAL
    # ... and the loader's, with and without a map
    for theta in (fake, None):
        assert call(B=0, theta=theta) == EINVAL
        assert call(size=(16, 0, 16), theta=theta) == EINVAL
        assert call(workspace=None, theta=theta) == EINVAL
        assert call(workspace=fake + 64, theta=theta) == EINVAL
        assert call(ws_bytes=ws - 1, theta=theta) == EINVAL
        assert call(image=None, theta=theta) == EINVAL
        assert call(crop=None, theta=theta) == EINVAL
        assert call(label_map=None, theta=theta) == EINVAL
        assert call(_sample(loader, label=None), theta=theta) == EINVAL
        assert call(_sample(loader, ct=None), theta=theta) == EINVAL
        assert call(_sample(loader, ct_shape=(8, 0, 8)), theta=theta) == EINVAL
        assert call(values=(ctypes.c_int32 * 3)(5, 7, 5), nvals=3, theta=theta) == EINVAL
        assert call(_sample(loader, ct_dtype=loader.DTYPE_I32), theta=theta) == EUNSUP
        assert call(_sample(loader, mr_shape=(8, 2049, 8)), theta=theta) == EUNSUP
        assert call(size=(512, 512, 513), theta=theta) == EUNSUP


def test_python_front_end_rejects_before_the_device():
    """Every argument error of the two keywords, raised with CPU tensors in hand: the keyword checks come before the first look at
    a sample's device (a correct call with CPU tensors fails later, on that check)."""
    from micformer_amd import elastic, loader, restore
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    ok = torch.zeros(1, 3, 2, 3, 4)
    theta = torch.zeros(1, 3, 4)
    for bad in [np.zeros((1, 3, 2, 2, 2), np.float32), [[0.0]], 1.0, torch.zeros(1, 3, 2, 2, 2, dtype=torch.float64),
                torch.zeros(1, 3, 2, 2, 2, dtype=torch.float16), torch.zeros(1, 3, 2, 2, 2, dtype=torch.int32)]:
        with pytest.raises(TypeError, match="displacement"):
            loader.load_batch([(ct, ct, None)], displacement=bad)
        with pytest.raises(TypeError, match="displacement"):
            loader.load_pair(ct, ct, displacement=bad)
        with pytest.raises(TypeError, match="displacement"):         # TypeError before ValueError
            loader.load_batch([(ct, ct, None)], displacement=bad, field_interpolation="nearest", padding_mode="reflect")
        with pytest.raises(TypeError, match="displacement"):
            loader.load_batch([(ct, ct, None)], displacement=bad, affine=torch.zeros(3, 3))
    for bad in [None, 0, 1, ("linear",), b"cubic"]:
        with pytest.raises(TypeError, match="field_interpolation"):
            loader.load_batch([(ct, ct, None)], displacement=ok, field_interpolation=bad)
        with pytest.raises(TypeError, match="field_interpolation"):  # ... before the ValueErrors of the other keywords
            loader.load_batch([(ct, ct, None)], displacement=torch.zeros(3), field_interpolation=bad, padding_mode="reflect")
        with pytest.raises(TypeError, match="field_interpolation"):
            loader.load_pair(ct, ct, displacement=torch.zeros(3), field_interpolation=bad, affine=torch.zeros(5))
    with pytest.raises(TypeError, match="affine"):
        loader.load_batch([(ct, ct, None)], displacement=torch.zeros(3), affine=theta.double())
    for bad in [None, 0]:
        with pytest.raises(TypeError, match="padding_mode"):         # padding_mode is read with a field alone
            loader.load_batch([(ct, ct, None)], displacement=torch.zeros(3), padding_mode=bad)
        with pytest.raises(TypeError, match="padding_mode"):
            loader.load_pair(ct, ct, displacement=torch.zeros(3), padding_mode=bad)
    for bad in ["bilinear", "trilinear", "LINEAR", "bspline", ""]:
        with pytest.raises(ValueError, match="field_interpolation"):
            loader.load_batch([(ct, ct, None)], displacement=ok, field_interpolation=bad)
        with pytest.raises(ValueError, match="field_interpolation"):
            loader.load_pair(ct, ct, displacement=ok[0], field_interpolation=bad)
    with pytest.raises(ValueError, match="padding_mode"):
        loader.load_batch([(ct, ct, None)], displacement=ok, padding_mode="reflect")
    for bad in [torch.zeros(3, 2, 3, 4), torch.zeros(1, 2, 2, 3, 4), torch.zeros(1, 4, 2, 3, 4), torch.zeros(1, 3, 2, 3), torch.zeros(24),
                torch.zeros(1, 1, 3, 2, 3, 4)]:
        with pytest.raises(ValueError, match="displacement must have shape"):
            loader.load_batch([(ct, ct, None)], displacement=bad)
    for bad in [torch.zeros(1, 3, 1, 3, 4), torch.zeros(1, 3, 2, 1, 4), torch.zeros(1, 3, 2, 2, 513), torch.zeros(1, 3, 2, 2, 0)]:
        with pytest.raises(ValueError, match="control grid"):
            loader.load_batch([(ct, ct, None)], displacement=bad)
    for bad in [torch.zeros(1, 3, 2, 3, 4), torch.zeros(3, 2, 3), torch.zeros(2, 2, 3, 4), torch.zeros(3, 1, 3, 4)]:
        with pytest.raises(ValueError, match="displacement"):
            loader.load_pair(ct, ct, displacement=bad)
    for bad in [torch.zeros(2, 3, 2, 3, 4), torch.zeros(3, 3, 2, 2, 2)]:      # B mismatch
        with pytest.raises(ValueError, match="displacement holds fields for"):
            loader.load_batch([(ct, ct, None)], displacement=bad)
    with pytest.raises(ValueError, match="displacement must be a CUDA"):      # device
        loader.load_batch([(ct, ct, None)], displacement=ok)
    with pytest.raises(ValueError, match="displacement must be a CUDA"):
        loader.load_pair(ct, ct, displacement=ok[0], field_interpolation="cubic", padding_mode="border")
    with pytest.raises(ValueError, match="affine must be a CUDA"):            # (the map's checks come first, as before)
        loader.load_batch([(ct, ct, None)], displacement=ok, affine=theta)
    # without a field nothing changes: neither keyword of the resample is read, and today's path goes on to the device check
    with pytest.raises(ValueError, match="CUDA"):
        loader.load_pair(ct, ct, padding_mode="anything")
    with pytest.raises(ValueError, match="ct must be a CUDA"):
        loader.load_pair(ct, ct, field_interpolation=7, padding_mode=None)
    with pytest.raises(ValueError, match="affine must be a CUDA"):
        loader.load_batch([(ct, ct, None)], affine=theta, field_interpolation="anything")
    assert elastic.interpolation("linear") == 0 and elastic.interpolation("cubic") == 1
    for fn in (loader.load_batch, loader.load_pair):
        assert list(inspect.signature(fn).parameters)[-4:] == ["displacement", "field_interpolation", "affine", "padding_mode"]
        assert inspect.signature(fn).parameters["displacement"].default is None
        assert inspect.signature(fn).parameters["field_interpolation"].default == "linear"
    for kw in ("displacement", "field_interpolation"):
        assert kw not in inspect.signature(restore.segment_pair).parameters      # inference is not augmented


def test_contiguity_is_checked():
    from micformer_amd import elastic

    class Fake:                                                       # the metadata of a non-contiguous device tensor
        shape, is_cuda = (2, 3, 5, 4, 6), True

        @staticmethod
        def is_contiguous():
            return False
    with pytest.raises(ValueError, match="contiguous"):
        elastic.fields(Fake, 2)
    Fake.is_contiguous = staticmethod(lambda: True)
    assert elastic.fields(Fake, 2) == (5, 4, 6)


# ---- draw_elastic -----------------------------------------------------------------------------------------------------------

def test_draw_elastic():
    from micformer_amd.elastic import draw_elastic
    a = draw_elastic(5, generator=torch.Generator().manual_seed(3))
    b = draw_elastic(5, generator=torch.Generator().manual_seed(3))
    c = draw_elastic(5, generator=torch.Generator().manual_seed(4))
    assert a.dtype == torch.float32 and tuple(a.shape) == (5, 3, 7, 7, 7) and a.device.type == "cpu" and a.is_contiguous()
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len({tuple(f.flatten().tolist()) for f in a}) == 5         # a different field per sample
    # units: +-magnitude voxels = +-2 magnitude / extent normalised, per component (x, y, z) <- (w, h, d)
    assert float(a.abs().max()) <= 2 * 5.0 / 128 and float(a.abs().max()) > 0.9 * 2 * 5.0 / 128
    wide = draw_elastic(40, size=(64, 96, 128), grid=(4, 5, 6), magnitude=(1.0, 2.0, 4.0), locked_borders=False,
                        generator=torch.Generator().manual_seed(5))
    assert tuple(wide.shape) == (40, 3, 4, 5, 6)
    for comp, (m, extent) in enumerate(((4.0, 128), (2.0, 96), (1.0, 64))):
        top = float(wide[:, comp].abs().max())
        assert 0.9 * 2 * m / extent < top <= 2 * m / extent, comp
    assert wide[:, :, 0].any() and wide[:, :, :, :, -1].any()
    # locked borders: the outermost control layer is zero, the inside is not
    for f in (a, draw_elastic(3, grid=(3, 4, 5), generator=torch.Generator().manual_seed(6))):
        assert not f[:, :, 0].any() and not f[:, :, -1].any() and not f[:, :, :, 0].any() and not f[:, :, :, -1].any()
        assert not f[:, :, :, :, 0].any() and not f[:, :, :, :, -1].any() and f[:, :, 1:-1, 1:-1, 1:-1].all()
    assert not draw_elastic(2, grid=(2, 7, 7)).any()                  # an axis of 2 points is all border
    # prob
    zero = draw_elastic(4, prob=0.0, generator=torch.Generator().manual_seed(1))
    assert torch.equal(zero.view(torch.int32), torch.zeros(4, 3, 7, 7, 7, dtype=torch.int32))         # exact +0.0
    some = draw_elastic(64, prob=0.5, generator=torch.Generator().manual_seed(2))
    assert 12 <= sum(not bool(f.any()) for f in some) <= 52
    # a magnitude of half the control spacing or more is rejected, per axis
    spacing = 127 / 6
    draw_elastic(1, magnitude=0.49 * spacing)
    for bad in (0.5 * spacing, 20.0, (1.0, 11.0, 1.0)):
        with pytest.raises(ValueError, match="half the control spacing"):
            draw_elastic(1, magnitude=bad)
    with pytest.raises(ValueError, match="half the control spacing"):
        draw_elastic(1, size=(16, 128, 128), grid=(7, 7, 7), magnitude=1.5)
    assert not draw_elastic(1, magnitude=0.0).any()
    doc = draw_elastic.__doc__
    assert "unpinned" in doc and "MONAI" in doc and "TorchIO" in doc and "defaults only" in doc
    with pytest.raises(ValueError):
        draw_elastic(0)
    with pytest.raises(ValueError):
        draw_elastic(2, prob=1.5)
    with pytest.raises(ValueError):
        draw_elastic(2, grid=(1, 7, 7))
    with pytest.raises(ValueError):
        draw_elastic(2, grid=(7, 7, 513))
    with pytest.raises(ValueError):
        draw_elastic(2, magnitude=(1.0, 2.0))
    with pytest.raises(ValueError):
        draw_elastic(2, magnitude=-1.0)
    with pytest.raises(TypeError):
        draw_elastic(2.0)
    with pytest.raises(TypeError):
        draw_elastic(2, magnitude="large")


@pytest.mark.parametrize("mode", E.MODES)
def test_default_draws_do_not_fold(mode):
    """At the defaults (128^3, a 7^3 grid, +-5 voxels) n -> n + u(n) keeps a positive finite-difference Jacobian determinant
    everywhere, in voxel units, for several seeds."""
    from micformer_amd.elastic import draw_elastic
    size = (128, 128, 128)
    low = np.inf
    for seed in (11, 12, 13):
        field = draw_elastic(1, generator=torch.Generator().manual_seed(seed))[0].numpy()
        u = E.displacement(field, size, mode, optimize=True).astype(np.float32)                        # (x, y, z), normalised
        pos = [np.arange(e, dtype=np.float32).reshape([-1 if a == ax else 1 for a in range(3)]) + u[2 - ax] * (e / 2.0)
               for ax, e in enumerate(size)]                          # voxel position on axis z, y, x
        inner = tuple(slice(0, e - 1) for e in size)
        J = [[np.diff(pos[i], axis=j)[inner] for j in range(3)] for i in range(3)]                    # forward differences
        det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])
               + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
        low = min(low, float(det.min()))
        assert np.isfinite(det).all()
    print(f"{mode}: smallest Jacobian determinant over three default draws: {low:.3f}")
    assert low > 0.0


# ---- the device code and the host program -------------------------------------------------------------------------------------------

def test_neither_resample_kernel_uses_scratch():
    sizes, _, _ = abi_header.device_asm("volume_elastic.hip")
    assert sum("elastic_resample_kernel" in k for k in sizes) == 1, sizes
    assert all(v == 0 for k, v in sizes.items() if "elastic_resample_kernel" in k), sizes
    sizes, _, _ = abi_header.device_asm("volume_affine.hip")
    assert sum("affine_resample_kernel" in k for k in sizes) == 1, sizes
    assert all(v == 0 for k, v in sizes.items() if "affine_resample_kernel" in k), sizes


def test_control_grid_functions_keep_every_tap_in_range(tmp_path):
    """tests/elastic_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "elastic_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "elastic_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every tap in range" in r.stdout
