"""CPU checks of the patch sampler's crop through a map.  The first group judges the judge: the numpy referee
(tests/patch_warp_ref.py) against torch's own F.grid_sample on the CPU, that its comparison catches the mistakes it must catch, and
that every case the GPU tests use leaves at most MAX_EXCLUDED of its label voxels uncompared.  The rest needs the feature:
include/micformer_patch_warp.h against the ctypes table of micformer_amd/patch_warp.py and the built library, argument errors caught
before any launch, the compiled device code's scratch use, and the host program tests/patch_warp_index_main.cpp (the coordinate code of
the kernel under the address and undefined-behaviour sanitizers: a stand-alone program, nothing is preloaded), whose printed results
are compared with the referee's."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_header
import elastic_ref as E
import normalise_ref as N
import patch_warp_ref as W
import patches_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_patch_warp.h"
NAMES = {"micf_patch_sample_warped"}
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "elastic", "intensity", "restore", "postprocess", "surface", "blend",
                "patches")


def _case(seed=9601, shape=(13, 17, 11), patch=(8, 6, 10), field=True):
    g = np.random.default_rng(seed)
    ct, mr = W.image(g, shape, np.int16), W.image(g, shape, np.float32)
    lab = W.VALUES[g.integers(0, len(W.VALUES), size=shape)].astype(np.int16)
    theta = W.generic_maps(g, 1, patch, rotate=0.4, shift=2.0)[0]
    fld = g.uniform(-0.12, 0.12, (3, 4, 3, 5)).astype(np.float32) if field else None
    return (ct, mr, lab), theta, fld


# ---- the referee against torch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
@pytest.mark.parametrize("mode", [None, "linear", "cubic"])
def test_referee_is_grid_sample_on_the_scan(padding_mode, mode):
    """The per-voxel scan index i as a normalised scan coordinate s' = (2 i + 1) / L - 1 fed to F.grid_sample(align_corners=False) on
    the normalised scan: bilinear for the image, nearest for the label (zeros padding on class + 1, so that 0 marks outside)."""
    sample, theta, fld = _case(field=mode is not None)
    draw = (0.0, 0, 0, 0.9, 0.1, 0.5)
    ref = W.sample(*sample, draw, (8, 6, 10), theta=theta, field=fld, mode=mode or "linear", padding_mode=padding_mode, pad_class=200)
    shape = sample[0].shape
    for c, plane in enumerate(ref["planes"]):
        i = plane["index"]
        grid = np.stack([(2.0 * i[2] + 1.0) / shape[2] - 1.0, (2.0 * i[1] + 1.0) / shape[1] - 1.0, (2.0 * i[0] + 1.0) / shape[0] - 1.0], -1)
        norm = torch.from_numpy(N.normalise(sample[c], "minmax").astype(np.float64))[None, None]
        got = F.grid_sample(norm, torch.from_numpy(grid)[None], mode="bilinear", padding_mode=padding_mode, align_corners=False)[0, 0]
        err = np.abs(got.numpy() - plane["value"])
        tol = 2.0 ** -23 * (plane["tapmax"] + plane["spread"] * max(shape)) + 1e-12          # float32 rounding, generously
        assert (err <= tol).all(), float((err - tol).max())
        assert plane["outside"].any() == (padding_mode == "zeros")
    i = ref["planes"][0]["index"]
    grid = np.stack([(2.0 * i[2] + 1.0) / shape[2] - 1.0, (2.0 * i[1] + 1.0) / shape[1] - 1.0, (2.0 * i[0] + 1.0) / shape[0] - 1.0], -1)
    cmap1 = torch.from_numpy(P.full_class_map(sample[2]).astype(np.float64) + 1.0)[None, None]
    near = F.grid_sample(cmap1, torch.from_numpy(grid)[None], mode="nearest", padding_mode="zeros", align_corners=False)[0, 0].numpy()
    want = np.where(near == 0, 200, near - 1).astype(np.uint8)
    sure = ref["label"]["sure"]
    assert sure.mean() > 0.99 and np.array_equal(want[sure], ref["label"]["cls"][sure])
    assert (ref["label"]["cls"] == 200).any() and len(np.unique(ref["label"]["cls"])) >= 9


def test_identity_map_is_the_plain_crop():
    """Without a map and a field the referee is patches_ref.sample: the same window, padding and pad_class."""
    sample, _, _ = _case()
    for padding_mode in ("zeros", "border"):
        for patch, draw in (((8, 4, 16), (0.0, 0, 0, 0.3, 0.9, 0.5)), ((16, 32, 8), (1.0, 0.4, 0.6, 0, 0, 0))):
            ref = W.sample(*sample, draw, patch, padding_mode=padding_mode, pad_class=255, exact=True)
            plain = P.sample(*sample, draw, patch, padding_mode=padding_mode, pad_class=255)
            assert np.array_equal(np.stack([p["value"] for p in ref["planes"]]), plain["image"].astype(np.float64))
            assert np.array_equal(ref["label"]["cls"], plain["label"]) and ref["label"]["sure"].all()
            assert np.array_equal(ref["origin"], plain["origin"]) and np.array_equal(ref["picked"], plain["picked"])


# ---- the comparison must catch these ---------------------------------------------------------------------------------------------

def _half_voxel(patch):
    """A translation by exactly half a voxel on every axis: every label index is a tie (exact in float32 on a power-of-two patch)."""
    theta = W.A.IDENTITY.copy()
    theta[:, 3] = [1.0 / patch[2], 1.0 / patch[1], 1.0 / patch[0]]
    return theta


@pytest.mark.parametrize("mutate,expect", [("o+half", "image"), ("o+half", "label"), ("theta_T", "image"), ("theta_T", "label"),
                                           ("zyx", "image"), ("zyx", "label"), ("half_up", "label"), ("class0", "label"),
                                           ("field_after", "image"), ("field_after", "label")])
def test_the_comparison_fails_for(mutate, expect):
    sample, theta, fld = _case()
    patch, kw = (8, 6, 10), dict(theta=theta, field=fld, mode="cubic", pad_class=255)
    if mutate == "half_up":                                           # only a tie tells the two roundings apart
        patch, kw = (8, 4, 16), dict(theta=_half_voxel((8, 4, 16)), pad_class=255, exact=True)
    draw = (0.0, 0, 0, 0.9, 0.1, 0.5)
    good = W.sample(*sample, draw, patch, **kw)
    assert W.compare(W.as_got(good), good)[0] == []
    bad = W.sample(*sample, draw, patch, mutate=mutate, **kw)
    names, info = W.compare(W.as_got(bad), good)
    assert expect in names, (mutate, names, info)
    if mutate in ("half_up", "class0"):
        assert "image" not in names


def test_cases_leave_few_label_voxels_uncompared():
    """The share of label voxels within eps of a rounding boundary, from the referee alone, for every case the GPU tests use; and the
    premises of the bound: |u| <= 0.25."""
    worst = 0.0
    for name in W.CASES:
        _, _, _, _, fields, _ = W.case(name)
        assert fields is None or float(np.abs(fields).max()) <= W.FIELD_AMPLITUDE
        for r in W.case_reference(name, "zeros"):
            worst = max(worst, 1.0 - float(r["label"]["sure"].mean()))
            for p in r["planes"]:
                assert np.isfinite(p["value"]).all()
    for r in W.extremes_reference("zeros"):
        worst = max(worst, 1.0 - float(r["label"]["sure"].mean()))
    print(f"worst excluded share {worst:.2e}")
    assert worst <= W.MAX_EXCLUDED
    for name in ("cubic", "dense"):
        patch, _, _, _, fields, mode = W.case(name)
        assert float(np.abs(E.displacement(fields[0], patch, mode)).max()) <= 0.25


def test_extremes_are_what_the_header_says():
    """NaN and +inf entries: image 0 and pad_class everywhere; 1e30: outside everywhere but on the centre plane; a NaN control point:
    0 / pad_class exactly on the voxels whose taps include it."""
    patch, _, _, _, _ = W.extremes()
    for padding_mode in ("zeros", "border"):
        refs = W.extremes_reference(padding_mode)
        for b in (1, 2):
            assert all((p["value"] == 0).all() for p in refs[b]["planes"]) and (refs[b]["label"]["cls"] == 255).all()
        r = refs[3]
        off = np.ones(patch, bool)
        off[patch[0] // 2] = False
        assert (r["label"]["cls"][off] == 255).all() and (r["label"]["cls"][~off] != 255).any()
        if padding_mode == "zeros":
            assert (r["planes"][0]["value"][off] == 0).all() and (r["planes"][0]["value"][~off] != 0).any()
        tainted = np.isnan(E.displacement(W.extremes()[4][4], patch, "linear")).any(axis=0)
        assert 0.02 < tainted.mean() < 0.9 and (refs[4]["label"]["cls"][tainted] == 255).all()
        assert all((p["value"][tainted] == 0).all() and (p["value"][~tainted] != 0).any() for p in refs[4]["planes"])


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, patch_warp, patches
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(patch_warp.SIGNATURES) == NAMES
    assert patch_warp.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert patch_warp.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {patch_warp.SIGNATURES[name]}"
        assert ret == "int" and name not in patch_warp.INT64_RETURNS
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    # micf_patch_sample's arguments, then the map and the field, the stream last
    plain = patches.SIGNATURES["micf_patch_sample"]
    assert patch_warp.SIGNATURES["micf_patch_sample_warped"] == plain[:-1] + "pipiiii" + "p"
    assert abi_header.defines(HEADER, "MICF_") == {}                   # (the modes are micformer_patches.h's and micformer_elastic.h's)
    build = abi_header.build_module()
    assert "volume_patch_warp.hip" in build.SOURCES
    text = open(os.path.join(abi_header.INCLUDE, HEADER)).read()
    for phrase in ("pad_class, in BOTH padding modes", "one rounded add", "bit for bit", "BEFORE the map"):
        assert phrase in text, phrase


def test_table_is_disjoint_from_the_others():
    from micformer_amd import patch_warp
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(patch_warp.SIGNATURES) & set(other), module


def _sample(loader, **kw):
    s = loader.LoaderSample()
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    s.ct, s.mr, s.label = fake, fake, fake
    for name in ("ct_shape", "mr_shape", "label_shape"):
        getattr(s, name)[:] = (8, 9, 10)
    s.ct_dtype, s.mr_dtype, s.label_dtype = loader.DTYPE_I16, loader.DTYPE_F32, loader.DTYPE_I32
    for k, v in kw.items():
        if k.endswith("_shape"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd import loader, patch_warp, patches
    lib = patch_warp.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)
    need = patches.lib.micf_patch_index_bytes(8 * 9 * 10, 7, 1)

    def call(sample=None, B=1, values=vals, nvals=7, idx=fake, nbytes=need, draws=fake, patch=(8, 8, 8), pad=0, pad_class=0, clamp=0,
             image=fake, label_map=fake, origins=fake, picked=fake, affine=fake, flag=0, field=fake, grid=(5, 5, 5), interp=0):
        s = sample if sample is not None else _sample(loader)
        a, n = (ctypes.c_void_p * 1)(idx), (ctypes.c_int64 * 1)(nbytes)
        return lib.micf_patch_sample_warped(ctypes.addressof(s), B, ctypes.addressof(a), ctypes.addressof(n),
                                            None if values is None else ctypes.addressof(values), nvals, draws, *patch, pad, pad_class,
                                            clamp, image, label_map, origins, picked, affine, flag, field, *grid, interp, None)

    # every call fails: nothing below may reach a launch.  `bad` makes an otherwise valid call invalid at the very end of the checks.
    bad = dict(nbytes=need - 1)
    assert call(**bad) == EINVAL
    # the map and the field
    assert call(affine=fake + 2, **bad) == EINVAL and call(field=fake + 1, **bad) == EINVAL
    for flag in (-1, 2, 7):
        assert call(flag=flag, patch=(512, 512, 513)) == EINVAL      # (before the limits)
    for interp in (-1, 2):
        assert call(interp=interp, patch=(512, 512, 513)) == EINVAL
    for grid in [(1, 5, 5), (5, 0, 5), (5, 5, -3)]:
        assert call(grid=grid, patch=(512, 512, 513)) == EINVAL
    assert call(affine=fake + 2, patch=(512, 512, 513)) == EINVAL and call(field=fake + 2, grid=(513, 5, 5)) == EINVAL
    for grid in [(513, 5, 5), (5, 513, 5), (5, 5, 1 << 20)]:
        assert call(grid=grid) == EUNSUP
        assert call(grid=grid, **bad) == EINVAL                       # EINVAL first
    # without a field the grid and the interpolation are not looked at: the call gets as far as the last check
    assert call(field=None, grid=(0, 0, 0), interp=9, patch=(512, 512, 513)) == EUNSUP
    assert call(affine=None, field=None, patch=(512, 512, 513)) == EUNSUP
    # micf_patch_sample's own conditions
    assert call(B=0) == EINVAL and call(idx=None) == EINVAL and call(values=None) == EINVAL and call(nvals=255) == EINVAL
    assert call(_sample(loader, mr_shape=(8, 9, 11))) == EINVAL and call(_sample(loader, ct=None)) == EINVAL
    assert call(draws=None) == EINVAL and call(image=None) == EINVAL and call(origins=None) == EINVAL and call(picked=None) == EINVAL
    assert call(label_map=None) == EINVAL and call(_sample(loader, label=None)) == EINVAL
    for patch in [(0, 8, 8), (8, -1, 8), (8, 8, 0)]:
        assert call(patch=patch) == EINVAL
    for mode in (-1, 2):
        assert call(pad=mode) == EINVAL and call(clamp=mode) == EINVAL
    assert call(pad_class=256) == EINVAL and call(pad_class=-1) == EINVAL
    assert call(image=fake + 8) == EINVAL and call(label_map=fake + 4) == EINVAL               # Pw % 8 == 0: 16- and 8-byte stores
    assert call(image=fake + 4, patch=(8, 8, 12)) == EINVAL and call(label_map=fake + 2, patch=(8, 8, 12)) == EINVAL
    assert call(image=fake + 1, patch=(8, 8, 13)) == EINVAL
    assert call(image=fake + 8, label_map=fake + 4, patch=(512, 512, 516)) == EUNSUP          # Pw % 4 == 0: 8 and 4 bytes are enough
    assert call(draws=fake + 2) == EINVAL and call(origins=fake + 2) == EINVAL and call(picked=fake + 1) == EINVAL
    assert call(_sample(loader, ct_dtype=loader.DTYPE_I32)) == EUNSUP
    assert call(patch=(512, 512, 513)) == EUNSUP and call(patch=(512, 512, 513), pad_class=256) == EINVAL


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import patch_warp, patches
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    draws = torch.zeros(1, 6)
    theta = torch.zeros(1, 3, 4)
    field = torch.zeros(1, 3, 2, 2, 2)
    call = patch_warp.sample_warped_patches
    # every TypeError comes before the first ValueError: patch_size is wrong in each of these
    for kw in (dict(affine=theta.double()), dict(affine=[[1.0]]), dict(displacement=field.long()), dict(displacement="field"),
               dict(field_interpolation=3), dict(padding_mode=None), dict(clamp=1), dict(pad_class=1.0), dict(pad_class=True)):
        with pytest.raises(TypeError):
            call([(ct, ct, None)], [], draws, (0, 4, 4), **dict(dict(affine=theta), **kw))
    with pytest.raises(TypeError, match="draws"):
        call([(ct, ct, None)], [], draws.double(), (0, 4, 4), affine=theta)
    for kw in (dict(field_interpolation="quintic"), dict(padding_mode="reflect"), dict(clamp="upper"), dict(pad_class=256),
               dict(patch_size=(0, 4, 4)), dict()):                   # (the last: the samples are not on the device)
        args = dict(dict(patch_size=(4, 4, 4), affine=theta, displacement=field), **kw)
        with pytest.raises(ValueError):
            call([(ct, ct, None)], [], draws, **args)
    # sample_patches forwards a map or a field to this module, and only then (sample_batch indexes first: tests/test_gpu_patch_warp.py)
    with pytest.raises(TypeError, match="affine must be a float32 tensor"):
        patches.sample_patches([(ct, ct, None)], [], draws, patch_size=(0, 4, 4), affine=theta.double())
    with pytest.raises(TypeError, match="displacement must be a float32 tensor"):
        patches.sample_patches([(ct, ct, None)], [], draws, patch_size=(0, 4, 4), displacement=field.half())
    with pytest.raises(ValueError, match="CUDA"):
        patches.sample_patches([(ct, ct, None)], [], draws, patch_size=(4, 4, 4), field_interpolation=3)   # both None: not read
    doc = patch_warp.__doc__
    assert "draw_affine(len(samples), size=patch_size" in doc and "bit for bit" in doc and "pad_class" in doc


# ---- the device code and the host program ----------------------------------------------------------------------------------------

def test_no_kernel_uses_scratch():
    sizes, _, _ = abi_header.device_asm("volume_patch_warp.hip")
    assert sum("patch_warp_kernel" in k for k in sizes) == 9, sizes   # runs of 8 / 4 / 1 x no field / linear / cubic
    assert sum("patch_locate_kernel" in k for k in sizes) == 1, sizes
    assert all(v == 0 for v in sizes.values()), sizes


def _f32(b):
    return np.frombuffer(struct.pack("I", b), np.float32)[0]


def _bits(x):
    return struct.unpack("I", struct.pack("f", float(x)))[0]


def _clamp(x, lo, hi):
    """affine_coords.h's clampf: NaN becomes lo."""
    x = x if x > lo else lo
    return x if x < hi else hi


def test_host_program_agrees_with_the_referee(tmp_path):
    """tests/patch_warp_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "patch_warp_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "patch_warp_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[-1] == ["patch_warp_coords:", "done"]
    seen, fields, expect = {}, {}, {}
    with np.errstate(over="ignore", invalid="ignore"):
        for kind, *f in lines[:-1]:
            seen[kind] = seen.get(kind, 0) + 1
            if kind == "index":
                sb, o, Pe, L, fin, ib, k, inside, z0, z1, zin0, zin1, zw, b0, b1, bw = (int(x) for x in f)
                s = _f32(sb)
                assert fin == int(np.isfinite(s)), f
                # the kernel's float32 arithmetic, restated: s + 1 rounded, one fmaf (exact in float64 here, rounded once), an exact
                # halving, one rounded add
                s1 = np.float32(s + np.float32(1.0))
                i = np.float32(np.float32(o) + np.float32(np.float32(np.float64(s1) * Pe - 1.0) * np.float32(0.5)))
                if abs(float(s)) <= 4.0:
                    assert _bits(i) == ib, f
                    exact = o + ((float(s) + 1.0) * Pe - 1.0) / 2.0
                    eps = W.eps_axes((Pe,) * 3, (L,) * 3, False)[0]
                    assert abs(float(i) - exact) <= eps, (f, float(i), exact)
                    if abs(exact - np.floor(exact) - 0.5) > eps:      # the referee's rounding, where it is beyond doubt
                        r64 = np.rint(exact)
                        assert inside == int(0 <= r64 <= L - 1) and k == int(np.clip(r64, 0, L - 1)), f
                else:
                    assert np.isnan(i) or abs(float(i)) > 1e20, f
                i = _f32(ib)                                          # from the index on: the header's rule on the kernel's own index
                r32 = np.rint(_clamp(i, np.float32(-1.0), np.float32(L)))
                assert inside == int(0 <= r32 <= L - 1) and k == int(np.clip(r32, 0, L - 1)), f
                c = _clamp(i, np.float32(-1.0), np.float32(L))
                k0 = int(np.floor(c))
                assert (z0, z1, zin0, zin1) == (min(max(k0, 0), L - 1), min(k0 + 1, L - 1), int(0 <= k0 < L), int(0 <= k0 + 1 < L)), f
                assert zw == _bits(np.float32(c - np.float32(k0))), f
                c = _clamp(i, np.float32(0.0), np.float32(L - 1))
                k0 = int(np.floor(c))
                assert (b0, b1) == (k0, min(k0 + 1, L - 1)) and bw == _bits(np.float32(c - np.float32(k0))), f
                if not fin or abs(float(s)) > 1e20:                   # NaN, +-inf, +-1e30, +-FLT_MAX: outside, whatever P and o
                    assert inside == 0 and (zin0, zin1) in ((0, 0), (0, 1)) and 0 <= k < L, f
            elif kind == "row":
                Pe, o, worst = int(f[0]), int(f[1]), float(f[2])
                assert worst <= W.eps_axes((Pe,) * 3, (37,) * 3, False)[0], f
                assert worst == 0.0 or Pe & (Pe - 1), f
            elif kind == "field":
                taps, gd, gh, gw, Pd, Ph, Pw, z, y, x = (int(v) for v in f[:10])
                fields.setdefault((taps, gd, gh, gw, Pd, Ph, Pw), []).append((z, y, x, [_f32(int(b)) for b in f[10:]]))
            elif kind == "recomputed":
                gw, Pw, per, r2, r4 = (int(v) for v in f)
                runs = -(-Pw // per)
                for got in (r2, r4):                                  # once per run and once more per cell boundary inside a run
                    assert runs <= got <= (Pw if gw >= Pw else runs + gw), f
                    assert got == Pw or gw < Pw, f
            else:
                raise AssertionError(kind)
    assert seen["index"] == 10 * 10 * 2 * 19 and seen["row"] == 2048 and len(fields) == 8
    nan_at = {(5, 4, 6): 37}
    for (taps, gd, gh, gw, Pd, Ph, Pw), rows in fields.items():
        n = 3 * gd * gh * gw
        i = np.arange(n, dtype=np.uint64)
        fld = (((((i * np.uint64(2654435761)) >> np.uint64(20)) & np.uint64(1023)).astype(np.int64) - 512) / 4096.0).astype(np.float32)
        if (gd, gh, gw) in nan_at:
            fld[nan_at[(gd, gh, gw)]] = np.nan
        u = E.displacement(fld.reshape(3, gd, gh, gw), (Pd, Ph, Pw), "cubic" if taps == 4 else "linear")
        assert len(rows) == Pd * Ph * Pw
        got = np.zeros((3, Pd, Ph, Pw))
        for z, y, x, v in rows:
            got[:, z, y, x] = v
        assert np.array_equal(np.isnan(got), np.isnan(u)) and (np.isnan(u).any() == ((gd, gh, gw) in nan_at))
        assert np.nanmax(np.abs(got - u)) <= 1e-6, (taps, gd, gh, gw)
