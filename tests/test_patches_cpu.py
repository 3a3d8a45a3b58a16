"""CPU checks of the patch sampler.  The first group checks the numpy referee (tests/patches_ref.py) alone -- against brute force,
and that its comparison catches the mistakes it must catch; those tests judge the judge and do not touch the library.  The rest
needs the feature: draw_patches' rule, include/micformer_patches.h against the ctypes table of micformer_amd/patches.py and the built library,
argument errors caught before any launch, the compiled device code's scratch use, and the host program
tests/patches_index_main.cpp (csrc/patches_coords.h under the address and undefined-behaviour sanitizers: a stand-alone program,
nothing is preloaded), whose printed results are compared with the referee's."""
import ctypes
import importlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import abi_header
import loader_ref as R
import patches_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_patches.h"
NAMES = {"micf_patch_index_bytes", "micf_patch_index_workspace", "micf_patch_index", "micf_patch_sample"}
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "elastic", "intensity", "restore", "postprocess", "surface", "blend")


def _scan(seed=9301, shape=(9, 11, 13)):
    g = np.random.default_rng(seed)
    ct = g.integers(-200, 900, shape).astype(np.int16)
    mr = g.random(shape, dtype=np.float32) * 300
    values = np.array((0, 0, 0) + R.MMWHS_LABEL_VALUES + (421,))
    return ct, mr, values[g.integers(0, len(values), shape)].astype(np.int16)


# ---- the referee against brute force ---------------------------------------------------------------------------------------------

def test_every_rank_visits_each_voxel_of_the_class_once():
    ct, mr, lab = _scan()
    cmap = P.full_class_map(lab)
    assert set(np.unique(cmap)) == set(range(8)) | {255}
    for c in (1, 4, 7):
        n = int((cmap == c).sum())
        present = sorted(set(np.unique(cmap)) - {0, 255})
        u_class = P.steer(present.index(c), len(present))
        seen = []
        for r in range(n):
            origin, picked = P.locate(cmap, cmap.shape, (1.0, u_class, P.steer(r, n), 0, 0, 0), (4, 4, 4))
            assert picked[0] == c and cmap[tuple(picked[1:])] == c
            seen.append(tuple(picked[1:]))
        assert len(set(seen)) == n and seen == sorted(seen)           # each voxel once, in flat (z, y, x) order
    counts = P.class_counts(lab)
    assert counts.sum() == cmap.size and counts[-1] == (cmap == 255).sum() and counts[3] == (cmap == 3).sum()


@pytest.mark.parametrize("L,Pe,want", [(10, 4, (0, 6)), (7, 7, (0, 0)), (5, 9, (-2, -2)), (4, 9, (-3, -2)), (1, 2, (-1, 0)),
                                       (2048, 1, (0, 2047)), (1, 2048, (-1024, -1023))])
def test_origin_bounds(L, Pe, want):
    assert P.bounds(L, Pe) == want
    lb, ub = want
    need = max(Pe - L, 0)
    assert lb == -need // 2 and ub - lb == (L - Pe if need == 0 else need % 2)        # (Python's -need // 2 floors -need)
    # every origin of the range, and only those, comes out of the draws
    got = {P.locate(None, (L, 8, 8), (0.0, 0, 0, u, 0, 0), (Pe, 8, 8))[0][0] for u in np.linspace(0, 0.9999, 4099, dtype=np.float32)}
    assert got == set(range(lb, ub + 1))


def test_draw_index_edges():
    below_one = struct.unpack("f", struct.pack("I", 0x3F7FFFFF))[0]
    for n in (1, 2, 7, 2 ** 31 - 1):
        assert P.draw_index(0.0, n) == 0 and P.draw_index(-1.0, n) == 0 and P.draw_index(float("nan"), n) == 0
        assert P.draw_index(1.0, n) == n - 1 and P.draw_index(7.5, n) == n - 1
        assert P.draw_index(below_one, n) == min(int(np.float64(np.float32(below_one)) * n), n - 1) <= n - 1
    assert P.draw_index(below_one, 2 ** 31 - 1) == 2 ** 31 - 1 - 128   # (1 - 2^-24) n, truncated


def test_a_forced_sample_without_foreground_or_label_falls_back():
    ct, mr, lab = _scan()
    draw = (1.0, 0.3, 0.6, 0.2, 0.5, 0.9)
    a = P.locate(None, lab.shape, draw, (4, 5, 6))
    b = P.locate(np.where(P.full_class_map(lab) == 255, 255, 0).astype(np.uint8), lab.shape, draw, (4, 5, 6))
    c = P.locate(P.full_class_map(lab), lab.shape, (0.0,) + draw[1:], (4, 5, 6))
    assert a == b == c and a[1] == list(P.RANDOM_PICK)


# ---- the comparison must catch these ---------------------------------------------------------------------------------------------

def _as_got(ref):
    return dict(image=ref["image"].astype(np.float16), label=ref["label"], origin=ref["origin"], picked=ref["picked"])


@pytest.mark.parametrize("mutate,kw,expect", [
    ("rank+1", dict(patch_size=(4, 4, 4)), "picked"),
    ("lb_floor", dict(patch_size=(12, 14, 13), force=0.0), "origin"),                 # need 3 on z and y: odd
    ("pad_side", dict(patch_size=(12, 14, 13)), "image"),
    ("pad_side", dict(patch_size=(12, 14, 13)), "label"),
    ("label_edge", dict(patch_size=(12, 14, 16), padding_mode="border", pad_class=255), "label"),
    ("no_upper", dict(patch_size=(4, 4, 4), corner=True), "origin"),
])
def test_the_comparison_fails_for(mutate, kw, expect):
    ct, mr, lab = _scan()
    kw = dict(kw)
    cmap = P.full_class_map(lab)
    u_voxel = 0.4
    if kw.pop("corner", False):                                       # the last voxel of class 2: near the far corner
        lab = lab.copy()
        lab[-1, -1, -1] = R.MMWHS_LABEL_VALUES[1]
        cmap = P.full_class_map(lab)
        u_voxel = P.steer(int((cmap == 2).sum()) - 1, int((cmap == 2).sum()))
    draw = (kw.pop("force", 1.0), P.steer(1, 7), u_voxel, 0.0, 0.0, 0.0)
    good = P.sample(ct, mr, lab, draw, **kw)
    assert P.compare(_as_got(good), good) == []
    bad = P.sample(ct, mr, lab, draw, mutate=mutate, **kw)
    assert expect in P.compare(_as_got(bad), good), (mutate, P.compare(_as_got(bad), good))


# ---- draw_patches ------------------------------------------------------------------------------------------------------------

def test_draw_patches_rule():
    from micformer_amd.patches import draw_patches
    d = draw_patches(2, generator=torch.Generator().manual_seed(1))
    assert d.dtype == torch.float32 and tuple(d.shape) == (2, 6) and d.device.type == "cpu" and d.is_contiguous()
    assert d[:, 0].tolist() == [0.0, 1.0]                             # B = 2, p = 1/3: round(1.33) = 1, one forced
    assert draw_patches(5, oversample_foreground_percent=0.0)[:, 0].tolist() == [0.0] * 5
    assert draw_patches(5, oversample_foreground_percent=1.0)[:, 0].tolist() == [1.0] * 5
    for B in (1, 2, 3, 8, 9):
        for p in (0.0, 1 / 3, 0.5, 0.33, 1.0):
            got = draw_patches(B, oversample_foreground_percent=p, generator=torch.Generator().manual_seed(B))
            assert np.array_equal(got[:, 0].numpy(), P.forced_column(B, p)), (B, p)
            assert float(got[:, 1:].min()) >= 0.0 and float(got[:, 1:].max()) < 1.0
    a = draw_patches(4, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, draw_patches(4, generator=torch.Generator().manual_seed(3)))
    assert not torch.equal(a, draw_patches(4, generator=torch.Generator().manual_seed(4)))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            draw_patches(bad)
    with pytest.raises(TypeError):
        draw_patches(2.0)
    with pytest.raises(ValueError):
        draw_patches(2, oversample_foreground_percent=1.5)
    doc = importlib.import_module("micformer_amd.patches").__doc__
    assert "UNPINNED" in doc and "10 000" in doc and "nnU-Net" in doc


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, patches
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(patches.SIGNATURES) == NAMES
    assert patches.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert patches.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {patches.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in patches.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert abi_header.defines(HEADER, "MICF_PATCH_") == {
        "MICF_PATCH_SEGMENT": patches.SEGMENT, "MICF_PATCH_PAD_ZEROS": patches.PADDING_MODES["zeros"],
        "MICF_PATCH_PAD_BORDER": patches.PADDING_MODES["border"], "MICF_PATCH_CLAMP_BOTH": patches.CLAMPS["both"],
        "MICF_PATCH_CLAMP_LOWER": patches.CLAMPS["lower"]}
    assert patches.SEGMENT == P.SEGMENT
    build = abi_header.build_module()
    assert "volume_patches.hip" in build.SOURCES
    assert "SEGMENT" in patches.__all__


def test_table_is_disjoint_from_the_others():
    from micformer_amd import patches
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(patches.SIGNATURES) & set(other), module


def test_queries_are_pure_and_validate():
    from micformer_amd import normalise, patches
    lib = patches.lib
    q = lib.micf_patch_index_bytes
    V = 363 * 512 * 512
    segs = -(-V // patches.SEGMENT)
    assert q(V, 7, 1) == q(V, 7, 1) == 1536 + -(-7 * (-(-segs // 4) * 4) * 2 // 256) * 256
    assert q(V, 7, 0) == q(1, 0, 0) == 1536 and q(1, 7, 1) == 1536 + 256
    assert q(0, 7, 1) == -1 and q(V, -1, 1) == -1 and q(V, 255, 1) == -1
    assert lib.micf_patch_index_workspace(3) == normalise.lib.micf_volume_loader_norm_workspace(3) > 0
    assert lib.micf_patch_index_workspace(0) == -1


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
    from micformer_amd import loader, patches
    lib = patches.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)
    need = lib.micf_patch_index_bytes(8 * 9 * 10, 7, 1)
    ws = lib.micf_patch_index_workspace(1)

    def arrays(index, nbytes):
        return (ctypes.c_void_p * 1)(index), (ctypes.c_int64 * 1)(nbytes)

    def index(sample=None, B=1, values=vals, nvals=7, modes=(0, 0), p=(1.0, 99.0), workspace=fake, ws_bytes=ws, idx=fake,
              nbytes=need, ptrs=True, sizes=True):
        s = sample if sample is not None else _sample(loader)
        a, n = arrays(idx, nbytes)
        return lib.micf_patch_index(ctypes.addressof(s), B, None if values is None else ctypes.addressof(values), nvals, modes[0],
                                    modes[1], p[0], p[1], workspace, ws_bytes, ctypes.addressof(a) if ptrs else None,
                                    ctypes.addressof(n) if sizes else None, None)

    def sample(sample=None, B=1, values=vals, nvals=7, idx=fake, nbytes=need, ptrs=True, sizes=True, draws=fake, patch=(8, 8, 8),
               pad=0, pad_class=0, clamp=0, image=fake, label_map=fake, origins=fake, picked=fake):
        s = sample if sample is not None else _sample(loader)
        a, n = arrays(idx, nbytes)
        return lib.micf_patch_sample(ctypes.addressof(s), B, ctypes.addressof(a) if ptrs else None,
                                     ctypes.addressof(n) if sizes else None, None if values is None else ctypes.addressof(values),
                                     nvals, draws, *patch, pad, pad_class, clamp, image, label_map, origins, picked, None)

    for call in (index, sample):
        # NULLs, counts
        assert call(B=0) == EINVAL
        assert call(ptrs=False) == EINVAL and call(sizes=False) == EINVAL and call(idx=None) == EINVAL
        assert call(values=None) == EINVAL and call(nvals=-1) == EINVAL and call(nvals=255) == EINVAL
        assert call(values=(ctypes.c_int32 * 3)(5, 7, 5), nvals=3) == EINVAL
        assert call(values=(ctypes.c_int32 * 2)(5, 0), nvals=2) == EINVAL
        assert call(_sample(loader, ct=None)) == EINVAL and call(_sample(loader, mr=None)) == EINVAL
        # unequal shapes
        assert call(_sample(loader, mr_shape=(8, 9, 11))) == EINVAL
        assert call(_sample(loader, label_shape=(9, 9, 10))) == EINVAL
        assert call(_sample(loader, ct_shape=(8, 0, 10))) == EINVAL
        # too short an index buffer, misalignment
        assert call(nbytes=need - 1) == EINVAL and call(nbytes=0) == EINVAL
        assert call(idx=fake + 128) == EINVAL
        assert call(_sample(loader, ct=fake + 1)) == EINVAL and call(_sample(loader, label=fake + 2)) == EINVAL
        # limits: EINVAL first
        big = dict(ct_shape=(8, 2049, 8), mr_shape=(8, 2049, 8), label_shape=(8, 2049, 8))
        assert call(_sample(loader, **big), nbytes=1 << 40) == EUNSUP
        assert call(_sample(loader, **big), nbytes=1 << 40, B=0) == EINVAL
        assert call(_sample(loader, ct_dtype=loader.DTYPE_I32)) == EUNSUP
        huge = dict(ct_shape=(2048, 2048, 512), mr_shape=(2048, 2048, 512), label_shape=(2048, 2048, 512))
        assert call(_sample(loader, **huge), nbytes=1 << 40) == EUNSUP                # 2^31 voxels
    assert index(workspace=None) == EINVAL and index(workspace=fake + 64) == EINVAL and index(ws_bytes=ws - 1) == EINVAL
    for modes in [(3, 0), (0, -1)]:
        assert index(modes=modes) == EINVAL
    for p in [(-0.5, 99.0), (50.0, 50.0), (float("nan"), 99.0)]:
        assert index(p=p) == EINVAL
    assert sample(draws=None) == EINVAL and sample(image=None) == EINVAL and sample(origins=None) == EINVAL
    assert sample(picked=None) == EINVAL
    assert sample(label_map=None) == EINVAL                           # the sample has a label
    assert sample(_sample(loader, label=None)) == EINVAL              # ... and here it has none
    for patch in [(0, 8, 8), (8, -1, 8), (8, 8, 0)]:
        assert sample(patch=patch) == EINVAL
    for mode in (-1, 2, 9):
        assert sample(pad=mode) == EINVAL and sample(clamp=mode) == EINVAL
    assert sample(pad_class=256) == EINVAL and sample(pad_class=-1) == EINVAL
    assert sample(image=fake + 2) == EINVAL and sample(label_map=fake + 4) == EINVAL          # Pw % 8 == 0: vector stores
    assert sample(image=fake + 1, patch=(8, 8, 13)) == EINVAL
    assert sample(draws=fake + 2) == EINVAL and sample(origins=fake + 2) == EINVAL and sample(picked=fake + 1) == EINVAL
    assert sample(patch=(512, 512, 513)) == EUNSUP and sample(patch=(1 << 20, 1 << 20, 1 << 20)) == EUNSUP
    assert sample(patch=(512, 512, 513), pad_class=256) == EINVAL


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import patches
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    draws = torch.zeros(1, 6)
    with pytest.raises(ValueError, match="CUDA"):
        patches.index_scans([(ct, ct, None)])
    with pytest.raises(ValueError, match="normalisation"):
        patches.index_scans([(ct, ct, None)], normalisation="robust")
    with pytest.raises(ValueError, match="at least one"):
        patches.index_scans([])
    for kw, err in [(dict(padding_mode="reflect"), ValueError), (dict(padding_mode=None), TypeError), (dict(clamp="upper"), ValueError),
                    (dict(pad_class=256), ValueError), (dict(pad_class=-1), ValueError), (dict(pad_class=1.0), TypeError),
                    (dict(patch_size=(0, 4, 4)), ValueError), (dict(patch_size=(4, 4)), ValueError)]:
        with pytest.raises(err):
            patches.sample_patches([(ct, ct, None)], [], draws, **kw)
    with pytest.raises(TypeError, match="draws"):
        patches.sample_patches([(ct, ct, None)], [], draws.double())
    with pytest.raises(TypeError):
        patches.index_scans([(ct.float().double(), ct, None)])


def test_patch_index_views():
    """.stats and .class_counts are views of the index buffer at the header's offsets (the front end's shape and foreign-index
    checks need device tensors: tests/test_gpu_patches.py has them; the C entry points' shape rule is checked above)."""
    from micformer_amd import patches
    buf = torch.zeros(2048, dtype=torch.uint8)
    idx = patches.PatchIndex(buf, (4, 5, 7), (torch.int16, torch.int16, torch.int32), patches.MMWHS_LABEL_VALUES, (0, 0), (1.0, 99.0))
    assert tuple(idx.stats.shape) == (2, 2) and idx.stats.dtype == torch.float64
    assert tuple(idx.class_counts.shape) == (9,) and idx.class_counts.dtype == torch.int32 and idx.has_label
    buf[96:112].view(torch.float64)[:] = torch.tensor([1.5, 2.5], dtype=torch.float64)           # channel 0 at byte 96
    buf[112 + 96:112 + 112].view(torch.float64)[:] = torch.tensor([-3.0, 4.0], dtype=torch.float64)  # channel 1 at byte 112 + 96
    buf[256:256 + 36].view(torch.int32)[:] = torch.arange(9, dtype=torch.int32)                  # the counts at byte 256
    assert idx.stats.tolist() == [[1.5, 2.5], [-3.0, 4.0]] and idx.class_counts.tolist() == list(range(9))
    text = abi_header.read_header(HEADER) + open(os.path.join(abi_header.INCLUDE, HEADER)).read()
    assert "byte 112 c + 96" in text and "at byte 256" in text


# ---- the device code and the host program ----------------------------------------------------------------------------------------

def test_no_kernel_uses_scratch():
    sizes, _, _ = abi_header.device_asm("volume_patches.hip")
    for name, n in (("patch_crop_kernel", 2), ("patch_locate_kernel", 1), ("patch_count_kernel", 1), ("patch_index_init_kernel", 1)):
        assert sum(name in k for k in sizes) == n, sizes
    assert all(v == 0 for v in sizes.values()), sizes


def _f32(bits):
    return struct.unpack("f", struct.pack("I", bits))[0]


def test_host_program_agrees_with_the_referee(tmp_path):
    """tests/patches_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "patches_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "patches_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[-1] == ["patches_coords:", "done"]
    seen = {}
    hashed = None
    for kind, *f in lines[:-1]:
        seen[kind] = seen.get(kind, 0) + 1
        v = [int(x) for x in f]
        if kind == "segment":
            assert v == [P.SEGMENT]
        elif kind == "bounds":
            assert P.bounds(v[0], v[1]) == (v[2], v[3]), v
        elif kind == "random":
            lb, ub = P.bounds(v[1], v[2])
            assert lb + P.draw_index(_f32(v[0]), ub - lb + 1) == v[3], v
        elif kind == "centred":
            lb, ub = P.bounds(v[1], v[2])
            o = max(v[0] - v[2] // 2, lb)
            assert (o if v[3] else min(o, ub)) == v[4], v
        elif kind == "index":
            assert P.draw_index(_f32(v[0]), v[1]) == v[2], v
        elif kind == "segments":
            V, nseg = v[0], -(-v[0] // P.SEGMENT)
            assert v[1:] == [nseg, V - (nseg - 1) * P.SEGMENT, min(V, P.SEGMENT), 1536 + -(-7 * (-(-nseg // 4) * 4) * 2 // 256) * 256, 1536], v
        elif kind == "unflatten":
            assert list(np.unravel_index(v[0], (2048, 2048, 2048))) == v[1:], v
        elif kind == "locate":
            if hashed is None:
                i = np.arange(v[0], dtype=np.uint64)
                hashed = np.flatnonzero((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)) < 3)
            assert v[0] % P.SEGMENT != 0 and hashed[v[1]] == v[2], v
        else:
            raise AssertionError(kind)
    assert seen["bounds"] == 81 and seen["index"] == 35 and seen["locate"] == 6 and seen["segments"] == 7
    extents = {int(f[0]) for kind, *f in lines[:-1] if kind == "bounds"}
    assert {1, 2048} <= extents
    assert {int(f[1]) for kind, *f in lines[:-1] if kind == "index"} >= {1, 2 ** 31 - 1}
    assert {int(f[0]) for kind, *f in lines[:-1] if kind == "index"} >= {0, 0x3F7FFFFF, 0x3F800000, 0xBF800000, 0x7FC00000}
