"""CPU checks of the loader's z-score / percentile-clip normalisations: the referee (tests/normalise_ref.py) against the fixture made
by the real reference functions (tests/golden/f12_normalise.npz) and against its own edge rules, include/micformer_normalise.h
against the ctypes table of micformer_amd/normalise.py and the built library, argument errors caught before any launch, and the
compiled device code's scratch use."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import abi_header
import loader_ref as R
import normalise_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_normalise.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "f12_normalise.npz")
OTHER_TABLES = ("_lib", "metrics", "loader", "restore", "postprocess", "surface")


# ---- the referee ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["zscore", "percentile"])
def test_referee_matches_the_reference_fixture(mode):
    g = np.load(GOLDEN)
    assert int(g["seed"]) == R.F11_SEED and os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden",
                                                                                                      "f11_loader.npz"))
    a = R.f11_inputs(int(g["seed"]))
    image, cmap, crop, st = N.load_pair(a["ct"], a["mr"], a["ct_label"], size=tuple(int(s) for s in g["size"]), normalisation=mode)
    s = int(g["stride"])
    assert np.array_equal(cmap, g["class_map"])
    assert np.array_equal(crop, g[f"{mode}_crop"])
    assert np.array_equal(st, g[f"{mode}_stats"])                   # numpy on float64, on both sides
    fails, share, A = N.close(g[f"{mode}_lattice"], image[:, ::s, ::s, ::s])
    print(f"{mode}: referee vs fixture: {fails} failing points, share beyond A = {A:.2e}: {share:.2e}")
    assert fails == 0 and share <= N.MAX_SHARE


def test_referee_edge_rules():
    zeros = np.zeros((3, 4, 5), np.float32)
    assert not N.normalise(zeros, "zscore").any()                                        # all zero -> all zero
    const = np.full((3, 4, 5), 7, np.int16)
    const[0, 0, :2] = 0
    z = N.normalise(const, "zscore")
    assert np.isnan(z[const != 0]).all() and (z[const == 0] == 0).all()                  # constant -> NaN off the zeros
    one = np.zeros((3, 4, 5), np.float32)
    one[1, 2, 3] = 4.0
    assert np.isnan(N.normalise(one, "percentile")).all()                                # one positive voxel: high == low
    assert np.isnan(N.normalise(np.full((2, 2, 2), 3, np.int16), "percentile")).all()    # high == low
    assert np.isnan(N.normalise(-np.ones((2, 2, 2), np.float32), "percentile")).all()    # no positive voxel
    assert np.isnan(N.stats(zeros, "zscore")).all() and np.isnan(N.stats(zeros, "percentile")).all()
    neg = np.float32([[[-0.0, 2.0, -2.0, 0.0, 6.0]]])                                   # -0.0 is zero; negatives count for z-score
    assert np.array_equal(N.stats(neg, "zscore"), [2.0, np.sqrt(32.0 / 3.0)])
    assert np.array_equal(N.stats(neg, "percentile", (0, 100)), [2.0, 6.0])              # ... and not for the percentiles
    assert np.array_equal(N.normalise(neg, "percentile", (0, 100)), np.float32([[[0, 0, 0, 0, 1]]]))
    v = np.array([[[-5, 0, 3, 9]]], np.int16)                                           # int16 is z-scored as float32: no truncation
    m, s = np.float32(7.0 / 3.0), np.float32(np.std([-5.0, 3.0, 9.0]))
    assert np.array_equal(N.normalise(v, "zscore"), np.float32([[[(np.float32(-5) - m) / s, 0, (np.float32(3) - m) / s,
                                                                  (np.float32(9) - m) / s]]]))
    assert np.array_equal(N.normalise(v, "minmax"), R.normalize(v))


def test_closeness_measure():
    want = np.float32([1e-5, 0.5, 8.0, np.nan])
    got = want.astype(np.float16)
    assert N.close(got, want)[:2] == (0, 0.0)
    off = got.copy()
    off[0] = np.float16(1e-5 + 5e-7)                                                    # many fp16 steps, but within A = 8 * 2^-20
    assert R.fp16_steps(off[:1], got[:1])[0] > 1 and N.close(off, want)[:2] == (0, 0.0)
    off[2] = np.nextafter(off[2], np.float16(9))                                        # one fp16 step at 8: passes, counts for the share
    assert N.close(off, want)[:2] == (0, 0.25)
    off[1] = np.float16(0.5 + 2 ** -9)                                                  # two fp16 steps, beyond A
    assert N.close(off, want)[0] == 1
    assert N.close(np.float16([1.0]), np.float32([np.nan]))[0] == 1
    assert N.ulps(1.0, np.nextafter(1.0, 2.0)) == 1 and N.ulps(np.nan, np.nan) == 0 and N.ulps(-0.0, 0.0) == 0


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, normalise
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(normalise.SIGNATURES) == {"micf_volume_loader_norm_workspace", "micf_volume_loader_norm"}
    assert normalise.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert normalise.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {normalise.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in normalise.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert set(normalise.INT64_RETURNS) <= set(d)
    consts = abi_header.defines(HEADER, "MICF_NORM_")
    assert consts == {"MICF_NORM_MINMAX": normalise.MINMAX, "MICF_NORM_ZSCORE": normalise.ZSCORE,
                      "MICF_NORM_PERCENTILE": normalise.PERCENTILE}
    assert normalise.MODES == {"minmax": 0, "zscore": 1, "percentile": 2}
    assert '#include "micformer_loader.h"' in open(os.path.join(abi_header.INCLUDE, HEADER)).read()
    assert len(abi_header.parse_header("micformer_loader.h")) == 2          # the loader's header keeps its two entry points


def test_table_is_disjoint_from_the_others():
    from micformer_amd import normalise
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(normalise.SIGNATURES) & set(other), module
    from micformer_amd import loader
    assert set(loader.SIGNATURES) == {"micf_volume_loader_workspace", "micf_volume_loader"}


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.normalise import lib
    a = lib.micf_volume_loader_norm_workspace(1)
    assert a == lib.micf_volume_loader_norm_workspace(1) and a > 0 and a % 256 == 0
    assert lib.micf_volume_loader_norm_workspace(9) >= 9 * (a - 256)
    assert lib.micf_volume_loader_norm_workspace(0) == -1 and lib.micf_volume_loader_norm_workspace(-2) == -1


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
    from micformer_amd import loader, normalise
    lib = normalise.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20
    vals = (ctypes.c_int32 * 7)(*loader.MMWHS_LABEL_VALUES)
    ws = lib.micf_volume_loader_norm_workspace(1)

    def call(sample=None, B=1, size=(16, 16, 16), values=vals, nvals=7, modes=(1, 2), p=(1.0, 99.0), workspace=fake, ws_bytes=ws,
             image=fake, label_map=fake, crop=fake, stats=None):
        s = sample if sample is not None else _sample(loader)
        return lib.micf_volume_loader_norm(ctypes.addressof(s), B, *size, None if values is None else ctypes.addressof(values),
                                           nvals, modes[0], modes[1], p[0], p[1], workspace, ws_bytes, image, label_map, crop,
                                           stats, None)

    for modes in [(3, 0), (0, -1), (0, 3), (7, 7)]:
        assert call(modes=modes) == EINVAL
    for p in [(-0.5, 99.0), (1.0, 100.5), (50.0, 50.0), (99.0, 1.0), (float("nan"), 99.0), (1.0, float("nan"))]:
        assert call(p=p) == EINVAL
        assert call(p=p, modes=(0, 1)) == EINVAL                      # checked whether or not a channel reads them
    assert call(stats=fake + 4) == EINVAL                             # float64 alignment
    # ... and the loader's own checks
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
    assert call(_sample(loader, mr=fake + 2)) == EINVAL
    assert call(_sample(loader, ct_shape=(8, 0, 8))) == EINVAL
    assert call(values=None) == EINVAL
    assert call(values=(ctypes.c_int32 * 3)(5, 7, 5), nvals=3) == EINVAL
    assert call(_sample(loader, ct_dtype=loader.DTYPE_I32)) == EUNSUP
    assert call(_sample(loader, mr_shape=(8, 2049, 8))) == EUNSUP
    assert call(_sample(loader, ct_shape=(2048, 1024, 1024))) == EUNSUP
    assert call(size=(512, 512, 513)) == EUNSUP


def test_python_front_end_rejects_before_the_device():
    """Every argument error of the three keywords, raised with CPU tensors in hand: the keyword checks come before the first look
    at a device (a correct call with CPU tensors fails later, on the device check)."""
    from micformer_amd import loader, normalise, restore
    ct = torch.zeros(4, 5, 6, dtype=torch.int16)
    for bad in ["z-score", "", "MINMAX", ("minmax", "zs"), ("zscore",), ("zscore", "minmax", "percentile"), []]:
        with pytest.raises(ValueError, match="normalisation"):
            loader.load_pair(ct, ct, normalisation=bad)
    for bad in [None, 1, ("zscore", 2), (None, "minmax"), {"ct": "zscore"}]:
        with pytest.raises(TypeError, match="normalisation"):
            loader.load_pair(ct, ct, normalisation=bad)
    for bad in [(99, 1), (50, 50), (-1, 99), (1, 100.5), (1,), (1, 50, 99), (float("nan"), 99)]:
        with pytest.raises(ValueError, match="percentiles"):
            loader.load_pair(ct, ct, normalisation="percentile", percentiles=bad)
        with pytest.raises(ValueError, match="percentiles"):
            loader.load_batch([(ct, ct, None)], percentiles=bad)       # also when no channel reads them
    for bad in [None, 5, "19", ("a", "b"), (None, 99)]:
        with pytest.raises(TypeError, match="percentiles"):
            loader.load_pair(ct, ct, normalisation="percentile", percentiles=bad)
    with pytest.raises(ValueError, match="normalisation"):
        restore.segment_pair(None, ct, ct, normalisation="zs")
    with pytest.raises(ValueError, match="percentiles"):
        restore.segment_pair(None, ct, ct, normalisation="percentile", percentiles=(60, 40))
    for ok in ["zscore", ("minmax", "percentile"), ["percentile", "zscore"]]:
        with pytest.raises(ValueError, match="CUDA"):
            loader.load_pair(ct, ct, normalisation=ok, percentiles=(0, 100), return_stats=True)
    assert normalise.modes("percentile") == (2, 2) and normalise.modes(("zscore", "minmax")) == (1, 0)
    assert normalise.percentile_pair((0, 100)) == (0.0, 100.0) and normalise.percentile_pair([50, 50.5]) == (50.0, 50.5)


# ---- the device code ----------------------------------------------------------------------------------------------------------

def test_volume_normalise_device_code_uses_no_scratch():
    sizes, asm, flags = abi_header.device_asm("volume_normalise.hip")
    assert not any("fast-math" in f or "-Ofast" in f for f in flags)     # the normalisers need the IEEE divide
    assert len(sizes) == 9 and all(v == 0 for v in sizes.values()), sizes
    assert "v_div_fixup_f32" in asm and "v_div_fmas_f32" in asm          # the correctly rounded fp32 divide sequence
    assert "v_div_fixup_f64" in asm                                      # ... and the float64 one of the statistics
    assert "ds_add_u32" in asm and "global_atomic_add_f32" not in asm and "global_atomic_add_f64" not in asm   # integer counts only
