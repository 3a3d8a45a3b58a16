"""Test-time mirroring of sliding-window inference, the CPU half: the flip codes of micformer_amd.mirror, the float64 referee of
tests/sw_mirror_ref.py against the un-mirrored referee, the derived bound of the GPU comparison shown to hold a float32 restatement
and to reject four wrong blends, and the C-ABI of include/micformer_mirror.h (no GPU: header, ctypes table, exports, argument
errors)."""
import ctypes
import importlib

import pytest
import torch

import abi_header
import sw_blend_ref as S
import sw_mirror_ref as M

HEADER = "micformer_mirror.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "elastic", "intensity", "restore", "postprocess", "surface", "blend",
                "patches", "patch_warp")
# (volume, roi, overlap, sw_batch_size): the shapes of tests/test_gpu_sw_blend.py
SHAPES = [((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 1), ((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 7),
          ((1, 2, 20, 12, 37), (16, 16, 16), 0.25, 3), ((1, 2, 33, 16, 16), (16, 16, 16), 0.5, 4),
          ((1, 2, 24, 40, 17), (16, 24, 8), 0.5, 2), ((1, 2, 32, 16, 20), (16, 16, 16), 0.75, 64),
          ((1, 2, 10, 16, 20), (16, 16, 16), 0.5, 5)]
# (shape index, mirror axes): the pairs of tests/test_gpu_sw_mirror.py that the bound was checked on
PAIRS = [(0, (0, 1, 2)), (2, (2,)), (4, (0, 2)), (6, (1,)), (3, (0, 1))]
MODES = ("constant", "gaussian")


# ---- the flip codes -------------------------------------------------------------------------------------------------------------

def test_flip_codes_are_all_subsets_in_ascending_order():
    from micformer_amd import mirror
    assert mirror.flip_codes(()) == [0] and mirror.flip_codes([]) == [0]
    assert mirror.flip_codes((0,)) == [0, 1] and mirror.flip_codes((1,)) == [0, 2] and mirror.flip_codes((2,)) == [0, 4]
    assert mirror.flip_codes((0, 2)) == mirror.flip_codes([2, 0]) == [0, 1, 4, 5]
    assert mirror.flip_codes((0, 1)) == [0, 1, 2, 3] and mirror.flip_codes((1, 2)) == [0, 2, 4, 6]
    assert mirror.flip_codes((2, 0, 1)) == list(range(8))
    for axes in [(), (1,), (0, 2), (0, 1, 2)]:
        assert mirror.flip_codes(axes) == M.flip_codes(axes)


@pytest.mark.parametrize("bad", [(3,), (-1,), (0, 0), (0, 1, 2, 0), (1.0,), (True,), ("0",), "01", 1, None, (0, None)])
def test_bad_mirror_axes_are_a_value_error(bad):
    from micformer_amd import mirror
    from micformer_amd.inference import sliding_window_inference
    with pytest.raises(ValueError, match="mirror_axes"):
        mirror.flip_codes(bad)
    with pytest.raises(ValueError, match="mirror_axes"):      # checked before any device is touched
        sliding_window_inference(torch.zeros(1, 1, 4, 4, 4), 4, 1, lambda w: w, mirror_axes=bad)


def test_mirror_axes_is_keyword_only_and_defaults_to_none():
    import inspect
    from micformer_amd import inference, restore
    for fn in (inference.sliding_window_inference, restore.segment_pair):
        p = inspect.signature(fn).parameters["mirror_axes"]
        assert p.default == ()
    assert inspect.signature(inference.sliding_window_inference).parameters["mirror_axes"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- the referee ----------------------------------------------------------------------------------------------------------------

def _case(index, axes):
    shape, roi, overlap = SHAPES[index][:3]
    x = S.dyadic_input(shape, sum(shape))
    preds = [S.dyadic_predictor(c) for c in M.crops(x, roi, overlap, axes)]
    return shape, roi, overlap, x, preds


@pytest.mark.parametrize("shape,roi,overlap", sorted({s[:3] for s in SHAPES}))
@pytest.mark.parametrize("mode", MODES)
def test_referee_without_axes_is_the_blend_referee(shape, roi, overlap, mode):
    x = S.dyadic_input(shape, sum(shape))
    assert M.items(shape, roi, overlap, ()) == [w + (0,) for w in S.plan(shape, roi, overlap)[2]]
    got = M.sliding_window(x, S.dyadic_predictor, roi, overlap, (), mode=mode)
    assert torch.equal(got, S.sliding_window(x, S.dyadic_predictor, roi, overlap, mode=mode))


def test_items_are_window_major_and_crops_are_flipped_windows():
    shape, roi, overlap = SHAPES[4][:3]
    its = M.items(shape, roi, overlap, (0, 2))
    wins = S.plan(shape, roi, overlap)[2]
    assert its[:5] == [wins[0] + (0,), wins[0] + (1,), wins[0] + (4,), wins[0] + (5,), wins[1] + (0,)] and len(its) == 4 * len(wins)
    x = S.dyadic_input(shape, 1)
    c, plain = M.crops(x, roi, overlap, (0, 2)), S.crops(x, roi, overlap)
    assert torch.equal(c[4], plain[1]) and torch.equal(c[5], plain[1].flip(2)) and torch.equal(c[7], plain[1].flip(2, 4))
    assert torch.equal(M.flip(plain[0], 2), plain[0].flip(3)) and M.flip(plain[0], 0) is plain[0]


def _float32_restatement(shape, preds, roi, overlap, axes, mode):
    """The device's sums restated in float32 on the CPU: acc + w * p term by term in item order, then one division."""
    pads, padded, _ = S.plan(shape, roi, overlap)
    w, _ = S.importance_map(roi, mode)
    num = torch.zeros((shape[0], 3) + padded, dtype=torch.float32)
    den = torch.zeros((shape[0],) + padded, dtype=torch.float32)
    for (b, z, y, x, f), p in zip(M.items(shape, roi, overlap, axes), preds):
        num[b, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w * M.flip(p[0], f)
        den[b, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w
    out = num / den[:, None]
    (pd, ph, pw), (D, H, W) = pads, shape[2:]
    return out[:, :, pd // 2:pd // 2 + D, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W]


@pytest.mark.parametrize("index,axes", PAIRS)
@pytest.mark.parametrize("mode", MODES)
def test_float32_restatement_stays_inside_the_derived_bound_and_mirroring_matters(index, axes, mode):
    """The dyadic predictor's ramps run in WINDOW coordinates, so it is not flip-equivariant: mirroring changes the result."""
    shape, roi, overlap, x, preds = _case(index, axes)
    ref = M.blend(shape, preds, roi, overlap, axes, mode=mode)
    bound, n_max, F = M.bound(shape, roi, overlap, axes, preds)
    assert F == 2 ** len(axes) and len(preds) == F * len(S.plan(shape, roi, overlap)[2])
    err = float((_float32_restatement(shape, preds, roi, overlap, axes, mode).double() - ref).abs().max())
    plain = S.sliding_window(x, S.dyadic_predictor, roi, overlap, mode=mode)
    away = float((plain - ref).abs().max())
    print(f"{shape} roi {roi} axes {axes} {mode}: n_max {n_max}, F {F}, float32 error {err / bound:.3g} bounds, "
          f"un-mirrored {away / bound:.3g} bounds away")
    assert err <= bound
    assert away > 100 * bound


@pytest.mark.parametrize("index,axes", PAIRS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_bound_rejects_a_wrong_blend(mutation, mode, index, axes):
    """What the GPU comparison can see: each mutated referee leaves the derived bound measured against the true one.  Exchanging
    the D and W bits on the way back changes nothing where neither is mirrored, which is asserted too."""
    shape, roi, overlap, _, preds = _case(index, axes)
    ref = M.blend(shape, preds, roi, overlap, axes, mode=mode)
    bound, _, _ = M.bound(shape, roi, overlap, axes, preds)
    err = float((M.blend(shape, preds, roi, overlap, axes, mode=mode, mutate=mutation) - ref).abs().max())
    print(f"{mutation} {shape} axes {axes} {mode}: {err / bound:.3g} bounds")
    if mutation == "swap_bits" and not {0, 2} & set(axes):
        assert err == 0.0
    else:
        assert err > 100 * bound


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, mirror
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(mirror.SIGNATURES) == {"micf_sw_mirror_window_batch", "micf_sw_mirror_accumulate"}
    assert mirror.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert mirror.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {mirror.SIGNATURES[name]}"
        assert ret == "int" and name not in mirror.INT64_RETURNS, name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    # the arguments of the entry points they stand beside
    main = abi_header.parse_header("micformer_hip.h")
    assert d["micf_sw_mirror_window_batch"][1] == main["micf_sw_window_batch"][1]
    assert d["micf_sw_mirror_accumulate"][1] == abi_header.parse_header("micformer_blend.h")["micf_sw_blend_accumulate"][1]
    build = abi_header.build_module()
    assert "sliding_window.hip" in build.SOURCES


def test_table_is_disjoint_from_the_others_and_the_main_table_is_untouched():
    from micformer_amd import _lib, mirror
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(mirror.SIGNATURES) & set(other), module
    assert not set(mirror.SIGNATURES) & set(abi_header.parse_header("micformer_hip.h")) and len(_lib.SIGNATURES) == 97


def test_kernels_use_no_scratch():
    sizes, _, _ = abi_header.device_asm("sliding_window.hip")
    # the crop, the store-and-sum accumulate in 2 row forms x taps / no taps x flip / no flip, the atomic accumulate, the normalise
    assert len(sizes) == 11 and all("sw_" in k for k in sizes), sorted(sizes)
    assert sum("sw_accumulate_kernel" in k for k in sizes) == 8 and sum("sw_crop_kernel" in k for k in sizes) == 1
    assert set(sizes.values()) == {0}, sizes


def _coords(*rows):
    arr = (ctypes.c_int32 * (5 * len(rows)))(*[v for r in rows for v in r])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_invalid_arguments_return_error_codes_before_any_launch():
    """Validation reads host memory only, so it runs without a GPU (the pointers are never dereferenced on an error path)."""
    from micformer_amd.mirror import lib
    crop, acc = lib.micf_sw_mirror_window_batch, lib.micf_sw_mirror_accumulate
    EINVAL, EUNSUPPORTED = -1, -2
    keep, c = _coords((0, 0, 0, 0, 0))
    fake = 4096                                       # a non-NULL "device pointer"
    dims = (1, 1, 3, 16, 16, 16, 8, 8, 8)             # n, B, C | K, D, H, W, rd, rh, rw
    assert crop(None, fake, c, *dims, None) == EINVAL and crop(fake, None, c, *dims, None) == EINVAL
    assert crop(fake, fake, None, *dims, None) == EINVAL
    assert acc(None, fake, fake, c, *dims, fake, 1e-3, None) == EINVAL and acc(fake, None, fake, c, *dims, fake, 1e-3, None) == EINVAL
    assert acc(fake, fake, None, c, *dims, fake, 1e-3, None) == EINVAL and acc(fake, fake, fake, None, *dims, fake, 1e-3, None) == EINVAL
    assert acc(None, fake, fake, c, *dims, None, 1.0, None) == EINVAL                   # (NULL taps alone are no error: GPU test)
    for floor in (0.0, -1e-3, float("nan")):
        assert acc(fake, fake, fake, c, *dims, fake, floor, None) == EINVAL             # floor <= 0 with taps
    keep65, many = _coords(*[(0, 0, 0, 0, 0)] * 65)
    for n, cc in ((0, c), (-1, c), (65, many)):
        assert crop(fake, fake, cc, n, *dims[1:], None) == EINVAL, n
        assert acc(fake, fake, fake, cc, n, *dims[1:], fake, 1e-3, None) == EINVAL, n
        assert acc(fake, fake, fake, cc, n, *dims[1:], None, 1.0, None) == EINVAL, n
    for bad in [(1, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 9, 0, 0, 0), (0, 0, 9, 0, 0), (0, 0, 0, 9, 0), (0, -1, 0, 0, 0),
                (0, 0, 0, 0, 8), (0, 0, 0, 0, -1), (0, 8, 8, 8, 64)]:
        k, w = _coords(bad)
        assert crop(fake, fake, w, *dims, None) == EINVAL, bad
        assert acc(fake, fake, fake, w, *dims, fake, 1e-3, None) == EINVAL, bad
        assert acc(fake, fake, fake, w, *dims, None, 1.0, None) == EINVAL, bad
    k2, second = _coords((0, 8, 8, 8, 7), (0, 8, 8, 9, 0))                               # every item is checked, not the first
    assert crop(fake, fake, second, 2, *dims[1:], None) == EINVAL
    assert acc(fake, fake, fake, second, 2, *dims[1:], None, 1.0, None) == EINVAL
    big = (1, 1, 1, 2048, 1024, 1024, 2048, 1024, 1024)                                  # a window of 2^31 voxels
    assert crop(fake, fake, c, *big, None) == EUNSUPPORTED
    assert acc(fake, fake, fake, c, *big, fake, 1e-3, None) == EUNSUPPORTED and acc(fake, fake, fake, c, *big, None, 1.0, None) == EUNSUPPORTED
    k3, off = _coords((0, 1, 0, 0, 0))
    assert crop(fake, fake, off, *big, None) == EINVAL                                   # (leaving the volume comes first)
