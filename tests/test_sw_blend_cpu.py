"""Sliding-window inference with Gaussian blending, the CPU half: the importance map of micformer_amd.blend against its definition
(restated in tests/sw_blend_ref.py), the referee against the constant-mode oracle, the derived bound of the GPU comparison shown to
reject four wrong blends, and the C-ABI of include/micformer_blend.h (no GPU: header, ctypes table, exports, argument errors)."""
import ctypes
import importlib
import math

import pytest
import torch

import abi_header
import sw_blend_ref as S
from oracle import micformer_ref as R

HEADER = "micformer_blend.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "restore", "postprocess", "surface", "affine")
# (volume, roi, overlap, sw_batch_size): the shapes of tests/test_gpu_sw_blend.py
SHAPES = [((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 1), ((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 7),
          ((1, 2, 20, 12, 37), (16, 16, 16), 0.25, 3), ((1, 2, 33, 16, 16), (16, 16, 16), 0.5, 4),
          ((1, 2, 24, 40, 17), (16, 24, 8), 0.5, 2), ((1, 2, 32, 16, 20), (16, 16, 16), 0.75, 64),
          ((1, 2, 10, 16, 20), (16, 16, 16), 0.5, 5)]


# ---- the map ------------------------------------------------------------------------------------------------------------------

def test_map_at_16_cubed_sits_on_the_floor_of_1e_3():
    from micformer_amd import blend
    m = blend.importance_map(16, "gaussian", 0.125)
    ref, floor = S.importance_map((16, 16, 16), "gaussian", 0.125)
    assert m.dtype == torch.float32 and tuple(m.shape) == (16, 16, 16) and torch.equal(m, ref)
    assert floor == float(torch.tensor(1e-3, dtype=torch.float32)) == float(m.min()) == blend.gaussian_taps(16)[1]
    assert abs(float(m.max()) - 0.91051) < 5e-6
    assert abs(float((m == m.min()).double().mean()) - 0.576) < 1e-3


def test_map_at_4_cubed_is_not_clamped():
    from micformer_amd import blend
    m = blend.importance_map((4, 4, 4), "gaussian", 0.5)
    ref, floor = S.importance_map((4, 4, 4), "gaussian", 0.5)
    unfloored, _ = S.importance_map((4, 4, 4), "gaussian", 0.5, floored=False)
    assert torch.equal(m, ref) and torch.equal(m, unfloored)
    assert floor == float(m.min()) == blend.gaussian_taps(4, 0.5)[1] and abs(floor - 0.43009) < 5e-6


@pytest.mark.parametrize("roi,scale", [((16, 16, 16), 0.125), ((16, 24, 8), 0.125), ((16, 24, 8), (0.125, 0.25, 0.5)), ((5, 7, 3), 0.3)])
def test_map_matches_the_definition_and_is_symmetric(roi, scale):
    from micformer_amd import blend
    m = blend.importance_map(roi, "gaussian", scale)
    ref, floor = S.importance_map(roi, "gaussian", scale)
    assert tuple(m.shape) == roi and m.dtype == torch.float32 and torch.equal(m, ref)
    for axis in range(3):
        assert torch.equal(m, m.flip(axis)), axis
    # the separable closed form in float64, from scratch
    sc = [scale] * 3 if isinstance(scale, float) else scale
    g = [torch.exp(-((torch.arange(n, dtype=torch.float64) - (n - 1) / 2) ** 2) / (2 * (s * n) ** 2)) for n, s in zip(roi, sc)]
    want = (g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).clamp_min(floor)
    assert float((m.double() - want).abs().max()) <= 4 * 2.0 ** -24
    # what the device computes: two float32 multiplies in this order, then the clamp
    taps, fl = blend.gaussian_taps(roi, scale)
    assert fl == floor and [t.numel() for t in taps] == list(roi)
    z, y, x = roi[0] // 3, roi[1] - 1, roi[2] // 2
    assert float(m[z, y, x]) == max(float((taps[0][z] * taps[1][y]) * taps[2][x]), floor)


def test_per_axis_sigma_scale_changes_each_axis_on_its_own():
    from micformer_amd import blend
    a = blend.importance_map((8, 8, 8), "gaussian", (0.25, 0.25, 0.25))
    assert torch.equal(a, blend.importance_map(8, "gaussian", 0.25))
    b = blend.importance_map((8, 8, 8), "gaussian", (0.25, 0.25, 0.5))
    assert torch.allclose(b[:, :, 3] / b[3, 3, 3], a[:, :, 3] / a[3, 3, 3], rtol=1e-6, atol=0)     # axes 0 and 1 keep their profile
    assert float(b[3, 3, 0]) > float(a[3, 3, 0])                       # the wider axis falls off more slowly
    assert not torch.equal(b, b.transpose(0, 2)) and torch.equal(b, b.transpose(0, 1))


def test_constant_map_is_ones_and_ignores_sigma_scale():
    from micformer_amd import blend
    from micformer_amd.inference import importance_map
    assert importance_map is blend.importance_map
    assert torch.equal(importance_map((3, 4, 5)), torch.ones(3, 4, 5)) and importance_map(2, "constant", -1.0).dtype == torch.float32


@pytest.mark.parametrize("bad", [0.0, -0.125, (0.125, 0.125), (0.1, 0.2, 0.0), (0.1, 0.2, 0.3, 0.4), float("nan"), "wide", None])
def test_bad_sigma_scale_is_a_value_error(bad):
    from micformer_amd import blend
    with pytest.raises(ValueError, match="sigma_scale"):
        blend.importance_map(16, "gaussian", bad)


def test_unknown_mode_is_not_implemented():
    from micformer_amd import blend
    from micformer_amd.inference import sliding_window_inference
    with pytest.raises(NotImplementedError):
        blend.importance_map(16, "spline")
    with pytest.raises(NotImplementedError):
        sliding_window_inference(torch.zeros(1, 1, 4, 4, 4), 4, 1, lambda w: w, mode="spline")
    with pytest.raises(ValueError, match="sigma_scale"):      # checked before any device is touched
        sliding_window_inference(torch.zeros(1, 1, 4, 4, 4), 4, 1, lambda w: w, mode="gaussian", sigma_scale=(0.1, 0.2))


# ---- the referee ----------------------------------------------------------------------------------------------------------------

def _integer_predictor(scale):
    """K = 3 integer-valued channels (of an integer-valued window) times `scale`."""
    def predict(x):
        n, c, d, h, w = x.shape
        zz = torch.arange(d, dtype=torch.float32).view(1, d, 1, 1)
        yy = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
        xx = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
        a, b = x[:, 0].float(), x[:, 1].float()
        return scale * torch.stack([2 * a - b + zz, a + b + yy - xx, b - a + zz - yy], 1)
    return predict


@pytest.mark.parametrize("shape,roi,overlap", sorted({s[:3] for s in SHAPES}))
def test_referee_with_an_all_ones_map_is_the_constant_mode_oracle(shape, roi, overlap):
    """The oracle sums and divides in float32, so it is pinned to 1e-12 only where float32 is exact: integer predictions times the
    least common multiple of the visit counts (every sum and every quotient is then an integer below 2^24).  With the dyadic
    predictor of the GPU tests the sums are still exact and the oracle's one float32 division is all that separates the two."""
    counts = [int(c) for c in S.visits(shape, roi, overlap).unique()]
    g = torch.Generator().manual_seed(sum(shape))
    xi = torch.round(torch.randn(shape, generator=g) * 4)
    predict = _integer_predictor(float(math.lcm(*counts)))
    want = R.sliding_window_inference(xi, predict, roi=roi, overlap=overlap).double()
    got = S.sliding_window(xi, predict, roi, overlap, mode="constant")
    assert got.shape == want.shape == (shape[0], 3) + shape[2:] and float(want.abs().max()) * max(counts) < 2 ** 24
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(got, S.sliding_window(xi, predict, roi, overlap, wmap=torch.ones(roi)))
    x = S.dyadic_input(shape, sum(shape))
    want = R.sliding_window_inference(x, S.dyadic_predictor, roi=roi, overlap=overlap).double()
    got = S.sliding_window(x, S.dyadic_predictor, roi, overlap, mode="constant")
    assert float((got - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())


def _float32_restatement(shape, preds, roi, overlap, sigma_scale=0.125):
    """The device's sums restated in float32 on the CPU: acc + w * p term by term in window order, then one division."""
    pads, padded, wins = S.plan(shape, roi, overlap)
    w, _ = S.importance_map(roi, "gaussian", sigma_scale)
    num = torch.zeros((shape[0], 3) + padded, dtype=torch.float32)
    den = torch.zeros((shape[0],) + padded, dtype=torch.float32)
    for (b, z, y, x), p in zip(wins, preds):
        num[b, :, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w * p[0]
        den[b, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += w
    out = num / den[:, None]
    (pd, ph, pw), (D, H, W) = pads, shape[2:]
    return out[:, :, pd // 2:pd // 2 + D, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W]


@pytest.mark.parametrize("shape,roi,overlap", sorted({s[:3] for s in SHAPES}))
def test_float32_restatement_stays_inside_the_derived_bound(shape, roi, overlap):
    x = S.dyadic_input(shape, sum(shape))
    preds = [S.dyadic_predictor(c) for c in S.crops(x, roi, overlap)]
    ref = S.blend(shape, preds, roi, overlap)
    bound, n_max = S.bound(shape, roi, overlap, preds)
    err = float((_float32_restatement(shape, preds, roi, overlap).double() - ref).abs().max())
    print(f"{shape} roi {roi}: n_max {n_max}, float32 error {err:.3g}, bound {bound:.3g}")
    assert 0 < err <= bound / 2
    if roi == (16, 24, 8):
        assert n_max == 18


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_bound_rejects_a_wrong_blend(mutation):
    """What the GPU comparison can see: each mutated referee leaves the derived bound measured against the true one."""
    shape, roi, overlap = SHAPES[4][:3] if mutation == "swap_axes" else SHAPES[0][:3]     # (the swap needs the non-cubic roi)
    x = S.dyadic_input(shape, sum(shape))
    preds = [S.dyadic_predictor(c) for c in S.crops(x, roi, overlap)]
    ref = S.blend(shape, preds, roi, overlap)
    bound, _ = S.bound(shape, roi, overlap, preds)
    err = float((S.blend(shape, preds, roi, overlap, mutate=mutation) - ref).abs().max())
    print(f"{mutation}: error {err:.3g}, bound {bound:.3g}")
    assert err > 10 * bound


def test_swapped_taps_are_invisible_on_a_cubic_roi():
    """... which is why the GPU shapes include a non-cubic one."""
    assert torch.equal(S.importance_map((16, 16, 16), swap_axes=True)[0], S.importance_map((16, 16, 16))[0])


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, blend
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(blend.SIGNATURES) == {"micf_sw_blend_accumulate"}
    assert blend.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert blend.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {blend.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in blend.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert set(blend.INT64_RETURNS) <= set(d)
    # micf_sw_accumulate_batch's arguments, then the taps and the floor in front of the stream
    batch = abi_header.parse_header("micformer_hip.h")["micf_sw_accumulate_batch"][1]
    assert d["micf_sw_blend_accumulate"][1] == batch[:-1] + "pf" + batch[-1]
    build = abi_header.build_module()
    assert "sliding_window.hip" in build.SOURCES


def test_table_is_disjoint_from_the_others_and_the_main_table_is_untouched():
    from micformer_amd import _lib, blend
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(blend.SIGNATURES) & set(other), module
    assert "micf_sw_blend_accumulate" not in abi_header.parse_header("micformer_hip.h") and len(_lib.SIGNATURES) == 97


def test_invalid_arguments_return_einval_before_any_launch():
    """Validation reads host memory only, so it runs without a GPU (the pointers are never dereferenced on an error path)."""
    from micformer_amd.blend import lib
    f = lib.micf_sw_blend_accumulate
    one = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    c = ctypes.cast(one, ctypes.c_void_p)
    fake = 4096                                       # a non-NULL "device pointer"
    ok_tail = (1, 1, 3, 16, 16, 16, 8, 8, 8)
    assert f(None, fake, fake, c, *ok_tail, fake, 1e-3, None) == -1
    assert f(fake, fake, fake, None, *ok_tail, fake, 1e-3, None) == -1
    assert f(fake, fake, fake, c, *ok_tail, None, 1e-3, None) == -1                      # NULL taps
    assert f(fake, fake, fake, c, *ok_tail, fake, 0.0, None) == -1                       # floor <= 0
    assert f(fake, fake, fake, c, *ok_tail, fake, float("nan"), None) == -1
    assert f(fake, fake, fake, c, 0, 1, 3, 16, 16, 16, 8, 8, 8, fake, 1e-3, None) == -1  # n = 0
    many = (ctypes.c_int32 * (4 * 65))()
    assert f(fake, fake, fake, ctypes.cast(many, ctypes.c_void_p), 65, 1, 3, 16, 16, 16, 8, 8, 8, fake, 1e-3, None) == -1
    for bad in [(1, 0, 0, 0), (-1, 0, 0, 0), (0, 9, 0, 0), (0, 0, 9, 0), (0, 0, 0, 9), (0, -1, 0, 0)]:
        w = (ctypes.c_int32 * 4)(*bad)
        assert f(fake, fake, fake, ctypes.cast(w, ctypes.c_void_p), *ok_tail, fake, 1e-3, None) == -1, bad
