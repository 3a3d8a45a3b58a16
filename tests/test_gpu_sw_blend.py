"""Sliding-window inference with Gaussian blending on the device (micformer_amd.inference mode="gaussian", csrc/sliding_window.hip) against
the float64 referee of tests/sw_blend_ref.py fed the DEVICE's own per-window predictions.

The synthetic predictor is dyadic (every value exact in float32 on either side), so the only error is the blend's, and the bound is
derived, not measured: |got - ref| <= (3 n_max + 2) * 2^-24 * max|p| with n_max the most windows on one voxel (at most 2 n roundings
in the numerator, n in the denominator, one division).  tests/test_sw_blend_cpu.py shows that an unfloored map, a dropped window, a
division by the visit count and swapped tap vectors all leave this bound by orders of magnitude."""
import ctypes
import functools

import pytest
import torch

import sw_blend_ref as S
from sw_head import filled_head as _head

pytestmark = pytest.mark.gpu

# (volume, roi, overlap, sw_batch_size)
SHAPES = [((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 1),      # two samples in one batch
          ((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 7),      # ... and a window count (60) that is no multiple of 7
          ((1, 2, 20, 12, 37), (16, 16, 16), 0.25, 3),     # H padded; odd W: dword rows; the clipped last start at an odd x0 (21)
          ((1, 2, 33, 16, 16), (16, 16, 16), 0.5, 4),      # one extra voxel
          ((1, 2, 24, 40, 17), (16, 24, 8), 0.5, 2),       # non-cubic; n_max = 18
          ((1, 2, 32, 16, 20), (16, 16, 16), 0.75, 64),    # the cap of 64 windows per call
          ((1, 2, 10, 16, 20), (16, 16, 16), 0.5, 5)]      # image smaller than the ROI


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _case(shape, roi, overlap, sigma_scale=0.125):
    """-> (input, referee, bound, n_max); the predictions are the device's, window by window.  Computed once per case."""
    x = S.dyadic_input(shape, sum(shape))
    preds = [S.dyadic_predictor(c.cuda()).cpu() for c in S.crops(x, roi, overlap)]
    assert all(torch.equal(p, S.dyadic_predictor(c)) for p, c in zip(preds[:3], S.crops(x, roi, overlap)[:3]))     # (dyadic: same bits)
    ref = S.blend(shape, preds, roi, overlap, sigma_scale=sigma_scale)
    bound, n_max = S.bound(shape, roi, overlap, preds)
    return x, ref, bound, n_max


@pytest.mark.parametrize("shape,roi,overlap,sw", SHAPES)
def test_gaussian_blend_matches_the_referee(shape, roi, overlap, sw):
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    x, ref, bound, n_max = _case(shape, roi, overlap)
    got = sliding_window_inference(x.cuda(), roi, sw, S.dyadic_predictor, overlap=overlap, mode="gaussian")
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = float((got.cpu().double() - ref).abs().max())
    print(f"{shape} roi {roi} sw {sw}: n_max {n_max}, error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    if roi == (16, 24, 8):
        assert n_max == 18


def test_gaussian_blend_is_bit_identical_across_runs_and_batch_sizes():
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    shape, roi, overlap, _ = SHAPES[0]
    x = _case(shape, roi, overlap)[0].cuda()
    first = sliding_window_inference(x, roi, 1, S.dyadic_predictor, overlap=overlap, mode="gaussian")
    again = sliding_window_inference(x, roi, 1, S.dyadic_predictor, overlap=overlap, mode="gaussian")
    assert torch.equal(first, again)
    for sw in (3, 64):
        assert torch.equal(first, sliding_window_inference(x, roi, sw, S.dyadic_predictor, overlap=overlap, mode="gaussian")), sw


def test_dword_and_16_byte_rows_give_the_same_bits():
    """The same windows through the 16-byte rows (everything a multiple of 4) and the dword rows (accumulator views one float off a
    16-byte boundary): one accumulate expression, so bit-equal sums."""
    _need_gpu()
    from micformer_amd import blend
    g = torch.Generator().manual_seed(3)
    pred = torch.randn((4, 2, 8, 8, 16), generator=g).cuda()
    chunk = [(0, 0, 0, 0), (1, 4, 8, 4), (0, 2, 4, 8), (0, 1, 3, 5)]        # (x0 = 5: dword rows for this window in either run)
    taps, floor = blend.device_taps((8, 8, 16), 0.125, "cuda")
    out_a, ws_a = torch.zeros(2, 2, 12, 16, 24, device="cuda"), torch.zeros(2, 12, 16, 24, device="cuda")
    blend.accumulate(pred, out_a, ws_a, chunk, taps, floor)
    buf_o, buf_w = torch.zeros(2 * 2 * 12 * 16 * 24 + 1, device="cuda"), torch.zeros(2 * 12 * 16 * 24 + 1, device="cuda")
    out_b, ws_b = buf_o[1:].view(2, 2, 12, 16, 24), buf_w[1:].view(2, 12, 16, 24)
    assert out_b.data_ptr() % 16 == 4
    blend.accumulate(pred, out_b, ws_b, chunk, taps, floor)
    assert torch.equal(out_a, out_b) and torch.equal(ws_a, ws_b) and float(ws_a.sum()) > 0
    w = blend.importance_map((8, 8, 16), "gaussian", 0.125, device="cuda")
    assert torch.equal(ws_a[1, 4:12, 8:16, 4:20], w) and torch.equal(out_a[1, :, 4:12, 8:16, 4:20], w * pred[1])   # window 1 is alone in its sample
    assert float(buf_o[0]) == 0.0 and float(buf_w[0]) == 0.0
    want = torch.zeros(2, 12, 16, 24, dtype=torch.float64)
    for b, z, y, x in chunk:
        want[b, z:z + 8, y:y + 8, x:x + 16] += w.cpu().double()
    assert float((ws_a.cpu().double() - want).abs().max()) <= 3 * 2.0 ** -24 * float(want.max())


@pytest.mark.parametrize("shape,roi,overlap,sw", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_constant_predictions_come_back_unchanged(shape, roi, overlap, sw):
    """A predictor that returns one constant per class gives it back everywhere within 2 float32 steps -- for constants that are
    powers of two: the numerator is then the weight sum scaled exactly, term by term, so any difference means that numerator and
    denominator saw different weights or windows.  For other constants float32 itself does not allow 2 steps (the CPU float32
    restatement of the same sums is off by up to 7 steps at n_max = 8 and 12 at n_max = 18); they are held to the derived bound."""
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    const = torch.tensor([0.25, -2.0, 128.0, 0.3, -1.7, 123.456], dtype=torch.float32)

    def predictor(win):
        return const.to(win.device).view(1, 6, 1, 1, 1).expand(win.shape[0], 6, *win.shape[2:]).contiguous()

    got = sliding_window_inference(torch.zeros(shape, device="cuda"), roi, sw, predictor, overlap=overlap, mode="gaussian").cpu()
    n_max = int(S.visits(shape, roi, overlap).max())
    for k in range(6):
        step = float(torch.nextafter(const[k].abs(), torch.tensor(float("inf"))) - const[k].abs())
        err = float((got[:, k] - const[k]).abs().max())
        print(f"{shape} class {k} ({float(const[k])}): {err / step:.1f} steps")
        assert err <= (2 * step if k < 3 else (3 * n_max + 2) * 2.0 ** -24 * float(const[k].abs())), (k, err / step)


def test_per_axis_sigma_scale_matches_the_referee():
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    shape, roi, overlap, sw = SHAPES[4]
    scale = (0.125, 0.25, 0.5)
    x, ref, bound, _ = _case(shape, roi, overlap, scale)
    got = sliding_window_inference(x.cuda(), roi, sw, S.dyadic_predictor, overlap=overlap, mode="gaussian", sigma_scale=scale)
    assert float((got.cpu().double() - ref).abs().max()) <= bound
    assert float((ref - _case(shape, roi, overlap)[1]).abs().max()) > 100 * bound            # (the scales do matter)


def test_importance_map_on_the_device_is_the_host_map():
    _need_gpu()
    from micformer_amd.inference import importance_map
    assert torch.equal(importance_map((16, 24, 8), "gaussian", 0.125, device="cuda").cpu(), S.importance_map((16, 24, 8))[0])


def test_tiny_head_as_predictor_eager_graph_and_no_fused_epilogue():
    """The tiny MicFormer Head (embed 24, depths 1-1-1-1) on 32^3 windows of a 48 x 32 x 64 volume: eager against the referee fed
    head(window) from the same device; graph=True against eager; and the Head's fused accumulate epilogue, which knows no
    weights, is never entered in Gaussian mode (it is in constant mode)."""
    _need_gpu()
    from oracle import fill
    from micformer_amd.inference import sliding_window_inference
    head = _head(24, (1, 1, 1, 1))
    calls = []
    inner = head.forward_accumulate
    head.forward_accumulate = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    x = fill.make_volume(1, 48, 32, 64, "SW.x")
    roi = (32, 32, 32)
    # The referee is fed the very predictions the blend received (a forward hook copies each head(window) of the eager run): the
    # head's own logits differ in their last bits from one call to the next (atomically added partial sums; printed below), and
    # the bound has room for the blend's roundings only.
    preds = []
    with torch.no_grad():
        c0 = S.crops(x, roi, 0.5)[0].cuda()
        again = float((head(c0) - head(c0)).abs().max())
        hook = head.register_forward_hook(lambda mod, args, y: preds.append(y.float().cpu()))
        got = sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5, mode="gaussian")
        hook.remove()
        assert len(preds) == len(S.plan(x.shape, roi, 0.5)[2]) and all(p.shape == (1, 8) + roi for p in preds)
        direct = head(S.crops(x, roi, 0.5)[-1].cuda()).float().cpu()
        print(f"head(window) twice: {again:.3g} apart; hooked vs direct prediction of the last window: {float((preds[-1] - direct).abs().max()):.3g}")
        assert float((preds[-1] - direct).abs().max()) <= 1e-5          # (the hook did see this window's logits)
        got_g = sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5, mode="gaussian", graph=True)
        assert not calls
        if head.can_accumulate(roi):
            sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5)
            assert calls                                           # (the spy does see the constant mode's fused path)
    ref = S.blend(x.shape, preds, roi, 0.5)
    bound, n_max = S.bound(x.shape, roi, 0.5, preds)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"tiny head: n_max {n_max}, error {err:.3g}, bound {bound:.3g}, graph - eager {float((got_g - got).abs().max()):.3g}")
    assert got.shape == (1, 8, 48, 32, 64) and err <= bound
    assert float((got_g - got).abs().max()) <= 1e-5


def test_entry_point_rejects_bad_arguments():
    """MICF_EINVAL for n = 65, a window past the volume, NULL taps and floor <= 0, with real device buffers and before any launch
    (the buffers stay zero)."""
    _need_gpu()
    from micformer_amd import _lib, blend
    f = blend.lib.micf_sw_blend_accumulate
    pred, out, ws = torch.ones(1, 3, 8, 8, 8, device="cuda"), torch.zeros(1, 3, 16, 16, 16, device="cuda"), torch.zeros(1, 16, 16, 16, device="cuda")
    taps, floor = blend.device_taps(8, 0.125, "cuda")
    p, o, w, t, s = pred.data_ptr(), out.data_ptr(), ws.data_ptr(), taps.data_ptr(), _lib.stream()

    def coords(*rows):
        arr = (ctypes.c_int32 * (4 * len(rows)))(*[v for r in rows for v in r])
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    keep, one = coords((0, 8, 8, 8))
    dims = (1, 3, 16, 16, 16, 8, 8, 8)
    keep65, many = coords(*[(0, 0, 0, 0)] * 65)
    assert f(p, o, w, many, 65, *dims, t, floor, s) == -1
    for bad in [(0, 9, 8, 8), (0, 8, 9, 8), (0, 8, 8, 9), (1, 0, 0, 0), (0, -1, 0, 0)]:
        k, c = coords(bad)
        assert f(p, o, w, c, 1, *dims, t, floor, s) == -1, bad
    assert f(p, o, w, one, 1, *dims, None, floor, s) == -1
    assert f(p, o, w, one, 1, *dims, t, 0.0, s) == -1 and f(p, o, w, one, 1, *dims, t, -1e-3, s) == -1
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(ws.sum()) == 0.0
    assert f(p, o, w, one, 1, *dims, t, floor, s) == 0                       # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert torch.equal(ws[0, 8:, 8:, 8:], blend.importance_map(8, "gaussian", device="cuda")) and float(ws[0, :8].sum()) == 0.0
