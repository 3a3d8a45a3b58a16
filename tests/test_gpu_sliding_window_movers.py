"""The movers of sliding-window inference (csrc/sliding_window.hip) against torch slicing and float64 sums, entry point by entry
point.  The crop entry points share one kernel and the store-and-sum accumulates another, so comparing them with each other
(tests/test_gpu_sw_mirror.py) no longer says that either is right: here each is held to a reference of its own.  Predictions are
dyadic (multiples of 1/64), so every sum is exact in float32 and the comparisons are equalities."""
import pytest
import torch

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
ROI = (8, 12, 16)
# the chunk of test_gpu_sw_mirror.py::test_code_0_is_the_plain_crop_and_the_plain_blend (x0 = 5: dword rows), roi (8, 8, 16)
CHUNK = [(0, 0, 0, 0), (1, 4, 8, 4), (0, 2, 4, 8), (0, 1, 3, 5)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dyadic(shape, g):
    return (torch.randn(shape, generator=g) * 64).round() / 64


@pytest.mark.parametrize("x0,W", [(4, 24), (3, 23)], ids=["16-byte rows", "dword rows"])
def test_single_window_crop_and_accumulate(x0, W):
    """micf_sw_window is the torch slice; micf_sw_accumulate applied twice gives the float64 sum and a count of 2 inside the window,
    zeros outside; an origin that leaves the volume (or overflows int32 when the extent is added) is MICF_EINVAL before any launch."""
    _need_gpu()
    from micformer_amd import _lib
    crop, acc = _lib.lib.micf_sw_window, _lib.lib.micf_sw_accumulate
    g = torch.Generator().manual_seed(x0)
    D, H = 11, 14
    z0, y0 = 3, 2
    dims = (D, H, W) + ROI
    inside = (slice(None), slice(z0, z0 + ROI[0]), slice(y0, y0 + ROI[1]), slice(x0, x0 + ROI[2]))
    vol = torch.randn((3, D, H, W), generator=g).cuda()
    win = torch.zeros((3,) + ROI, device="cuda")
    s = _lib.stream()
    assert crop(vol.data_ptr(), win.data_ptr(), 3, *dims, z0, y0, x0, s) == 0
    assert torch.equal(win, vol[inside])
    preds = [_dyadic((3,) + ROI, g).cuda() for _ in range(2)]
    assert not torch.equal(preds[0], preds[1])
    out, count = torch.zeros(3, D, H, W, device="cuda"), torch.zeros(D, H, W, device="cuda")
    for p in preds:
        assert acc(p.data_ptr(), out.data_ptr(), count.data_ptr(), 3, *dims, z0, y0, x0, s) == 0
    want, cnt = torch.zeros(3, D, H, W, dtype=torch.float64), torch.zeros(D, H, W)
    want[inside] = preds[0].cpu().double() + preds[1].cpu().double()
    cnt[inside[1:]] = 2
    assert torch.equal(out.cpu().double(), want) and torch.equal(count.cpu(), cnt)
    for t in (win, out, count):
        t.zero_()
    for bad in [(-1, y0, x0), (z0, -1, x0), (z0, y0, -1), (z0 + 1, y0, x0), (z0, y0 + 1, x0), (z0, y0, W - ROI[2] + 1),
                (INT32_MAX, y0, x0), (z0, INT32_MAX, x0), (z0, y0, INT32_MAX)]:
        assert crop(vol.data_ptr(), win.data_ptr(), 3, *dims, *bad, s) == -1, bad
        assert acc(preds[0].data_ptr(), out.data_ptr(), count.data_ptr(), 3, *dims, *bad, s) == -1, bad
    torch.cuda.synchronize()
    assert float(win.abs().sum()) == 0.0 and float(out.abs().sum()) == 0.0 and float(count.sum()) == 0.0


def test_window_batch_is_the_torch_slice():
    _need_gpu()
    from micformer_amd import ops
    vol = torch.randn((2, 3, 12, 16, 24), generator=torch.Generator().manual_seed(5)).cuda()
    win = ops.sw_window_batch(vol, CHUNK, (8, 8, 16))
    assert torch.equal(win, torch.stack([vol[b, :, z:z + 8, y:y + 8, x:x + 16] for b, z, y, x in CHUNK]))


def test_blend_accumulate_adds_onto_running_sums_in_place():
    """Taps of ones and floor 1 make every weight 1, so with dyadic predictions two rounds over four overlapping windows are exact
    sums: order and addressing are pinned without leaning on how the fused multiply-add rounds."""
    _need_gpu()
    from micformer_amd import blend
    roi = (8, 8, 16)
    pred = _dyadic((4, 2) + roi, torch.Generator().manual_seed(7)).cuda()
    taps = torch.ones(sum(roi), device="cuda")
    out, ws = torch.zeros(2, 2, 12, 16, 24, device="cuda"), torch.zeros(2, 12, 16, 24, device="cuda")
    want, cnt = torch.zeros(2, 2, 12, 16, 24, dtype=torch.float64), torch.zeros(2, 12, 16, 24)
    for _ in range(2):
        blend.accumulate(pred, out, ws, CHUNK, taps, 1.0)
        for (b, z, y, x), p in zip(CHUNK, pred.cpu()):
            want[b, :, z:z + 8, y:y + 8, x:x + 16] += p.double()
            cnt[b, z:z + 8, y:y + 8, x:x + 16] += 1
    assert torch.equal(out.cpu().double(), want) and torch.equal(ws.cpu(), cnt) and float(cnt.max()) == 6
