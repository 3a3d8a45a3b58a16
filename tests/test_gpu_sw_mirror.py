"""Test-time mirroring on the device (micformer_amd.inference mirror_axes=, micformer_amd/mirror.py, csrc/sliding_window.hip) against the
float64 referee of tests/sw_mirror_ref.py fed the DEVICE's own per-item predictions.

The synthetic predictor is dyadic (every value exact in float32 on either side) and not flip-equivariant (its ramps run in window
coordinates), so the only error is the blend's and mirroring changes the result.  The bound is derived, not measured:
|got - ref| <= (3 n_max F + 2) * 2^-24 * max|p| with n_max the most windows on one voxel and F = 2^k flips of each (at most 2 n F
roundings in the numerator, n F in the denominator, one division).  tests/test_sw_mirror_cpu.py shows that a prediction that is
not flipped back, exchanged D / W bits, a dropped item and a denominator that counts a window once all leave this bound by
hundreds of bounds or more."""
import ctypes
import functools

import pytest
import torch

import sw_blend_ref as S
import sw_mirror_ref as M
from sw_head import filled_head as _head

pytestmark = pytest.mark.gpu

# (volume, roi, overlap, sw_batch_size): the shapes of tests/test_gpu_sw_blend.py
SHAPES = [((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 1), ((2, 2, 40, 24, 56), (16, 16, 16), 0.5, 7),
          ((1, 2, 20, 12, 37), (16, 16, 16), 0.25, 3), ((1, 2, 33, 16, 16), (16, 16, 16), 0.5, 4),
          ((1, 2, 24, 40, 17), (16, 24, 8), 0.5, 2), ((1, 2, 32, 16, 20), (16, 16, 16), 0.75, 64),
          ((1, 2, 10, 16, 20), (16, 16, 16), 0.5, 5)]
# (shape index, mirror axes)
CASES = [(0, (0, 1, 2)),      # two samples, all eight flips
         (2, (2,)),           # H padded; odd W: dword rows, reversed one float at a time
         (4, (0, 2)),         # non-cubic; n_max = 18
         (6, (1,)),           # image smaller than the ROI
         (3, (0, 1)),         # one extra voxel
         (1, (0, 1, 2)),      # sw 7: 768 items, no multiple of 7
         (5, (0, 1, 2))]      # sw 64: the cap of 64 items per call (80 items)
MODES = ("constant", "gaussian")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _predictions(index, axes):
    """-> (input, the device's prediction of every item, on the host).  Computed once per case."""
    shape, roi, overlap, _ = SHAPES[index]
    x = S.dyadic_input(shape, sum(shape))
    crops = M.crops(x, roi, overlap, axes)
    preds = [S.dyadic_predictor(c.cuda()).cpu() for c in crops]
    assert all(torch.equal(p, S.dyadic_predictor(c)) for p, c in zip(preds[:3], crops[:3]))     # (dyadic: same bits)
    return x, preds


@functools.lru_cache(maxsize=None)
def _case(index, axes, mode):
    """-> (input, referee, bound, n_max, F)."""
    shape, roi, overlap, _ = SHAPES[index]
    x, preds = _predictions(index, axes)
    bound, n_max, F = M.bound(shape, roi, overlap, axes, preds)
    return x, M.blend(shape, preds, roi, overlap, axes, mode=mode), bound, n_max, F


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("index,axes", CASES)
def test_mirrored_blend_matches_the_referee(index, axes, mode):
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    shape, roi, overlap, sw = SHAPES[index]
    x, ref, bound, n_max, F = _case(index, axes, mode)
    got = sliding_window_inference(x.cuda(), roi, sw, S.dyadic_predictor, overlap=overlap, mode=mode, mirror_axes=axes)
    plain = sliding_window_inference(x.cuda(), roi, sw, S.dyadic_predictor, overlap=overlap, mode=mode)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = float((got.cpu().double() - ref).abs().max())
    away = float((got - plain).abs().max())
    print(f"{shape} roi {roi} sw {sw} axes {axes} {mode}: n_max {n_max}, F {F}, error {err:.3g}, bound {bound:.3g}, "
          f"un-mirrored {away / bound:.3g} bounds away")
    assert err <= bound
    assert away > 100 * bound
    if index in (1, 5):
        items = len(M.items(shape, roi, overlap, axes))
        assert (items, items % sw) == ((768, 5) if index == 1 else (80, 16))     # a last chunk that is not full; more than 64 items


@pytest.mark.parametrize("mode", MODES)
def test_mirrored_blend_is_bit_identical_across_runs_and_batch_sizes(mode):
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    shape, roi, overlap, _ = SHAPES[0]
    x = _predictions(0, (0, 1, 2))[0].cuda()
    run = lambda sw: sliding_window_inference(x, roi, sw, S.dyadic_predictor, overlap=overlap, mode=mode, mirror_axes=(0, 1, 2))
    first = run(1)
    assert torch.equal(first, run(1))
    for sw in (3, 64):
        assert torch.equal(first, run(sw)), sw


def test_code_0_is_the_plain_crop_and_the_plain_blend():
    _need_gpu()
    from micformer_amd import blend, mirror, ops
    g = torch.Generator().manual_seed(5)
    vol = torch.randn((2, 3, 12, 16, 24), generator=g).cuda()
    chunk = [(0, 0, 0, 0), (1, 4, 8, 4), (0, 2, 4, 8), (0, 1, 3, 5)]        # (x0 = 5: dword rows)
    items = [c + (0,) for c in chunk]
    roi = (8, 8, 16)
    assert torch.equal(mirror.window_batch(vol, items, roi), ops.sw_window_batch(vol, chunk, roi))
    pred = torch.randn((4, 2) + roi, generator=g).cuda()
    taps, floor = blend.device_taps(roi, 0.125, "cuda")
    out_a, ws_a = torch.zeros(2, 2, 12, 16, 24, device="cuda"), torch.zeros(2, 12, 16, 24, device="cuda")
    out_b, ws_b = torch.zeros_like(out_a), torch.zeros_like(ws_a)
    for _ in range(2):                                                      # (the second round adds onto non-zero sums)
        blend.accumulate(pred, out_a, ws_a, chunk, taps, floor)
        mirror.accumulate(pred, out_b, ws_b, items, taps, floor)
    assert torch.equal(out_a, out_b) and torch.equal(ws_a, ws_b) and float(ws_a.sum()) > 0
    # without taps: w = 1, the constant mode's sums (exact for these few terms up to one rounding each: compare to float64)
    out_c, ws_c = torch.zeros_like(out_a), torch.zeros_like(ws_a)
    mirror.accumulate(pred, out_c, ws_c, items)
    want, cnt = torch.zeros(2, 2, 12, 16, 24, dtype=torch.float64), torch.zeros(2, 12, 16, 24)
    for (b, z, y, x), p in zip(chunk, pred.cpu()):
        want[b, :, z:z + 8, y:y + 8, x:x + 16] += p.double()
        cnt[b, z:z + 8, y:y + 8, x:x + 16] += 1
    assert torch.equal(ws_c.cpu(), cnt)
    assert float((out_c.cpu().double() - want).abs().max()) <= 3 * 2.0 ** -24 * float(want.abs().max())


@pytest.mark.parametrize("x0,W", [(4, 24), (3, 23)], ids=["16-byte rows", "dword rows"])
@pytest.mark.parametrize("code", range(8))
def test_every_code_is_torch_flip(code, x0, W):
    """A non-cubic (8, 12, 16) window, so that no two axes can stand in for each other: the crop is torch.flip of the plain crop,
    and a lone item in a zeroed accumulator is w * torch.flip(pred), exactly."""
    _need_gpu()
    from micformer_amd import blend, mirror
    roi, dims = (8, 12, 16), [a + 2 for a in range(3) if code >> a & 1]
    g = torch.Generator().manual_seed(code)
    vol = torch.randn((2, 3, 11, 14, W), generator=g).cuda()
    b, z0, y0 = 1, 3, 2
    win = mirror.window_batch(vol, [(b, z0, y0, x0, code)], roi)
    plain = vol[b:b + 1, :, z0:z0 + 8, y0:y0 + 12, x0:x0 + 16]
    assert win.shape == (1, 3) + roi and torch.equal(win, plain.flip(dims) if dims else plain)
    pred = torch.randn((1, 5) + roi, generator=g).cuda()
    w = blend.importance_map(roi, "gaussian", 0.125, device="cuda")
    taps, floor = blend.device_taps(roi, 0.125, "cuda")
    for t, wmap in ((taps, w), (None, torch.ones_like(w))):
        out, ws = torch.zeros(2, 5, 11, 14, W, device="cuda"), torch.zeros(2, 11, 14, W, device="cuda")
        mirror.accumulate(pred, out, ws, [(b, z0, y0, x0, code)], t, floor)
        back = pred[0].flip([d - 1 for d in dims]) if dims else pred[0]
        assert torch.equal(out[b, :, z0:z0 + 8, y0:y0 + 12, x0:x0 + 16], wmap * back)
        assert torch.equal(ws[b, z0:z0 + 8, y0:y0 + 12, x0:x0 + 16], wmap)
        out[b, :, z0:z0 + 8, y0:y0 + 12, x0:x0 + 16] = 0
        ws[b, z0:z0 + 8, y0:y0 + 12, x0:x0 + 16] = 0
        assert float(out.abs().sum()) == 0.0 and float(ws.abs().sum()) == 0.0                 # nothing else was written


def _off_by_one_float(shape):
    """A contiguous view of `shape` that starts one float past a 16-byte boundary, and its buffer."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.zeros(n + 1, device="cuda")
    view = buf[1:].view(shape)
    assert view.data_ptr() % 16 == 4
    return view, buf


def test_dword_and_16_byte_rows_give_the_same_bits():
    """The same items through the 16-byte rows (everything a multiple of 4) and the dword rows (volume and accumulator views one
    float off a 16-byte boundary; an odd x0 in either run), all eight codes; and a window of rw = 6, which has no 16-byte form, against
    torch.flip."""
    _need_gpu()
    from micformer_amd import blend, mirror
    g = torch.Generator().manual_seed(3)
    roi = (8, 8, 16)
    items = [(0, 0, 0, 0, 0), (1, 4, 8, 4, 4), (0, 2, 4, 8, 7), (0, 1, 3, 5, 5), (1, 0, 0, 8, 1), (0, 4, 8, 0, 2), (1, 3, 1, 3, 6),
             (0, 0, 8, 8, 3)]
    vol = torch.randn((2, 2, 12, 16, 24), generator=g).cuda()
    vol_b, _ = _off_by_one_float(vol.shape)
    vol_b.copy_(vol)
    win = mirror.window_batch(vol, items, roi)
    assert torch.equal(win, mirror.window_batch(vol_b, items, roi))
    for i, (b, z, y, x, f) in enumerate(items):
        assert torch.equal(win[i].cpu(), M.flip(vol[b, :, z:z + 8, y:y + 8, x:x + 16].cpu(), f)), i
    pred = torch.randn((8, 2) + roi, generator=g).cuda()
    taps, floor = blend.device_taps(roi, 0.125, "cuda")
    for t in (taps, None):
        out_a, ws_a = torch.zeros(2, 2, 12, 16, 24, device="cuda"), torch.zeros(2, 12, 16, 24, device="cuda")
        mirror.accumulate(pred, out_a, ws_a, items, t, floor)
        (out_b, buf_o), (ws_b, buf_w) = _off_by_one_float(out_a.shape), _off_by_one_float(ws_a.shape)
        mirror.accumulate(pred, out_b, ws_b, items, t, floor)
        assert torch.equal(out_a, out_b) and torch.equal(ws_a, ws_b) and float(ws_a.sum()) > 0
        assert float(buf_o[0]) == 0.0 and float(buf_w[0]) == 0.0
        # ... and the sums are the right ones: float64 of the same terms.  With n items on a voxel and w <= 1 every running sum stays
        # below n max|p|, and each of the n fused multiply-adds rounds once: at most n^2 2^-24 max|p| in all
        w = blend.importance_map(roi, "gaussian" if t is not None else "constant", 0.125).double()
        want, n = torch.zeros(2, 2, 12, 16, 24, dtype=torch.float64), torch.zeros(2, 12, 16, 24)
        for (b, z, y, x, f), p in zip(items, pred.cpu()):
            want[b, :, z:z + 8, y:y + 8, x:x + 16] += w * M.flip(p, f).double()
            n[b, z:z + 8, y:y + 8, x:x + 16] += 1
        assert float((out_a.cpu().double() - want).abs().max()) <= float(n.max()) ** 2 * 2.0 ** -24 * float(pred.abs().max())
    # rw = 6 in a volume of W = 20 (x0, W multiples of 4 or not: dword rows either way)
    roi6 = (4, 5, 6)
    vol6 = torch.randn((1, 2, 6, 7, 20), generator=g).cuda()
    items6 = [(0, 1, 2, 4, f) for f in range(8)] + [(0, 2, 0, 13, 4), (0, 0, 1, 14, 7)]
    win6 = mirror.window_batch(vol6, items6, roi6)
    pred6 = torch.randn((len(items6), 3) + roi6, generator=g).cuda()
    for i, (b, z, y, x, f) in enumerate(items6):
        assert torch.equal(win6[i].cpu(), M.flip(vol6[b, :, z:z + 4, y:y + 5, x:x + 6].cpu(), f)), i
        out, ws = torch.zeros(1, 3, 6, 7, 20, device="cuda"), torch.zeros(1, 6, 7, 20, device="cuda")
        mirror.accumulate(pred6[i:i + 1], out, ws, [items6[i]])
        assert torch.equal(out[0, :, z:z + 4, y:y + 5, x:x + 6].cpu(), M.flip(pred6[i].cpu(), f)) and float(ws.sum()) == 4 * 5 * 6


@pytest.mark.parametrize("mode", MODES)
def test_a_pointwise_predictor_gives_the_unmirrored_result(mode):
    """A predictor that works voxel by voxel commutes with every flip, so mirroring averages F equal predictions: the result is the
    un-mirrored referee's, within the mirrored bound."""
    _need_gpu()
    from micformer_amd.inference import sliding_window_inference
    shape, roi, overlap, sw = SHAPES[4]
    axes = (0, 1, 2)

    def pointwise(x):
        a, b = x[:, 0].float(), x[:, 1].float()
        return torch.stack([2 * a - b, a / 2 + b / 4, b - a], 1)

    x = S.dyadic_input(shape, sum(shape))
    preds = [pointwise(c) for c in S.crops(x, roi, overlap)]
    ref = S.blend(shape, preds, roi, overlap, mode=mode)
    bound, _, F = M.bound(shape, roi, overlap, axes, preds)
    got = sliding_window_inference(x.cuda(), roi, sw, pointwise, overlap=overlap, mode=mode, mirror_axes=axes)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"pointwise {mode}: F {F}, error {err:.3g}, bound {bound:.3g}")
    assert F == 8 and err <= bound


@pytest.mark.parametrize("mode", MODES)
def test_tiny_head_as_predictor_eager_graph_and_no_fused_epilogue(mode):
    """The tiny MicFormer Head (embed 24, depths 1-1-1-1) on 32^3 windows of a 48 x 32 x 64 volume under the flips of D and W: eager
    against the referee fed the very head(item) the blend received (a forward hook copies them: the head's logits differ in their
    last bits from call to call, and the bound has room for the blend's roundings only); graph=True against eager; and the Head's
    fused accumulate epilogue, which knows no flips, is never entered -- in the constant mode either, where it serves the
    un-mirrored call."""
    _need_gpu()
    from oracle import fill
    from micformer_amd.inference import GraphedPredictor, sliding_window_inference
    head = _head(24, (1, 1, 1, 1))
    calls = []
    inner = head.forward_accumulate
    head.forward_accumulate = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    x = fill.make_volume(1, 48, 32, 64, "SW.x")
    roi, axes = (32, 32, 32), (0, 2)
    preds = []
    with torch.no_grad():
        hook = head.register_forward_hook(lambda mod, args, y: preds.append(y.float().cpu()))
        got = sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5, mode=mode, mirror_axes=axes)
        hook.remove()
        its = M.items(x.shape, roi, 0.5, axes)
        assert len(preds) == len(its) == 24 and all(p.shape == (1, 8) + roi for p in preds)
        last = M.crops(x, roi, 0.5, axes)[-1].cuda()
        assert float((preds[-1] - head(last).float().cpu()).abs().max()) <= 1e-5          # (the hook did see the last item's logits)
        graphed = GraphedPredictor(head)
        got_g = sliding_window_inference(x.cuda(), roi, 4, graphed, overlap=0.5, mode=mode, mirror_axes=axes)
        assert len(graphed.graphs) == 1                                  # 24 items in chunks of 4: one shape, one graph
        got_g1 = sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5, mode=mode, mirror_axes=axes, graph=True)
        assert not calls
        if mode == "constant" and head.can_accumulate(roi):
            sliding_window_inference(x.cuda(), roi, 1, head, overlap=0.5)
            assert calls                                           # (the spy does see the un-mirrored call's fused path)
    ref = M.blend(x.shape, preds, roi, 0.5, axes, mode=mode)
    bound, n_max, F = M.bound(x.shape, roi, 0.5, axes, preds)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"tiny head {mode}: n_max {n_max}, F {F}, error {err:.3g}, bound {bound:.3g}, graph - eager "
          f"{float((got_g - got).abs().max()):.3g} / {float((got_g1 - got).abs().max()):.3g}")
    assert got.shape == (1, 8, 48, 32, 64) and err <= bound
    assert float((got_g - got).abs().max()) <= 1e-5 and float((got_g1 - got).abs().max()) <= 1e-5


def test_mirrored_logits_is_the_mean_of_the_predictions_flipped_back():
    _need_gpu()
    from oracle import fill
    from micformer_amd import mirror
    head = _head(24, (1, 1, 1, 1))
    x = fill.make_volume(1, 32, 32, 32, "SW.x").cuda()
    seen, preds = [], []
    hook = head.register_forward_hook(lambda mod, args, y: (seen.append(args[0].clone()), preds.append(y.float().cpu())) and None)
    got = mirror.mirrored_logits(head, x, (0, 1, 2))
    hook.remove()
    assert len(preds) == 8 and got.shape == (1, 8, 32, 32, 32) and got.dtype == torch.float32
    for f in range(8):
        assert torch.equal(seen[f], M.flip(x, f)), f                     # the model saw the flipped image, bit for bit
    want = sum(M.flip(p, f).double() for f, p in enumerate(preds)) / 8
    bound = (3 * 8 + 2) * 2.0 ** -24 * max(float(p.abs().max()) for p in preds)
    err = float((got.cpu().double() - want).abs().max())
    plain = float((got.cpu().double() - preds[0].double()).abs().max())
    print(f"mirrored_logits: error {err:.3g}, bound {bound:.3g}; the un-mirrored logits are {plain / bound:.3g} bounds away")
    assert err <= bound < plain
    assert mirror.mirrored_logits(head, x, ()).shape == got.shape and len(preds) == 8        # (no axes: one forward, hook removed)


def test_segment_pair_restores_the_mirrored_logits(monkeypatch):
    """segment_pair(mirror_axes=(0, 1, 2)) is restore_labels of mirror.mirrored_logits of the loaded pair (a RawBatch: the
    validation transform runs inside the Head, on the flipped raw image): a spy keeps the very logits (the Head's differ in their
    last bits from call to call), and the labels must be theirs exactly."""
    _need_gpu()
    import numpy as np
    from micformer_amd import data, loader, mirror, restore
    g = np.random.default_rng(41)
    shape, size = (41, 50, 37), (32, 32, 32)
    ct = torch.from_numpy(g.integers(-1000, 3000, size=shape, dtype=np.int16)).cuda()
    mr = torch.from_numpy(g.integers(0, 1500, size=shape, dtype=np.int16)).cuda()
    head = _head(24, (1, 1, 1, 1))
    kept = []
    inner = mirror.mirrored_logits

    def spy(model, x, axes):
        kept.append((x.clone(), tuple(axes), inner(model, x, axes)))
        return kept[-1][2]

    monkeypatch.setattr(mirror, "mirrored_logits", spy)
    seen = []
    hook = head.register_forward_hook(lambda mod, args, y: seen.append(args[0].image.clone()))
    got = restore.segment_pair(head, ct, mr, size=size, mirror_axes=(0, 1, 2))
    hook.remove()
    assert len(kept) == 1 and kept[0][1] == (0, 1, 2) and kept[0][0].shape == (1, 2) + size
    image, _, _ = loader.load_pair(ct, mr, None, size=size)
    x, _ = data.prepare_raw_batch(image.unsqueeze(0), None, None)
    assert isinstance(x, data.RawBatch) and x.params is None and torch.equal(kept[0][0].image, x.image)
    assert len(seen) == 8 and all(torch.equal(s.float(), M.flip(x.image.float(), f)) for f, s in enumerate(seen))    # the flipped raw image
    logits = kept[0][2]
    assert float((logits - inner(head, x, (0, 1, 2))).abs().max()) <= 1e-5
    assert got.shape == shape and got.dtype == torch.int16 and torch.equal(got, restore.restore_labels(logits, shape))
    restore.segment_pair(head, ct, mr, size=size)
    assert len(kept) == 1                                                 # no axes: the un-mirrored path, as before
    with torch.no_grad():
        plain = restore.restore_labels(head(x).float().contiguous(), shape)
    print(f"segment_pair: mirroring changes {float((plain != got).double().mean()):.3%} of the labels")
    assert not torch.equal(plain, got)


def test_entry_points_reject_bad_arguments_and_leave_the_buffers_alone():
    """MICF_EINVAL for n = 65, a window past the volume, a flip code of 8 and floor <= 0 with taps, with real device buffers and
    before any launch (the buffers stay zero); NULL taps alone are the constant mode."""
    _need_gpu()
    from micformer_amd import _lib, blend, mirror
    crop, acc = mirror.lib.micf_sw_mirror_window_batch, mirror.lib.micf_sw_mirror_accumulate
    vol, win = torch.ones(1, 3, 16, 16, 16, device="cuda"), torch.zeros(1, 3, 8, 8, 8, device="cuda")
    pred, out, ws = torch.ones(1, 3, 8, 8, 8, device="cuda"), torch.zeros(1, 3, 16, 16, 16, device="cuda"), torch.zeros(1, 16, 16, 16, device="cuda")
    taps, floor = blend.device_taps(8, 0.125, "cuda")
    v, wn, p, o, w, t, s = vol.data_ptr(), win.data_ptr(), pred.data_ptr(), out.data_ptr(), ws.data_ptr(), taps.data_ptr(), _lib.stream()

    def coords(*rows):
        arr = (ctypes.c_int32 * (5 * len(rows)))(*[x for r in rows for x in r])
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    keep, one = coords((0, 8, 8, 8, 5))
    dims = (1, 3, 16, 16, 16, 8, 8, 8)
    keep65, many = coords(*[(0, 0, 0, 0, 0)] * 65)
    assert crop(v, wn, many, 65, *dims, s) == -1 and acc(p, o, w, many, 65, *dims, t, floor, s) == -1
    assert acc(p, o, w, many, 65, *dims, None, 1.0, s) == -1
    for bad in [(0, 9, 8, 8, 0), (0, 8, 9, 8, 0), (0, 8, 8, 9, 0), (1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 8, 8, 8, 8), (0, 8, 8, 8, -1)]:
        k, c = coords(bad)
        assert crop(v, wn, c, 1, *dims, s) == -1, bad
        assert acc(p, o, w, c, 1, *dims, t, floor, s) == -1 and acc(p, o, w, c, 1, *dims, None, 1.0, s) == -1, bad
    assert acc(p, o, w, one, 1, *dims, t, 0.0, s) == -1 and acc(p, o, w, one, 1, *dims, t, -1e-3, s) == -1
    assert crop(None, wn, one, 1, *dims, s) == -1 and acc(p, None, w, one, 1, *dims, t, floor, s) == -1
    torch.cuda.synchronize()
    assert float(win.abs().sum()) == 0.0 and float(out.abs().sum()) == 0.0 and float(ws.sum()) == 0.0
    assert crop(v, wn, one, 1, *dims, s) == 0 and acc(p, o, w, one, 1, *dims, None, -1.0, s) == 0     # good arguments run; floor ignored
    torch.cuda.synchronize()
    assert float(win.sum()) == 3 * 512 and torch.equal(ws[0, 8:, 8:, 8:], torch.ones(8, 8, 8, device="cuda")) and float(ws[0, :8].sum()) == 0.0
    assert float(out.sum()) == 3 * 512
