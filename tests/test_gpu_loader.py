"""GPU tests of the volume loader (micformer_amd/loader.py, csrc/volume_loader.hip) against the CPU referee tests/loader_ref.py and
the fixture made by the real reference loader (tests/golden/f11_loader.npz).

Bounds.  Class map and crop_indexes: exact.  Image with source size = target size: bit-identical (every tap weight is 0 or 1).
Image otherwise: every element within ONE fp16 step of the referee and at most 1e-3 of the elements different at all -- both sides
sum the same eight fp32 products; order and fma contraction move the fp32 sum by a few 2^-24 relative, which changes the fp16
rounding only when the sum lies that close to a rounding boundary (spacing 2^-11 relative)."""
import os

import numpy as np
import pytest
import torch

import loader_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f11_loader.npz")
MAX_SHARE = 1e-3
VALUES = np.array((0,) + R.MMWHS_LABEL_VALUES + (421, -3), np.int32)


def _image(g, shape, dtype):
    """A raw volume with a margin at its minimum (zero after normalisation) on some sides."""
    if dtype == np.int16:
        v = g.integers(-1000, 3000, size=shape, dtype=np.int16)
        lo = np.int16(-1024)
    else:
        v = g.random(shape, dtype=np.float32) * np.float32(900.0) + np.float32(0.5)
        lo = np.float32(0.0)
    for ax, n in enumerate(shape):
        cut = n // 9
        if cut:
            sl = [slice(None)] * 3
            sl[ax] = slice(0, cut)
            v[tuple(sl)] = lo
            sl[ax] = slice(n - cut // 2, n) if cut // 2 else slice(n, n)
            v[tuple(sl)] = lo
    v.flat[0] = lo
    return v


def _label(g, shape, dtype):
    return VALUES[g.integers(0, len(VALUES), size=shape)].astype(dtype)


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _compare(got, want, exact, tag):
    """got: device (image, label_map, crop); want: the referee's numpy triple."""
    image, cmap, crop = (None if t is None else t.cpu().numpy() for t in got)
    r_image, r_cmap, r_crop = want
    assert image.dtype == np.float16 and image.shape == r_image.shape
    assert np.array_equal(crop, r_crop), (tag, crop.tolist(), r_crop.tolist())
    if r_cmap is None:
        assert cmap is None
    else:
        assert cmap.dtype == np.uint8 and np.array_equal(cmap, r_cmap), tag
    steps = R.fp16_steps(image, r_image)
    share = float((steps != 0).mean())
    print(f"{tag}: share of image elements that differ from the referee {share:.3e}, max {int(steps.max())} fp16 step(s)")
    if exact:
        assert np.array_equal(image.view(np.uint16), r_image.view(np.uint16)), tag
    else:
        assert steps.max() <= 1, tag
        assert share <= MAX_SHARE, (tag, share)
    return share


CASES = {
    # name: (ct shape, ct dtype, mr shape, mr dtype, label dtype, target size)
    "full_363x512x512": ((363, 512, 512), np.int16, (363, 512, 512), np.float32, np.int16, (128, 128, 128)),
    "160x300x277": ((160, 300, 277), np.float32, (160, 300, 277), np.int16, np.int32, (128, 128, 128)),
    "up_50x70x90": ((50, 70, 90), np.int16, (50, 70, 90), np.float32, np.int16, (64, 96, 128)),
    "129x128x255": ((129, 128, 255), np.int16, (129, 128, 255), np.int16, np.int32, (128, 128, 128)),
    "extent_1": ((1, 45, 37), np.int16, (30, 1, 1), np.float32, np.int16, (24, 40, 56)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_loader_matches_referee(name):
    from micformer_amd import loader
    ct_shape, ct_dt, mr_shape, mr_dt, lab_dt, size = CASES[name]
    g = np.random.default_rng(len(name) + ct_shape[0])
    ct, mr, lab = _image(g, ct_shape, ct_dt), _image(g, mr_shape, mr_dt), _label(g, ct_shape, lab_dt)
    got = loader.load_pair(_dev(ct), _dev(mr), _dev(lab), size=size)
    assert got[0].shape == (2,) + size and got[1].shape == size and got[2].shape == (3, 2)
    want = R.load_pair(ct, mr, lab, size=size)
    assert (want[1] == 255).any()
    _compare(got, want, exact=False, tag=name)


def test_loader_matches_the_reference_loader_fixture():
    from micformer_amd import loader
    g = np.load(GOLDEN)
    a = R.f11_inputs(int(g["seed"]))
    image, cmap, crop = loader.load_pair(_dev(a["ct"]), _dev(a["mr"]), _dev(a["ct_label"]))
    st = int(g["stride"])
    assert np.array_equal(cmap.cpu().numpy(), g["class_map"])
    assert np.array_equal(crop.cpu().numpy(), g["crop_indexes"])
    steps = R.fp16_steps(image.cpu().numpy()[:, ::st, ::st, ::st], g["image_lattice"])
    print(f"f11: {int((steps != 0).sum())} of {steps.size} stored points differ from the reference, max {int(steps.max())} step(s)")
    assert steps.max() <= 1
    assert float((steps != 0).mean()) <= MAX_SHARE


@pytest.mark.parametrize("shape", [(32, 32, 32), (20, 24, 28)])
def test_identity_size_is_bit_identical(shape):
    """Source size = target size: the output is the rounded normalised value; this also pins the IEEE fp32 divide."""
    from micformer_amd import loader
    g = np.random.default_rng(shape[1])
    ct, mr, lab = _image(g, shape, np.int16), _image(g, shape, np.float32), _label(g, shape, np.int16)
    got = loader.load_pair(_dev(ct), _dev(mr), _dev(lab), size=shape)
    want = R.load_pair(ct, mr, lab, size=shape)
    _compare(got, want, exact=True, tag=f"identity {shape}")
    direct = np.stack([R.normalize(ct), R.normalize(mr)]).astype(np.float16)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint16), direct.view(np.uint16))


def test_no_label_and_all_zero_image():
    from micformer_amd import loader
    g = np.random.default_rng(5)
    ct, mr = _image(g, (17, 19, 23), np.int16), _image(g, (11, 29, 13), np.float32)
    got = loader.load_pair(_dev(ct), _dev(mr), size=(16, 24, 32))
    assert got[1] is None
    _compare(got, R.load_pair(ct, mr, None, size=(16, 24, 32)), exact=False, tag="no label")
    # every voxel at the minimum except the first one of the source, which the 8^3 output's taps do not reach with weight > 0 ...
    ct = np.zeros((64, 64, 64), np.int16)
    ct[0, 0, 0] = 100
    mr = np.zeros((64, 64, 64), np.float32)
    mr[0, 0, 0] = 2.0
    got = loader.load_pair(_dev(ct), _dev(mr), size=(8, 8, 8))
    want = R.load_pair(ct, mr, None, size=(8, 8, 8))
    assert not want[0].any()                                          # ... so the resized image is all zero
    assert np.array_equal(got[2].cpu().numpy(), np.zeros((3, 2), np.int32))
    _compare(got, want, exact=True, tag="all zero")


def test_constant_volume_gives_nan_like_the_reference():
    from micformer_amd import loader
    g = np.random.default_rng(6)
    ct = np.full((9, 10, 11), 37, np.int16)
    mr = _image(g, (9, 10, 11), np.float32)
    image, _, crop = loader.load_pair(_dev(ct), _dev(mr), size=(12, 12, 12))
    r_image, _, r_crop = R.load_pair(ct, mr, None, size=(12, 12, 12))
    image = image.cpu().numpy()
    assert np.isnan(r_image[0]).all() and np.isnan(image[0]).all()
    assert R.fp16_steps(image[1], r_image[1]).max() <= 1
    assert np.array_equal(crop.cpu().numpy(), r_crop) and np.array_equal(r_crop, [[0, 12]] * 3)      # NaN != 0 everywhere
    image, _, _ = loader.load_pair(_dev(mr), _dev(np.full((4, 4, 4), 0.25, np.float32)), size=(12, 12, 12))
    assert np.isnan(image[1].cpu().numpy()).all() and not np.isnan(image[0].cpu().numpy()).any()


def test_int16_range_beyond_32767_uses_int32_arithmetic():
    """The documented deviation: the reference's int16 `image - min` wraps here; the loader gives the int32 result."""
    from micformer_amd import loader
    g = np.random.default_rng(7)
    shape = (24, 24, 24)
    ct = g.integers(-32768, 32768, size=shape, dtype=np.int16)
    ct.flat[5], ct.flat[77] = -32768, 32767
    mr = _image(g, shape, np.int16)
    got = loader.load_pair(_dev(ct), _dev(mr), size=shape)
    want = R.load_pair(ct.astype(np.int32), mr.astype(np.int32), None, size=shape)
    _compare(got, want, exact=True, tag="wide int16 (identity size)")
    got = loader.load_pair(_dev(ct), _dev(mr), size=(16, 20, 36))
    want = R.load_pair(ct.astype(np.int32), mr.astype(np.int32), None, size=(16, 20, 36))
    _compare(got, want, exact=False, tag="wide int16")
    assert float(got[0].min()) >= 0.0 and float(got[0].max()) <= 1.0   # (int16 arithmetic would leave [0, 1])


def _batch(g, n, with_label=True):
    samples = []
    for i in range(n):
        cs = (11 + 7 * i % 23, 30 - i, 17 + 3 * i)
        ms = (25 - 2 * i % 9, 13 + i, 41 - 3 * i)
        ct = _image(g, cs, np.int16 if i % 2 == 0 else np.float32)
        mr = _image(g, ms, np.float32 if i % 3 == 0 else np.int16)
        lab = _label(g, (cs[0] + 1, cs[1], cs[2] + 2), np.int16 if i % 2 else np.int32) if with_label else None
        samples.append((ct, mr, lab))
    return samples


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.uint8) if x.dtype == torch.float16 else x,
                                                        y.view(torch.uint8) if y.dtype == torch.float16 else y)
               for x, y in zip(a, b))


def test_load_batch_equals_load_pair_and_is_deterministic():
    from micformer_amd import loader
    g = np.random.default_rng(8)
    size = (24, 32, 40)
    host = _batch(g, 3)
    dev = [tuple(_dev(a) for a in s) for s in host]
    image, cmap, crop = loader.load_batch(dev, size=size)
    assert image.shape == (3, 2) + size and cmap.shape == (3,) + size and crop.shape == (3, 3, 2)
    for b in range(3):
        assert _same(loader.load_pair(*dev[b], size=size), (image[b], cmap[b], crop[b])), b
        _compare((image[b], cmap[b], crop[b]), R.load_pair(*host[b], size=size), exact=False, tag=f"batch sample {b}")
    out = (torch.full_like(image, 7.0), torch.full_like(cmap, 9), torch.full_like(crop, -5))
    res = loader.load_batch(dev, size=size, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
    assert _same(out, (image, cmap, crop))                            # a second run: bit-identical
    with pytest.raises(ValueError):
        loader.load_batch(dev, size=size, out=(out[0], None, out[2]))
    with pytest.raises(ValueError):
        loader.load_batch(dev, size=size, out=(out[0].float(), out[1], out[2]))
    with pytest.raises(ValueError):
        loader.load_batch([dev[0], (dev[1][0], dev[1][1], None)], size=size)          # mixed label presence
    with pytest.raises(ValueError):
        loader.load_pair(dev[0][0].transpose(0, 1), dev[0][1], size=size)              # not contiguous
    with pytest.raises(ValueError):
        loader.load_pair(dev[0][0][0], dev[0][1], size=size)                           # wrong rank


def test_load_batch_beyond_one_launch_chunk_and_unaligned_sources():
    """11 samples (the descriptors travel 8 per launch), sources that start off a 16-byte boundary with odd element counts."""
    from micformer_amd import loader
    g = np.random.default_rng(9)
    size = (16, 16, 24)
    host = _batch(g, 11)
    dev = []
    for ct, mr, lab in host:
        off = []
        for a in (ct, mr, lab):
            buf = torch.empty(a.size + 3, dtype=torch.from_numpy(a).dtype, device="cuda")
            buf[3:].copy_(torch.from_numpy(a).reshape(-1))
            off.append(buf[3:].view(a.shape))
        assert off[0].data_ptr() % 16 != 0 and off[0].is_contiguous()
        dev.append(tuple(off))
    image, cmap, crop = loader.load_batch(dev, size=size)
    for b in range(11):
        _compare((image[b], cmap[b], crop[b]), R.load_pair(*host[b], size=size), exact=False, tag=f"chunked sample {b}")


def test_capture_and_replay_under_a_graph():
    from micformer_amd import loader
    g = np.random.default_rng(10)
    size = (24, 24, 24)
    host = _batch(g, 2)
    dev = [tuple(_dev(a) for a in s) for s in host]
    eager = loader.load_batch(dev, size=size)
    out = (torch.zeros_like(eager[0]), torch.zeros_like(eager[1]), torch.zeros_like(eager[2]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loader.load_batch(dev, size=size, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    # new contents in the same source buffers: the replay reads them
    host2 = _batch(np.random.default_rng(11), 2)
    for d, h in zip(dev, host2):
        for t, a in zip(d, h):
            t.copy_(torch.from_numpy(a))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, loader.load_batch(dev, size=size))
    assert not _same(out, eager)


def test_end_to_end_loss_bits_match_the_referee_fed_chain():
    """load_batch -> data.prepare_raw_batch -> tiny Head -> MDiceLoss against the same chain fed with the referee's sample; source
    size = target size 32^3, so the loader's image is bit-identical to the referee's."""
    from micformer_amd import data, loader
    from micformer_amd.loss.dice import MDiceLoss
    from micformer_amd.models.MICFormer_self import Head
    from oracle import fill
    g = np.random.default_rng(12)
    shape = (32, 32, 32)
    host = [(_image(g, shape, np.int16), _image(g, shape, np.float32), _label(g, shape, np.int16)) for _ in range(2)]
    image, cmap, _ = loader.load_batch([tuple(_dev(a) for a in s) for s in host], size=shape)
    ref = [R.load_pair(*s, size=shape) for s in host]
    r_image = torch.from_numpy(np.stack([r[0] for r in ref])).cuda()
    r_cmap = torch.from_numpy(np.stack([r[1] for r in ref])).cuda()
    assert int((cmap == 255).sum()) > 0
    assert torch.equal(image.view(torch.int16), r_image.view(torch.int16)) and torch.equal(cmap, r_cmap)
    model = Head(embed_dim=24, num_classes=8, depths=(1, 1, 1, 1))
    with torch.no_grad():
        for name, t in model.state_dict().items():
            t.copy_(fill.fill_tensor(name, t))
    model = model.cuda().eval()
    params = torch.tensor([[1, 0, 1, 0.07, -0.03], [0, 1, 0, -0.05, 0.09]], dtype=torch.float32).cuda()
    crit = MDiceLoss()
    losses = []
    for img, lab in ((image, cmap), (r_image, r_cmap)):
        x, y = data.prepare_raw_batch(img, lab, params)
        with torch.no_grad():
            losses.append(crit(model(x), y).float().reshape(1).clone())
    assert torch.isfinite(losses[0]).all()
    assert torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32)), (float(losses[0]), float(losses[1]))
