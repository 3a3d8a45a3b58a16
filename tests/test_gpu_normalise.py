"""GPU tests of the loader's z-score / percentile-clip normalisations (micformer_amd/normalise.py, csrc/volume_normalise.hip) against
the CPU referee tests/normalise_ref.py and the fixture made by the real reference functions (tests/golden/f12_normalise.npz).

Bounds.  Class map and crop_indexes: exact.  A "minmax" channel: bit-equal to what load_pair gives without the keyword.  A "zscore"
or "percentile" channel: normalise_ref.close -- every element within one fp16 step OR within A = 2^-20 * max(1, max |referee|), and at
most 1e-3 of the elements different and more than A away (the referee's docstring has the reasoning).  stats: min / max exact,
mean / std within 1e-9 relative of numpy on float64, percentiles within 4 float64 ulp of np.percentile on float64."""
import os

import numpy as np
import pytest
import torch

import loader_ref as R
import normalise_ref as N
from tiny_model import tiny_head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f12_normalise.npz")
VALUES = np.array((0,) + R.MMWHS_LABEL_VALUES + (421, -3), np.int32)
TINY = (2, 2, 2)                           # target of the tests that read `stats` alone


def _raw(g, shape, dtype):
    """A raw volume with zero margins on some sides, zeros inside, negatives and positives."""
    if dtype == np.int16:
        v = g.integers(-400, 2000, size=shape, dtype=np.int16)
    else:
        v = (g.random(shape, dtype=np.float32) * np.float32(1500.0) - np.float32(200.0))
    v[g.random(shape) < 0.05] = 0
    for ax, n in enumerate(shape):
        cut = n // 9
        if cut:
            sl = [slice(None)] * 3
            sl[ax] = slice(0, cut)
            v[tuple(sl)] = 0
            sl[ax] = slice(n - cut // 2, n) if cut // 2 else slice(n, n)
            v[tuple(sl)] = 0
    return v


def _label(g, shape, dtype=np.int16):
    return VALUES[g.integers(0, len(VALUES), size=shape)].astype(dtype)


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _pair(normalisation):
    return (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)


def _check_stats(stats, want, modes, tag):
    stats = stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (2, 2)
    for c, mode in enumerate(modes):
        for j in range(2):
            got, ref = stats[c, j], want[c, j]
            if mode == "minmax":
                assert got == ref, (tag, c, j, got, ref)
            elif mode == "percentile":
                d = N.ulps(got, ref)
                print(f"{tag}: channel {c} percentile {j}: {got!r} vs numpy {ref!r}: {d} ulp")
                assert d <= 4, (tag, c, j, got, ref)
            else:
                if np.isnan(ref):
                    assert np.isnan(got), (tag, c, j, got)
                    continue
                rel = abs(got - ref) / abs(ref) if ref != 0 else abs(got)
                print(f"{tag}: channel {c} {'mean' if j == 0 else 'std'}: {got!r} vs numpy {ref!r}: relative {rel:.2e}")
                assert rel <= 1e-9, (tag, c, j, got, ref)


def _check(host, size, normalisation, percentiles=(1, 99), tag="", dev=None):
    """One load_pair call (on the device tensors `dev`, by default copies of `host`) against the referee: every output and stats."""
    from micformer_amd import loader
    modes = _pair(normalisation)
    ct, mr, lab = host
    dev = tuple(_dev(a) for a in host) if dev is None else dev
    got = loader.load_pair(*dev, size=size, normalisation=normalisation, percentiles=percentiles, return_stats=True)
    image, cmap, crop, stats = got
    r_image, r_cmap, r_crop, r_stats = N.load_pair(ct, mr, lab, size=size, normalisation=modes, percentiles=percentiles)
    assert image.dtype == torch.float16 and tuple(image.shape) == (2,) + tuple(size)
    assert np.array_equal(crop.cpu().numpy(), r_crop), (tag, crop.tolist(), r_crop.tolist())
    if lab is None:
        assert cmap is None
    else:
        assert np.array_equal(cmap.cpu().numpy(), r_cmap), tag
    image = image.cpu().numpy()
    today = None
    for c, mode in enumerate(modes):
        if mode == "minmax":
            if today is None:
                today = loader.load_pair(*dev, size=size)[0].cpu().numpy()
            assert np.array_equal(image[c].view(np.uint16), today[c].view(np.uint16)), (tag, c)
        else:
            fails, share, A = N.close(image[c], r_image[c])
            print(f"{tag}: channel {c} {mode}: {fails} failing elements, share different beyond A = {A:.2e}: {share:.2e}")
            assert fails == 0, (tag, c)
            assert share <= N.MAX_SHARE, (tag, c, share)
    _check_stats(stats, r_stats, modes, tag)
    return got


def _f11():
    a = R.f11_inputs()
    return a["ct"], a["mr"], a["ct_label"]


def _up():
    g = np.random.default_rng(50)
    return _raw(g, (50, 70, 90), np.int16), _raw(g, (50, 70, 90), np.float32), _label(g, (50, 70, 90))


PAIRS = ["zscore", "percentile", ("minmax", "zscore"), ("percentile", "minmax"), ("zscore", "percentile")]


@pytest.mark.parametrize("normalisation", PAIRS, ids=[p if isinstance(p, str) else "+".join(p) for p in PAIRS])
def test_each_mode_matches_the_referee(normalisation):
    _check(_f11(), (128, 128, 128), normalisation, tag="40x56x48+33x61x52")
    _check(_up(), (64, 96, 128), normalisation, tag="50x70x90")


def test_other_dtypes_and_percentiles():
    """float32 CT, int16 MR, int32 label, no label; percentiles other than (1, 99)."""
    g = np.random.default_rng(51)
    host = (_raw(g, (21, 34, 27), np.float32), _raw(g, (30, 19, 33), np.int16), _label(g, (21, 34, 27), np.int32))
    _check(host, (32, 24, 40), "zscore", tag="f32+i16")
    _check(host, (32, 24, 40), "percentile", percentiles=(5, 90.5), tag="f32+i16 (5, 90.5)")
    _check(host[:2] + (None,), (32, 24, 40), ("percentile", "zscore"), percentiles=(0, 100), tag="no label")


def test_mid_size_case():
    """Many blocks per volume, and sums far above 2^24 (where a float32 accumulator stops being exact)."""
    g = np.random.default_rng(52)
    shape = (160, 300, 277)
    host = (_raw(g, shape, np.int16), _raw(g, shape, np.float32), None)
    assert host[0].size > 1 << 23 and float(np.abs(host[1]).sum(dtype=np.float64)) > 100 * (1 << 24)
    _check(host, (32, 32, 32), ("percentile", "zscore"), tag="160x300x277 p+z")
    _check(host, (32, 32, 32), ("zscore", "percentile"), tag="160x300x277 z+p")


def test_the_reference_fixture():
    from micformer_amd import loader
    g = np.load(GOLDEN)
    a = R.f11_inputs(int(g["seed"]))
    st = int(g["stride"])
    for mode in ("zscore", "percentile"):
        image, cmap, crop, stats = loader.load_pair(_dev(a["ct"]), _dev(a["mr"]), _dev(a["ct_label"]), normalisation=mode,
                                                    return_stats=True)
        assert np.array_equal(cmap.cpu().numpy(), g["class_map"])
        assert np.array_equal(crop.cpu().numpy(), g[f"{mode}_crop"])
        _check_stats(stats, g[f"{mode}_stats"], (mode, mode), f"f12 {mode}")
        got, want = image.cpu().numpy()[:, ::st, ::st, ::st], g[f"{mode}_lattice"]
        steps = R.fp16_steps(got, want)
        A = 2.0 ** -20 * max(1.0, float(np.abs(want.astype(np.float32)).max()))
        far = np.abs(got.astype(np.float64) - want.astype(np.float64)) > A
        share = float(((steps != 0) & far).mean())
        print(f"f12 {mode}: {int(((steps > 1) & far).sum())} failing points, share different beyond A = {A:.2e}: {share:.2e}")
        assert not ((steps > 1) & far).any()
        assert share <= N.MAX_SHARE


def test_tails_and_alignment():
    """Extents of 1, voxel counts that are no multiple of 8, sources at odd element offsets into a larger buffer."""
    g = np.random.default_rng(53)
    host = (_raw(g, (1, 45, 37), np.int16), _raw(g, (30, 1, 1), np.float32), _label(g, (1, 45, 37)))
    host[1][:] = g.random((30, 1, 1), dtype=np.float32) * 90 - 10
    for normalisation in ("zscore", "percentile", ("percentile", "zscore")):
        _check(host, (24, 40, 56), normalisation, tag="extent 1")
    for shape_ct, shape_mr, skip in [((7, 9, 11), (5, 13, 3), 3), ((3, 5, 7), (11, 1, 9), 1), ((13, 17, 19), (23, 7, 5), 5)]:
        ct, mr, lab = _raw(g, shape_ct, np.int16), _raw(g, shape_mr, np.float32), _label(g, shape_ct)
        off = []
        for a in (ct, mr, lab):
            buf = torch.empty(a.size + skip, dtype=torch.from_numpy(a).dtype, device="cuda")
            buf[skip:].copy_(torch.from_numpy(a).reshape(-1))
            off.append(buf[skip:].view(a.shape))
        assert off[0].data_ptr() % 16 != 0 and off[1].data_ptr() % 16 != 0
        for normalisation in ("zscore", "percentile"):
            _check((ct, mr, lab), (16, 16, 24), normalisation, tag=f"unaligned {shape_ct}", dev=tuple(off))


def _same(a, b):
    def bits(t):
        return t.view(torch.uint8) if t.dtype == torch.float16 else (t.view(torch.int64) if t.dtype == torch.float64 else t)
    return all((x is None and y is None) or torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def _batch(g, n):
    samples = []
    for i in range(n):
        cs = (11 + 7 * i % 23, 30 - i, 17 + 3 * i)
        ms = (25 - 2 * i % 9, 13 + i, 41 - 3 * i)
        ct = _raw(g, cs, np.int16 if i % 2 == 0 else np.float32)
        mr = _raw(g, ms, np.float32 if i % 3 == 0 else np.int16)
        samples.append((ct, mr, _label(g, (cs[0] + 1, cs[1], cs[2] + 2), np.int16 if i % 2 else np.int32)))
    return samples


@pytest.mark.parametrize("normalisation", [("zscore", "percentile"), ("percentile", "minmax"), "zscore"],
                         ids=["zscore+percentile", "percentile+minmax", "zscore"])
def test_nine_samples_equal_nine_calls(normalisation):
    """B = 9 crosses the 8-sample launch chunk; every sample has its own shapes and dtypes."""
    from micformer_amd import loader
    size = (16, 24, 20)
    dev = [tuple(_dev(a) for a in s) for s in _batch(np.random.default_rng(54), 9)]
    kw = dict(size=size, normalisation=normalisation, percentiles=(2, 97.5), return_stats=True)
    image, cmap, crop, stats = loader.load_batch(dev, **kw)
    assert image.shape == (9, 2) + size and cmap.shape == (9,) + size and crop.shape == (9, 3, 2) and stats.shape == (9, 2, 2)
    for b in range(9):
        assert _same(loader.load_pair(*dev[b], **kw), (image[b], cmap[b], crop[b], stats[b])), b
    # ... and one of them against the referee
    _check(tuple(t.cpu().numpy() for t in dev[8]), size, normalisation, percentiles=(2, 97.5), tag="sample 8 of 9")


def _stats_of(vol, mode, percentiles=(1, 99)):
    """`stats` of one volume under `mode` (as the MR of a pair whose CT is a small min-max volume) against numpy."""
    from micformer_amd import loader
    vol = np.ascontiguousarray(vol)
    if vol.ndim == 1:                                                 # (zeros enter neither statistic: pad to rows of 16)
        vol = np.concatenate([vol, np.zeros(-vol.size % 16, vol.dtype)]).reshape(1, -1, 16)
    ct = np.arange(8, dtype=np.int16).reshape(2, 2, 2)
    res = loader.load_pair(_dev(ct), _dev(vol), size=TINY, normalisation=("minmax", mode), percentiles=percentiles,
                           return_stats=True)
    want = np.stack([N.stats(ct, "minmax"), N.stats(vol, mode, percentiles)])
    _check_stats(res[3], want, ("minmax", mode), f"{mode} {percentiles}")
    return res[3].cpu().numpy()[1]


def test_select_ties_inside_one_bin():
    g = np.random.default_rng(55)
    v = np.float32([1.5, 2.5, 1000.0])[g.integers(0, 3, size=5001)]
    for p in [(1, 99), (30, 70), (0, 100), (33.3, 66.7)]:
        _stats_of(v, "percentile", p)
    _stats_of(np.int16([7, 8, 300])[g.integers(0, 3, size=4999)], "percentile", (10, 64))
    _stats_of(np.full(777, 2.25, np.float32), "percentile")


def test_select_int16_extremes():
    g = np.random.default_rng(56)
    v = np.int16([1, 32767, 0, -32768, -1])[g.integers(0, 5, size=(9, 31, 17))]
    for p in [(1, 99), (0, 100), (39, 41), (59, 61)]:
        _stats_of(v, "percentile", p)


def test_select_float32_over_sixty_decades():
    g = np.random.default_rng(57)
    v = (10.0 ** g.uniform(-30, 30, size=4000)).astype(np.float32)
    v[g.random(4000) < 0.1] *= -1
    v[17] = np.float32(1e-40)                                         # a subnormal: the smallest positive value
    assert v[17] > 0 and v[17] < np.finfo(np.float32).tiny
    for p in [(1, 99), (0, 100), (0, 0.01), (25, 75), (49.99, 50.01)]:
        _stats_of(v, "percentile", p)


def test_select_ranks_across_a_top_digit_boundary():
    """k and k + 1 in different bins of the first (most significant) digit: float32's 11-bit digit changes at every quarter
    binade, the int16 key's at every multiple of 32."""
    g = np.random.default_rng(58)
    below = np.nextafter(np.float32(2.0), np.float32(0)) - g.random(50, dtype=np.float32) * np.float32(0.2)
    above = np.float32(2.0) + g.random(51, dtype=np.float32) * np.float32(0.2)
    v = g.permutation(np.concatenate([below, above, np.zeros(5, np.float32)]).astype(np.float32))
    got = _stats_of(v, "percentile", (49.5, 99))                     # n = 101: h = 49.5, v[49] < 2 <= v[50]
    assert np.sort(v[v > 0])[49] < 2.0 <= np.sort(v[v > 0])[50] and got[0] < 2.0 + 0.2
    vi = g.permutation(np.concatenate([np.full(40, 31), np.full(10, 30), np.full(51, 32)]).astype(np.int16))
    assert _stats_of(vi, "percentile", (49.5, 50.5))[0] == 31.5
    vi = g.permutation(np.concatenate([np.full(50, 2047), np.full(51, 2048), np.full(9, -2048)]).astype(np.int16))
    assert _stats_of(vi, "percentile", (49.5, 50.5))[0] == 2047.5


def test_select_one_and_two_positives():
    v = np.zeros((3, 5, 7), np.float32)
    v[1, 2, 3] = 7.5
    assert _stats_of(v, "percentile").tolist() == [7.5, 7.5]
    v[2, 4, 6] = 1.25
    v[0, 0, 0] = -9.0
    _stats_of(v, "percentile")
    assert _stats_of(v, "percentile", (0, 100)).tolist() == [1.25, 7.5]
    vi = np.zeros((3, 5, 7), np.int16)
    vi[0, 1, 2] = 12
    assert _stats_of(vi, "percentile").tolist() == [12.0, 12.0]
    vi[2, 1, 2] = 400
    _stats_of(vi, "percentile", (10, 60))


def test_select_half_ranks_on_an_even_count_and_exclusions():
    g = np.random.default_rng(59)
    v = (g.random(1000, dtype=np.float32) * 100 + 1).astype(np.float32)
    _stats_of(v, "percentile", (50, 50.5))
    _stats_of(g.integers(1, 500, size=1000).astype(np.int16), "percentile", (50, 50.5))
    w = np.concatenate([v, -v, np.zeros(300, np.float32), np.float32([-0.0] * 7)])   # negatives and zeros: not selected from
    a, b = _stats_of(g.permutation(w), "percentile", (0, 100))
    assert a == float(v.min()) and b == float(v.max())
    _stats_of(g.permutation(w), "percentile", (50, 50.5))


def test_zscore_statistics_are_exact():
    g = np.random.default_rng(60)
    v = g.integers(32766, 32768, size=(32, 32, 32)).astype(np.int16)    # variance 1/4 on a mean of 2^15: lost by a float accumulator
    m, s = _stats_of(v, "zscore")
    assert abs(s - 0.5) < 1e-3
    v = (g.standard_normal((37, 41, 43)) * 3.0 + 3000.0).astype(np.float32)
    m, s = _stats_of(v, "zscore")
    assert abs(m - 3000) < 0.1 and abs(s - 3) < 0.1
    v = (g.standard_normal((19, 23, 29)) * 50.0).astype(np.float32)     # zeros masked, negatives included, -0.0 is zero
    v[g.random(v.shape) < 0.3] = 0
    v[0, 0, :5] = -0.0
    _stats_of(v, "zscore")
    vi = g.integers(-3000, 500, size=(19, 23, 29)).astype(np.int16)
    vi[g.random(vi.shape) < 0.3] = 0
    _stats_of(vi, "zscore")
    _stats_of(np.full((4, 4, 4), -32768, np.int16), "zscore")


def test_edge_rules():
    from micformer_amd import loader
    size = (6, 6, 6)
    other = _dev(np.arange(27, dtype=np.int16).reshape(3, 3, 3))

    def mr_image(vol, mode):
        return loader.load_pair(other, _dev(vol), size=size, normalisation=("minmax", mode))[0][1].cpu().numpy()

    for dtype in (np.float32, np.int16):
        zeros = np.zeros((6, 6, 6), dtype)
        assert not mr_image(zeros, "zscore").any()                                    # z-score, all zero: all zeros
        const = np.full((6, 6, 6), 7, dtype)
        const[:, :, -2:] = 0                                                          # (at the far end: a tap pair reads x and x + 1,
        z = mr_image(const, "zscore")                                                 # and 0 * NaN is NaN; source size = target size)
        assert np.array_equal(np.isnan(z), np.isnan(N.load_pair(const, const, None, size, normalisation="zscore")[0][1]))
        assert np.isnan(z[const != 0]).all() and not z[const == 0].any()              # z-score, constant: NaN off the zeros
        one = zeros.copy()
        one[1, 2, 3] = 9
        assert np.isnan(mr_image(one, "percentile")).all()                            # one positive voxel: high == low
        assert np.isnan(mr_image(const, "percentile")).all()                          # high == low
        assert np.isnan(mr_image(-np.abs(const), "percentile")).all()                 # no positive voxel
    image, _, crop = loader.load_pair(other, _dev(np.zeros((6, 6, 6), np.float32)), size=size, normalisation="zscore")
    assert not image[1].any() and not torch.isnan(image[0]).any()


def test_two_runs_are_bit_identical():
    from micformer_amd import loader
    dev = tuple(_dev(a) for a in _up())
    for normalisation in ("zscore", "percentile", ("percentile", "zscore")):
        kw = dict(size=(64, 96, 128), normalisation=normalisation, return_stats=True)
        assert _same(loader.load_pair(*dev, **kw), loader.load_pair(*dev, **kw)), normalisation


def test_capture_and_replay_under_a_graph():
    from micformer_amd import loader
    size = (24, 24, 24)
    dev = [tuple(_dev(a) for a in s) for s in _batch(np.random.default_rng(61), 2)]
    kw = dict(size=size, normalisation=("percentile", "zscore"))
    eager = loader.load_batch(dev, **kw)
    out = (torch.zeros_like(eager[0]), torch.zeros_like(eager[1]), torch.zeros_like(eager[2]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loader.load_batch(dev, out=out, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    for seed in (62, 63):                                             # new contents in the same source buffers: the replay reads them
        before = tuple(t.clone() for t in out)
        for d, h in zip(dev, _batch(np.random.default_rng(seed), 2)):
            for t, a in zip(d, h):
                t.copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, loader.load_batch(dev, **kw))
        assert not _same(out, before)


def test_segment_pair_passes_the_normalisation_through():
    from micformer_amd import data, loader, restore
    g = np.random.default_rng(64)
    shape, size = (41, 50, 37), (32, 32, 32)
    ct = torch.from_numpy(g.integers(-1000, 3000, size=shape, dtype=np.int16)).cuda()
    mr = torch.from_numpy((g.random(shape, dtype=np.float32) * 1500).astype(np.float32)).cuda()
    model = tiny_head()
    kw = dict(normalisation="percentile", percentiles=(2, 98))
    image, _, _ = loader.load_pair(ct, mr, None, size=size, **kw)
    x, _ = data.prepare_raw_batch(image.unsqueeze(0), None, None)
    with torch.no_grad():
        logits = model(x)
    want = restore.restore_labels(logits.float().contiguous(), shape)
    got = restore.segment_pair(model, ct, mr, size=size, **kw)
    assert got.shape == shape and got.dtype == torch.int16 and torch.equal(got, want)
    assert not torch.equal(got, restore.segment_pair(model, ct, mr, size=size))       # (the default normalisation segments differently)
