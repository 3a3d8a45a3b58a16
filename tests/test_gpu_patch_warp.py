"""GPU tests of the patch sampler's crop through a map (micformer_amd/patch_warp.py, csrc/volume_patch_warp.hip) against the numpy
referee tests/patch_warp_ref.py, which restates include/micformer_patch_warp.h and is itself held to F.grid_sample by
tests/test_patch_warp_cpu.py.

Bounds (the header's).  EPS = 2^-20; a coordinate is within eps_axis = P EPS + (L + P) 2^-24 voxels for a map and 2 P EPS + (L + P)
2^-24 with a field (|u| <= 0.25).  An image element may differ from the float64 referee by u16(ref) + S (eps_z + eps_y + eps_x) +
8 * 2^-23 * max|tap| (S the spread of its 8 taps, u16 the float16 spacing at |ref|); a label voxel is compared where its float64 index
is further than eps_axis from every k + 1/2 and must then be equal, and at most patch_warp_ref.MAX_EXCLUDED of a case's voxels are
left out so (the CPU test asserts that of the referee alone).  origins and picked: exact.  Identity map on power-of-two patches, a
zero field, batch independence, graph replay and forwarding: bit for bit."""
import functools

import numpy as np
import pytest
import torch

import patch_warp_ref as W
import patches_ref as P

pytestmark = pytest.mark.gpu


def _t(a):
    """A device copy of a host array (the shared cases are read-only: torch wants a writable source)."""
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _dev(sample):
    return tuple(_t(a) for a in sample)


def _np(out):
    return [None if t is None else t.cpu().numpy() for t in out]


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x.view(np.uint8), y.view(np.uint8)))
               for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _nine_dev():
    samples, _ = W.nine()
    return tuple(_dev(s) for s in samples)


def _devs(samples):
    """The device copies of samples of patch_warp_ref.nine() (made once), by identity of the host arrays."""
    host, _ = W.nine()
    where = {id(s[0]): b for b, s in enumerate(host)}
    return [_nine_dev()[where[id(s[0])]] for s in samples]


def _run(devs, draws, patch, theta=None, fields=None, mode="linear", **kw):
    from micformer_amd import patch_warp
    return _np(patch_warp.sample_warped_batch(devs, _t(np.asarray(draws, np.float32)), patch, affine=_t(theta), displacement=_t(fields),
                                              field_interpolation=mode, **kw))


def _check(got, refs, tag):
    """Every sample of a call against its referee: prints the figures, then asserts."""
    image, label_map, origins, picked = got
    assert image.dtype == np.float16 and origins.dtype == np.int32 and picked.dtype == np.int32
    assert label_map is None or label_map.dtype == np.uint8
    for b, ref in enumerate(refs):
        one = dict(image=image[b], label=None if label_map is None else label_map[b], origin=origins[b], picked=picked[b])
        bad, info = W.compare(one, ref)
        print(f"{tag} sample {b}: origin {origins[b].tolist()} picked {picked[b].tolist()} worst error / bound {info['worst']:.3f} "
              f"failing {info['failing']} label excluded {info['excluded']:.2e} -> {bad or 'ok'}")
        assert np.isfinite(image[b].astype(np.float32)).all(), (tag, b)
        assert bad == [], (tag, b, bad, info)
        assert info["excluded"] <= W.MAX_EXCLUDED, (tag, b, info)


def _case_run(name, padding_mode, pad_class=255, **kw):
    patch, samples, draws, theta, fields, mode = W.case(name)
    return _run(_devs(samples), draws, patch, theta, fields, mode, padding_mode=padding_mode, pad_class=pad_class, **kw)


# ---- the identity: the plain crop, bit for bit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("scan_shape", W.POW2_SCANS, ids=str)
@pytest.mark.parametrize("patch", W.POW2_PATCHES, ids=str)
def test_identity_map_is_sample_patches_bit_for_bit(scan_shape, patch):
    """Power-of-two patch extents: every quantity of the rule is exact and i = o + x.  Both padding modes, pad_class 0 and 255,
    forced and random draws, clamp="lower", a mixed normalisation; (5, 30, 40) is shorter than the patch in d (negative origins).
    The map as an identity tensor, as None next to a zero field, and with neither."""
    from micformer_amd import patch_warp, patches
    g = np.random.default_rng(9701 + scan_shape[0] + patch[2])
    scans = [(W.image(g, scan_shape, np.int16), W.image(g, scan_shape, np.float32),
              W.VALUES[g.integers(0, len(W.VALUES), size=scan_shape)].astype(np.int16)),
             (W.image(g, scan_shape, np.float32), W.image(g, scan_shape, np.int16),
              W.VALUES[g.integers(0, len(W.VALUES), size=scan_shape)].astype(np.int32)),
             (W.image(g, scan_shape, np.int16), W.image(g, scan_shape, np.int16),
              W.VALUES[g.integers(0, len(W.VALUES), size=scan_shape)].astype(np.int16))]
    devs = [_dev(s) for s in scans]
    draws = _t(np.float32([(0.0, 0, 0, 0.99, 0.0, 0.5), (1.0, 0.99, 1.0, 0, 0, 0), (1.0, 0.2, 0.0, 0, 0, 0)]))
    theta = _t(np.stack([W.A.IDENTITY] * 3))
    zero = torch.zeros(3, 3, 2, 3, 4, device="cuda")
    for normalisation in ("minmax", ("zscore", "percentile")):
        idx = patches.index_scans(devs, normalisation=normalisation)
        for padding_mode, pad_class, clamp in (("zeros", 0, "both"), ("border", 255, "lower"), ("border", 0, "both"), ("zeros", 255, "lower")):
            kw = dict(padding_mode=padding_mode, pad_class=pad_class, clamp=clamp)
            plain = _np(patches.sample_patches(devs, idx, draws, patch_size=patch, **kw))
            assert (plain[3][1:, 0] > 0).all() and plain[3][0, 0] == 0
            if scan_shape[0] < patch[0]:
                assert (plain[2][:, 0] <= 0).all() and (plain[2][:, 0] < 0).any()
            assert (plain[1] == pad_class).any()
            for how, extra in (("theta", dict(affine=theta)), ("zero field", dict(displacement=zero, field_interpolation="cubic")),
                               ("neither", dict())):
                got = _np(patch_warp.sample_warped_patches(devs, idx, draws, patch, **extra, **kw))
                assert _same(got, plain), (normalisation, kw, how)


def test_half_voxel_translation_rounds_ties_to_even():
    """A translation by exactly half a voxel on a power-of-two patch is exact in float32 too: every label index is a tie, none is
    excluded, and the label must be the half-to-even one."""
    patch = W.POW2_PATCHES[0]
    samples, draws = W.nine()
    theta = W.A.IDENTITY.copy()
    theta[:, 3] = [1.0 / patch[2], 1.0 / patch[1], 1.0 / patch[0]]
    got = _run(_devs(samples[:2]), draws[:2], patch, np.stack([theta] * 2), padding_mode="zeros", pad_class=255)
    refs = [W.sample(*samples[b], draws[b], patch, theta=theta, pad_class=255, exact=True) for b in range(2)]
    assert all(r["label"]["sure"].all() for r in refs)
    _check(got, refs, "half voxel")
    up = W.sample(*samples[0], draws[0], patch, theta=theta, pad_class=255, exact=True, mutate="half_up")
    assert not np.array_equal(up["label"]["cls"], refs[0]["label"]["cls"])


# ---- generic maps ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
@pytest.mark.parametrize("name", ["maps-4", "maps-1"])
def test_generic_maps_meet_the_bounds(name, padding_mode):
    """Nine samples (a chunk of 8 and one more): rotate +-0.26 rad, scale +-0.15, shift +-3 voxels; CT int16 with MR float32 and the
    reverse, label int16 and int32; x runs of 4 (Pw = 28) and the per-element path (Pw = 13)."""
    got = _case_run(name, padding_mode)
    refs = W.case_reference(name, padding_mode)
    _check(got, refs, f"{name} {padding_mode}")
    assert (got[3][:, 0] > 0).sum() == 4 and len(np.unique(got[1])) >= 9
    if padding_mode == "zeros":
        assert np.mean([p["outside"].mean() for r in refs for p in r["planes"]]) > 0.02
    # without a label: the forced draws fall back to random crops, the image follows the same rule
    patch, samples, draws, theta, _, _ = W.case(name)
    bare = [(ct, mr, None) for ct, mr, _ in samples[:3]]
    none = _run([d[:2] + (None,) for d in _devs(samples[:3])], draws[:3], patch, theta[:3], padding_mode=padding_mode)
    assert none[1] is None
    _check(none, [W.sample(*s, draws[b], patch, theta=theta[b], padding_mode=padding_mode) for b, s in enumerate(bare)],
           f"{name} {padding_mode} no label")


NORMALISATIONS = ["zscore", "percentile", ("zscore", "minmax"), ("minmax", "percentile")]


@pytest.mark.parametrize("normalisation", NORMALISATIONS, ids=[p if isinstance(p, str) else "+".join(p) for p in NORMALISATIONS])
def test_other_normalisations(normalisation):
    """The referee is fed the statistics of the scan's index (what the kernel reads), which separates the warp from the statistics."""
    from micformer_amd import patch_warp, patches
    samples, draws = W.nine()
    n = 3
    devs = _devs(samples[:n])
    idx = patches.index_scans(devs, normalisation=normalisation, percentiles=(2, 98))
    for padding_mode, patch in (("zeros", W.PATCHES[0]), ("border", W.PATCHES[1])):
        theta = W.nine_maps(patch)[:n]
        got = _np(patch_warp.sample_warped_patches(devs, idx, _t(draws[:n]), patch, affine=_t(theta), padding_mode=padding_mode,
                                                   pad_class=255))
        refs = [W.sample(*samples[b], draws[b], patch, theta=theta[b], padding_mode=padding_mode, pad_class=255,
                         normalisation=normalisation, percentiles=(2, 98), stats=idx[b].stats.cpu().numpy()) for b in range(n)]
        _check(got, refs, f"{normalisation} {padding_mode}")


def test_map_per_modality():
    """[B, 2, 3, 4]: map 0 for CT and its label, map 1 -- the same map composed with affine_ref.MR_REORIENT -- for MR."""
    _, _, _, theta, _, _ = W.case("per-modality")
    assert theta.shape == (3, 2, 3, 4)
    for padding_mode in ("zeros", "border"):
        got = _case_run("per-modality", padding_mode)
        _check(got, W.case_reference("per-modality", padding_mode), f"per modality {padding_mode}")
    one = _run(_devs(W.case("per-modality")[1]), W.case("per-modality")[2], W.PATCHES[0], theta[:, 0].copy(), padding_mode="border",
               pad_class=255)
    assert np.array_equal(one[0][:, 0], got[0][:, 0]) and np.array_equal(one[1], got[1]) and not np.array_equal(one[0][:, 1], got[0][:, 1])


# ---- fields ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cubic", "linear", "cubic-no-map", "dense", "dense-no-map"])
def test_fields_meet_the_bounds(name):
    """A drawn (5, 5, 5) field, cubic and linear, and a dense field (grid = patch size, a cell per voxel), with and without a map;
    x runs of 8, 4 and 1."""
    for padding_mode in ("zeros", "border"):
        got = _case_run(name, padding_mode)
        _check(got, W.case_reference(name, padding_mode), f"{name} {padding_mode}")


@pytest.mark.parametrize("mode", ["linear", "cubic"])
def test_zero_field_is_the_map_only_call_bit_for_bit(mode):
    for name, grid in (("maps-4", (5, 5, 5)), ("maps-1", (2, 3, 7)), ("maps-1", W.PATCHES[1])):
        patch, samples, draws, theta, _, _ = W.case(name)
        devs = _devs(samples)
        plain = _run(devs, draws, patch, theta, padding_mode="border", pad_class=255)
        zero = np.zeros((len(samples), 3) + tuple(grid), np.float32)
        assert _same(_run(devs, draws, patch, theta, zero, mode, padding_mode="border", pad_class=255), plain), (name, grid)


# ---- batch, extremes, graph, forwarding ----------------------------------------------------------------------------------------

def test_each_sample_is_its_own_call_and_two_runs_agree():
    patch, samples, draws, theta, fields, mode = W.case("cubic")
    devs = _devs(samples)
    kw = dict(padding_mode="zeros", pad_class=255, normalisation=("percentile", "zscore"))
    got = _run(devs, draws, patch, theta, fields, mode, **kw)
    assert _same(got, _run(devs, draws, patch, theta, fields, mode, **kw))
    for b in range(W.BATCH):
        alone = _run(devs[b:b + 1], draws[b:b + 1], patch, theta[b:b + 1], fields[b:b + 1], mode, **kw)
        assert _same([t[b:b + 1] for t in got], alone), b


@pytest.mark.parametrize("padding_mode", ["zeros", "border"])
def test_coordinate_extremes(padding_mode):
    """NaN, +inf and 1e30 map entries and a NaN control point (coordinates tests/patch_warp_index_main.cpp ran under the sanitizers
    first): image 0 and pad_class where s is not finite, everything else within the bounds, the other samples untouched."""
    patch, samples, draws, theta, fields = W.extremes()
    devs = _devs(samples)
    got = _run(devs, draws, patch, theta, fields, "linear", padding_mode=padding_mode, pad_class=255)
    _check(got, W.extremes_reference(padding_mode), f"extremes {padding_mode}")
    for b in (1, 2):
        assert not got[0][b].view(np.uint16).any() and (got[1][b] == 255).all()
    off = np.ones(patch, bool)
    off[patch[0] // 2] = False
    assert (got[1][3][off] == 255).all() and (got[1][3][~off] != 255).any()
    if padding_mode == "zeros":
        assert not got[0][3][:, off].view(np.uint16).any() and got[0][3][:, ~off].view(np.uint16).any()
    for b in (0, 5):
        alone = _run(devs[b:b + 1], draws[b:b + 1], patch, theta[b:b + 1], fields[b:b + 1], "linear", padding_mode=padding_mode,
                     pad_class=255)
        assert _same([t[b:b + 1] for t in got], alone), b


def test_capture_and_replay_under_a_graph():
    """One capture with out=, replayed after draws.copy_(), theta.copy_() and field.copy_(), against eager calls; a single stream."""
    from micformer_amd import patch_warp, patches
    patch, samples, draws, theta, fields, mode = W.case("cubic")
    devs = _devs(samples[:3])
    idx = patches.index_scans(devs)
    d, th, fl = _t(draws[:3]), _t(theta[:3]), _t(fields[:3])
    kw = dict(affine=th, displacement=fl, field_interpolation=mode, pad_class=255)
    eager = _np(patch_warp.sample_warped_patches(devs, idx, d, patch, **kw))
    out = (torch.zeros(3, 2, *patch, dtype=torch.float16, device="cuda"), torch.zeros(3, *patch, dtype=torch.uint8, device="cuda"),
           torch.zeros(3, 3, dtype=torch.int32, device="cuda"), torch.zeros(3, 4, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            res = patch_warp.sample_warped_patches(devs, idx, d, patch, out=out, **kw)
    assert all(r is o for r, o in zip(res, out))
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(_np(out), eager)
    for rows in ([3, 4, 5], [6, 7, 8]):                               # new contents in the same tensors: the replay reads them
        d.copy_(_t(draws[rows]))
        th.copy_(_t(theta[rows]))
        fl.copy_(_t(fields[rows]))
        graph.replay()
        torch.cuda.synchronize()
        replayed = _np(out)
        want = _np(patch_warp.sample_warped_patches(devs, idx, d.clone(), patch, affine=th.clone(), displacement=fl.clone(),
                                                    field_interpolation=mode, pad_class=255))
        assert _same(replayed, want) and not _same(replayed, eager)


def test_sample_patches_forwards_a_map_or_a_field():
    from micformer_amd import patch_warp, patches
    patch, samples, draws, theta, fields, mode = W.case("cubic")
    devs = _devs(samples[:3])
    idx = patches.index_scans(devs)
    d, th, fl = _t(draws[:3]), _t(theta[:3]), _t(fields[:3])
    kw = dict(padding_mode="border", pad_class=7, clamp="lower")
    for extra in (dict(affine=th), dict(displacement=fl, field_interpolation=mode), dict(affine=th, displacement=fl, field_interpolation=mode)):
        want = _np(patch_warp.sample_warped_patches(devs, idx, d, patch, **extra, **kw))
        assert _same(_np(patches.sample_patches(devs, idx, d, patch_size=patch, **extra, **kw)), want)
        assert _same(_np(patches.sample_batch(devs, d, patch_size=patch, **extra, **kw)), want)
        assert _same(_np(patch_warp.sample_warped_batch(devs, d, patch, **extra, **kw)), want)
    # with both None: the plain crop, as before -- exactly the referee's window, label and picks
    plain = _np(patches.sample_patches(devs, idx, d, patch_size=patch, field_interpolation="cubic", **kw))
    for b in range(3):
        want = P.sample(*samples[b], draws[b], patch, **kw)
        one = dict(image=plain[0][b], label=plain[1][b], origin=plain[2][b], picked=plain[3][b])
        assert P.compare(one, want) == [], b
    assert not _same(plain, _np(patches.sample_patches(devs, idx, d, patch_size=patch, affine=th, **kw)))
    with pytest.raises(ValueError, match="affine holds maps for 2 samples"):
        patches.sample_patches(devs, idx, d, patch_size=patch, affine=th[:2].contiguous())
    with pytest.raises(ValueError, match="control grid"):
        patches.sample_patches(devs, idx, d, patch_size=patch, displacement=torch.zeros(3, 3, 1, 5, 5, device="cuda"))
    with pytest.raises(ValueError, match="affine must have shape"):
        patch_warp.sample_warped_patches(devs, idx, d, patch, affine=torch.zeros(3, 4, 3, device="cuda"))
