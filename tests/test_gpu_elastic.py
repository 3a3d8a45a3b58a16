"""GPU tests of the loader's elastic resample (micformer_amd/elastic.py, csrc/volume_elastic.hip) against the float64 referee
tests/elastic_ref.py, which tests/test_elastic_cpu.py holds to F.interpolate, scipy's map_coordinates and F.grid_sample.

The cases (elastic_ref.CASES) reuse affine_ref.case(): CT int16 (37, 45, 29) with its label, MR float32 (41, 33, 47), output
(24, 20, 28).  "nine": the nine samples and their nine maps with fields on a (5, 4, 6) grid (a second chunk of 8); "dense": two
samples, a map per modality, one vector per output voxel; "minimal": two samples, no map, a (2, 2, 2) grid.  Fields uniform in
+-0.12 normalised.

Bounds: the affine tests' with EPS = 2^-19.  A coordinate: eps_axis = extent * 2^-19 voxels.  An image element: |got - ref| <=
u16(ref) + S * (eps_z + eps_y + eps_x) + 8 * 2^-23 * max|tap|, no element excepted.  The label: equal to the referee wherever the
float64 index is further than eps_axis from every k + 0.5; at most 2e-3 of a sample's voxels are excluded so.  crop_indexes: exact.
stats: the bits of the call without a map."""
import functools

import numpy as np
import pytest
import torch

import affine_ref as A
import elastic_ref as E

pytestmark = pytest.mark.gpu

SHAPES = (A.CT_SHAPE, A.MR_SHAPE)
PADDINGS = ("zeros", "border")


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases are read-only)


@functools.lru_cache(maxsize=None)
def _device_case(name):
    samples, theta, fields = E.case(name)
    return [tuple(_dev(a) for a in s) for s in samples], _dev(theta), _dev(fields)


@functools.lru_cache(maxsize=None)
def _loaded(name, mode, padding_mode):
    """A case, min-max, as numpy: (image, label_map, crop); computed once per (case, interpolation, padding)."""
    from micformer_amd import loader
    dev, theta, fields = _device_case(name)
    return tuple(t.cpu().numpy() for t in loader.load_batch(dev, size=E.SIZE, displacement=fields, field_interpolation=mode,
                                                            affine=theta, padding_mode=padding_mode))


def _check_plane(got16, ref, shape, tag):
    """Every element of one float16 plane within the bound of its referee; prints the worst ratio before it asserts."""
    got = got16.astype(np.float64)
    err = np.abs(got - ref["value"])
    bound = E.image_bound(ref, shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    print(f"{tag}: worst error / bound {float(ratio[worst]):.3f} at {worst}: got {got[worst]!r} ref {ref['value'][worst]!r} "
          f"index {ref['index'][(slice(None),) + worst].tolist()}; failing elements {int((~(err <= bound)).sum())}")
    assert np.isfinite(got).all(), tag
    assert (err <= bound).all(), (tag, worst, float(got[worst]), float(ref["value"][worst]))


def _bytes(t):
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.uint8)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))


ALL = [(n, m, p) for n in sorted(E.CASES) for m in E.MODES for p in PADDINGS]


# ---- against the referee ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode,padding_mode", ALL)
def test_image_meets_the_bound(name, mode, padding_mode):
    image, _, _ = _loaded(name, mode, padding_mode)
    refs = E.case_reference(name, mode, padding_mode)
    assert image.dtype == np.float16 and image.shape == (len(refs), 2) + E.SIZE
    for b, r in enumerate(refs):
        for c in range(2):
            _check_plane(image[b, c], r["planes"][c], SHAPES[c], f"{name} {mode} {padding_mode} sample {b} channel {c}")
    if name == "nine" and padding_mode == "zeros":
        share = float(np.mean([p["outside"].mean() for r in refs for p in r["planes"]]))
        print(f"voxels with a tap outside the array: {share:.1%}")
        assert share >= 0.10


@pytest.mark.parametrize("name,mode,padding_mode", ALL)
def test_label_equals_the_referee_away_from_rounding_boundaries(name, mode, padding_mode):
    _, label_map, _ = _loaded(name, mode, padding_mode)
    refs = E.case_reference(name, mode, padding_mode)
    assert label_map.dtype == np.uint8 and label_map.shape == (len(refs),) + E.SIZE
    for b, r in enumerate(refs):
        sure, want = r["label"]["sure"], r["label"]["cls"]
        excluded = 1.0 - float(sure.mean())
        bad = np.argwhere(sure & (label_map[b] != want))
        print(f"{name} {mode} {padding_mode} sample {b}: excluded {excluded:.2e}, different among the excluded "
              f"{int((~sure & (label_map[b] != want)).sum())}, failing {len(bad)}" + (f", first at {bad[0].tolist()}" if len(bad) else ""))
        assert excluded <= E.MAX_EXCLUDED
        assert len(bad) == 0, (b, bad[0].tolist())
        assert len(np.unique(want)) == 9                              # 0, the seven classes and 255 all occur


@pytest.mark.parametrize("name,mode,padding_mode", ALL)
def test_crop_indexes_are_the_loaders_rule_on_the_referee(name, mode, padding_mode):
    _, _, crop = _loaded(name, mode, padding_mode)
    refs = E.case_reference(name, mode, padding_mode)
    assert crop.dtype == np.int32 and crop.shape == (len(refs), 3, 2)
    for b, r in enumerate(refs):
        assert np.array_equal(crop[b], r["crop"]), (b, crop[b].tolist(), r["crop"].tolist())


@pytest.mark.parametrize("mode", E.MODES)
def test_another_normalisation_pair_and_the_statistics(mode):
    """stats: the bits of the call without a map or a field.  Image: the bound against the referee fed those statistics."""
    from micformer_amd import loader
    dev, theta, fields = _device_case("nine")
    samples, host_theta, host_fields = E.case("nine")
    n, normalisation = 2, ("zscore", "percentile")
    kw = dict(size=E.SIZE, normalisation=normalisation, percentiles=(2, 98), return_stats=True)
    plain = loader.load_batch(dev[:n], **kw)
    for padding_mode in PADDINGS:
        image, label_map, crop, stats = loader.load_batch(dev[:n], displacement=fields[:n].clone(), field_interpolation=mode,
                                                          affine=theta[:n].clone(), padding_mode=padding_mode, **kw)
        assert stats.dtype == torch.float64 and torch.equal(stats.view(torch.int64), plain[3].view(torch.int64))
        image, st = image.cpu().numpy(), stats.cpu().numpy()
        for b in range(n):
            r = E.load_pair(*samples[b], host_fields[b], mode, host_theta[b], E.SIZE, padding_mode, normalisation=normalisation,
                            percentiles=(2, 98), stats=st[b])
            for c in range(2):
                _check_plane(image[b, c], r["planes"][c], SHAPES[c], f"{mode} {padding_mode} sample {b} channel {c}")
            assert np.array_equal(label_map[b].cpu().numpy()[r["label"]["sure"]], r["label"]["cls"][r["label"]["sure"]])
    mm = loader.load_batch(dev[:n], size=E.SIZE, displacement=fields[:n].clone(), affine=theta[:n].clone(), return_stats=True)
    assert torch.equal(mm[3].view(torch.int64), loader.load_batch(dev[:n], size=E.SIZE, return_stats=True)[3].view(torch.int64))


# ---- against the affine call --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", E.MODES)
def test_a_zero_field_is_the_affine_call_bit_for_bit(mode):
    from micformer_amd import loader
    dev, theta, _ = _device_case("nine")
    _, both, _ = _device_case("dense")
    for grid in ((5, 4, 6), (2, 2, 2)):
        for padding_mode in PADDINGS:
            zero = torch.zeros((E.BATCH, 3) + grid, device="cuda")
            kw = dict(size=E.SIZE, padding_mode=padding_mode)
            assert _same(loader.load_batch(dev, displacement=zero, field_interpolation=mode, affine=theta, **kw),
                         loader.load_batch(dev, affine=theta, **kw)), (grid, padding_mode)
            assert _same(loader.load_batch(dev[:2], displacement=zero[:2], field_interpolation=mode, affine=both, **kw),
                         loader.load_batch(dev[:2], affine=both, **kw)), (grid, padding_mode)
            eye = _dev(np.repeat(A.IDENTITY[None], E.BATCH, 0))
            assert _same(loader.load_batch(dev, displacement=zero, field_interpolation=mode, **kw),
                         loader.load_batch(dev, affine=eye, **kw)), (grid, padding_mode)


@pytest.mark.parametrize("mode", E.MODES)
def test_the_deformation_comes_first_and_is_shared_by_the_modalities(mode):
    """A per-modality map (the MR re-orientation) and a non-zero field: the MR plane meets the bound against the referee of
    s = theta_mr . (n + u, 1); the CT plane and the label are those of the call with the identity for both."""
    from micformer_amd import loader
    dev, _, fields = _device_case("nine")
    samples, _, host_fields = E.case("nine")
    b = 1
    both = np.stack([A.IDENTITY, A.MR_REORIENT])
    got = loader.load_pair(*dev[b], size=E.SIZE, displacement=fields[b].clone(), field_interpolation=mode, affine=_dev(both),
                           padding_mode="border")
    ident = loader.load_pair(*dev[b], size=E.SIZE, displacement=fields[b].clone(), field_interpolation=mode, padding_mode="border")
    assert torch.equal(got[0][0].view(torch.int16), ident[0][0].view(torch.int16)) and torch.equal(got[1], ident[1])
    assert not torch.equal(got[0][1].view(torch.int16), ident[0][1].view(torch.int16))
    r = E.load_pair(*samples[b], host_fields[b], mode, both, E.SIZE, "border")
    image = got[0].cpu().numpy()
    for c in range(2):
        _check_plane(image[c], r["planes"][c], SHAPES[c], f"re-oriented MR after the field, {mode}, channel {c}")
    # the other order, theta_mr . n + u, is a different plane: the test tells them apart
    u = r["u"]
    moved = np.stack([u[0], -u[2], u[1]])                            # u carried through the signed permutation
    wrong = E.sample_image(A.R.normalize(samples[b][1]), *E.indices(A.MR_REORIENT, moved, E.SIZE, A.MR_SHAPE), "border")
    assert not (np.abs(image[1].astype(np.float64) - wrong["value"]) <= E.image_bound(wrong, A.MR_SHAPE)).all()


# ---- determinism, batching, capture ---------------------------------------------------------------------------------------------------

def test_two_runs_are_bit_equal_and_a_sample_alone_equals_the_sample_in_the_batch():
    from micformer_amd import loader
    dev, theta, fields = _device_case("nine")
    for mode, padding_mode in (("cubic", "zeros"), ("linear", "border")):
        kw = dict(size=E.SIZE, field_interpolation=mode, padding_mode=padding_mode)
        batch = loader.load_batch(dev, displacement=fields, affine=theta, **kw)
        assert _same(batch, loader.load_batch(dev, displacement=fields, affine=theta, **kw))
        for x, y in zip(batch, _loaded("nine", mode, padding_mode)):                            # ... and to the run the other tests read
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.view(np.uint8))
        for b in (0, 7, 8):                                           # both chunks
            one = loader.load_pair(*dev[b], displacement=fields[b].clone(), affine=theta[b].clone(), **kw)
            assert _same(one, tuple(t[b] for t in batch)), (mode, padding_mode, b)
    kw = dict(size=E.SIZE, normalisation=("percentile", "zscore"), field_interpolation="cubic", return_stats=True)
    batch = loader.load_batch(dev, displacement=fields, affine=theta, **kw)
    assert _same(batch, loader.load_batch(dev, displacement=fields, affine=theta, **kw))
    assert _same(loader.load_pair(*dev[8], displacement=fields[8].clone(), affine=theta[8].clone(), **kw), tuple(t[8] for t in batch))


def test_out_is_written_in_place():
    from micformer_amd import loader
    dev, theta, fields = _device_case("nine")
    out = (torch.zeros((E.BATCH, 2) + E.SIZE, dtype=torch.float16, device="cuda"),
           torch.zeros((E.BATCH,) + E.SIZE, dtype=torch.uint8, device="cuda"), torch.zeros((E.BATCH, 3, 2), dtype=torch.int32, device="cuda"))
    got = loader.load_batch(dev, size=E.SIZE, displacement=fields, field_interpolation="cubic", affine=theta, padding_mode="border",
                            out=out)
    assert all(g is o for g, o in zip(got, out))
    for x, y in zip(out, _loaded("nine", "cubic", "border")):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.view(np.uint8))
    nolab = loader.load_pair(dev[0][0], dev[0][1], None, size=E.SIZE, displacement=fields[0].clone(), field_interpolation="cubic",
                             affine=theta[0].clone(), padding_mode="border")
    assert nolab[1] is None and np.array_equal(nolab[0].cpu().numpy().view(np.uint8), _loaded("nine", "cubic", "border")[0][0].view(np.uint8))


def test_a_captured_graph_reads_the_new_field():
    from micformer_amd import loader
    dev, theta, fields = _device_case("nine")
    dev, theta = dev[:2], theta[:2].clone()
    field, other = fields[:2].clone(), fields[2:4].clone()
    kw = dict(size=E.SIZE, normalisation=("minmax", "zscore"), field_interpolation="cubic", affine=theta, padding_mode="zeros")
    eager = loader.load_batch(dev, displacement=field, **kw)
    want = loader.load_batch(dev, displacement=other, **kw)
    assert not _same(eager, want)
    out = tuple(torch.zeros_like(t) for t in eager)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loader.load_batch(dev, displacement=field, out=out, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, eager)
    field.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, want)


# ---- fields no grid holds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", E.MODES)
def test_non_finite_and_huge_fields(mode):
    """NaN, +-inf and 1e30 control values: finite output, 0 / class 0 wherever s is non-finite (every voxel whose taps include the
    value), the referee's values elsewhere, no error.  (tests/elastic_index_main.cpp has swept the control-grid functions and
    tests/affine_index_main.cpp has pushed the same values through the coordinate functions on the host: every address in range.)"""
    from micformer_amd import loader
    dev, theta, _ = _device_case("nine")
    samples, host_theta, _ = E.case("nine")
    grid = (5, 4, 6)
    fields = []
    for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        f = np.zeros((2, 3) + grid, np.float32)                       # one entry of one component, and every entry
        f[0, 1, 2, 1, 3] = v
        f[1] = v
        fields += [f[0], f[1]]
    mixed = np.zeros((3,) + grid, np.float32)                         # inf - inf inside one stencil
    mixed[0, 2, 2, 2], mixed[0, 2, 2, 3] = np.inf, -np.inf
    fields.append(mixed)
    n = len(fields)
    sel = [dev[b % 2] for b in range(n)]
    maps = _dev(np.stack([host_theta[b % 2] for b in range(n)]))
    for padding_mode in PADDINGS:
        image, label_map, crop = loader.load_batch(sel, size=E.SIZE, displacement=_dev(np.stack(fields)), field_interpolation=mode,
                                                   affine=maps, padding_mode=padding_mode)
        torch.cuda.synchronize()
        image, label_map, crop = image.cpu().numpy(), label_map.cpu().numpy(), crop.cpu().numpy()
        assert np.isfinite(image).all()
        for b in range(n):
            r = E.load_pair(*samples[b % 2], fields[b], mode, host_theta[b % 2], E.SIZE, padding_mode)
            lost = ~np.isfinite(r["u"]).all(axis=0)
            if not np.isfinite(fields[b]).all():
                assert lost.any() and lost.all() == (b % 2 == 1)
                assert not image[b][:, lost].any() and not label_map[b][lost].any()
            for c in range(2):
                _check_plane(image[b, c], r["planes"][c], SHAPES[c], f"{mode} {padding_mode} field {b} channel {c}")
            assert np.array_equal(label_map[b][r["label"]["sure"]], r["label"]["cls"][r["label"]["sure"]])
            if lost.all():
                assert not crop[b].any()
