"""GPU tests of the patch sampler (micformer_amd/patches.py, csrc/volume_patches.hip) against the numpy referee tests/patches_ref.py,
which restates the rule of include/micformer_patches.h (nnU-Net's sampling rule; parity with nnU-Net itself is unpinned).

Bounds.  origins, picked, label_map, .class_counts and the min / max .stats: exact.  The image is held to two bounds: (1) equal as
numbers (NaN where NaN) to the same window cut from this library's own load_batch(samples, size=<scan shape>, normalisation=...) --
at identity size that call's trilinear weights are exactly (1, 0) and its nearest indices the identity, so it is the already-merged
per-element arithmetic and not the code under test; (2) normalise_ref.close against the float64-statistics referee: 0 failing
elements and a share <= normalise_ref.MAX_SHARE, the existing rule unchanged."""
import numpy as np
import pytest
import torch

import loader_ref as R
import normalise_ref as N
import patches_ref as P

pytestmark = pytest.mark.gpu

VALUES = np.array((0, 0) + R.MMWHS_LABEL_VALUES + (421, -3), np.int32)
NAN = float("nan")


def _image(g, shape, dtype):
    if dtype == np.int16:
        v = g.integers(-400, 2000, size=shape, dtype=np.int16)
    else:
        v = g.random(shape, dtype=np.float32) * np.float32(1500.0) - np.float32(200.0)
    v[g.random(shape) < 0.05] = 0
    return v


def _label(g, shape, dtype=np.int16, values=VALUES):
    return values[g.integers(0, len(values), size=shape)].astype(dtype)


def _dev(sample):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in sample)


def _np(out):
    return [None if t is None else t.cpu().numpy() for t in out]


def _modes(normalisation):
    return (normalisation, normalisation) if isinstance(normalisation, str) else tuple(normalisation)


class Scan:
    """A host sample, its device copy, and what the checks of every patch of it share: the referee's normalised volumes and this
    library's own identity-size load_batch image, each computed once per normalisation."""

    def __init__(self, ct, mr, lab):
        self.host = (ct, mr, lab)
        self.dev = _dev(self.host)
        self._norm, self._own = {}, {}
        self.cmap = None if lab is None else P.full_class_map(lab)

    def normalised(self, normalisation, percentiles=(1, 99)):
        key = (_modes(normalisation), percentiles)
        if key not in self._norm:
            self._norm[key] = tuple(N.normalise(v, m, percentiles) for v, m in zip(self.host[:2], key[0]))
        return self._norm[key]

    def own(self, normalisation, percentiles=(1, 99)):
        from micformer_amd import loader
        key = (_modes(normalisation), percentiles)
        if key not in self._own:
            image, _, _ = loader.load_batch([self.dev], size=self.host[0].shape, normalisation=normalisation, percentiles=percentiles)
            self._own[key] = image[0].cpu().numpy()
        return self._own[key]


def _check(scans, draws, got, patch_size, normalisation="minmax", percentiles=(1, 99), padding_mode="zeros", pad_class=0,
           clamp="both", tag=""):
    """Every sample of a call against the referee (exact fields, image bound 2) and against load_batch's own window (bound 1)."""
    image, label_map, origins, picked = got
    assert image.dtype == np.float16 and origins.dtype == np.int32 and picked.dtype == np.int32
    assert label_map is None or label_map.dtype == np.uint8
    for b, (scan, draw) in enumerate(zip(scans, draws)):
        want = P.sample(*scan.host, draw, patch_size, normalisation=normalisation, percentiles=percentiles, padding_mode=padding_mode,
                        pad_class=pad_class, clamp=clamp, normalised=scan.normalised(normalisation, percentiles), cmap=scan.cmap)
        one = dict(image=image[b], label=None if label_map is None else label_map[b], origin=origins[b], picked=picked[b])
        fails, share, A = N.close(one["image"], want["image"])
        print(f"{tag} sample {b}: origin {origins[b].tolist()} picked {picked[b].tolist()} image fails {fails} share {share:.2e}")
        assert P.compare(one, want) == [], (tag, b, origins[b], want["origin"], picked[b], want["picked"])
        own = scan.own(normalisation, percentiles)
        window = np.stack([P.crop(own[c], origins[b].tolist(), patch_size, "edge" if padding_mode == "border" else "constant", 0)
                           for c in range(2)])
        assert np.array_equal(image[b], window, equal_nan=True), (tag, b)


def _run(scans, draws, patch_size, **kw):
    from micformer_amd import patches
    d = torch.tensor(np.asarray(draws, np.float32)).cuda()
    return _np(patches.sample_batch([s.dev for s in scans], d, patch_size=patch_size, **kw))


# ---- picks -----------------------------------------------------------------------------------------------------------------------

def _picks_label(g, shape=(20, 30, 40)):
    """Every MM-WHS value and strays; class 3 only at the scan's first voxel, class 6 only at its last, class 5 absent."""
    lab = _label(g, shape)
    for v in (500, 600, 820):
        lab[lab == v] = 0
    lab.flat[0] = 500
    lab.flat[-1] = 820
    return lab


def test_picks_at_every_segment_boundary():
    from micformer_amd import patches
    g = np.random.default_rng(9401)
    shape = (20, 30, 40)                                              # 24000 voxels: 11 whole segments and one of 1472
    scan = Scan(_image(g, shape, np.int16), _image(g, shape, np.float32), _picks_label(g, shape))
    cmap = P.full_class_map(scan.host[2])
    present = [c for c in range(1, 8) if (cmap == c).any()]
    assert present == [1, 2, 3, 4, 6, 7] and set(np.unique(cmap)) == {0, 1, 2, 3, 4, 6, 7, 255}
    draws = []
    for c in (1, 7):
        flat = np.flatnonzero(cmap.ravel() == c)
        n = len(flat)
        ranks = {0, n - 1}
        for s in range(1, -(-cmap.size // P.SEGMENT)):                # the ranks on both sides of every segment boundary
            k = int((flat < s * P.SEGMENT).sum())
            ranks |= {k - 1, k}
        assert len(ranks) == 24
        draws += [(1.0, P.steer(present.index(c), 6), P.steer(r, n), 0.1, 0.2, 0.3) for r in sorted(ranks)]
    draws += [(1.0, P.steer(2, 6), 0.7, 0, 0, 0), (1.0, P.steer(4, 6), 0.2, 0, 0, 0)]          # the one-voxel classes 3 and 6
    draws += [(0.5, u, 0.5, 0.9, 0.9, 0.9) for u in (0.0, 0.17, 0.34, 0.5, 0.67, 0.84, 0.999)]  # every present class; 5 is skipped
    draws += [(0.49, 0.5, 0.5, 0.4, 0.5, 0.6), (0.0, 0.5, 0.5, 0.99, 0.0, 0.5)]                  # not forced
    idx = patches.index_scans([scan.dev])
    assert np.array_equal(idx[0].class_counts.cpu().numpy(), P.class_counts(scan.host[2]))
    d = torch.tensor(np.asarray(draws, np.float32)).cuda()
    got = _np(patches.sample_patches([scan.dev] * len(draws), idx * len(draws), d, patch_size=(8, 8, 8)))
    _check([scan] * len(draws), draws, got, (8, 8, 8), tag="picks")
    picked = got[3]
    assert picked[48].tolist() == [3, 0, 0, 0] and picked[49].tolist() == [6, 19, 29, 39]
    assert sorted(set(picked[50:57, 0].tolist())) == present and (picked[57:, 0] == 0).all() and (picked[57:, 1:] == -1).all()


def test_no_foreground_and_no_label_fall_back_to_random_crops():
    g = np.random.default_rng(9402)
    shape = (20, 30, 40)
    ct, mr = _image(g, shape, np.int16), _image(g, shape, np.int16)
    draws = [(1.0, 0.3, 0.6, 0.2, 0.5, 0.9), (1.0, 0.9, 0.1, 0.99, 0.0, 0.4)]
    empty = Scan(ct, mr, _label(g, shape, values=np.array((0, 421, -3))))
    got = _run([empty] * 2, draws, (8, 12, 16))
    _check([empty] * 2, draws, got, (8, 12, 16), tag="no foreground")
    bare = Scan(ct, mr, None)
    none = _run([bare] * 2, draws, (8, 12, 16))
    assert none[1] is None
    _check([bare] * 2, draws, none, (8, 12, 16), tag="no label")
    assert np.array_equal(got[2], none[2]) and (got[3] == np.array(P.RANDOM_PICK)).all() and (none[3] == np.array(P.RANDOM_PICK)).all()


def test_many_segments():
    """(130, 160, 200): 2032 segments, strips of 8 per thread in the locate step; 64 ranks spread over every class."""
    from micformer_amd import patches
    g = np.random.default_rng(9403)
    shape = (130, 160, 200)
    scan = Scan(_image(g, shape, np.int16), _image(g, shape, np.int16), _label(g, shape, np.int32))
    assert -(-scan.host[0].size // P.SEGMENT) > 1000
    idx = patches.index_scans([scan.dev])
    counts = P.class_counts(scan.host[2])
    assert np.array_equal(idx[0].class_counts.cpu().numpy(), counts)
    assert np.array_equal(idx[0].stats.cpu().numpy(), np.array([[v.min(), v.max()] for v in scan.host[:2]], np.float64))
    draws = []
    for i in range(64):
        c, n = i % 7, int(counts[1 + i % 7])
        r = [0, n - 1, n // 2][i // 7] if i // 7 < 3 else int(g.integers(0, n))
        draws.append((1.0, P.steer(c, 7), P.steer(r, n), 0, 0, 0))
    d = torch.tensor(np.asarray(draws, np.float32)).cuda()
    got = _np(patches.sample_patches([scan.dev] * 64, idx * 64, d, patch_size=(8, 8, 16)))
    _check([scan] * 64, draws, got, (8, 8, 16), tag="many segments")
    assert sorted(set(got[3][:, 0].tolist())) == list(range(1, 8))


# ---- origins -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def odd_scan():
    g = np.random.default_rng(9404)
    shape = (37, 41, 45)
    lab = _label(g, shape)
    lab[-2, -1, -3] = 850                                             # class 7's last voxel, near the far corner
    lab[-1] = np.where(lab[-1] == 850, 0, lab[-1])
    lab[-2, -1, -2:] = 0
    return Scan(_image(g, shape, np.int16), _image(g, shape, np.float32), lab)


@pytest.mark.parametrize("patch_size", [(16, 24, 32), (37, 41, 45), (40, 45, 45), (40, 45, 48)], ids=str)
@pytest.mark.parametrize("clamp", ["both", "lower"])
def test_origins(odd_scan, patch_size, clamp):
    """A patch inside the scan, equal to it, and larger by an odd (3) and an even (4) amount on different axes; random draws over
    the range and outside it; forced picks at the first and last voxel of a class and in the middle."""
    cmap = P.full_class_map(odd_scan.host[2])
    n7 = int((cmap == 7).sum())
    assert np.unravel_index(np.flatnonzero(cmap.ravel() == 7)[-1], cmap.shape) == (35, 40, 42)
    draws = [(0.0, 0, 0, 0.0, 0.5, 0.999), (0.0, 0, 0, 0.999, 0.0, 0.5), (0.0, 0, 0, -1.0, 1.0, NAN), (0.0, 0, 0, 2.0, NAN, -0.0),
             (NAN, 0.5, 0.5, 0.3, 0.6, 0.9),                                                     # force NaN: not forced
             (1.0, P.steer(6, 7), P.steer(n7 - 1, n7), 0, 0, 0), (1.0, P.steer(6, 7), 1.0, 0, 0, 0), (1.0, 1.0, 2.0, 0, 0, 0),
             (1.0, -1.0, -1.0, 0, 0, 0), (1.0, NAN, NAN, 0, 0, 0), (1.0, P.steer(3, 7), 0.5, 0, 0, 0)]
    got = _run([odd_scan] * len(draws), draws, patch_size, clamp=clamp, pad_class=255)
    _check([odd_scan] * len(draws), draws, got, patch_size, clamp=clamp, pad_class=255, tag=f"origins {patch_size} {clamp}")
    assert got[3][5].tolist() == got[3][6].tolist() == got[3][7].tolist() == [7, 35, 40, 42]
    assert got[3][8].tolist() == got[3][9].tolist() == [1] + [int(i) for i in np.argwhere(cmap == 1)[0]]
    if patch_size == (16, 24, 32):
        assert got[2][5].tolist() == ([21, 17, 13] if clamp == "both" else [27, 28, 26])      # lower: runs past the far end


# ---- content -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def content_scans():
    g = np.random.default_rng(9405)
    shape = (21, 26, 45)
    a = Scan(_image(g, shape, np.int16), _image(g, shape, np.float32), _label(g, shape, np.int32))
    b = Scan(_image(g, shape, np.float32), _image(g, shape, np.int16), _label(g, shape, np.int16))
    return a, b


@pytest.mark.parametrize("normalisation", ["minmax", "zscore", "percentile", ("zscore", "minmax"), ("minmax", "percentile")], ids=str)
def test_content(content_scans, normalisation):
    """Every normalisation and two mixed pairs; int16 / float32 images and int32 / int16 labels; both padding modes; pad_class 0 and
    255; Pw = 32 (vector stores) and 13 (scalar); odd x origins; padding on both sides of z (need 3) and past the far end (lower)."""
    from micformer_amd import loader, patches
    percentiles = (2, 97)
    devs = [s.dev for s in content_scans]
    idx = patches.index_scans(devs, normalisation=normalisation, percentiles=percentiles)
    _, _, _, stats = loader.load_batch(devs, size=(2, 2, 2), normalisation=normalisation, percentiles=percentiles, return_stats=True)
    for b, scan in enumerate(content_scans):
        assert torch.equal(idx[b].stats.view(torch.int64), stats[b].view(torch.int64))             # exactly load_batch's
        assert np.array_equal(idx[b].class_counts.cpu().numpy(), P.class_counts(scan.host[2]))
        for c, mode in enumerate(_modes(normalisation)):
            if mode == "minmax":
                assert idx[b].stats[c].tolist() == [float(scan.host[c].min()), float(scan.host[c].max())]
    for Pw, ux in ((32, P.steer(5, 14)), (13, P.steer(7, 33))):
        patch = (24, 16, Pw)
        draws = [(0.0, 0, 0, 0.0, 0.3, ux), (1.0, 0.99, 1.0, 0, 0, 0)]                              # odd x origin; last voxel of class 7
        for padding_mode, pad_class, clamp in (("zeros", 0, "both"), ("border", 255, "lower"), ("border", 0, "both"), ("zeros", 255, "lower")):
            kw = dict(normalisation=normalisation, percentiles=percentiles, padding_mode=padding_mode, pad_class=pad_class, clamp=clamp)
            d = torch.tensor(np.asarray(draws, np.float32)).cuda()
            got = _np(patches.sample_patches(devs, idx, d, patch_size=patch, padding_mode=padding_mode, pad_class=pad_class, clamp=clamp))
            _check(content_scans, draws, got, patch, tag=f"content {normalisation} {Pw} {padding_mode} {clamp}", **kw)
            assert got[2][0, 2] % 2 == 1 and got[2][0, 0] < 0
            assert (got[1] == pad_class).any()


@pytest.fixture(scope="module")
def int16_scans():
    """The production configuration -- int16 CT, int16 MR, int16 label (and the same pair without a label) -- which alone takes the
    crop kernel's vector-load branch (two aligned 16-byte loads per array and a shift); w is odd, so the byte offset of a group's
    first element takes all eight 2-byte values over the rows.  Class 7's last voxel is the array's last element."""
    g = np.random.default_rng(9408)
    shape = (21, 26, 45)
    ct, mr, lab = _image(g, shape, np.int16), _image(g, shape, np.int16), _label(g, shape, np.int16)
    lab.flat[-1] = 850
    return Scan(ct, mr, lab), Scan(ct, mr, None)


@pytest.mark.parametrize("normalisation", ["minmax", "zscore", "percentile", ("zscore", "minmax"), ("minmax", "percentile")], ids=str)
def test_content_of_an_all_int16_scan(int16_scans, normalisation):
    """The vector-load branch of the crop: every normalisation and two mixed pairs, both padding modes, pad_class 0 and 255, Pw = 32,
    odd and even x origins in rows of odd length (every 2-byte offset of the first element inside its 16-byte vector), windows
    across the near and far border of z and y (whole groups outside: the branch's own border and pad_class handling), across the
    far border of x (groups that fall back to per-element loads next to groups that do not), and one that ends on the array's last
    row and element.  Held to the same two bounds as every other test."""
    from micformer_amd import patches
    labelled, bare = int16_scans
    percentiles = (2, 97)
    assert all(a.dtype == np.int16 for a in labelled.host) and labelled.host[0].shape[2] % 2 == 1
    cmap = labelled.cmap
    n7 = int((cmap == 7).sum())
    assert np.flatnonzero(cmap.ravel() == 7)[-1] == cmap.size - 1
    last = (1.0, P.steer(6, 7), P.steer(n7 - 1, n7), 0, 0, 0)                                      # the array's last element
    cases = [((24, 16, 32), [(0.0, 0, 0, 0.0, 0.3, P.steer(5, 14)), (0.0, 0, 0, 0.99, 0.9, P.steer(6, 14)), last]),   # z: need 3
             ((16, 32, 32), [(0.0, 0, 0, 0.5, 0.0, P.steer(13, 14)), (0.0, 0, 0, 0.2, 0.99, P.steer(0, 14)), last])]  # y: need 6
    idx = {s: patches.index_scans([s.dev], normalisation=normalisation, percentiles=percentiles) for s in int16_scans}
    offsets = set()
    for patch, draws in cases:
        assert patch[2] % 8 == 0
        d = torch.tensor(np.asarray(draws, np.float32)).cuda()
        for padding_mode, pad_class, clamp in (("zeros", 0, "both"), ("border", 255, "lower"), ("border", 0, "both"), ("zeros", 255, "lower")):
            kw = dict(normalisation=normalisation, percentiles=percentiles, padding_mode=padding_mode, pad_class=pad_class, clamp=clamp)
            got = {}
            for scan in int16_scans:
                got[scan] = _np(patches.sample_patches([scan.dev] * 3, idx[scan] * 3, d, patch_size=patch, padding_mode=padding_mode,
                                                       pad_class=pad_class, clamp=clamp))
                _check([scan] * 3, draws, got[scan], patch, tag=f"int16 {normalisation} {patch} {padding_mode} {clamp}", **kw)
            _, label_map, origins, picked = got[labelled]
            assert got[bare][1] is None and np.array_equal(got[bare][2][:2], origins[:2])
            assert {int(origins[0, 2]) % 2, int(origins[1, 2]) % 2} == {0, 1}
            assert (origins[:2, :2].min(axis=0) < 0).any()                                         # a border of z or y is crossed
            assert (label_map == pad_class).any() and set(range(1, 8)) <= set(np.unique(label_map).tolist())
            assert picked[2].tolist() == [7, 20, 25, 44]
            assert (origins[2] + np.array(patch) >= np.array(cmap.shape)).all()                    # it ends on (or past) the last row
            d_, h_, w_ = cmap.shape
            for o in origins.tolist():                             # first-element offsets of the groups that lie inside a row
                zz = np.clip(np.arange(o[0], o[0] + patch[0]), 0, d_ - 1)[:, None, None]
                yy = np.clip(np.arange(o[1], o[1] + patch[1]), 0, h_ - 1)[None, :, None]
                xx = (o[2] + 8 * np.arange(patch[2] // 8))[None, None, :]
                ok = (xx >= 0) & (xx + 8 <= w_)
                offsets |= set((((zz * h_ + yy) * w_ + xx)[np.broadcast_to(ok, (patch[0], patch[1], patch[2] // 8))] % 8).tolist())
    assert offsets == set(range(8))


def test_front_end_rejects_unequal_shapes_and_foreign_indexes():
    from micformer_amd import patches
    ct = torch.zeros(4, 5, 6, dtype=torch.int16, device="cuda")
    lab = torch.zeros(4, 5, 6, dtype=torch.int32, device="cuda")
    draws = torch.zeros(1, 6, device="cuda")
    for bad in [(ct, torch.zeros(4, 5, 7, device="cuda"), None), (ct, ct, torch.zeros(3, 5, 6, dtype=torch.int16, device="cuda")),
                (ct, torch.zeros(5, 4, 6, dtype=torch.int16, device="cuda"), lab)]:
        with pytest.raises(ValueError, match="must have the same shape"):
            patches.index_scans([bad])
        with pytest.raises(ValueError, match="must have the same shape"):
            patches.sample_patches([bad], [], draws)
    with pytest.raises(ValueError, match="1 samples but 0 indexes"):
        patches.sample_patches([(ct, ct, lab)], [], draws)
    idx = patches.index_scans([(ct, ct, lab)])
    with pytest.raises(ValueError, match="index 0 was built for a scan of shape"):                # other dtypes: a foreign index
        patches.sample_patches([(ct, ct.float(), lab)], idx, draws)
    with pytest.raises(ValueError, match="index 0 was built for a scan of shape"):
        patches.sample_patches([(ct, ct, None)], idx, draws)


# ---- batch -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nine():
    g = np.random.default_rng(9406)
    scans = []
    for b in range(9):
        shape = (12 + 3 * b, 30 - 2 * b, 17 + 5 * (b % 4))
        scans.append(Scan(_image(g, shape, np.int16 if b % 2 else np.float32), _image(g, shape, np.float32 if b % 3 else np.int16),
                          _label(g, shape, np.int32 if b % 2 else np.int16)))
    draws = np.concatenate([P.forced_column(9, 1 / 3)[:, None], g.random((9, 5), dtype=np.float32)], axis=1)
    draws[4, 0] = 1.0
    return scans, draws


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_batch_of_nine(nine):
    from micformer_amd import patches
    scans, draws = nine
    patch, kw = (16, 16, 24), dict(normalisation=("percentile", "zscore"), padding_mode="border", pad_class=255)
    got = _run(scans, draws, patch, **kw)
    _check(scans, draws, got, patch, tag="nine", **kw)
    assert (got[3][[4, 6, 7, 8], 0] > 0).all() and (got[3][[0, 1, 2, 3, 5], 0] == 0).all()
    assert _same(got, _run(scans, draws, patch, **kw))                # two runs: bit-identical
    for b in (0, 4, 8):                                               # each sample equals its single-sample call
        assert _same([t[b:b + 1] for t in got], _run(scans[b:b + 1], draws[b:b + 1], patch, **kw))
    perm = [8, 3, 0, 5, 1, 7, 2, 6, 4]
    assert _same([t[perm] for t in got], _run([scans[i] for i in perm], draws[perm], patch, **kw))
    # a stored index, and out=
    devs = [s.dev for s in scans]
    idx = patches.index_scans(devs, normalisation=kw["normalisation"])
    d = torch.tensor(draws).cuda()
    out = (torch.zeros(9, 2, *patch, dtype=torch.float16, device="cuda"), torch.zeros(9, *patch, dtype=torch.uint8, device="cuda"),
           torch.zeros(9, 3, dtype=torch.int32, device="cuda"), torch.zeros(9, 4, dtype=torch.int32, device="cuda"))
    res = patches.sample_patches(devs, idx, d, patch_size=patch, padding_mode="border", pad_class=255, out=out)
    assert all(r is o for r, o in zip(res, out)) and _same(_np(out), got)
    # a foreign index raises
    with pytest.raises(ValueError, match="index 0 was built for a scan"):
        patches.sample_patches(devs, idx[1:] + idx[:1], d, patch_size=patch)
    other = patches.index_scans(devs[:1], normalisation="minmax")
    with pytest.raises(ValueError, match="another normalisation"):
        patches.sample_patches(devs, idx[:8] + [patches.PatchIndex(idx[8].buffer, idx[8].shape, idx[8].dtypes, idx[8].label_values,
                                                                   other[0].modes, idx[8].percentiles)], d, patch_size=patch)
    with pytest.raises(ValueError, match="out label_map"):
        patches.sample_patches(devs, idx, d, patch_size=patch, out=(out[0], None, out[2], out[3]))


def test_capture_and_replay_under_a_graph(nine):
    """One capture with out=, replayed with new draws written into the same tensor, against eager calls; a single stream."""
    from micformer_amd import patches
    scans, draws = nine
    devs = [s.dev for s in scans[:3]]
    patch = (16, 16, 24)
    idx = patches.index_scans(devs)
    d = torch.tensor(draws[:3]).cuda()
    eager = _np(patches.sample_patches(devs, idx, d, patch_size=patch))
    out = (torch.zeros(3, 2, *patch, dtype=torch.float16, device="cuda"), torch.zeros(3, *patch, dtype=torch.uint8, device="cuda"),
           torch.zeros(3, 3, dtype=torch.int32, device="cuda"), torch.zeros(3, 4, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            patches.sample_patches(devs, idx, d, patch_size=patch, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(_np(out), eager)
    for rows in ([3, 4, 5], [6, 7, 8]):                               # new draws in the same tensor: the replay reads them
        d.copy_(torch.tensor(draws[rows]))
        d[:, 0] = 1.0
        graph.replay()
        torch.cuda.synchronize()
        replayed = _np(out)
        want = _np(patches.sample_patches(devs, idx, d.clone(), patch_size=patch))
        assert _same(replayed, want) and not _same(replayed, eager)
        assert (replayed[3][:, 0] > 0).all()


def test_outputs_feed_the_training_chain_without_a_copy():
    """32^3 patches -> data.prepare_raw_batch -> tiny Head -> MDiceLoss, against the same chain fed with the referee's patches."""
    from micformer_amd import data, patches
    from micformer_amd.loss.dice import MDiceLoss
    from tiny_model import tiny_head
    g = np.random.default_rng(9407)
    shape = (40, 36, 50)
    scans = [Scan(_image(g, shape, np.int16), _image(g, shape, np.float32), _label(g, shape)) for _ in range(2)]
    draws = [(0.0, 0.1, 0.2, 0.3, 0.4, 0.5), (1.0, 0.6, 0.7, 0, 0, 0)]
    d = torch.tensor(np.asarray(draws, np.float32)).cuda()
    image, label_map, origins, picked = patches.sample_batch([s.dev for s in scans], d, patch_size=(32, 32, 32))
    ref = [P.sample(*s.host, dr, (32, 32, 32)) for s, dr in zip(scans, draws)]
    r_image = torch.from_numpy(np.stack([r["image"].astype(np.float16) for r in ref])).cuda()
    r_label = torch.from_numpy(np.stack([r["label"] for r in ref])).cuda()
    assert torch.equal(label_map, r_label) and int((label_map == 255).sum()) > 0
    assert torch.equal(image.view(torch.int16), r_image.view(torch.int16))            # min-max: one IEEE divide, the same bits
    model, crit = tiny_head(), MDiceLoss()
    params = torch.tensor([[1, 0, 1, 0.07, -0.03], [0, 1, 0, -0.05, 0.09]], dtype=torch.float32).cuda()
    losses = []
    for img, lab in ((image, label_map), (r_image, r_label)):
        ptr = img.data_ptr()
        x, y = data.prepare_raw_batch(img, lab, params)
        assert img.data_ptr() == ptr and img.is_contiguous()
        with torch.no_grad():
            losses.append(crit(model(x), y).float().reshape(1).clone())
    assert torch.isfinite(losses[0]).all()
    assert torch.equal(losses[0].view(torch.int32), losses[1].view(torch.int32)), (float(losses[0]), float(losses[1]))
