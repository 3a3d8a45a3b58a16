"""GPU tests of the connected components (micformer_amd/postprocess.py, csrc/volume_components.hip) against the referee
tests/components_ref.py (scipy.ndimage.label per class on the host).  Every result is an integer: every comparison is exact
equality.  The shapes are small on purpose: what matters is that they cross the 64 x 8 x 8 tile on every axis, with remainders."""
import functools
import itertools

import numpy as np
import pytest
import torch

import components_ref as C
from tiny_model import tiny_head

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 70), (5, 1, 1), (3, 5, 7), (9, 17, 65), (17, 33, 130), (40, 70, 130)]
CONNS = [6, 18, 26]
SCENES = {
    # name: (shape, index) -> uint8 class map, and its class count
    "noise_0.2": (lambda s, i: C.binary_noise(s, 0.2, i), 2),
    "noise_0.31": (lambda s, i: C.binary_noise(s, 0.31, i), 2),
    "noise_0.5": (lambda s, i: C.binary_noise(s, 0.5, i), 2),
    "noise_0.9": (lambda s, i: C.binary_noise(s, 0.9, i), 2),
    "classes8": (lambda s, i: C.class_noise(s, 8, i), 8),
    "blobs8": (lambda s, i: C.blobs(s, 8, i), 8),
    "zeros": (lambda s, i: np.zeros(s, np.uint8), 2),
    "ones": (lambda s, i: np.ones(s, np.uint8), 2),
    "checkerboard": (lambda s, i: C.checkerboard(s), 2),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def scene(name):
    make, K = SCENES[name]
    return [make(s, i) for i, s in enumerate(SHAPES)], K


@functools.lru_cache(maxsize=None)
def scene_reference(name, conn):
    vols, K = scene(name)
    return [C.components(v, K, None, conn) for v in vols]


@functools.lru_cache(maxsize=None)
def island_scene():
    """8-class blobs with planted islands at a shape that crosses tiles on every axis, and its int16 / int32 label volumes with
    three voxels of a value that names no class."""
    cmap = C.blobs_with_islands((40, 70, 130), 8, seed=5, islands=40)
    forms = {torch.uint8: cmap}
    for dtype, np_dtype in ((torch.int16, np.int16), (torch.int32, np.int32)):
        v = C.to_values(cmap, C.MMWHS_LABEL_VALUES, np_dtype)
        v[3, 4, 5] = v[20, 69, 129] = v[39, 0, 64] = 77
        forms[dtype] = v
    return forms


def form_args(dtype):
    return (dict(label_values=None, num_classes=8), None) if dtype == torch.uint8 else (dict(label_values=C.MMWHS_LABEL_VALUES), C.MMWHS_LABEL_VALUES)


# ---- labels and sizes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name", list(SCENES))
def test_labels_and_sizes_equal_the_referee(name, conn):
    from micformer_amd import postprocess as P
    vols, K = scene(name)
    want = scene_reference(name, conn)
    labels, sizes = P.connected_components([dev(v) for v in vols], num_classes=K, label_values=None, connectivity=conn, return_sizes=True)
    for shape, lab, siz, (wl, ws) in zip(SHAPES, labels, sizes, want):
        assert lab.dtype == torch.int32 and siz.dtype == torch.int32 and tuple(lab.shape) == shape
        n = len(np.unique(wl)) - (1 if (wl == 0).any() else 0)
        bad_l, bad_s = int((lab.cpu().numpy() != wl).sum()), int((siz.cpu().numpy() != ws).sum())
        print(f"{name} conn {conn} {shape}: {n} components, labels differing {bad_l}, sizes differing {bad_s}")
        assert bad_l == 0 and bad_s == 0, (name, conn, shape)
    if name == "checkerboard":
        on = int(vols[-1].sum())
        ncomp = len(torch.unique(labels[-1])) - 1
        assert ncomp == (on if conn == 6 else 1)


@pytest.mark.parametrize("flipped", [False, True], ids=["root_first", "root_last"])
@pytest.mark.parametrize("conn", CONNS)
def test_a_long_chain_is_one_component(conn, flipped):
    from micformer_amd import postprocess as P
    s = C.snake((17, 33, 130))
    if flipped:
        s = np.ascontiguousarray(s[::-1, ::-1, ::-1])
    wl, ws = C.components(s, 2, None, conn)
    assert len(np.unique(wl)) == 2 and int(ws.max()) == int(s.sum())          # the referee sees one component
    lab, siz = P.connected_components(dev(s), num_classes=2, label_values=None, connectivity=conn, return_sizes=True)
    assert np.array_equal(lab.cpu().numpy(), wl) and np.array_equal(siz.cpu().numpy(), ws)
    if flipped:
        assert int(np.flatnonzero(s.ravel())[0]) + 1 == int(lab.max())       # the root: the first voxel, the far end of the chain


def _contact_cases():
    """(offset, first voxel, second voxel) of every pair of voxels in a (12, 20, 132) volume: the 13 offsets that follow a voxel
    in linear order, each swept along all three axes through every position, the other two coordinates at the tile face that the
    offset crosses (7 -> 8, 8 -> 7 along z and y; 63 -> 64, 64 -> 63 along x).  Sweeping an axis on which the offset is 0 moves a
    pair along the face it crosses: a z- or y-face contact visits every lane, an x-face contact every row and plane of a tile.
    13 * (12 + 20 + 132) placements, less the 27 that leave the volume and the 26 that two sweeps share: 2079."""
    shape = (12, 20, 132)
    cases = {}
    for o in itertools.product((-1, 0, 1), repeat=3):
        if o <= (0, 0, 0):
            continue
        base = [(8 if o[0] < 0 else 7), (8 if o[1] < 0 else 7), (64 if o[2] < 0 else 63)]
        for axis in range(3):
            for t in range(shape[axis]):
                a = list(base)
                a[axis] = t
                b = [a[i] + o[i] for i in range(3)]
                if all(0 <= b[i] < shape[i] for i in range(3)):
                    cases[(o, tuple(a))] = (o, tuple(a), tuple(b))
    return shape, list(cases.values())


@pytest.mark.parametrize("conn", CONNS)
def test_contact_kinds_across_every_boundary(conn):
    from micformer_amd import postprocess as P
    shape, cases = _contact_cases()
    assert len(cases) == 2079
    vols = torch.zeros((len(cases),) + shape, dtype=torch.uint8)
    for i, (_, a, b) in enumerate(cases):
        vols[i][a] = 1
        vols[i][b] = 1
    labels, sizes = P.connected_components(vols.cuda(), num_classes=2, label_values=None, connectivity=conn, return_sizes=True)
    assert int((labels != 0).sum()) == 2 * len(cases) and int((sizes != 0).sum()) == 2 * len(cases)
    labels, sizes = labels.cpu().numpy(), sizes.cpu().numpy()
    rank = {6: 1, 18: 2, 26: 3}[conn]
    wrong = []
    for i, (o, a, b) in enumerate(cases):
        la, lb = (a[0] * shape[1] + a[1]) * shape[2] + a[2] + 1, (b[0] * shape[1] + b[1]) * shape[2] + b[2] + 1
        joined = sum(abs(v) for v in o) <= rank
        want = (min(la, lb), min(la, lb), 2, 2) if joined else (la, lb, 1, 1)
        got = (int(labels[i][a]), int(labels[i][b]), int(sizes[i][a]), int(sizes[i][b]))
        if got != want:
            wrong.append((o, a, b, got, want))
    assert not wrong, wrong[:10]


# ---- ties ---------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_root_and_classes_do_not_interact():
    from micformer_amd import postprocess as P
    vol = np.zeros((10, 12, 140), np.uint8)
    vol[1, 2, 60:70] = 1                                   # class 1: two components of 10 voxels, both across a tile face
    vol[9, 11, 125:135] = 1
    vol[8, 0, 0] = 1                                       # and a smaller one
    vol[0, 0, 0:10] = 2                                    # class 2: one component of 10 voxels, before class 1's in linear order
    vol[5, 5, 5] = 3                                       # class 3: size 1 against size 1
    vol[5, 5, 7] = 3
    got = P.keep_largest_components(dev(vol), num_classes=4, label_values=None).cpu().numpy()
    want = C.keep_largest(vol, 4)
    assert np.array_equal(got, want)
    assert got[1, 2, 60:70].all() and not got[9, 11, 125:135].any() and got[8, 0, 0] == 0
    assert (got[0, 0, 0:10] == 2).all()
    assert got[5, 5, 5] == 3 and got[5, 5, 7] == 0
    # the same with the later component one voxel larger: it wins
    vol[9, 11, 135] = 1
    got = P.keep_largest_components(dev(vol), num_classes=4, label_values=None).cpu().numpy()
    assert np.array_equal(got, C.keep_largest(vol, 4))
    assert not got[1, 2, 60:70].any() and got[9, 11, 125:136].all()


# ---- the filters --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.int32], ids=["uint8", "int16", "int32"])
@pytest.mark.parametrize("conn", [6, 26])
def test_filters_equal_the_referee(dtype, conn):
    from micformer_amd import postprocess as P
    vol = island_scene()[dtype]
    kw, values = form_args(dtype)
    x = dev(vol)
    keep = P.keep_largest_components(x, connectivity=conn, **kw)
    assert keep.dtype == dtype and keep.shape == x.shape and torch.equal(x, dev(vol))        # the input is left alone
    want = C.keep_largest(vol, 8, values, conn)
    removed = int((want != vol).sum())
    print(f"keep largest {dtype} conn {conn}: {removed} voxels removed")
    assert removed > 40
    assert np.array_equal(keep.cpu().numpy(), want)
    if values is not None:
        assert (keep.cpu().numpy() == 77).sum() == 3                                         # values that name no class pass through
    # a subset of the classes; a class that is absent from the volume
    sub = P.keep_largest_components(x, connectivity=conn, classes=(2, 5), **kw)
    assert np.array_equal(sub.cpu().numpy(), C.keep_largest(vol, 8, values, conn, classes=(2, 5)))
    gone = vol.copy()
    gone[vol == (3 if values is None else values[2])] = 0
    assert np.array_equal(P.keep_largest_components(dev(gone), connectivity=conn, **kw).cpu().numpy(), C.keep_largest(gone, 8, values, conn))
    # in place equals out of place
    y = x.clone()
    assert P.keep_largest_components(y, connectivity=conn, out=y, **kw) is y
    assert torch.equal(y, keep)
    # remove small: 1 removes nothing, 2, and exactly a component's size (kept) against one more (removed)
    _, sizes = C.components(vol, 8, values, conn)
    a_size = int(np.sort(np.unique(sizes[sizes > 2]))[0])
    for m in (1, 2, a_size, a_size + 1):
        got = P.remove_small_components(x, m, connectivity=conn, **kw).cpu().numpy()
        want = C.remove_small(vol, m, 8, values, conn)
        assert np.array_equal(got, want), m
        if m == 1:
            assert np.array_equal(got, vol)
    at = np.argwhere(sizes == a_size)[0]
    assert C.remove_small(vol, a_size, 8, values, conn)[tuple(at)] != 0 and C.remove_small(vol, a_size + 1, 8, values, conn)[tuple(at)] == 0
    z = x.clone()
    P.remove_small_components(z, 5, connectivity=conn, classes=(1, 7), out=z, **kw)
    assert np.array_equal(z.cpu().numpy(), C.remove_small(vol, 5, 8, values, conn, classes=(1, 7)))


def test_monai_named_callables():
    from micformer_amd import postprocess as P
    vol = island_scene()[torch.int16]
    x = dev(vol)
    assert torch.equal(P.KeepLargestConnectedComponent()(x), P.keep_largest_components(x))
    assert torch.equal(P.KeepLargestConnectedComponent(applied_labels=[1, 4], connectivity=6)(x),
                       P.keep_largest_components(x, classes=[1, 4], connectivity=6))
    assert torch.equal(P.RemoveSmallObjects(min_size=9)(x), P.remove_small_components(x, 9))


# ---- batching, workspace, determinism ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 9, 17])
def test_mixed_shapes_in_one_call_equal_one_call_each(B):
    from micformer_amd import postprocess as P
    shapes = [SHAPES[(3 * i + 2) % len(SHAPES)] for i in range(B)]
    vols = [dev(C.to_values(C.blobs_with_islands(s, 8, seed=i, islands=6), C.MMWHS_LABEL_VALUES, np.int16)) for i, s in enumerate(shapes)]
    labels, sizes = P.connected_components(vols, return_sizes=True)
    kept = P.keep_largest_components(vols)
    small = P.remove_small_components(vols, 4, connectivity=6)
    assert len(labels) == len(sizes) == len(kept) == len(small) == B
    for i, v in enumerate(vols):
        l1, s1 = P.connected_components(v, return_sizes=True)
        assert torch.equal(labels[i], l1) and torch.equal(sizes[i], s1), i
        assert torch.equal(kept[i], P.keep_largest_components(v)), i
        assert torch.equal(small[i], P.remove_small_components(v, 4, connectivity=6)), i
    # a [B, d, h, w] tensor is a batch too
    if B == 9:
        stack = torch.stack([vols[0]] * 3)
        assert torch.equal(P.keep_largest_components(stack), torch.stack([kept[0]] * 3))


def test_nothing_is_written_beyond_the_queried_workspace():
    from micformer_amd import postprocess as P
    shapes = [(17, 33, 130), (3, 5, 7), (40, 70, 130)]
    vols = [dev(C.class_noise(s, 8, i)) for i, s in enumerate(shapes)]
    n = P.workspace_bytes(shapes)
    pad = 4096
    for run in ("labels", "keep", "small"):
        ws = torch.full((n + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        if run == "labels":
            P.connected_components(vols, num_classes=8, label_values=None, return_sizes=True, workspace=ws)
        elif run == "keep":
            P.keep_largest_components(vols, num_classes=8, label_values=None, workspace=ws)
        else:
            P.remove_small_components(vols, 3, num_classes=8, label_values=None, workspace=ws)
        assert bool((ws[n:] == 0xA5).all()), run
    with pytest.raises(ValueError, match="workspace"):
        P.keep_largest_components(vols, num_classes=8, label_values=None, workspace=ws[: n - 1])


def test_two_runs_are_bit_identical():
    from micformer_amd import postprocess as P
    x = dev(island_scene()[torch.int16])
    noise = dev(C.binary_noise((40, 70, 130), 0.31, 3))
    for v, kw in ((x, {}), (noise, dict(num_classes=2, label_values=None, connectivity=6))):
        a = P.connected_components(v, return_sizes=True, **kw)
        b = P.connected_components(v, return_sizes=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(P.keep_largest_components(v, **kw), P.keep_largest_components(v, **kw))
        assert torch.equal(P.remove_small_components(v, 6, **kw), P.remove_small_components(v, 6, **kw))


def test_capture_and_replay_under_a_graph():
    from micformer_amd import postprocess as P
    shapes = [(17, 33, 130), (9, 17, 65)]
    make = lambda seed: [C.to_values(C.blobs_with_islands(s, 8, seed=seed + i, islands=8), C.MMWHS_LABEL_VALUES, np.int16)
                         for i, s in enumerate(shapes)]
    vols = [dev(v) for v in make(0)]
    eager = P.keep_largest_components(vols)
    eager_small = P.remove_small_components(vols, 5)
    out = [torch.zeros_like(t) for t in vols]
    out_small = [torch.zeros_like(t) for t in vols]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            P.keep_largest_components(vols, out=out)
            P.remove_small_components(vols, 5, out=out_small)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager)) and all(torch.equal(a, b) for a, b in zip(out_small, eager_small))
    # fresh contents in the same buffers: the replay reads them
    fresh = make(50)
    for t, v in zip(vols, fresh):
        t.copy_(torch.from_numpy(v))
    graph.replay()
    torch.cuda.synchronize()
    for o, os_, v in zip(out, out_small, fresh):
        assert np.array_equal(o.cpu().numpy(), C.keep_largest(v, 8, C.MMWHS_LABEL_VALUES))
        assert np.array_equal(os_.cpu().numpy(), C.remove_small(v, 5, 8, C.MMWHS_LABEL_VALUES))
    assert not any(torch.equal(a, b) for a, b in zip(out, eager))


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_segment_pair_with_keep_largest():
    from micformer_amd import postprocess as P, restore
    g = np.random.default_rng(41)
    shape, size = (41, 50, 37), (32, 32, 32)
    ct = torch.from_numpy(g.integers(-1000, 3000, size=shape, dtype=np.int16)).cuda()
    mr = torch.from_numpy(g.integers(0, 1500, size=shape, dtype=np.int16)).cuda()
    model = tiny_head()
    plain = restore.segment_pair(model, ct, mr, size=size)
    clean = restore.segment_pair(model, ct, mr, size=size, keep_largest=True)
    assert clean.dtype == torch.int16 and clean.shape == plain.shape
    assert torch.equal(clean, P.keep_largest_components(plain))
    assert np.array_equal(clean.cpu().numpy(), C.keep_largest(plain.cpu().numpy(), 8, C.MMWHS_LABEL_VALUES))
    assert torch.equal(plain, restore.segment_pair(model, ct, mr, size=size, keep_largest=False))


def test_clean_up_takes_a_far_island_out_of_hd95():
    from micformer_amd import metrics, postprocess as P
    gt = np.zeros((24, 40, 72), np.uint8)
    gt[4:7, 6:9, 8:11] = 1                                 # 27 voxels, 26 of them on the edge
    gt[14:20, 22:36, 40:66] = 2
    pred = gt.copy()
    island = pred.copy()
    island[22, 38, 69:72] = 1                              # a 3-voxel island of class 1 in the far corner: 3 of 29 edge voxels

    def hd95(p):
        return metrics.hausdorff_distance(dev(p)[None], dev(gt)[None], num_classes=3, percentile=95).cpu()

    without, with_island = hd95(pred), hd95(island)
    print(f"HD95 per class without the island {without.tolist()}, with it {with_island.tolist()}")
    assert float(without[0, 0]) == 0.0 and float(with_island[0, 0]) > 50.0 and float(with_island[0, 1]) == float(without[0, 1])
    cleaned = P.keep_largest_components(dev(island), num_classes=3, label_values=None)
    assert np.array_equal(cleaned.cpu().numpy(), pred)
    assert torch.equal(hd95(cleaned.cpu().numpy()), without)


# ---- one mid-size case ----------------------------------------------------------------------------------------------------------

def test_mid_size_blobs_against_the_referee():
    from micformer_amd import postprocess as P
    vol = C.blobs_with_islands((128, 128, 128), 8, seed=9, islands=200, sigma=6.0)
    wl, ws = C.components(vol, 8, None, 26)
    lab, siz = P.connected_components(dev(vol), num_classes=8, label_values=None, return_sizes=True)
    print(f"128^3 blobs: {len(np.unique(wl)) - 1} components, the largest {int(ws.max())} voxels")
    assert np.array_equal(lab.cpu().numpy(), wl) and np.array_equal(siz.cpu().numpy(), ws)
    assert np.array_equal(P.keep_largest_components(dev(vol), num_classes=8, label_values=None).cpu().numpy(), C.keep_largest(vol, 8))
