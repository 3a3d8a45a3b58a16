"""micformer_amd.surface on the MI355X against the referee (tests/surface_distance_ref.py): spaced HD at several percentiles,
ASD / ASSD, surface Dice with and without distances equal to the tolerance, bit-equality with the voxel-unit HD at unit spacing,
the input forms (uint8, one-hot, int16 / int32 label values, a restore_labels output), run-to-run and graph-replay identity and
the degenerate cases.  Shapes are the smallest that reach each path: W past one 256-thread tile and one 64-line group, a long
last axis over a mid axis of 3 and of 5, odd extents everywhere."""
import functools
import math

import pytest
import torch

import surface_distance_ref as R
import surface_metrics_ref as M
from test_gpu_surface_metrics import _assert_same, _degenerate, _shift

pytestmark = pytest.mark.gpu

EXACT = (3.0, 0.5, 1.25)             # every product and sum is exact in float64; distances equal to 0.5, 1.0 and 2.0 occur
SPACINGS = {"aniso": ((0.6, 0.35, 0.35), (1.6, 0.43, 0.43)),      # tie-free at the tolerances below
            "exact": (EXACT, (0.6, 0.35, 0.35))}
CASES = [((9, 12, 70), 4, "shells"), ((17, 6, 130), 8, "blobs"), ((33, 40, 261), 8, "blobs"), ((3, 530, 20), 4, "blobs"),
         ((530, 5, 24), 4, "blobs")]
PCTS = (None, 5, 50, 95)


def _taus(K):
    return [(0.5, 1.0, 2.0)[i % 3] for i in range(K - 1)]


def _blobs(B, D, H, W, K, grow):
    """K - 1 solid ellipsoids per sample (later classes overwrite earlier ones where they meet), few enough edge voxels for the
    brute-force referee."""
    z, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    lab = torch.zeros((B, D, H, W), dtype=torch.uint8)
    for b in range(B):
        for k in range(1, K):
            f = [((0.21 + 0.37 * k * (a + 1) + 0.05 * b) % 0.7) + 0.15 for a in range(3)]
            r = [max(1.2, (0.16 + 0.02 * (k % 3)) * n + grow) for n in (D, H, W)]
            inside = (((z - f[0] * D) / r[0]) ** 2 + ((y - f[1] * H) / r[1]) ** 2 + ((x - f[2] * W) / r[2]) ** 2) <= 1.0
            lab[b][inside] = k
    return lab


@functools.lru_cache(maxsize=None)
def _case(shape, K, mode):
    from oracle import fill
    if mode == "shells":
        gt = fill.make_label_map(2, *shape, num_classes=K).to(torch.uint8)
        pred = _shift(gt, (1, -1, 2))
    else:
        gt = _blobs(2, *shape, K, 0.0)
        pred = _shift(_blobs(2, *shape, K, 0.6), (0, 1, -2))
    return pred, gt, M.memberships(pred, K), M.memberships(gt, K)


@functools.lru_cache(maxsize=None)
def _referee(shape, K, mode, spacing):
    _, _, pm, gm = _case(shape, K, mode)
    return R.SurfaceReferee(pm, gm, SPACINGS[spacing] if isinstance(spacing, str) else spacing)


@pytest.mark.parametrize("spacing", sorted(SPACINGS))
@pytest.mark.parametrize("shape,K,mode", CASES, ids=["x".join(map(str, c[0])) for c in CASES])
def test_distances_match_referee(shape, K, mode, spacing):
    """Checks 1 and 2: nan / inf patterns equal, finite values within 1 float32 ulp of the referee's float64 result."""
    from micformer_amd import surface
    pred, gt, _, _ = _case(shape, K, mode)
    ref, sp, tau = _referee(shape, K, mode, spacing), SPACINGS[spacing], _taus(K)
    for b in range(2):                      # the condition under which `<=` cannot flip on a rounding: exact arithmetic, or no near tie
        equal, near = ref.ties(tau, b)
        assert sp[b] == EXACT or (equal == 0 and near == 0), (b, equal, near)
    if spacing == "exact" and mode == "blobs":
        assert ref.ties(tau, 0)[0] > 0      # distances equal to the tolerance do occur, and count as within
    p, g = pred.cuda(), gt.cuda()
    r = surface.surface_distances(p, g, num_classes=K, spacing=sp, percentiles=PCTS, thresholds=tau)
    for name, got, want in [("hd", r.hd, ref.hd(PCTS)), ("hd_directed", r.hd_directed, ref.hd(PCTS, directed=True)),
                            ("asd", r.asd, ref.asd()), ("assd", r.assd, ref.assd()), ("nsd", r.nsd, ref.nsd(tau))]:
        print(name, got.cpu().flatten()[:8].tolist(), want.flatten()[:8].tolist())
        _assert_same(got, want)
    inc = mode == "shells"                  # (the background's edge set is only small enough for brute force there)
    r = surface.surface_distances(p, g, num_classes=K, include_background=inc, spacing=sp, percentiles=(100,))
    assert r.nsd is None
    _assert_same(r.hd, ref.hd((100,), include_background=inc))
    _assert_same(r.asd, ref.asd(include_background=inc))


@pytest.mark.parametrize("shape,K,mode", [CASES[0], CASES[2]], ids=["9x12x70", "33x40x261"])
def test_unit_spacing_equals_voxel_hd_bit_for_bit(shape, K, mode):
    from micformer_amd import metrics, surface
    pred, gt, _, _ = _case(shape, K, mode)
    p, g = pred.cuda(), gt.cuda()
    pcts = (None, 5, 50, 95, 100)
    for inc in (False, True):
        got = [surface.surface_distances(p, g, num_classes=K, include_background=inc, percentiles=pcts[:4]),
               surface.surface_distances(p, g, num_classes=K, include_background=inc, spacing=(1, 1, 1), percentiles=pcts[4:])]
        for i, pct in enumerate(pcts):
            r, j = got[i // 4], i % 4
            for directed in (False, True):
                want = metrics.hausdorff_distance(p, g, num_classes=K, include_background=inc, percentile=pct, directed=directed)
                mine = (r.hd_directed if directed else r.hd)[..., j]
                assert torch.equal(mine.cpu().view(torch.int32), want.cpu().view(torch.int32)), (pct, directed, mine, want)
            assert torch.equal(surface.hausdorff_distance_mm(p, g, num_classes=K, include_background=inc, percentile=pct).cpu()
                               .view(torch.int32), r.hd[..., j].cpu().view(torch.int32))


def _bits(r):
    return [None if t is None else t.cpu().view(torch.int32) for t in r]


def _same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def test_input_forms_give_bit_equal_results():
    from micformer_amd import surface
    from micformer_amd.loader import MMWHS_LABEL_VALUES
    shape, K, mode = CASES[1]
    pred, gt, _, _ = _case(shape, K, mode)
    kw = dict(spacing=SPACINGS["exact"], percentiles=(None, 95), thresholds=_taus(K))
    base = surface.surface_distances(pred.cuda(), gt.cuda(), num_classes=K, **kw)
    oh = [torch.nn.functional.one_hot(t.long(), K).permute(0, 4, 1, 2, 3).contiguous().cuda() for t in (pred, gt)]
    assert _same_bits(base, surface.surface_distances(oh[0], oh[1], **kw))
    lut = torch.tensor((0,) + MMWHS_LABEL_VALUES)
    for dtype in (torch.int16, torch.int32):
        vp, vg = lut[pred.long()].to(dtype), lut[gt.long()].to(dtype)
        assert _same_bits(base, surface.surface_distances(vp.cuda(), vg.cuda(), **kw))                 # the default label values
        stripes = torch.arange(shape[2]) % 3 == 0                                                    # an unlisted value is background
        vp[(vp == 0) & stripes] = 421
        vg[(vg == 0) & ~stripes] = -7
        assert _same_bits(base, surface.surface_distances(vp.cuda(), vg.cuda(), label_values=MMWHS_LABEL_VALUES, **kw))
    other = (3, 1, 9)                                                                                # K = 4 from the values alone
    p4, g4, _, _ = _case(*CASES[0])
    lut4 = torch.tensor((0,) + other)
    got = surface.surface_distances(lut4[p4.long()].short().cuda(), lut4[g4.long()].short().cuda(), label_values=other, **dict(kw, thresholds=_taus(4)))
    assert _same_bits(got, surface.surface_distances(p4.cuda(), g4.cuda(), num_classes=4, **dict(kw, thresholds=_taus(4))))


def test_restored_labels_score_against_a_label_volume():
    """logits -> restore_labels (int16, the dataset's label values, the scan's grid) -> surface_distances, no remap in between."""
    from micformer_amd import restore, surface
    from micformer_amd.loader import MMWHS_LABEL_VALUES
    from oracle import fill
    grid, K = (9, 11, 13), 8
    small = fill.make_label_map(1, 6, 7, 8)
    torch.manual_seed(0)
    logits = (fill.one_hot(small) * 3.0 + 0.3 * torch.randn(1, K, 6, 7, 8)).contiguous().cuda()
    labels = restore.restore_labels(logits, grid)
    assert labels.dtype == torch.int16 and tuple(labels.shape) == grid
    lut = torch.tensor((0,) + MMWHS_LABEL_VALUES)
    truth = lut[fill.make_label_map(1, *grid)[0]].short()
    truth[0, 0, 0] = 421                                                                             # not a label value: background
    sp, tau = (1.6, 0.43, 0.43), [1.0] * (K - 1)
    r = surface.surface_distances(labels, truth.cuda(), spacing=sp, percentiles=(95,), thresholds=tau)
    ref = R.SurfaceReferee(R.label_memberships(labels[None], MMWHS_LABEL_VALUES), R.label_memberships(truth[None], MMWHS_LABEL_VALUES), [sp])
    assert ref.ties(tau, 0) == (0, 0)
    _assert_same(r.hd, ref.hd((95,)))
    _assert_same(r.assd, ref.assd())
    _assert_same(r.nsd, ref.nsd(tau))
    m = surface.SurfaceDistanceMetric(symmetric=True)(labels, truth.cuda(), spacing=sp)
    assert torch.equal(m.cpu().view(torch.int32), r.assd.cpu().view(torch.int32))
    d = surface.SurfaceDiceMetric(tau)(labels, truth.cuda(), spacing=sp)
    assert torch.equal(d.cpu().view(torch.int32), r.nsd.cpu().view(torch.int32))


def test_two_calls_and_graph_replays_are_bit_identical():
    from micformer_amd import surface
    shape, K, mode = CASES[2]
    pred, gt, _, _ = _case(shape, K, mode)
    kw = dict(num_classes=K, spacing=SPACINGS["aniso"], percentiles=(None, 95), thresholds=_taus(K))
    p, g = pred.cuda(), gt.cuda()
    first = surface.surface_distances(p, g, **kw)
    assert _same_bits(first, surface.surface_distances(p, g, **kw))
    swapped = surface.surface_distances(g, p, **kw)
    ws = torch.empty(surface.workspace_bytes(p.shape, K), dtype=torch.uint8, device="cuda")
    sp_, sg_ = p.clone(), g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        surface.surface_distances(sp_, sg_, workspace=ws, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = surface.surface_distances(sp_, sg_, workspace=ws, **kw)
    graph.replay()
    assert _same_bits(captured, first)
    sp_.copy_(g)
    sg_.copy_(p)
    graph.replay()
    assert _same_bits(captured, swapped)


def test_degenerate_cases_follow_the_rules():
    from micformer_amd import surface
    pred, gt = _degenerate()
    tau = [1.0] * 7
    for sp in (EXACT, (1.6, 0.43, 0.43)):
        ref = R.SurfaceReferee(M.memberships(pred, 8), M.memberships(gt, 8), [sp])
        pcts = (None, 50, 95, 100)
        r = surface.surface_distances(pred.cuda(), gt.cuda(), num_classes=8, spacing=sp, percentiles=pcts, thresholds=tau)
        _assert_same(r.hd, ref.hd(pcts))
        _assert_same(r.hd_directed, ref.hd(pcts, directed=True))
        _assert_same(r.asd, ref.asd())
        _assert_same(r.assd, ref.assd())
        _assert_same(r.nsd, ref.nsd(tau))
    hd, asd, assd, nsd = r.hd.cpu(), r.asd.cpu(), r.assd.cpu(), r.nsd.cpu()
    # class 5 (index 4) is empty in gt, class 6 in pred, class 7 in both; class 3 is one voxel on both sides: no edge at all
    assert torch.isinf(hd[0, 4]).all() and torch.isinf(hd[0, 5]).all() and torch.isnan(hd[0, 6]).all() and torch.isnan(hd[0, 2]).all()
    assert math.isinf(float(asd[0, 4, 0])) and math.isnan(float(asd[0, 4, 1]))         # pred -> nothing; nothing -> pred
    assert math.isnan(float(asd[0, 5, 0])) and math.isinf(float(asd[0, 5, 1]))
    assert math.isinf(float(assd[0, 4])) and math.isinf(float(assd[0, 5])) and math.isnan(float(assd[0, 6]))
    assert float(nsd[0, 4]) == 0.0 and float(nsd[0, 5]) == 0.0 and math.isnan(float(nsd[0, 6]))
    swapped = surface.surface_distances(gt.cuda(), pred.cuda(), num_classes=8, spacing=sp, percentiles=pcts, thresholds=tau)
    assert torch.equal(swapped.asd.cpu().view(torch.int32), asd.flip(-1).view(torch.int32))         # the other direction, same rules
    assert torch.equal(swapped.hd.cpu().view(torch.int32), hd.view(torch.int32))
