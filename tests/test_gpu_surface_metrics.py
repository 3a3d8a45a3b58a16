"""micformer_amd.metrics on the MI355X against the referee (tests/surface_metrics_ref.py): HD at every percentile / directed /
include_background setting, IoU, the degenerate cases, both input forms, run-to-run bit-identity, the full 512x512x256 volume
against the bounded referee, and the logits -> argmax mask -> metric path."""
import math

import numpy as np
import pytest
import torch

import surface_metrics_ref as R

pytestmark = pytest.mark.gpu


def _assert_same(got, want):
    got, want = got.detach().cpu().float(), want.float()
    assert got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (got, want)
    gi, wi = torch.isinf(got), torch.isinf(want)
    assert torch.equal(gi, wi), (got, want)
    fin = ~(gn | gi)
    a, b = got[fin].numpy(), want[fin].numpy()
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 1, (a, b)


def _shift(t, s):
    """t shifted by s voxels along (D, H, W), background (0) filling the vacated faces (no wrap-around)."""
    out = torch.zeros_like(t)
    src = [slice(max(0, -k), t.shape[i + 1] - max(0, k)) for i, k in enumerate(s)]
    dst = [slice(max(0, k), t.shape[i + 1] - max(0, -k)) for i, k in enumerate(s)]
    out[:, dst[0], dst[1], dst[2]] = t[:, src[0], src[1], src[2]]
    return out


def _pair(B, D, H, W, mode):
    from oracle import fill
    gt = fill.make_label_map(B, D, H, W)
    if mode == "shift":
        pred = _shift(gt, (2, -1, 1))
    elif mode == "dilate":
        m = torch.nn.functional.max_pool3d(gt.float()[:, None], 3, 1, 1)[:, 0].long()
        pred = m
    else:
        pred = fill.make_label_map(B, D, H, W).flip(3)
    return pred.to(torch.uint8), gt.to(torch.uint8)


@pytest.mark.parametrize("shape,mode", [((48, 48, 48), "shift"), ((37, 52, 61), "dilate"), ((128, 128, 128), "shift")])
def test_hd_and_iou_match_referee(shape, mode):
    from micformer_amd import metrics
    pred, gt = _pair(2, *shape, mode)
    ref = R.PairDistances(R.memberships(pred, 8), R.memberships(gt, 8))
    p, g = pred.cuda(), gt.cuda()
    for inc in (False, True):
        for pct in (None, 5, 50, 95, 100):
            for directed in (False, True):
                got = metrics.hausdorff_distance(p, g, num_classes=8, include_background=inc, percentile=pct, directed=directed)
                _assert_same(got, ref.hd(inc, pct, directed))
        for ie in (True, False):
            _assert_same(metrics.mean_iou(p, g, num_classes=8, include_background=inc, ignore_empty=ie),
                         R.mean_iou(pred, gt, 8, inc, ie))


def _degenerate():
    s = (14, 15, 16)
    lab_p = torch.zeros((1,) + s, dtype=torch.uint8)
    lab_g = torch.zeros((1,) + s, dtype=torch.uint8)
    lab_p[0, 5, 4:7, 6:9] = 1            # class 1: a one-voxel plate vs a voxel in it
    lab_g[0, 5, 5, 7] = 1
    lab_p[0, 3, 2, 4:12] = 2             # class 2: one-voxel lines
    lab_g[0, 3, 2, 6:9] = 2
    lab_p[0, 9, 9, 9] = 3                # class 3: the same single voxel
    lab_g[0, 9, 9, 9] = 3
    lab_p[0, :, 10:, :3] = 4             # class 4: touching the volume border
    lab_g[0, :6, 11:, :] = 4
    lab_p[0, 11:13, 1:4, 12:15] = 5      # class 5: empty in gt
    lab_g[0, 1:4, 1:4, 12:15] = 6        # class 6: empty in pred; class 7: empty in both
    lab_p[0, 0, 0, 0] = 255              # ignore value: no class
    lab_g[0, 13, 14, 15] = 255
    return lab_p, lab_g


def test_degenerate_cases_on_device():
    from micformer_amd import metrics
    pred, gt = _degenerate()
    ref = R.PairDistances(R.memberships(pred, 8), R.memberships(gt, 8))
    for pct in (None, 0, 50, 95, 100):
        for directed in (False, True):
            got = metrics.hausdorff_distance(pred.cuda(), gt.cuda(), num_classes=8, percentile=pct, directed=directed)
            want = ref.hd(False, pct, directed)
            _assert_same(got, want)
    assert math.isinf(float(want[0, 4])) and math.isinf(float(want[0, 5])) and math.isnan(float(want[0, 6]))
    _assert_same(metrics.mean_iou(pred.cuda(), gt.cuda(), num_classes=8), R.mean_iou(pred, gt, 8))
    _assert_same(metrics.mean_iou(pred.cuda(), gt.cuda(), num_classes=8, ignore_empty=False), R.mean_iou(pred, gt, 8, ignore_empty=False))


def test_onehot_form_equals_class_map_and_multilabel_matches_referee():
    from micformer_amd import metrics
    from oracle import fill
    pred, gt = _pair(2, 40, 36, 44, "shift")
    oh_p = torch.nn.functional.one_hot(pred.long(), 8).permute(0, 4, 1, 2, 3).contiguous()     # int64, as the notebook's
    oh_g = fill.one_hot(gt.long())
    a = metrics.hausdorff_distance(pred.cuda(), gt.cuda(), num_classes=8, percentile=95)
    b = metrics.HausdorffDistanceMetric(include_background=False, percentile=95)(oh_p.cuda(), oh_g.cuda())
    assert torch.equal(a.cpu(), b.cpu())
    assert torch.equal(metrics.mean_iou(pred.cuda(), gt.cuda(), num_classes=8).cpu(),
                       metrics.MeanIoU(include_background=False)(oh_p.cuda(), oh_g.cuda()).cpu())
    # overlapping planes: class 1 also covers class 2's voxels, plus a plane with a non-1 value that is no member
    mp, mg = oh_p.float().clone(), oh_g.clone()
    mp[:, 1] = torch.clamp(mp[:, 1] + mp[:, 2], max=1)
    mg[:, 3] = mg[:, 3] * 0.5 + mg[:, 4]
    for pct in (None, 95):
        _assert_same(metrics.hausdorff_distance(mp.cuda(), mg.cuda(), percentile=pct), R.hausdorff_distance(mp, mg, percentile=pct))
    _assert_same(metrics.mean_iou(mp.cuda(), mg.cuda()), R.mean_iou(mp, mg))


def test_two_calls_are_bit_identical():
    from micformer_amd import metrics
    pred, gt = _pair(2, 64, 64, 64, "other")
    p, g = pred.cuda(), gt.cuda()
    a = metrics.hausdorff_distance(p, g, num_classes=8, percentile=95)
    b = metrics.hausdorff_distance(p, g, num_classes=8, percentile=95)
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_full_size_against_bounded_referee():
    from micformer_amd import metrics
    from oracle import fill
    gt = torch.zeros(1, 512, 512, 256, dtype=torch.uint8)          # shells kept off the faces: the shift below cuts nothing
    gt[:, 8:504, 8:504, 8:248] = fill.make_label_map(1, 496, 496, 240).to(torch.uint8)
    pred = _shift(gt, (1, -2, 1))
    ref = R.PairDistances(R.memberships(pred, 8), R.memberships(gt, 8), sq_fn=R.bounded_surface_sq(4))
    p, g = pred.cuda(), gt.cuda()
    for pct in (None, 95):
        _assert_same(metrics.hausdorff_distance(p, g, num_classes=8, percentile=pct), ref.hd(False, pct, False))
    _assert_same(metrics.mean_iou(p, g, num_classes=8), R.mean_iou(pred, gt, 8))


def test_logits_argmax_mask_to_metrics():
    from micformer_amd import metrics, ops
    from oracle import fill
    B, D, H, W = 2, 32, 40, 36
    gt = fill.make_label_map(B, D, H, W).to(torch.uint8)
    torch.manual_seed(0)
    logits = (fill.one_hot(gt.long()) * 2.0 + torch.randn(B, 8, D, H, W)).contiguous()
    mask, _ = ops.argmax_meandice(logits.cuda(), gt.cuda())
    m = mask.cpu()
    assert torch.equal(m, logits.argmax(1).to(torch.uint8))
    _assert_same(metrics.hausdorff_distance(mask, gt.cuda(), num_classes=8, percentile=95),
                 R.hausdorff_distance(m, gt, 8, percentile=95))
    _assert_same(metrics.mean_iou(mask, gt.cuda(), num_classes=8), R.mean_iou(m, gt, 8))
