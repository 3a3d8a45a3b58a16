"""CPU checks of the surface metrics: the referee (tests/surface_metrics_ref.py) against brute force and against scipy, the
workspace queries of include/micformer_metrics.h (tests/test_abi.py has the entry points), and argument errors caught before any launch."""
import math

import numpy as np
import pytest
import torch

import surface_metrics_ref as R


def _shell(shape, centre, r0, r1):
    idx = np.indices(shape).astype(np.float64)
    r = np.sqrt(sum((idx[i] - centre[i]) ** 2 for i in range(3)))
    return (r >= r0) & (r < r1)


def _brute_sq(src, tgt):
    a = torch.from_numpy(np.stack(np.nonzero(src), 1)).double()
    b = torch.from_numpy(np.stack(np.nonzero(tgt), 1)).double()
    return (torch.cdist(a, b) ** 2).min(1).values.round().long().numpy()


def test_referee_edt_matches_brute_force_on_random_volumes():
    g = np.random.default_rng(0)
    for shape in [(7, 9, 11), (12, 5, 8), (1, 9, 13), (6, 1, 1)]:
        for _ in range(3):
            src = g.random(shape) < 0.3
            tgt = g.random(shape) < 0.05
            if not src.any() or not tgt.any():
                continue
            assert np.array_equal(R.surface_sq(src, tgt), _brute_sq(src, tgt))


def _scipy_hd(p, gmask, percentile, directed):
    """MONAI 1.1 restated on scipy (binary_erosion + distance_transform_edt + np.percentile), rule 4 applied to empty sets."""
    nd = pytest.importorskip("scipy.ndimage")
    u = p | gmask
    if not u.any():
        return math.nan
    idx = np.nonzero(u)
    box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)
    pc, gc = np.squeeze(p[box]), np.squeeze(gmask[box])
    ep, eg = nd.binary_erosion(pc) ^ pc, nd.binary_erosion(gc) ^ gc

    def one(src, tgt):
        if not src.any() and not tgt.any():
            return math.nan
        if not src.any() or not tgt.any():
            return math.inf
        d = nd.distance_transform_edt(~tgt)[src]
        return float(d.max()) if not percentile else float(np.percentile(d, percentile))
    d1 = one(ep, eg)
    return d1 if directed else max(d1, one(eg, ep))


def _cases():
    s = (14, 15, 16)
    g = np.random.default_rng(1)
    shell_a = _shell(s, (7, 7, 8), 3, 6)
    shell_b = _shell(s, (6.5, 8, 7.5), 2.5, 5.5)
    noisy = shell_b ^ (g.random(s) < 0.03)
    plate = np.zeros(s, bool)
    plate[5, 4:7, 6:9] = True
    plate_g = np.zeros(s, bool)
    plate_g[5, 5, 7] = True
    line = np.zeros(s, bool)
    line[3, 2, 4:12] = True
    line_g = np.zeros(s, bool)
    line_g[3, 2, 6:9] = True
    one = np.zeros(s, bool)
    one[4, 4, 4] = True
    two = np.zeros(s, bool)
    two[9, 10, 3] = True
    border = np.zeros(s, bool)
    border[:, :6, :5] = True
    border_g = np.zeros(s, bool)
    border_g[:7, :4, :] = True
    empty = np.zeros(s, bool)
    return {"shells": (shell_a, noisy), "plate": (plate, plate_g), "line": (line, line_g), "voxel_same": (one, one),
            "voxel_pair": (one, two), "border": (border, border_g), "pred_empty": (empty, shell_a),
            "gt_empty": (shell_b, empty), "both_empty": (empty, empty), "voxel_vs_shell": (one, shell_a)}


@pytest.mark.parametrize("name", sorted(_cases()))
@pytest.mark.parametrize("percentile", [None, 0, 50, 95, 100])
@pytest.mark.parametrize("directed", [False, True])
def test_referee_matches_scipy(name, percentile, directed):
    p, gm = _cases()[name]
    ref = R.PairDistances(p[None, None], gm[None, None]).hd(include_background=True, percentile=percentile, directed=directed)
    want = _scipy_hd(p, gm, percentile, directed)
    got = float(ref[0, 0])
    if math.isnan(want):
        assert math.isnan(got)
    else:
        assert got == np.float32(want), (got, want)


def test_referee_squeeze_quirk():
    """A 1x3x3 plate: 9 edge voxels in 3-D, 8 once squeezed to 2-D (the centre is interior); a single voxel has no edge."""
    p = np.zeros((4, 5, 5), bool)
    p[2, 1:4, 1:4] = True
    ep, _ = R.mask_edges(p, p)
    assert ep.shape == (3, 3) and int(ep.sum()) == 8
    one = np.zeros((4, 5, 5), bool)
    one[1, 1, 1] = True
    e1, e2 = R.mask_edges(one, one)
    assert e1.ndim == 0 and not e1.any() and not e2.any()


def test_referee_iou_rules():
    lab_p = torch.tensor([[[[0, 1, 1], [2, 2, 255]]]], dtype=torch.uint8)
    lab_g = torch.tensor([[[[0, 1, 0], [2, 255, 255]]]], dtype=torch.uint8)
    iou = R.mean_iou(lab_p, lab_g, num_classes=4, include_background=True)
    assert iou[0, 0] == np.float32(0.5) and iou[0, 1] == np.float32(0.5) and iou[0, 2] == np.float32(0.5)
    assert math.isnan(float(iou[0, 3]))
    assert float(R.mean_iou(lab_p, lab_g, num_classes=4, include_background=True, ignore_empty=False)[0, 3]) == 1.0


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_workspace_queries_are_pure_and_validate():
    from micformer_amd.metrics import lib
    a = lib.micf_surface_metrics_workspace(1, 8, 128, 128, 128)
    assert a == lib.micf_surface_metrics_workspace(1, 8, 128, 128, 128) and a > 2 * 8 * 128 ** 3 * 4
    assert lib.micf_surface_metrics_workspace(2, 8, 128, 128, 128) > a
    assert lib.micf_surface_metrics_workspace(0, 8, 8, 8, 8) == -1
    assert lib.micf_surface_metrics_workspace(1, 33, 8, 8, 8) == -2
    assert lib.micf_surface_metrics_workspace(1, 8, 8, 8, 2048) == -2
    assert lib.micf_mean_iou_workspace(2, 8, 8, 8, 8) >= 2 * 8 * 3 * 8
    assert lib.micf_mean_iou_workspace(1, 33, 8, 8, 8) == -2


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd.metrics import lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20                         # never dereferenced: every call below fails validation first
    ws = lib.micf_surface_metrics_workspace(1, 8, 8, 8, 8)
    hd = lib.micf_hausdorff_distance
    ok = (fake, fake, 0, 1, 8, 8, 8, 8, 1, 95.0, 0, fake, ws, fake, None)
    assert hd(None, *ok[1:]) == EINVAL
    assert hd(*ok[:1], None, *ok[2:]) == EINVAL
    assert hd(*ok[:11], None, *ok[12:]) == EINVAL                    # workspace
    assert hd(*ok[:13], None, None) == EINVAL                        # out
    assert hd(*ok[:2], 2, *ok[3:]) == EINVAL                         # form flag
    assert hd(*ok[:4], 33, *ok[5:]) == EUNSUP                        # K > 32
    assert hd(*ok[:9], 101.0, *ok[10:]) == EINVAL                    # percentile
    assert hd(*ok[:9], -1.0, *ok[10:]) == EINVAL
    assert hd(*ok[:9], float("nan"), *ok[10:]) == EINVAL
    assert hd(*ok[:8], 8, *ok[9:]) == EINVAL                         # first_class >= K
    assert hd(*ok[:12], ws - 1, *ok[13:]) == EINVAL                  # workspace too small
    iou = lib.micf_mean_iou
    ok = (fake, fake, 1, 1, 8, 8, 8, 8, 1, 1, fake, 4096, fake, None)
    assert iou(None, *ok[1:]) == EINVAL
    assert iou(*ok[:2], 7, *ok[3:]) == EINVAL
    assert iou(*ok[:4], 40, *ok[5:]) == EUNSUP
    assert iou(*ok[:10], None, *ok[11:]) == EINVAL


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import metrics
    x = torch.zeros(1, 8, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError):
        metrics.hausdorff_distance(x, x, num_classes=4, distance_metric="chessboard")
    with pytest.raises(ValueError):
        metrics.hausdorff_distance(x, x, num_classes=4, percentile=120)
    with pytest.raises(ValueError):
        metrics.mean_iou(x, x, num_classes=4)                         # CPU tensors
    with pytest.raises(ValueError):
        metrics.HausdorffDistanceMetric(distance_metric="taxicab")
