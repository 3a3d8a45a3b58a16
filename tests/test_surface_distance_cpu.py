"""CPU checks of the surface distances in physical units: the C-ABI of include/micformer_surface.h (header, ctypes table, bound
function objects, exported symbols, table disjoint from the others), argument errors caught before any launch, the Python
front end's checks, and the referee itself (tests/surface_distance_ref.py): brute force against scipy, and three wrong
implementations it must tell apart from the right one."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import abi_header
import surface_distance_ref as R
import surface_metrics_ref as M
import test_abi

HEADER = "micformer_surface.h"
EINVAL, EUNSUP = -1, -2


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, surface
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(surface.SIGNATURES) == {"micf_surface_distance_workspace", "micf_surface_distance"}
    assert surface.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert surface.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {surface.SIGNATURES[name]}"
        assert (name in surface.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert set(surface.INT64_RETURNS) <= set(d)
    consts = abi_header.defines(HEADER, "MICF_")
    assert consts["MICF_FORM_VALUES_I16"] == surface.FORM_VALUES_I16 and consts["MICF_FORM_VALUES_I32"] == surface.FORM_VALUES_I32
    assert consts["MICF_SURFACE_MAX_PERCENTILES"] == surface.MAX_PERCENTILES
    assert abi_header.defines("micformer_metrics.h", "MICF_FORM_") == {"MICF_FORM_LABEL": 0, "MICF_FORM_ONEHOT": 1}


def test_table_is_disjoint_from_every_other():
    from micformer_amd import surface
    for _, module, _ in test_abi.TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(other) & set(surface.SIGNATURES), module


def test_workspace_query_is_pure_and_validates():
    from micformer_amd import surface
    q = surface.lib.micf_surface_distance_workspace
    a = q(1, 8, 128, 128, 128)
    assert a == q(1, 8, 128, 128, 128) and 2 * 8 * 128 ** 3 * 4 < a < (8 * 8 + 24) * 128 ** 3
    assert q(2, 8, 128, 128, 128) > a
    assert q(0, 8, 8, 8, 8) == EINVAL and q(1, 8, 8, 0, 8) == EINVAL
    assert q(1, 33, 8, 8, 8) == EUNSUP and q(1, 8, 8, 8, 1025) == EUNSUP and q(1, 8, 513, 513, 8) == EUNSUP
    assert q(1, 8, 1024, 512, 8) > 0 and q(1, 8, 512, 1024, 8) > 0
    assert surface.workspace_bytes((2, 9, 12, 70), 4) == q(2, 4, 9, 12, 70) == surface.workspace_bytes((2, 4, 9, 12, 70), 4)
    with pytest.raises(_micf_error()):
        surface.workspace_bytes((1, 8, 8, 2048), 4)


def _micf_error():
    from micformer_amd import _lib
    return _lib.MicfError


def _doubles(*v):
    return (ctypes.c_double * len(v))(*v)


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd import surface
    lib = surface.lib
    fake = 1 << 20                         # never dereferenced: every call below fails validation first
    ws = lib.micf_surface_distance_workspace(1, 8, 8, 8, 8)
    addr = ctypes.addressof
    sp, pct, tau = _doubles(1.0, 0.5, 0.5), _doubles(95.0), _doubles(*[1.0] * 7)
    vals = (ctypes.c_int32 * 7)(205, 420, 500, 550, 600, 820, 850)

    def call(pred=fake, gt=fake, form=0, B=1, K=8, D=8, H=8, W=8, first=1, lv=None, nlv=0, spacing=sp, percentiles=pct, npct=1,
             thresholds=tau, workspace=fake, nbytes=ws, out=fake):
        ptr = lambda a: a if a is None or isinstance(a, int) else addr(a)          # noqa: E731
        return lib.micf_surface_distance(pred, gt, form, B, K, D, H, W, first, ptr(lv), nlv, ptr(spacing), ptr(percentiles), npct,
                                         ptr(thresholds), workspace, nbytes, out, None)

    for null in ("pred", "gt", "spacing", "percentiles", "workspace", "out"):
        assert call(**{null: None}) == EINVAL, null
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for axis in range(3):
            s = [1.0, 0.5, 0.5]
            s[axis] = bad
            assert call(spacing=_doubles(*s)) == EINVAL, (bad, axis)
    assert call(percentiles=_doubles(101.0)) == EINVAL and call(percentiles=_doubles(-1.0)) == EINVAL
    assert call(percentiles=_doubles(float("nan"))) == EINVAL
    assert call(percentiles=_doubles(5.0, 50.0, 95.0, 99.0, 100.0), npct=5) == EINVAL and call(npct=0) == EINVAL
    assert call(thresholds=_doubles(*([1.0] * 6 + [-0.5]))) == EINVAL
    assert call(thresholds=_doubles(*([float("nan")] + [1.0] * 6))) == EINVAL
    assert call(form=4) == EINVAL and call(form=-1) == EINVAL
    assert call(first=8) == EINVAL and call(first=-1) == EINVAL
    assert call(B=0) == EINVAL
    assert call(W=1025, nbytes=1 << 40) == EUNSUP                   # an extent past 1024
    assert call(D=513, H=513, nbytes=1 << 40) == EUNSUP             # min(D, H) past 512
    assert call(K=33, thresholds=_doubles(*[1.0] * 32)) == EUNSUP
    assert call(B=65, spacing=_doubles(*[1.0] * 195), nbytes=1 << 40) == EUNSUP
    assert call(spacing=_doubles(1.0, 1e-100, 1.0)) == EUNSUP       # a spacing past 2^+-256
    assert call(nbytes=ws - 1) == EINVAL                            # a short workspace
    assert call(workspace=fake + 8) == EINVAL                       # a misaligned one
    # label values: exactly K - 1, distinct, non-zero, within the volume's dtype; none for the two class-map forms
    assert call(lv=vals, nlv=7) == EINVAL
    assert call(form=2) == EINVAL and call(form=2, lv=vals, nlv=6) == EINVAL
    assert call(form=2, lv=(ctypes.c_int32 * 7)(205, 420, 500, 550, 600, 820, 0), nlv=7) == EINVAL
    assert call(form=2, lv=(ctypes.c_int32 * 7)(205, 420, 500, 550, 600, 820, 205), nlv=7) == EINVAL
    assert call(form=2, lv=(ctypes.c_int32 * 7)(205, 420, 500, 550, 600, 820, 40000), nlv=7) == EINVAL
    # (valid arguments are not tried here: they would launch)


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import surface
    x = torch.zeros(2, 8, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA"):
        surface.surface_distances(x, x, num_classes=4)                                  # CPU tensors
    with pytest.raises(ValueError, match="same shape"):
        surface.surface_distances(x, x[:, :7], num_classes=4)
    with pytest.raises(TypeError, match="uint8 class map or an int16 / int32 label volume"):
        surface.surface_distances(x.float(), x.float(), num_classes=4)                  # a float class map
    with pytest.raises(TypeError):
        surface.surface_distances(x.short(), x.int())
    with pytest.raises(ValueError, match="num_classes"):
        surface.surface_distances(x, x)
    for spacing in ((1.0, 1.0), [(1.0, 1.0, 1.0)] * 3, (1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (1.0, float("inf"), 1.0), "mm"):
        with pytest.raises(ValueError, match="spacing"):
            surface.surface_distances(x, x, num_classes=4, spacing=spacing)
    with pytest.raises(ValueError, match="class_thresholds"):
        surface.surface_distances(x, x, num_classes=4, thresholds=[1.0, 1.0])
    with pytest.raises(ValueError, match="class_thresholds"):
        surface.surface_dice(x, x, [1.0] * 4, num_classes=4)                            # 3 scored classes
    with pytest.raises(ValueError, match=">= 0"):
        surface.surface_distances(x, x, num_classes=4, thresholds=[1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="percentile"):
        surface.surface_distances(x, x, num_classes=4, percentiles=(101,))
    with pytest.raises(ValueError, match="percentiles"):
        surface.surface_distances(x, x, num_classes=4, percentiles=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="label_values"):
        surface.surface_distances(x.short(), x.short(), label_values=(1, 1, 2))
    with pytest.raises(ValueError, match="label_values"):
        surface.surface_distances(x.short(), x.short(), label_values=(1, 70000))
    with pytest.raises(ValueError, match="euclidean"):
        surface.SurfaceDistanceMetric(distance_metric="chessboard")
    with pytest.raises(ValueError, match="euclidean"):
        surface.SurfaceDiceMetric([1.0], distance_metric="taxicab")


# ---- the referee ------------------------------------------------------------------------------------------------------------

SHAPE, K = (9, 12, 70), 4
EXACT = (3.0, 0.5, 1.25)
SPACINGS = [(0.6, 0.35, 0.35), (1.6, 0.43, 0.43), EXACT]


def _fixture():
    from oracle import fill
    gt = fill.make_label_map(1, *SHAPE, num_classes=K).to(torch.uint8)
    pred = torch.zeros_like(gt)
    pred[:, 1:, :-1, 2:] = gt[:, :-1, 1:, :-2]                      # shifted by (1, -1, 2)
    return M.memberships(pred, K), M.memberships(gt, K)


@pytest.mark.parametrize("spacing", SPACINGS)
def test_referee_brute_force_equals_scipy(spacing):
    pytest.importorskip("scipy.ndimage")
    pm, gm = _fixture()
    for c in range(1, K):
        ep, eg = R.edge_points(pm[0, c], gm[0, c])
        assert len(ep) and len(eg)
        assert np.array_equal(R.brute_d2(ep, eg, spacing), R.scipy_d2(ep, eg, spacing))
        assert np.array_equal(R.brute_d2(eg, ep, spacing), R.scipy_d2(eg, ep, spacing))


def test_referee_at_unit_spacing_is_the_voxel_unit_referee():
    pm, gm = _fixture()
    ref, old = R.SurfaceReferee(pm, gm, [(1.0, 1.0, 1.0)]), M.PairDistances(pm, gm)
    for pct in (None, 5, 50, 95, 100):
        for directed in (False, True):
            assert torch.equal(ref.hd((pct,), directed=directed)[..., 0], old.hd(False, pct, directed))


def test_referee_rejects_the_voxel_nearest_neighbour_scaled_afterwards():
    pm, gm = _fixture()
    right = R.SurfaceReferee(pm, gm, [EXACT])
    wrong = R.SurfaceReferee(pm, gm, [EXACT], d2_fn=R.voxel_nearest_d2)
    asd_r, asd_w = float(right.asd()[0, 0, 0]), float(wrong.asd()[0, 0, 0])
    hd_r, hd_w = float(right.hd((95,), directed=True)[0, 0, 0]), float(wrong.hd((95,), directed=True)[0, 0, 0])
    print(asd_r, asd_w, hd_r, hd_w)
    assert asd_w > 1.1 * asd_r and hd_w > 1.1 * hd_r                # (class 1 here: ASD 1.19 against 0.50, HD95 3.04 against 2.00)


def test_referee_rejects_strict_comparison_at_a_tie():
    pm, gm = _fixture()
    ref, tau = R.SurfaceReferee(pm, gm, [EXACT]), [0.5, 1.0, 2.0]
    equal, near = ref.ties(tau, 0)
    assert equal > 0 and near == 0
    assert (ref.nsd(tau, wrong="strict") < ref.nsd(tau)).any()
    free = R.SurfaceReferee(pm, gm, [SPACINGS[0]])
    assert free.ties(tau, 0) == (0, 0) and torch.equal(free.nsd(tau, wrong="strict"), free.nsd(tau))


def test_referee_rejects_the_mean_of_the_two_directed_means():
    g = np.zeros((1, 2, 12, 12, 12), bool)
    p = np.zeros_like(g)
    g[0, 1, 2:10, 2:10, 2:10] = True                                # a large cube against a small one: unequal edge counts
    p[0, 1, 4:7, 4:7, 4:7] = True
    ref = R.SurfaceReferee(p, g, [EXACT])
    n_p, n_g, d = ref.rec(0, 1)
    assert n_p != n_g
    pooled = float(ref.assd()[0, 0])
    assert pooled == np.float32((d[0].sum() + d[1].sum()) / (n_p + n_g))
    assert abs(float(ref.assd(wrong="mean_of_means")[0, 0]) - pooled) > 1e-3 * pooled


def test_referee_empty_set_rules_and_label_values():
    p = np.zeros((1, 3, 6, 6, 6), bool)
    g = np.zeros_like(p)
    p[0, 0, 1:4, 1:4, 1:4] = True                                   # class 0: empty in gt; class 1: empty in pred; class 2: in both
    g[0, 1, 1:4, 1:4, 1:4] = True
    ref = R.SurfaceReferee(p, g, [EXACT])
    hd, asd, assd, nsd = ref.hd((95,), True), ref.asd(True), ref.assd(True), ref.nsd([1.0] * 3, True)
    assert math.isinf(float(hd[0, 0, 0])) and math.isinf(float(hd[0, 1, 0])) and math.isnan(float(hd[0, 2, 0]))
    assert math.isinf(float(asd[0, 0, 0])) and math.isnan(float(asd[0, 0, 1]))
    assert math.isnan(float(asd[0, 1, 0])) and math.isinf(float(asd[0, 1, 1])) and torch.isnan(asd[0, 2]).all()
    assert math.isinf(float(assd[0, 0])) and math.isnan(float(assd[0, 2]))
    assert float(nsd[0, 0]) == 0.0 and float(nsd[0, 1]) == 0.0 and math.isnan(float(nsd[0, 2]))
    lab = torch.tensor([[[[0, 205, 420], [421, -3, 205]]]], dtype=torch.int16)
    m = R.label_memberships(lab, (205, 420))
    assert m.shape == (1, 3, 1, 2, 3) and m[0, 1].sum() == 2 and m[0, 2].sum() == 1 and m[0, 0].sum() == 3
