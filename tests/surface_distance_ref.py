"""Referee of micformer_amd.surface (not collected): the surface distances of DESIGN.md "Surface distances in millimetres" on
the CPU.  Edges are those of surface_metrics_ref (MONAI's get_mask_edges); the distance of a source edge voxel is the minimum
over ALL target edge voxels of ((s_z dz)^2 + (s_y dy)^2) + (s_x dx)^2 in float64, in that order -- brute force, so the minimum
is exact by construction.  Percentiles by np.percentile, means by np.mean.  Needs numpy and torch only; scipy_d2 (the cross-check
against scipy.ndimage.distance_transform_edt) needs scipy."""
import math

import numpy as np
import torch

import surface_metrics_ref as M

PAIR_BUDGET = 1 << 22          # (source, target) pairs evaluated at once


def label_memberships(y, label_values):
    """int16 / int32 label volumes [B, D, H, W] -> bool [B, K, D, H, W]: class k >= 1 where the value is label_values[k - 1],
    class 0 everywhere else."""
    lab = y.cpu().numpy()
    planes = [lab == v for v in label_values]
    return np.stack([~np.any(planes, axis=0)] + planes, axis=1)


def edge_points(p, g):
    """Edge voxels of both masks, as integer coordinates [n, 3] inside the union box (MONAI squeezes one-voxel-thick axes away
    before eroding; along those every coordinate is 0, so the squeezed edges reshape back without loss)."""
    u = p | g
    if not u.any():
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in np.nonzero(u))
    shape = p[box].shape
    ep, eg = M.mask_edges(p, g)
    return np.argwhere(ep.reshape(shape)), np.argwhere(eg.reshape(shape))


def brute_d2(src, tgt, spacing):
    """float64 [n]: min over tgt of ((s_z dz)^2 + (s_y dy)^2) + (s_x dx)^2 for every row of src."""
    s = [float(v) for v in spacing]
    a, b = torch.from_numpy(src).double(), torch.from_numpy(tgt).double()
    out = torch.empty(len(a), dtype=torch.float64)
    step = max(1, PAIR_BUDGET // max(len(b), 1))
    for i in range(0, len(a), step):
        d = a[i:i + step, None, :] - b[None, :, :]
        z, y, x = s[0] * d[..., 0], s[1] * d[..., 1], s[2] * d[..., 2]
        out[i:i + step] = ((z * z + y * y) + x * x).min(dim=1).values
    return out.numpy()


def scipy_d2(src, tgt, spacing):
    """The same through scipy.ndimage.distance_transform_edt(sampling=spacing) (squared; scipy takes the root last)."""
    from scipy import ndimage
    pts = np.concatenate([src, tgt])
    shape = tuple(int(v) + 1 for v in pts.max(axis=0))
    mask = np.ones(shape, bool)
    mask[tuple(tgt.T)] = False
    _, idx = ndimage.distance_transform_edt(mask, sampling=spacing, return_indices=True, return_distances=True)
    near = idx[(slice(None),) + tuple(src.T)].T                     # nearest target of every source voxel
    return brute_d2_pairs(src, near, spacing)


def brute_d2_pairs(src, tgt, spacing):
    d = (src - tgt).astype(np.float64)
    z, y, x = spacing[0] * d[:, 0], spacing[1] * d[:, 1], spacing[2] * d[:, 2]
    return (z * z + y * y) + x * x


def voxel_nearest_d2(src, tgt, spacing):
    """A WRONG implementation: the nearest neighbour in voxel units, its distance scaled afterwards."""
    near = np.empty_like(src)
    b = tgt.astype(np.float64)
    for i, pnt in enumerate(src.astype(np.float64)):
        near[i] = tgt[np.argmin(((b - pnt) ** 2).sum(axis=1))]
    return brute_d2_pairs(src, near, spacing)


class SurfaceReferee:
    """Both directions' distances of every (b, c), computed once; scored for any percentile / threshold.  pm, gm: bool
    [B, K, D, H, W]; spacing: one triple per sample."""

    def __init__(self, pm, gm, spacing, d2_fn=brute_d2):
        self.B, self.K = pm.shape[:2]
        self.pm, self.gm, self.spacing, self.d2_fn = pm, gm, spacing, d2_fn
        self._rec = {}

    def rec(self, b, c):
        """(pred edge count, gt edge count, (distances pred -> gt, gt -> pred) or (None, None)); computed when first asked for."""
        if (b, c) not in self._rec:
            ep, eg = edge_points(self.pm[b, c], self.gm[b, c])
            if len(ep) and len(eg):
                d = (np.sqrt(self.d2_fn(ep, eg, self.spacing[b])), np.sqrt(self.d2_fn(eg, ep, self.spacing[b])))
            else:
                d = (None, None)
            self._rec[b, c] = (len(ep), len(eg), d)
        return self._rec[b, c]

    def _table(self, first, width, fn):
        out = torch.empty((self.B, self.K - first, width), dtype=torch.float64)
        for b in range(self.B):
            for c in range(first, self.K):
                out[b, c - first] = torch.tensor(fn(*self.rec(b, c)), dtype=torch.float64)
        return out.float()

    @staticmethod
    def _pct(d, percentile):
        return float(d.max()) if not percentile else float(np.percentile(d, percentile))

    def hd(self, percentiles, include_background=False, directed=False):
        def fn(n_p, n_g, d):
            if n_p == 0 and n_g == 0:
                return [math.nan] * len(percentiles)
            if n_p == 0 or n_g == 0:
                return [math.inf] * len(percentiles)
            return [self._pct(d[0], p) if directed else max(self._pct(d[0], p), self._pct(d[1], p)) for p in percentiles]
        return self._table(0 if include_background else 1, len(percentiles), fn)

    def asd(self, include_background=False):
        def fn(n_p, n_g, d):
            n = (n_p, n_g)
            return [math.nan if n[k] == 0 else (math.inf if n[1 - k] == 0 else float(np.mean(d[k]))) for k in range(2)]
        return self._table(0 if include_background else 1, 2, fn)

    def assd(self, include_background=False, wrong=None):
        def fn(n_p, n_g, d):
            if n_p == 0 and n_g == 0:
                return [math.nan]
            if n_p == 0 or n_g == 0:
                return [math.inf]
            if wrong == "mean_of_means":
                return [(float(np.mean(d[0])) + float(np.mean(d[1]))) / 2]
            return [float(np.mean(np.concatenate(d)))]
        return self._table(0 if include_background else 1, 1, fn)[..., 0]

    def nsd(self, thresholds, include_background=False, wrong=None):
        first = 0 if include_background else 1
        out = torch.empty((self.B, self.K - first), dtype=torch.float64)
        for b in range(self.B):
            for c in range(first, self.K):
                n_p, n_g, d = self.rec(b, c)
                tau = float(thresholds[c - first])
                if n_p == 0 and n_g == 0:
                    out[b, c - first] = math.nan
                elif n_p == 0 or n_g == 0:
                    out[b, c - first] = 0.0
                else:
                    within = sum(int((x < tau).sum() if wrong == "strict" else (x <= tau).sum()) for x in d)
                    out[b, c - first] = within / (n_p + n_g)
        return out.float()

    def ties(self, thresholds, b, include_background=False, rel=1e-9):
        """Of sample b: (distances equal to their class's tolerance, distances within rel * tau of it but not equal)."""
        first = 0 if include_background else 1
        equal = near = 0
        for c in range(first, self.K):
            n_p, n_g, d = self.rec(b, c)
            if d[0] is None:
                continue
            tau = float(thresholds[c - first])
            for x in d:
                equal += int((x == tau).sum())
                near += int(((np.abs(x - tau) <= rel * tau) & (x != tau)).sum())
        return equal, near
