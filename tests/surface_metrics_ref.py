"""Referee of micformer_amd.metrics (not collected): a numpy / torch-CPU restatement of MONAI 1.1's get_mask_edges,
get_surface_distance, compute_hausdorff_distance and compute_iou (rules 1-6 of DESIGN.md "Surface metrics").  Edges by slicing,
an exact squared EDT by a per-axis loop of vectorised minima, both cropped to the class's union box as MONAI does.  Needs
nothing beyond numpy and torch."""
import math

import numpy as np
import torch

INF = 1 << 40


def memberships(y, num_classes=None):
    """uint8 class map [B, D, H, W] (+ num_classes) or one-hot planes [B, K, D, H, W] -> bool numpy [B, K, D, H, W]."""
    y = y.cpu()
    if y.dim() == 4:
        lab = y.numpy()
        return np.stack([lab == c for c in range(num_classes)], axis=1)
    return (y.float() == 1.0).numpy()


def erode(m):
    """scipy.ndimage.binary_erosion(m) with the cross structure of m's rank and border_value 0; a 0-d array erodes to itself."""
    if m.ndim == 0:
        return m.copy()
    out = m.copy()
    for ax in range(m.ndim):
        n = m.shape[ax]

        def sl(a, b):
            return tuple(slice(a, b) if i == ax else slice(None) for i in range(m.ndim))
        prev = np.zeros_like(m)
        nxt = np.zeros_like(m)
        prev[sl(1, None)] = m[sl(0, n - 1)]
        nxt[sl(0, n - 1)] = m[sl(1, None)]
        out &= prev & nxt
    return out


def mask_edges(p, g):
    """get_mask_edges(p, g): edges of both masks inside their union box, squeezed as MONAI squeezes."""
    u = p | g
    if not u.any():
        return np.zeros((0,), bool), np.zeros((0,), bool)
    idx = np.nonzero(u)
    box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in idx)
    pc, gc = np.squeeze(p[box]), np.squeeze(g[box])
    return erode(pc) ^ pc, erode(gc) ^ gc


def sq_edt(t):
    """Exact squared Euclidean distance (int64) of every element of t's array to the nearest True of t (INF if none)."""
    f = torch.where(torch.from_numpy(np.ascontiguousarray(t)), 0, INF).to(torch.int64)
    for ax in range(f.dim()):
        n = f.shape[ax]
        has = (f < INF).any(dim=ax, keepdim=True).expand_as(f)
        out = f.clone()
        for j in range(1, n):
            live = out[has]
            if live.numel() == 0 or j * j >= int(live.max()):
                break
            a = f.narrow(ax, 0, n - j) + j * j
            b = f.narrow(ax, j, n - j) + j * j
            o1 = out.narrow(ax, j, n - j)
            o1.copy_(torch.minimum(o1, a))
            o2 = out.narrow(ax, 0, n - j)
            o2.copy_(torch.minimum(o2, b))
        f = out
    return f.numpy()


def surface_sq(src, tgt):
    """Squared distances (int64, unsorted) from every src edge to the nearest tgt edge; None if either set is empty."""
    if not src.any() or not tgt.any():
        return None
    return sq_edt(tgt)[src]


def directed_from(sq, n_src, n_tgt, percentile):
    """Rule 4 from the squared distances of one direction."""
    if n_src == 0 and n_tgt == 0:
        return math.nan
    if n_src == 0 or n_tgt == 0:
        return math.inf
    d = np.sqrt(sq.astype(np.float64))
    if not percentile:
        return float(d.max())
    return float(np.percentile(d, percentile))


class PairDistances:
    """Both directions' squared distances of every (b, c): computed once, scored for any percentile / directed setting."""

    def __init__(self, pm, gm, sq_fn=None):
        sq_fn = sq_fn or surface_sq
        B, K = pm.shape[:2]
        self.B, self.K = B, K
        self.rec = {}
        for b in range(B):
            for c in range(K):
                ep, eg = mask_edges(pm[b, c], gm[b, c])
                n_p, n_g = int(ep.sum()), int(eg.sum())
                self.rec[b, c] = (n_p, n_g, sq_fn(ep, eg) if n_p and n_g else None, sq_fn(eg, ep) if n_p and n_g else None)

    def hd(self, include_background=False, percentile=None, directed=False):
        first = 0 if include_background else 1
        out = torch.empty((self.B, self.K - first), dtype=torch.float64)
        for b in range(self.B):
            for c in range(first, self.K):
                n_p, n_g, s0, s1 = self.rec[b, c]
                d1 = directed_from(s0, n_p, n_g, percentile)
                v = d1 if directed else max(d1, directed_from(s1, n_g, n_p, percentile))
                out[b, c - first] = v
        return out.float()


def hausdorff_distance(y_pred, y, num_classes=None, include_background=False, percentile=None, directed=False):
    pm, gm = memberships(y_pred, num_classes), memberships(y, num_classes)
    return PairDistances(pm, gm).hd(include_background, percentile, directed)


def mean_iou(y_pred, y, num_classes=None, include_background=False, ignore_empty=True):
    pm, gm = memberships(y_pred, num_classes), memberships(y, num_classes)
    first = 0 if include_background else 1
    pm, gm = pm[:, first:], gm[:, first:]
    ax = tuple(range(2, pm.ndim))
    inter = (pm & gm).sum(axis=ax).astype(np.int64)
    P, G = pm.sum(axis=ax).astype(np.int64), gm.sum(axis=ax).astype(np.int64)
    U = P + G - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        q = inter.astype(np.float64) / U.astype(np.float64)
    if ignore_empty:
        q = np.where(G > 0, q, np.nan)
    else:
        q = np.where(U > 0, q, 1.0)
    return torch.from_numpy(q).float()


def bounded_surface_sq(R):
    """surface_sq for large volumes: search the offsets in increasing squared length up to R; every src voxel must resolve."""
    offs = [(dz, dy, dx) for dz in range(-R, R + 1) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
            if dz * dz + dy * dy + dx * dx <= R * R]
    offs.sort(key=lambda o: o[0] ** 2 + o[1] ** 2 + o[2] ** 2)

    def fn(src, tgt):
        if src.ndim != 3:
            return surface_sq(src, tgt)
        pts = np.stack(np.nonzero(src), axis=1).astype(np.int64)
        res = np.full(len(pts), -1, np.int64)
        shape = np.array(src.shape)
        todo = np.arange(len(pts))
        for o in offs:
            if todo.size == 0:
                break
            q = pts[todo] + np.array(o)
            ok = np.all((q >= 0) & (q < shape), axis=1)
            hit = np.zeros(todo.size, bool)
            hit[ok] = tgt[q[ok, 0], q[ok, 1], q[ok, 2]]
            res[todo[hit]] = o[0] ** 2 + o[1] ** 2 + o[2] ** 2
            todo = todo[~hit]
        assert todo.size == 0, f"{todo.size} edge voxels farther than {R} from the other edge set"
        return res
    return fn
