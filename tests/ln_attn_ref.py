"""Float64 referee of the fp32 per-op kernels csrc/layernorm.hip and csrc/window_attn.hip: plain torch, no kernel, no oracle import.

LayerNorm over the channel dim of token rows (rows = cat[x1 | x2] when x2 is given), forward and the written-out backward;
window attention on a channels-last [T, C] token grid, forward and the written-out backward.  Windows are found by index
arithmetic (window_tokens), in-window order (wd, wh, ww) row-major; q / k / v may be views with any leading dimension (columns
of a packed [T, 3C] matrix, a [T, C + 1] buffer, ...): everything is converted to float64 first, so the view's strides are
torch's business.  tests/test_ln_attn_ref_cpu.py holds this file to F.layer_norm, float64 autograd and the fp32 oracle.
"""
import torch


def f64(t):
    """float64 CPU copy (a float64 CPU tensor passes through with its autograd history: the CPU test differentiates the forward)."""
    if t is None or (t.dtype == torch.float64 and not t.is_cuda):
        return t
    return t.detach().cpu().double()


# ----------------------------------------------------------------------------- LayerNorm
def ln_rows(x1, x2=None):
    return f64(x1) if x2 is None else torch.cat([f64(x1), f64(x2)], 1)


def ln_fwd(x1, gamma, beta, eps, x2=None):
    """-> y [rows, C], mean [rows], rstd [rows] (biased variance, as nn.LayerNorm)."""
    x = ln_rows(x1, x2)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * f64(gamma) + f64(beta)
    return y, mean, rstd


def ln_bwd(dy, x1, gamma, eps, x2=None, add=None):
    """-> dx [rows, C] (+ add), dgamma [C], dbeta [C].  With xh = (x - mean) rstd and gd = gamma dy:
    dx = rstd (gd - mean_c(gd) - xh mean_c(gd xh)), dgamma = sum_rows dy xh, dbeta = sum_rows dy."""
    x, dy, g = ln_rows(x1, x2), f64(dy), f64(gamma)
    _, mean, rstd = ln_fwd(x, torch.ones_like(g), torch.zeros_like(g), eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = g * dy
    a = gd.mean(1, keepdim=True)
    b = (gd * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (gd - a - xh * b)
    if add is not None:
        dx = dx + f64(add)
    return dx, (dy * xh).sum(0), dy.sum(0)


# ----------------------------------------------------------------------------- window attention
def window_tokens(dims, ws):
    """[nwin, N] token indices: window (b, xd, xh, xw) row-major, in-window token (id, ih, iw) row-major, token index
    ((b D + d) H + h) W + w of the channels-last grid."""
    B, D, H, W = dims
    wd, wh, ww = ws
    assert D % wd == 0 and H % wh == 0 and W % ww == 0
    rows = []
    for b in range(B):
        for xd in range(D // wd):
            for xh in range(H // wh):
                for xw in range(W // ww):
                    rows.append([((b * D + xd * wd + i) * H + xh * wh + j) * W + xw * ww + k
                                 for i in range(wd) for j in range(wh) for k in range(ww)])
    return torch.tensor(rows, dtype=torch.long)


def _heads(t, idx, heads):
    """[T, C] -> [nwin, heads, N, hd]."""
    nwin, N = idx.shape
    return f64(t)[idx].reshape(nwin, N, heads, -1).transpose(1, 2)


def _tokens(tw, idx, T):
    """[nwin, heads, N, hd] -> [T, C]."""
    nwin, N = idx.shape
    out = torch.zeros(T, tw.shape[1] * tw.shape[3], dtype=torch.float64)
    out[idx.reshape(-1)] = tw.transpose(1, 2).reshape(nwin * N, -1)
    return out


def attn_probs(q, k, dims, heads, ws, scale):
    """-> (scores, P) [nwin, heads, N, N] with scores = (q scale) k^T, P = softmax over the key index."""
    idx = window_tokens(dims, ws)
    s = (_heads(q, idx, heads) * scale) @ _heads(k, idx, heads).transpose(-1, -2)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return s, e / e.sum(-1, keepdim=True)


def attn_fwd(q, k, v, dims, heads, ws, scale):
    """o [T, C] = per head and window softmax((q scale) k^T) v."""
    idx = window_tokens(dims, ws)
    _, p = attn_probs(q, k, dims, heads, ws, scale)
    return _tokens(p @ _heads(v, idx, heads), idx, q.shape[0])


def attn_bwd(q, k, v, d_o, dims, heads, ws, scale):
    """-> dq, dk, dv [T, C]: dP = do v^T, dS = P (dP - sum_j P dP), dq = scale dS k, dk = scale dS^T q, dv = P^T do."""
    idx = window_tokens(dims, ws)
    T = q.shape[0]
    qw, kw, vw, dow = (_heads(t, idx, heads) for t in (q, k, v, d_o))
    _, p = attn_probs(q, k, dims, heads, ws, scale)
    dp = dow @ vw.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return (_tokens(scale * (ds @ kw), idx, T), _tokens(scale * (ds.transpose(-1, -2) @ qw), idx, T),
            _tokens(p.transpose(-1, -2) @ dow, idx, T))


# ----------------------------------------------------------------------------- seeded inputs shared by the CPU and the GPU tests
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape) * 7919)
    return (torch.randn(*shape, generator=g) * scale).float()


def attn_inputs(dims, C, seed=0):
    """q [T, C], kv [T, 2C], do [T, C] (fp32)."""
    T = dims[0] * dims[1] * dims[2] * dims[3]
    return rnd(T, C, seed=seed + 1), rnd(T, 2 * C, seed=seed + 2), rnd(T, C, seed=seed + 3)


LARGE_SCORE_CASES = [((2, 2, 4, 6), 48, 3, (2, 2, 2)), ((2, 2, 4, 6), 192, 24, (2, 2, 2))]     # (dims, C, heads, window)


def large_score_inputs(dims, C, heads, ws, peak=60.0):
    """attn_inputs with q and k both scaled by one factor so that the largest |score| is `peak`: softmax rows close to one-hot,
    expf(s - max) down to e^-120."""
    q, kv, do = attn_inputs(dims, C, seed=40)
    s, _ = attn_probs(q, kv[:, :C], dims, heads, ws, (C // heads) ** -0.5)
    f = float((peak / s.abs().max()) ** 0.5)
    kv = kv.clone()
    kv[:, :C] *= f
    return q * f, kv, do


def fp32_errors(ref32, q, kv, do, dims, heads, ws):
    """Max abs error of an fp32 implementation `ref32(q, kv, dims, heads, ws) -> o` (and of its autograd gradients) against this
    file: {"o", "dq", "dkv"} -> float.  The yardstick of the large-score case: it never sees a kernel's output."""
    C = q.shape[1]
    scale = (C // heads) ** -0.5
    qr, kvr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o = ref32(qr, kvr, dims, heads, ws)
    gq, gkv = torch.autograd.grad((o * do).sum(), [qr, kvr])
    want_o = attn_fwd(q, kv[:, :C], kv[:, C:], dims, heads, ws, scale)
    dq, dk, dv = attn_bwd(q, kv[:, :C], kv[:, C:], do, dims, heads, ws, scale)
    err = lambda a, b: float((a.detach().double() - b).abs().max())
    return {"o": err(o, want_o), "dq": err(gq, dq), "dkv": err(gkv, torch.cat([dk, dv], 1))}
