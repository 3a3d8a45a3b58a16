"""tests/ln_attn_ref.py on the CPU: the float64 referee of test_gpu_ln_attn_arms.py states the right maps.  Its LayerNorm agrees
with R.layer_norm / F.layer_norm (forward, and the written-out backward with float64 autograd exactly and with fp32 autograd within
fp32 rounding); its window attention agrees with `_attn_ref` and R._to_windows of test_gpu_ops.py (the index arithmetic token for
token, outputs and gradients within fp32 rounding); q / k / v given as columns of one packed [T, 3C] matrix give the same bits as
contiguous copies.  The last test measures the yardstick of the large-score GPU case: the error of the fp32 CPU reference against
float64 on inputs whose scores reach +-60 (printed with -s; the GPU bound is 4 x that figure, so it never rests on a kernel).
"""
import pytest
import torch
import torch.nn.functional as F

import ln_attn_ref as L
import test_gpu_ops as G
from oracle import micformer_ref as R

FP32 = 1e-5          # "within fp32 rounding": 1e-5 of the tensor's max + 1e-6 (sums of <= 2048 terms of eps = 6e-8 each)


def near(got, want, what, rel=FP32):
    err = float((got.double() - want.double()).abs().max())
    scale = float(want.abs().max())
    assert err <= 1e-6 + rel * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("rows,C,c1", [(37, 6, 6), (33, 10, 6), (9, 96, 46), (70, 768, 384), (9, 2048, 2048)])
def test_layernorm_reference(rows, C, c1):
    x = L.rnd(rows, C, seed=1) * 2 + 0.3
    g, b = 1 + 0.1 * L.rnd(C, seed=2), 0.1 * L.rnd(C, seed=3)
    dy, add = L.rnd(rows, C, seed=4), L.rnd(rows, C, seed=5)
    x1, x2 = (x, None) if c1 == C else (x[:, :c1].contiguous(), x[:, c1:].contiguous())
    y, mean, rstd = L.ln_fwd(x1, g, b, 1e-5, x2)
    dx, dg, db = L.ln_bwd(dy, x1, g, 1e-5, x2, add=add)
    # float64 autograd of F.layer_norm: the written-out backward is the same map
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    y64 = F.layer_norm(xr, (C,), gr, br, 1e-5)
    gx, gg, gb = torch.autograd.grad((y64 * dy.double()).sum(), [xr, gr, br])
    for got, want, what in ((y, y64, "y"), (dx, gx + add.double(), "dx"), (dg, gg, "dgamma"), (db, gb, "dbeta")):
        near(got, want.detach(), what + " vs float64 autograd", rel=1e-12)
    near(mean, x.double().mean(1), "mean", rel=1e-12)
    near(rstd, 1 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5), "rstd", rel=1e-12)
    # the fp32 oracle the first-generation tests compare with
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
    y32 = R.layer_norm(xr, gr, br)
    assert torch.equal(y32, F.layer_norm(x, (C,), g, b, 1e-5))
    gx, gg, gb = torch.autograd.grad((y32 * dy).sum(), [xr, gr, br])
    for got, want, what in ((y32, y, "y"), (gx + add, dx, "dx"), (gg, dg, "dgamma"), (gb, db, "dbeta")):
        near(got.detach(), want, what + ": fp32 oracle vs the referee")


CASES = [((2, 4, 6, 4), 48, 3, (2, 2, 2)), ((1, 2, 2, 6), 48, 3, (1, 1, 3)), ((1, 7, 2, 3), 48, 3, (7, 1, 1)),
         ((1, 1, 6, 4), 48, 3, (1, 3, 2)), ((2, 2, 4, 6), 192, 24, (2, 2, 2)), ((1, 2, 4, 2), 15, 3, (2, 2, 2))]


@pytest.mark.parametrize("dims,C,heads,ws", CASES)
def test_window_index_arithmetic(dims, C, heads, ws):
    B, D, H, W = dims
    T = B * D * H * W
    ids = torch.arange(T, dtype=torch.float32).reshape(B, D, H, W, 1)
    idx = L.window_tokens(dims, ws)
    assert torch.equal(R._to_windows(ids, ws)[:, :, 0].long(), idx)
    assert torch.equal(idx.reshape(-1).sort().values, torch.arange(T))        # every token in exactly one window


@pytest.mark.parametrize("dims,C,heads,ws", CASES)
def test_window_attention_reference(dims, C, heads, ws):
    q, kv, do = L.attn_inputs(dims, C)
    scale = (C // heads) ** -0.5
    k, v = kv[:, :C], kv[:, C:]
    o = L.attn_fwd(q, k, v, dims, heads, ws, scale)
    dq, dk, dv = L.attn_bwd(q, k, v, do, dims, heads, ws, scale)
    # float64 autograd through the forward: the written-out backward is the same map
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    g = torch.autograd.grad((L.attn_fwd(q64, k64, v64, dims, heads, ws, scale) * do.double()).sum(), [q64, k64, v64])
    for got, want, what in zip((dq, dk, dv), g, ("dq", "dk", "dv")):
        near(got, want, what + " vs float64 autograd", rel=1e-12)
    # the fp32 oracle of test_gpu_ops.py
    qr, kvr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o32 = G._attn_ref(qr, kvr, dims, heads, ws)
    gq, gkv = torch.autograd.grad((o32 * do).sum(), [qr, kvr])
    near(o32.detach(), o, "o: _attn_ref vs the referee")
    near(gq, dq, "dq: _attn_ref vs the referee")
    near(gkv, torch.cat([dk, dv], 1), "dkv: _attn_ref vs the referee")


@pytest.mark.parametrize("dims,C,heads,ws", CASES)
def test_packed_qkv_view_equals_split(dims, C, heads, ws):
    q, kv, do = L.attn_inputs(dims, C)
    scale = (C // heads) ** -0.5
    qkv = torch.cat([q, kv], 1)
    packed = [qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]]
    assert not packed[1].is_contiguous()
    split = [t.contiguous() for t in packed]
    assert torch.equal(L.attn_fwd(*packed, dims, heads, ws, scale), L.attn_fwd(*split, dims, heads, ws, scale))
    for a, b in zip(L.attn_bwd(*packed, do, dims, heads, ws, scale), L.attn_bwd(*split, do, dims, heads, ws, scale)):
        assert torch.equal(a, b)
    # a [T, C + 1] buffer and a view at storage offset 1: the other two layouts the GPU test passes
    buf = torch.zeros(q.shape[0], C + 1)
    buf[:, :C] = q
    off = torch.zeros(kv.numel() + 1)
    off[1:] = kv.reshape(-1)
    kvo = off[1:].view_as(kv)
    assert torch.equal(L.attn_fwd(buf[:, :C], kvo[:, :C], kvo[:, C:], dims, heads, ws, scale), L.attn_fwd(*split, dims, heads, ws, scale))


@pytest.mark.parametrize("dims,C,heads,ws", L.LARGE_SCORE_CASES)
def test_large_score_yardstick(dims, C, heads, ws):
    """Scores reach +-60: the referee stays finite, rows are close to one-hot, and the fp32 CPU reference's error against it -- the
    figure test_gpu_ln_attn_arms.py multiplies by 4 -- is what fp32 gives: above zero, below 1e-4 of the tensor's max."""
    q, kv, do = L.large_score_inputs(dims, C, heads, ws)
    scale = (C // heads) ** -0.5
    s, p = L.attn_probs(q, kv[:, :C], dims, heads, ws, scale)
    assert abs(float(s.abs().max()) - 60.0) < 1e-3 and float(s.min()) < -40 and float(s.max()) > 40
    assert float(p.max(-1).values.median()) > 0.99
    o = L.attn_fwd(q, kv[:, :C], kv[:, C:], dims, heads, ws, scale)
    grads = L.attn_bwd(q, kv[:, :C], kv[:, C:], do, dims, heads, ws, scale)
    assert all(bool(torch.isfinite(t).all()) for t in (o,) + grads)
    errs = L.fp32_errors(G._attn_ref, q, kv, do, dims, heads, ws)
    scales = {"o": float(o.abs().max()), "dq": float(grads[0].abs().max()), "dkv": float(torch.cat(grads[1:], 1).abs().max())}
    for name in ("o", "dq", "dkv"):
        print(f"large scores C={C} heads={heads}: fp32 CPU reference vs float64, {name}: {errs[name]:.3e} (max |{name}| {scales[name]:.3e})")
        assert 0.0 < errs[name] <= 1e-4 * scales[name], (name, errs[name], scales[name])
