"""tests/bf16_ref.py on the CPU: the two gates of `check` pass an honest fp32-accumulating evaluation of the bf16-rounded operands and
FAIL each of the faults a bf16 kernel can have without the old gate (1.5e-2 of the maximum, against the fp32 mode of the same
kernel) noticing: a wrong conversion, a dropped slab, a clamped row, a scale folded in before the rounding, a silent fp32 product.
The honest evaluation is torch's own fp32 matmul / conv3d on the rounded operands: products of bf16 values are exact in fp32, so it
differs from the float64 referee by its summation order only -- as a correct kernel does.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R

SHAPES = [(200, 96, 384), (70, 48, 48), (100, 48, 16)]


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def f32(t):
    return t.float()


def show(name, c):
    print(f"  {name:44s} rel-L2 {c.l2:8.2e}  worst {c.worst:8.2e}  of bound 2: {c.ratio:8.2e}  {'pass' if c.ok else 'FAIL'}")
    return c


def lin_inputs(M, N, K):
    a, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3, scale=0.1)
    resid = rnd(M, N, seed=4)
    sc = torch.rand(2, generator=torch.Generator().manual_seed(5)) + 0.5
    return a, w, b, resid, sc


def lin_eval(a, w, b, conv=R.rb, resid=None, sc=None, fold=False, kdrop=0, clamp=False):
    """fp32 evaluation of conv(a) conv(w)^T + b, or of resid + s * (that) when resid and the per-sample scales sc are given (any
    number of equal samples), with the planted faults of the tests below.  fold: s multiplied into a BEFORE the rounding."""
    M, K = a.shape
    assert (resid is None) == (sc is None) and (sc is not None or not fold), "the DropPath scale comes with the residual"
    s = None
    if sc is not None:
        assert M % sc.numel() == 0, "equal samples"
        s = sc.repeat_interleave(M // sc.numel())[:, None]
    ar = f32(conv(a * s if fold else a))
    wr = f32(conv(w))
    if kdrop:
        ar, wr = ar[:, :K - kdrop], wr[:, :K - kdrop]
    y = ar @ wr.t() + (s * b if fold else b)     # (folded: the bias carries the scale too, so the rounding point is the ONLY fault)
    if clamp:                                   # the last row of a ragged 64-tile read from the row before it
        y[M - 1] = ar[M - 2] @ wr.t() + b
    if resid is not None:
        y = resid + (1.0 if fold else s) * y
    return y


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_forward_gates(M, N, K):
    a, w, b, resid, sc = lin_inputs(M, N, K)
    ref = R.linear_fwd(a, w, b)
    refs = R.linear_fwd(a, w, b, resid=resid, dp_scale=sc, rows_per_sample=M // 2)
    print(f"\nlinear forward {M} x {N} x {K}")
    ck = lambda name, got, r=ref: show(name, R.check(got, r.want, r.absdot, r.terms))
    honest = ck("honest (fp32 sum of the rounded operands)", lin_eval(a, w, b))
    assert honest.ok and honest.l2 < 1e-6 and honest.ratio < 0.25
    assert R.match(lin_eval(a, w, b), ref)[0] == "bf16"
    assert ck("honest, resid + s * lin", lin_eval(a, w, b, resid=resid, sc=sc), refs).ok
    assert not ck("operands truncated", lin_eval(a, w, b, conv=R.truncate)).ok
    assert not ck("last 16-deep k slab dropped", lin_eval(a, w, b, kdrop=16)).ok
    assert not ck("last ragged row from the row before", lin_eval(a, w, b, clamp=True)).ok
    assert not ck("DropPath scale folded in before rounding", lin_eval(a, w, b, resid=resid, sc=sc, fold=True), refs).ok
    # the two referees are never confusable: the fp32-operand result fails the bf16 referee and the other way round
    y32 = a @ w.t() + b
    c32 = ck("fp32 operands against the bf16 referee", y32)
    assert not c32.ok and c32.l2 > 1e-3
    assert R.match(y32, ref)[0] == "fp32"
    assert not show("bf16 operands against the fp32 referee", R.check(lin_eval(a, w, b), ref.want32, ref.absdot, ref.terms)).ok
    # exact rounding ties in one operand: half-away differs from half-even on every value whose last kept bit is even
    t = R.ties(M, K, seed=6)
    rt = R.linear_fwd(t, w, b)
    assert ck("ties, half-even", lin_eval(t, w, b), rt).ok
    wrong = f32(R.half_away(t)) @ f32(R.rb(w)).t() + b
    assert not ck("ties, half-away", wrong, rt).ok


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_gradient_referees_pass_an_honest_evaluation(M, N, K):
    """The data- and weight-gradient referees against torch's fp32 products of the rounded operands, and the fault of the scale
    folded into dy before the rounding on both."""
    a, w, _, _, sc = lin_inputs(M, N, K)
    dy, pre, base = rnd(M, N, seed=7), rnd(M, K, seed=8), rnd(M, K, seed=9)
    s = sc.repeat_interleave(M // 2)[:, None]
    dyr, wr, ar = f32(R.rb(dy)), f32(R.rb(w)), f32(R.rb(a))
    print(f"\nlinear gradients {M} x {N} x {K}")
    ck = lambda name, got, r: show(name, R.check(got, r.want, r.absdot, r.terms))
    ref = R.linear_bwd_data(dy, w, sc, M // 2, pre_act=pre, base=base)
    assert ck("data gradient", base + s * (dyr @ wr) * f32(R.gelu_grad(pre)), ref).ok
    ref = R.linear_bwd_data(dy, w, sc, M // 2)
    assert ck("data gradient, plain", s * (dyr @ wr), ref).ok
    assert not ck("data gradient, scale folded into dy", f32(R.rb(s * dy)) @ wr, ref).ok
    assert not ck("data gradient, fp32 operands", s * (dy @ w), ref).ok
    rw, rb_ = R.linear_bwd_weight(dy, a, dp_scale=sc, rows_per_sample=M // 2)
    assert ck("weight gradient", (s * dyr).t() @ ar, rw).ok
    assert not ck("weight gradient, scale folded into dy", f32(R.rb(s * dy)).t() @ ar, rw).ok
    assert not ck("weight gradient, dy slab of 16 tokens dropped", (s * dyr)[16:].t() @ ar[16:], rw).ok
    assert ck("bias gradient (unrounded dy)", (s * dy).sum(0), rb_).ok
    assert torch.equal(rb_.want, rb_.want32)
    assert not ck("bias gradient from the rounded dy", (s * dyr).sum(0), rb_).ok


def test_conv3_gates():
    dims, C, N = (1, 3, 5, 9), 8, 16
    B, D, H, W = dims
    T = B * D * H * W
    x1, x2 = rnd(T, C, seed=1), rnd(T, C, seed=2)
    w, b, dy = rnd(N, 2 * C, 3, 3, 3, seed=3, scale=(54 * C) ** -0.5), rnd(N, seed=4, scale=0.1), rnd(T, N, seed=5)
    vol = lambda t, c: t.reshape(B, D, H, W, c).permute(0, 4, 1, 2, 3).contiguous()
    tok = lambda t: t.permute(0, 2, 3, 4, 1).reshape(T, -1)

    def run(xa, xb, conv=R.rb, drop_tap=False, clamp=False):
        xr = vol(f32(conv(torch.cat([xa, xb], 1))), 2 * C).requires_grad_(True)
        wr = f32(conv(w)).clone()
        if drop_tap:
            wr[:, :, 2, 2, 2] = 0.0                  # the unpaired 27th tap
        wr.requires_grad_(True)
        y = F.conv3d(xr, wr, None, padding=1)
        gx, gw = torch.autograd.grad(y, (xr, wr), vol(f32(conv(dy)), N))
        y = tok(y.detach()) + b
        if clamp:
            y[T - 1] = y[T - 2]
        return {"y": y, "dx": tok(gx), "dw": gw, "db": dy.sum(0)}

    ref = R.conv3(x1, x2, w, b, dy, dims)
    print("\nconv3 (1, 3, 5, 9) x 16 channels")
    ck = lambda name, got, r: show(name, R.check(got, r.want, r.absdot, r.terms))
    honest = run(x1, x2)
    for k in ("y", "dx", "dw", "db"):
        c = ck(f"honest {k}", honest[k], ref[k])
        assert c.ok and c.l2 < 1e-6 and c.ratio < 0.25
    assert R.match(honest["y"], ref["y"])[0] == "bf16" and R.match(honest["db"], ref["db"])[0] == "both"
    trunc, exact = run(x1, x2, conv=R.truncate), run(x1, x2, conv=lambda t: t.double())
    for k in ("y", "dx", "dw"):
        assert not ck(f"operands truncated, {k}", trunc[k], ref[k]).ok
        c = ck(f"fp32 operands against the bf16 referee, {k}", exact[k], ref[k])
        assert not c.ok and c.l2 > 1e-3 and R.match(exact[k], ref[k])[0] == "fp32"
    assert not ck("27th tap dropped", run(x1, x2, drop_tap=True)["y"], ref["y"]).ok
    assert not ck("last token from the token before", run(x1, x2, clamp=True)["y"], ref["y"]).ok
    t1 = R.ties(T, C, seed=6)
    rt = R.conv3(t1, x2, w, b, dy, dims)
    assert ck("ties, half-even", run(t1, x2)["y"], rt["y"]).ok
    assert not ck("ties, half-away", run(t1, x2, conv=R.half_away)["y"], rt["y"]).ok      # (equal to RNE on every value that is no tie)


def test_conv_down_referee_pads_odd_extents():
    x, w, b = rnd(1, 5, 6, 7, 4, seed=1), rnd(8, 4, 2, 2, 2, seed=2), rnd(8, seed=3)
    dy = rnd(1, 3, 3, 4, 8, seed=4)
    ref = R.conv_down(x, w, b, dy)
    assert ref["y"].want.shape == (1, 3, 3, 4, 8) and ref["dx"].want.shape == x.shape and ref["dw"].want.shape == w.shape
    # the far corner cell (2, 2, 3) holds two real voxels, (4, 4, 6) and (4, 5, 6) at kernel positions (0, 0, 0) and (0, 1, 0): D and W are odd
    got = R.rb(w)[:, :, 0, 0, 0] @ R.rb(x)[0, 4, 4, 6] + R.rb(w)[:, :, 0, 1, 0] @ R.rb(x)[0, 4, 5, 6] + b.double()
    assert torch.allclose(ref["y"].want[0, 2, 2, 3], got, rtol=1e-12, atol=1e-12)


def test_conv_down_referee_passes_an_honest_evaluation():
    """y, dx, dw, db of the k = s = 2 convolution on an odd grid against torch's fp32 conv3d / autograd on the rounded operands; the
    fp32-operand evaluation matches the other referee."""
    x, w, b = rnd(1, 5, 6, 7, 16, seed=1), rnd(24, 16, 2, 2, 2, seed=2, scale=128 ** -0.5), rnd(24, seed=3, scale=0.1)
    dy = rnd(1, 3, 3, 4, 24, seed=4)
    ref = R.conv_down(x, w, b, dy)

    def run(conv):
        xr, wr = f32(conv(x)).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True), f32(conv(w)).requires_grad_(True)
        y = F.conv3d(F.pad(xr, (0, 1, 0, 0, 0, 1)), wr, None, stride=2)
        gx, gw = torch.autograd.grad(y, (xr, wr), f32(conv(dy)).permute(0, 4, 1, 2, 3).contiguous())
        return {"y": y.detach().permute(0, 2, 3, 4, 1) + b, "dx": gx.permute(0, 2, 3, 4, 1), "dw": gw, "db": dy.reshape(-1, 24).sum(0)}

    print("\nconv_down (1, 5, 6, 7), 16 -> 24")
    honest, exact = run(R.rb), run(lambda t: t.double())
    for k in ("y", "dx", "dw", "db"):
        which, c = R.match(honest[k], ref[k])
        show(f"honest {k}: matches {which}", c)
        assert which == ("both" if k == "db" else "bf16") and c.ratio < 0.25
    for k in ("y", "dx", "dw"):
        assert R.match(exact[k], ref[k])[0] == "fp32"
        assert R.match(honest[k] * (1 + 3e-5), ref[k])[0] is None           # neither referee: a wrong result is not a fallback


def test_two_source_and_gelu_operand_referees():
    """[a1 | a2] (forward, weight gradient) and GELU(a1) (weight gradient): accessors of the fp32 paths, so the honest evaluation is the
    fp32-operand one and must match want32 -- and the rounded evaluation must match want."""
    M, N, k1, k2 = 72, 48, 24, 40
    a1, a2, w, b, dy = rnd(M, k1, seed=1), rnd(M, k2, seed=2), rnd(N, k1 + k2, seed=3, scale=0.125), rnd(N, seed=4, scale=0.1), rnd(M, N, seed=5)
    a = torch.cat([a1, a2], 1)
    ref = R.linear_fwd(a1, w, b, a2=a2)
    assert R.match(a @ w.t() + b, ref)[0] == "fp32" and R.match(f32(R.rb(a)) @ f32(R.rb(w)).t() + b, ref)[0] == "bf16"
    rw, rb_ = R.linear_bwd_weight(dy, a1, a2=a2)
    assert rw.want.shape == (N, k1 + k2)
    assert R.match(dy.t() @ a, rw)[0] == "fp32" and R.match(f32(R.rb(dy)).t() @ f32(R.rb(a)), rw)[0] == "bf16"
    assert R.match(dy.sum(0), rb_)[0] == "both"
    rw, _ = R.linear_bwd_weight(dy, a1, a_gelu=True)
    g = F.gelu(a1)                                                          # (exact erf form, fp32)
    assert R.match(dy.t() @ g, rw)[0] == "fp32"
    assert R.match(dy.t() @ a1, rw)[0] is None                              # the activation forgotten


def test_rb_is_round_to_nearest_even_bit_for_bit():
    special = torch.tensor([0x3F7FFFFF, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0xBF7FFFFF, 0x3F800000,
                            0x7F7F7FFF, 0x00800000, 0x00808000], dtype=torch.int64)
    x = torch.cat([R._from_bits(special), R.ties(4096, seed=1), -R.ties(4096, seed=2).abs(), rnd(4096, seed=3), rnd(4096, seed=4, scale=1e-20),
                   rnd(4096, seed=5, scale=1e20)])
    assert torch.equal(R.rb(x), R.rb_int(x))
    # the carry into the exponent: 0x3F7FFFFF (just below 1) rounds to 1.0; ties go to the even neighbour, whatever the sign
    assert float(R.rb(R._from_bits(torch.tensor([0x3F7FFFFF])))) == 1.0
    assert R._bits(R.rb(R._from_bits(special[1:3])).float()).tolist() == [0x3F800000, 0x3F820000]
    assert R._bits(R.rb(R._from_bits(special[5:7])).float()).tolist() == [0xBF800000, 0xBF820000]
    t = R.ties(4096, seed=1)
    low = (R._bits(t) >> 16) & 1
    assert 0 < int(low.sum()) < t.numel()                                    # odd and even last bits both present
    assert bool((R._bits(t) & 0xFFFF == 0x8000).all())
    # half-away and truncation differ from RNE exactly where they should
    assert torch.equal(R.half_away(t) != R.rb(t), low == 0)
    assert torch.equal(R.truncate(t) != R.rb(t), low == 1)
