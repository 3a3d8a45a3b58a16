"""The bf16 GEMM and 3x3x3-convolution entry points against the bf16-operand referee (tests/bf16_ref.py): micf_linear_fwd /
_bwd_data / _bwd_weight / _bwd_weight_grouped and micf_conv3_fwd / _bwd_data / _bwd_weight / _bwd_weight_grouped in the benched
arithmetic mode, on plain randn operands (NOT bf16-representable) and on operands made of exact rounding ties, held to

  1. max|got - want| <= 1e-5 max|want|                        2. |got - want| <= (terms + 8) 2^-23 absdot  per element

where `want` is the operation in float64 on the operands rounded where the kernels round them.  test_bf16_ref_cpu.py shows that
these gates pass an honest evaluation and fail a truncating conversion, a half-away conversion of ties, a dropped 16-deep slab, a
clamped last row, a DropPath scale folded in before the rounding, and the fp32-operand result.

WHICH referee.  The bf16 instantiations run only where the LDS-DMA GEMM core (gemm_dma.h) or the direct convolution kernels
(conv3_fwdx / conv3_bwdx / conv3_wgradx) take the shape; the register-staged GEMM core behind every other shape ignores `dtype` and
computes in fp32.  The two referees are 200 x the gate apart, so a result matches one of them or is wrong, and every case states
which one it must match -- read off the dispatch in linear.hip / conv3.hip:
  * forward:         LDS-DMA when a2 is absent, N >= 48, M >= 64 and K % 16 == 0;
  * data gradient:   LDS-DMA when K >= 48 (K is the OUTPUT width here), M >= 64 and N % 16 == 0 -- so K = 16 and K = 24 are fp32,
                     and N = 16 is bf16;
  * weight gradient: LDS-DMA when a2 and a_gelu are absent, N, K >= 48, M >= 64, M % 16 == 0 and, with a DropPath scale, the token
                     split (rows_per_sample halved until it fits) is a multiple of 16 -- M = 80 / 208 at rows_per_sample = M / 2 are
                     fp32, at rows_per_sample = 16 bf16 with ONE slab per split;
  * conv3:           the direct kernels when N <= 16 (N == 16 for the weight gradient), channels-last, W >= 4.
A bf16 case that matched the fp32 referee would mean the benched mode fell back silently.

Every case prints one line: relative L2 distance, worst element over max|want|, worst ratio to bound 2, and the referee matched.
"""
import pytest
import torch

import bf16_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture()
def bf16():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micformer_amd import ops
    ops.set_compute_dtype("bf16")
    yield ops
    ops.set_compute_dtype("fp32")


def rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def scales(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) + 0.5).float()


def dev(t):
    return t.cuda().contiguous() if t is not None else None


class Report:
    """One printed line per compared tensor; the failed ones are asserted together at the end, so a run documents every distance."""

    def __init__(self, title):
        self.title, self.rows, self.bad = title, [], []

    def add(self, name, got, ref, expect):
        which, c = R.match(got, ref)
        self.rows.append(f"  {name:46s} rel-L2 {c.l2:8.2e}  worst {c.worst:8.2e}  of bound 2: {c.ratio:8.2e}  matches {which}")
        if which != expect:
            self.bad.append(f"{name}: matches {which}, must match {expect} (rel-L2 {c.l2:.2e}, worst {c.worst:.2e}, of bound 2 {c.ratio:.2e})")

    def close(self, name, got, want, atol=2e-5, rtol=1e-4):
        """A pointwise function after the product, against float64 of it on the kernel's own product (test_gpu_ops.close)."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        scale = max(float(want.abs().max()), 1e-30)
        err = float((got - want).abs().max())
        self.rows.append(f"  {name:46s} max abs err {err:8.2e} (scale {scale:8.2e}, gate {atol + rtol * scale:8.2e})")
        if not err <= atol + rtol * scale:
            self.bad.append(f"{name}: max abs err {err:.3e} (scale {scale:.3e})")

    def done(self):
        print("\n" + self.title + "\n" + "\n".join(self.rows))
        assert not self.bad, "\n".join(self.bad)


# ============================================================================= nn.Linear: forward and data gradient
# (M, N, K, forward's referee, data gradient's referee, tie-laden token operand)
LINEAR = [
    (64, 48, 16, "bf16", "fp32", False), (65, 80, 16, "bf16", "fp32", False), (127, 192, 16, "bf16", "fp32", False),
    (200, 48, 16, "bf16", "fp32", True), (127, 48, 48, "bf16", "bf16", False), (64, 192, 48, "bf16", "bf16", False),
    (127, 80, 48, "bf16", "bf16", True), (65, 48, 80, "bf16", "bf16", False), (200, 80, 80, "bf16", "bf16", False),
    (64, 80, 80, "bf16", "bf16", False), (65, 80, 384, "bf16", "bf16", False), (200, 192, 384, "bf16", "bf16", False),
    (250, 1536, 384, "bf16", "bf16", False),                # 2 x 5 x 5 x 5 tokens of the large model's last stage, its fc1
    (1100, 1536, 80, "bf16", "bf16", False),                # more than 256 tiles: the 64 x 64 kernel (not the skinny one) with a wrapping ring
    # fallbacks: N = 16; M = 7; K = 24
    (128, 16, 48, "fp32", "bf16", False), (7, 48, 48, "fp32", "fp32", False), (128, 48, 24, "fp32", "fp32", False),
]


@pytest.mark.parametrize("M,N,K,efwd,edg,tie", LINEAR)
def test_linear_forward_and_data_gradient(bf16, M, N, K, efwd, edg, tie):
    ops = bf16
    rep = Report(f"linear {M} x {N} x {K}" + (", ties" if tie else ""))
    a = R.ties(M, K, seed=1) if tie else rnd((M, K), 1)
    w, b, resid = rnd((N, K), 2, K ** -0.5), rnd((N,), 3, 0.1), rnd((M, N), 4)
    rps = M // 2 if M % 2 == 0 else M
    sc = scales(M // rps, 5)
    ca, cw, cb, cr, cs = dev(a), dev(w), dev(b), dev(resid), dev(sc)
    plain = R.linear_fwd(a, w, b)
    rep.add("forward, bias", ops.linear_fwd(ca, cw, cb), plain, efwd)
    rep.add("forward, resid + s * lin", ops.linear_fwd(ca, cw, cb, resid=cr, dp_scale=cs, rows_per_sample=rps),
            R.linear_fwd(a, w, b, resid=resid, dp_scale=sc, rows_per_sample=rps), efwd)
    y, pre = ops.linear_fwd(ca, cw, cb, act=1, want_pre=True)
    rep.add("forward, act = 1: pre_act", pre, plain, efwd)
    rep.close("forward, act = 1: y against gelu(pre_act)", y, R.gelu(pre.cpu()))

    dy = R.ties(M, N, seed=6) if tie else rnd((M, N), 6)
    pre_act, base = rnd((M, K), 7), rnd((M, K), 8)
    cdy = dev(dy)
    ref = R.linear_bwd_data(dy, w)
    d_plain = ops.linear_bwd_data(cdy, cw)
    rep.add("data gradient", d_plain, ref, edg)
    rep.add("data gradient, dp_scale", ops.linear_bwd_data(cdy, cw, dp_scale=cs, rows_per_sample=rps),
            R.linear_bwd_data(dy, w, sc, rps), edg)
    rep.close("data gradient, * gelu'(pre_act)", ops.linear_bwd_data(cdy, cw, pre_act=dev(pre_act)),
              d_plain.cpu().double() * R.gelu_grad(pre_act))
    out = dev(base).clone()
    ops.linear_bwd_data(cdy, cw, out=out, accumulate=True)
    rep.add("data gradient, accumulate", out, R.linear_bwd_data(dy, w, base=base), edg)
    k1 = K // 8 * 4
    d1, d2 = ops.linear_bwd_data(cdy, cw, k1=k1)
    assert d1.shape == (M, k1) and d2.shape == (M, K - k1)
    rep.add(f"data gradient, split at k1 = {k1}", torch.cat([d1, d2], 1), ref, edg)
    rep.done()


def test_linear_forward_two_sources_is_fp32(bf16):
    """a2 given: the concatenating accessor of the register-staged core, which has no bf16 form."""
    ops = bf16
    rep = Report("linear 128 x 96 x (24 | 24)")
    a1, a2, w, b = rnd((128, 24), 1), rnd((128, 24), 2), rnd((96, 48), 3, 48 ** -0.5), rnd((96,), 4, 0.1)
    rep.add("forward, [a1 | a2]", ops.linear_fwd(dev(a1), dev(w), dev(b), a2=dev(a2)), R.linear_fwd(a1, w, b, a2=a2), "fp32")
    rep.done()


# ============================================================================= nn.Linear: weight gradient
def run_wgrad(ops, dy, a, N, K, sc=None, rps=0, bias=True, workspace=True, a2=None, a_gelu=False):
    dw, db = torch.zeros(N, K, device="cuda"), (torch.zeros(N, device="cuda") if bias else None)
    if workspace:
        ops.linear_bwd_weight(dev(dy), dev(a), dw, db, a2=dev(a2), dp_scale=dev(sc), rows_per_sample=rps, a_gelu=a_gelu)
    else:                                    # the C-ABI without a workspace: every token split adds its partial atomically
        from micformer_amd._lib import call, f32
        cdy, ca, cs = dev(dy), dev(a), dev(sc)
        call("micf_linear_bwd_weight", f32(cdy), f32(cs), rps, f32(ca), None, a.shape[1], 0, f32(dw), f32(db), dy.shape[0], N, K,
             None, 0, 1)
    return dw, db


# (M, N, K, rows_per_sample (0: no DropPath scale), referee, tie-laden dy)
WGRAD = [
    (64, 48, 48, 0, "bf16", False), (64, 96, 192, 32, "bf16", False),
    (80, 96, 48, 0, "bf16", False), (80, 192, 192, 0, "bf16", True), (80, 48, 96, 16, "bf16", False),
    (208, 48, 192, 0, "bf16", False), (208, 192, 96, 16, "bf16", False),
    (4096, 192, 96, 0, "bf16", False), (4096, 48, 48, 2048, "bf16", False), (4096, 96, 192, 32, "bf16", True),
    # fallbacks: the token split of one sample is no multiple of 16; M is none
    (80, 96, 48, 40, "fp32", False), (208, 48, 192, 104, "fp32", False), (100, 48, 48, 0, "fp32", False),
]


@pytest.mark.parametrize("M,N,K,rps,expect,tie", WGRAD)
def test_linear_weight_gradient(bf16, M, N, K, rps, expect, tie):
    ops = bf16
    rep = Report(f"linear weight gradient {M} x {N} x {K}, rows_per_sample {rps}" + (", ties" if tie else ""))
    a, dy = rnd((M, K), 1), (R.ties(M, N, seed=2) if tie else rnd((M, N), 2))
    sc = scales(M // rps, 3) if rps else None
    rw, rb_ = R.linear_bwd_weight(dy, a, dp_scale=sc, rows_per_sample=rps)
    dw, db = run_wgrad(ops, dy, a, N, K, sc, rps)
    rep.add("dw", dw, rw, expect)
    rep.add("dbias (unrounded dy)", db, rb_, "both")
    dw, _ = run_wgrad(ops, dy, a, N, K, sc, rps, bias=False)
    rep.add("dw, no dbias", dw, rw, expect)
    if M == 4096:
        dw, db = run_wgrad(ops, dy, a, N, K, sc, rps, workspace=False)
        rep.add("dw, no workspace (atomic splits)", dw, rw, expect)
        rep.add("dbias, no workspace", db, rb_, "both")
    rep.done()


def test_linear_weight_gradient_fp32_accessors(bf16):
    """a_gelu and a2: accessors of the register-staged core only."""
    ops = bf16
    rep = Report("linear weight gradient 128 x 48 x 48, a_gelu / [a1 | a2]")
    a, a2, dy = rnd((128, 48), 1), rnd((128, 48), 2), rnd((128, 48), 3)
    rw, rb_ = R.linear_bwd_weight(dy, a, a_gelu=True)
    dw, db = run_wgrad(ops, dy, a, 48, 48, a_gelu=True)
    rep.add("dw, GELU(a1)", dw, rw, "fp32")
    rep.add("dbias", db, rb_, "both")
    rw, _ = R.linear_bwd_weight(dy, a, a2=a2)
    dw, _ = run_wgrad(ops, dy, a, 48, 96, a2=a2)
    rep.add("dw, [a1 | a2]", dw, rw, "fp32")
    rep.done()


@pytest.mark.parametrize("M,N,K,rps", [(208, 96, 48, 0), (4096, 48, 192, 2048)])
def test_linear_weight_gradient_grouped(bf16, M, N, K, rps):
    """micf_linear_bwd_weight_grouped on fp32-stored operands that are NOT bf16-representable: the rounding at the fragment read."""
    ops = bf16
    rep = Report(f"grouped linear weight gradient {M} x {N} x {K}, rows_per_sample {rps}")
    a, dy, t = rnd((M, K), 1), rnd((M, N), 2), R.ties(M, N, seed=4)
    sc = scales(M // rps, 3) if rps else None
    ca, cs = dev(a), dev(sc)
    items = [(dev(g), ca, torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda"), cs, rps) for g in (dy, t)]
    assert all(ops.wgrad_groupable(it[0], it[1], cs, rps) for it in items)
    ops.linear_bwd_weight_grouped(items)
    for name, g, it in zip(("randn dy", "tie-laden dy"), (dy, t), items):
        rw, rb_ = R.linear_bwd_weight(g, a, dp_scale=sc, rows_per_sample=rps)
        rep.add(f"dw, {name}", it[2], rw, "bf16")
        rep.add(f"dbias, {name}", it[3], rb_, "both")
    rep.done()


# (grid, referee): 36 output tokens are fewer than the LDS-DMA core's 64, 80 are not
@pytest.mark.parametrize("grid,expect", [((1, 5, 6, 7), "fp32"), ((1, 9, 8, 8), "bf16")])
def test_conv_down_as_the_step_runs_it(bf16, grid, expect):
    """PatchMerging's Conv3d(48 -> 96, k = s = 2) the way functional.ConvDownFn runs it in the step (space_to_depth + the linear GEMMs;
    odd extents padded) against F.conv3d in float64: forward and all three gradients."""
    from micformer_amd import functional as Fn
    B, D, H, W = grid
    C, N = 48, 96
    rep = Report(f"conv_down {grid}, {C} -> {N}")
    x, w, b = rnd((B, D, H, W, C), 1), rnd((N, C, 2, 2, 2), 2, (8 * C) ** -0.5), rnd((N,), 3, 0.1)
    dy = rnd((B, -(-D // 2), -(-H // 2), -(-W // 2), N), 4)
    ref = R.conv_down(x, w, b, dy)
    assert Fn.PATCH_GEMM
    ins = [dev(t).requires_grad_(True) for t in (x, w, b)]
    try:
        y = Fn.ConvDownFn.apply(*ins)
        y.backward(dev(dy))
    finally:
        Fn.clear_skip_tokens()
    rep.add("y", y, ref["y"], expect)
    rep.add("dx", ins[0].grad, ref["dx"], expect)
    rep.add("dw", ins[1].grad, ref["dw"], expect)
    rep.add("dbias", ins[2].grad, ref["db"], "both")
    rep.done()


# ============================================================================= 3x3x3 convolution, N = 16, inputs [x1 | x2]
def conv3_inputs(dims, C, N=16, tie=False):
    B, D, H, W = dims
    T = B * D * H * W
    x1 = R.ties(T, C, seed=1) if tie else rnd((T, C), 1)
    x2, w, b = rnd((T, C), 2), rnd((N, 2 * C, 3, 3, 3), 3, (54 * C) ** -0.5), rnd((N,), 4, 0.1)
    dy = R.ties(T, N, seed=5) if tie else rnd((T, N), 5)
    return x1, x2, w, b, dy, rnd((T, 2 * C), 6)


_CONV3_REF = {}


def conv3_ref(dims, C, tie=False):
    """(inputs, referee, referee with a base under dx), computed once per shape and shared (never written)."""
    key = (dims, C, tie)
    if key not in _CONV3_REF:
        ins = conv3_inputs(dims, C, tie=tie)
        x1, x2, w, b, dy, base = ins
        ref = R.conv3(x1, x2, w, b, dy, dims)
        dxb = R.Ref(ref["dx"].want + base.double(), ref["dx"].want32 + base.double(), ref["dx"].absdot + base.double().abs(),
                    ref["dx"].terms + 1)
        _CONV3_REF[key] = (ins, ref, dxb)
    return _CONV3_REF[key]


def conv3_all(ops, rep, ins, ref, dxb, dims, C, expect, tag=""):
    x1, x2, w, b, dy, base = ins
    c1, c2, cw, cb, cdy = dev(x1), dev(x2), dev(w), dev(b), dev(dy)
    rep.add(tag + "y", ops.conv3_fwd(c1, cw, cb, dims, x2=c2), ref["y"], expect)
    rep.add(tag + "dx", torch.cat(ops.conv3_bwd_data(cdy, cw, dims, C, C), 1), ref["dx"], expect)
    cbase = dev(base)
    d1, d2 = cbase[:, :C].contiguous(), cbase[:, C:].contiguous()
    ops.conv3_bwd_data(cdy, cw, dims, C, C, dx1=d1, dx2=d2, acc1=True, acc2=True)
    rep.add(tag + "dx, acc1 / acc2", torch.cat([d1, d2], 1), dxb, expect)
    dw, db = torch.zeros_like(cw), torch.zeros(w.shape[0], device="cuda")
    ops.conv3_bwd_weight(cdy, c1, dw, db, dims, x2=c2)
    rep.add(tag + "dw", dw, ref["dw"], expect)
    rep.add(tag + "dbias (unrounded dy)", db, ref["db"], "both")


# TW = 8, every tile ragged, c1 = 24: a 16-channel chunk across the x1 | x2 seam;  TW = 16;  TW = 16 ragged, six channel chunks split
# over workgroups and added atomically;  256 token tiles: no channel split, the XCD reordering;  fallback: W < 4
CONV3 = [((1, 3, 5, 9), 24, "bf16", False), ((1, 3, 5, 9), 24, "bf16", True), ((2, 2, 4, 12), 48, "bf16", False),
         ((1, 3, 6, 19), 96, "bf16", False), ((2, 16, 32, 32), 24, "bf16", False), ((1, 4, 4, 3), 24, "fp32", False)]


@pytest.mark.parametrize("dims,C,expect,tie", CONV3)
def test_conv3(bf16, dims, C, expect, tie):
    rep = Report(f"conv3 {dims}, 2 x {C} -> 16" + (", ties" if tie else ""))
    ins, ref, dxb = conv3_ref(dims, C, tie)
    conv3_all(bf16, rep, ins, ref, dxb, dims, C, expect)
    rep.done()


def test_conv3_ncdhw_eight_channels_is_fp32(bf16):
    """N = 8 with NCDHW output and dy (Head.out_conv): the implicit GEMM on the register-staged core."""
    ops = bf16
    dims, C, N = (1, 4, 4, 8), 24, 8
    B, D, H, W = dims
    rep = Report(f"conv3 {dims}, 2 x {C} -> {N}, NCDHW")
    x1, x2, w, b, dy, _ = conv3_inputs(dims, C, N=N)
    ref = R.conv3(x1, x2, w, b, dy, dims)
    planes = lambda t: t.reshape(B, D, H, W, N).permute(0, 4, 1, 2, 3).contiguous()
    tokens = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, N)
    c1, c2, cw, cdy = dev(x1), dev(x2), dev(w), dev(planes(dy))
    rep.add("y", tokens(ops.conv3_fwd(c1, cw, dev(b), dims, x2=c2, ncdhw_out=True)), ref["y"], "fp32")
    rep.add("dx", torch.cat(ops.conv3_bwd_data(cdy, cw, dims, C, C, ncdhw=True), 1), ref["dx"], "fp32")
    dw, db = torch.zeros_like(cw), torch.zeros(N, device="cuda")
    ops.conv3_bwd_weight(cdy, c1, dw, db, dims, x2=c2, ncdhw=True)
    rep.add("dw", dw, ref["dw"], "fp32")
    rep.add("dbias", db, ref["db"], "both")
    rep.done()


def test_conv3_prepared_weights(bf16):
    """The prepared-weight form (Conv3PrepPlan: both re-laid-out copies written once, `prepared` = 1) against the same referee."""
    from micformer_amd._lib import call, f32
    ops = bf16
    dims, C = (1, 3, 6, 19), 96
    B, D, H, W = dims
    rep = Report(f"conv3 {dims}, 2 x {C} -> 16, prepared weights")
    (x1, x2, w, b, dy, _), ref, _ = conv3_ref(dims, C)
    c1, c2, cw, cb, cdy = dev(x1), dev(x2), dev(w), dev(b), dev(dy)
    fwd, bwd = ops.conv3_prepared_like(cw)
    assert fwd is not None and bwd is not None
    ops.Conv3PrepPlan([(cw, fwd, bwd)]).launch()
    T = B * D * H * W
    y, dx1, dx2 = (torch.empty(T, n, device="cuda") for n in (16, C, C))
    call("micf_conv3_fwd", f32(c1), C, f32(c2), C, f32(cw), f32(cb), f32(y), 0, B, D, H, W, 16, f32(fwd), fwd.numel(), 1, 1)
    call("micf_conv3_bwd_data", f32(cdy), 0, f32(cw), f32(dx1), C, 0, f32(dx2), C, 0, B, D, H, W, 16, f32(bwd), bwd.numel(), 1, 1)
    rep.add("y", y, ref["y"], "bf16")
    rep.add("dx", torch.cat([dx1, dx2], 1), ref["dx"], "bf16")
    rep.done()


@pytest.mark.parametrize("dims,C", [((2, 2, 4, 12), 48), ((1, 3, 5, 9), 24)])
def test_conv3_weight_gradient_grouped(bf16, dims, C):
    """micf_conv3_bwd_weight_grouped, 3 layers of one shape in one launch (conv3_wgradx_b16_kernel, blockIdx.z = layer), each against
    its own referee."""
    ops = bf16
    B, D, H, W = dims
    T = B * D * H * W
    rep = Report(f"grouped conv3 weight gradient {dims}, 2 x {C} -> 16, 3 layers")
    layers = [(rnd((T, 16), 10 * k + 1), rnd((T, C), 10 * k + 2), rnd((T, C), 10 * k + 3)) for k in range(3)]
    items = [(dev(dy), dev(x1), dev(x2), torch.zeros(16, 2 * C, 3, 3, 3, device="cuda"), torch.zeros(16, device="cuda"))
             for dy, x1, x2 in layers]
    ops.conv3_bwd_weight_grouped(items, dims)
    w0 = torch.zeros(16, 2 * C, 3, 3, 3)
    for k, ((dy, x1, x2), it) in enumerate(zip(layers, items)):
        ref = R.conv3(x1, x2, w0, None, dy, dims)
        rep.add(f"layer {k}: dw", it[3], ref["dw"], "bf16")
        rep.add(f"layer {k}: dbias", it[4], ref["db"], "both")
    rep.done()
