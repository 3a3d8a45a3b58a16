"""The patch-matrix-free head (head_tail_fused.hip) against its bf16-operand referee (tests/head_ref.py): the raw entry points
micf_head_tail_pack / _fwd_fused (with its _loss_fused and _sw forms) / _bwd_data_fused / _bwd_weight_fused on FREE wb, bf, b_out,
on plain randn operands (NOT bf16-representable) and on operands made of exact rounding ties, held to bf16_ref.check's two gates

  1. max|got - want| <= 1e-5 max|want|                        2. |got - want| <= (terms + 8) 2^-23 absdot  per element

where `want` is the map in float64 on the operands rounded where the kernels round them.  test_head_ref_cpu.py shows that these gates
pass an honest evaluation and fail a wrong conversion, a dropped neighbour slab, a bias counted for an out-of-volume neighbour or
without its lo half, b_out in a second slab, a dropped one-voxel chunk of the dy halo, a dropped reduction step, a halo across the
batch boundary, dBf from the rounded dy, and the fp32-operand result.

Every result must match the "bf16" referee, dBf (an fp32 sum of the unrounded dy) "both"; "fp32" would be a silent fallback.  The shapes
are the smallest at which each mechanism exists (1 x 4 x 16 coarse voxels per forward workgroup, 1 x 2 x 16 per data-gradient one, a
tile remap when the grid is a multiple of 8; 32 coarse voxels per weight-gradient step, min(42, steps) workgroup groups).
Every case prints one line per tensor: relative L2 distance, worst element over max|want|, worst ratio to bound 2, referee matched.
"""
import math

import pytest
import torch

import bf16_ref as R
import head_ref as H

pytestmark = pytest.mark.gpu

CO, P = 8, 4


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


def dev(t):
    return t.cuda().contiguous()


class Report:
    """One printed line per compared tensor; the failed ones are asserted together at the end, so a run documents every distance."""

    def __init__(self, title):
        self.title, self.rows, self.bad = title, [], []

    def add(self, name, got, ref, expect):
        which, c = R.match(got, ref)
        self.rows.append(f"  {name:46s} rel-L2 {c.l2:8.2e}  worst {c.worst:8.2e}  of bound 2: {c.ratio:8.2e}  matches {which}")
        if which != expect:
            self.bad.append(f"{name}: matches {which}, must match {expect} (rel-L2 {c.l2:.2e}, worst {c.worst:.2e}, of bound 2 {c.ratio:.2e})")

    def line(self, text, ok):
        self.rows.append("  " + text)
        if not ok:
            self.bad.append(text)

    def done(self):
        print("\n" + self.title + "\n" + "\n".join(self.rows))
        assert not self.bad, "\n".join(self.bad)


_INPUTS = {}


def inputs(dims, Ci, tie=False):
    """x, wb, bf, b_out, dy on the CPU, once per case and never written."""
    key = (dims, Ci, tie)
    if key not in _INPUTS:
        B, Dc, Hc, Wc = dims
        T, fine = B * Dc * Hc * Wc, (B, CO, P * Dc, P * Hc, P * Wc)
        if tie:
            x, wb, dy = R.ties(T, Ci, seed=1), R.ties(H.ROWS, Ci, seed=2, scale=Ci ** -0.5), R.ties(*fine, seed=5)
        else:
            x, wb, dy = rnd((T, Ci), 1), rnd((H.ROWS, Ci), 2, Ci ** -0.5), rnd(fine, 5)
        _INPUTS[key] = (x, wb, rnd((H.ROWS,), 3, 0.2), rnd((CO,), 4), dy)
    return _INPUTS[key]


# ============================================================================= forward and data gradient
# (grid, Ci, ties, forward workgroups, data-gradient workgroups)
FWD = [((1, 1, 4, 16), 96, False, 1, 2),        # one tile, every neighbour outside the volume
       ((2, 1, 4, 16), 96, False, 2, 4),        # the depth halo at the sample boundary
       ((2, 3, 8, 32), 96, False, 24, 48),      # both grids multiples of 8: the XCD remap; interior tiles along all three axes
       ((1, 5, 12, 16), 96, False, 15, 30),     # remap off
       ((1, 2, 4, 48), 192, False, 6, 12),      # three w tiles, the second instantiation
       ((1, 2, 4, 16), 96, True, 2, 4)]         # x, dy, wb of exact rounding ties


@pytest.mark.parametrize("dims,Ci,tie,gf,gd", FWD)
def test_forward_and_data_gradient(bf16, dims, Ci, tie, gf, gd):
    ops = bf16
    B, Dc, Hc, Wc = dims
    assert gf == B * Dc * (Hc // 4) * (Wc // 16) and gd == B * Dc * (Hc // 2) * (Wc // 16)       # (tail_fwd_any / _bwd_data_fused)
    rep = Report(f"head {dims}, Ci {Ci}" + (", ties" if tie else "") + f": grids {gf} / {gd}, remap {'on' if gf % 8 == 0 else 'off'} / "
                 f"{'on' if gd % 8 == 0 else 'off'}")
    x, wb, bf, b_out, dy = inputs(dims, Ci, tie)
    assert ops.head_tail_fused_supported(dims, Ci, CO, P)
    pf, pq = ops.head_tail_pack(dev(wb), dev(bf), dev(b_out), P)
    rep.add("logits", ops.head_tail_fwd_fused(dev(x), pf, dims, CO, P), H.head_fwd(x, wb, bf, b_out, dims), "bf16")
    rep.add("dx", ops.head_tail_bwd_data_fused(dev(dy), pq, dims, Ci, P), H.head_bwd_data(dy, wb, dims), "bf16")
    # x = 0: the composite bias alone.  A fine voxel has at most 8 in-volume neighbours; each one's hi + lo pair enters the fp32
    # accumulator as exact products with 1.0 (the x products add exact zeros), and an fp32 add rounds by at most half an ulp, 2^-24 of the
    # running sum.  2^-22 of the maximum is four such roundings at full scale, all in one direction; the 8-neighbour voxels, which set
    # the maximum, start their running sums from a single term.
    y0 = ops.head_tail_fwd_fused(torch.zeros_like(dev(x)), pf, dims, CO, P).cpu().double()
    want = H.bias_term(bf, b_out, dims)
    err, scale = float((y0 - want).abs().max()), float(want.abs().max())
    rep.line(f"{'logits at x = 0 against the bias term':46s} max abs err {err:8.2e} (scale {scale:8.2e}, gate {2.0 ** -22 * scale:8.2e})",
             err <= 2.0 ** -22 * scale)
    rep.done()


# ============================================================================= weight gradient
def wgrad_plan(ops, dims, Ci):
    """(steps, groups, steps per group, busy groups, steps of the last busy group) of micf_head_tail_bwd_weight_fused: the groups read
    off the workspace it asks for (groups * 36 slabs of 3 * Ci / 16 tiles of 256 floats + 48 dBf partials), the rest as its launch."""
    from micformer_amd import _lib
    B, Dc, Hc, Wc = dims
    need = int(_lib.lib.micf_head_tail_bwd_weight_fused_workspace(B, Dc, Hc, Wc, Ci))
    per_group = 36 * (3 * (Ci // 16) * 256 + 48)
    assert need > 0 and need % per_group == 0
    steps, groups = B * Dc * Hc * (Wc // 32), need // per_group
    spg = -(-steps // groups)
    busy = -(-steps // spg)
    return need, (steps, groups, spg, busy, steps - (busy - 1) * spg)


# (grid, Ci, ties, (steps, groups, steps per group, busy groups, steps of the last busy group))
WGRAD = [((1, 1, 4, 32), 96, False, (4, 4, 1, 4, 1)),
         ((1, 1, 4, 32), 96, True, (4, 4, 1, 4, 1)),              # x and dy of exact rounding ties
         ((1, 11, 4, 32), 96, False, (44, 42, 2, 22, 2)),         # 20 empty groups
         ((2, 11, 4, 32), 96, False, (88, 42, 3, 30, 1)),         # a short last group, 12 empty ones, two samples
         ((1, 2, 4, 64), 192, False, (16, 16, 1, 16, 1))]         # the second instantiation


@pytest.mark.parametrize("dims,Ci,tie,plan", WGRAD)
def test_weight_gradient(bf16, dims, Ci, tie, plan):
    ops = bf16
    need, got_plan = wgrad_plan(ops, dims, Ci)
    assert got_plan == plan, (got_plan, plan)
    rep = Report(f"head weight gradient {dims}, Ci {Ci}" + (", ties" if tie else "") + f": steps {plan[0]}, groups {plan[1]} x {plan[2]} steps, {plan[3]} busy, last one {plan[4]}")
    x, _, _, _, dy = inputs(dims, Ci, tie)
    cx, cdy = dev(x), dev(dy)
    ops.scratch(cx.device, need).fill_(math.nan)           # a partial row that is read but never written then shows up
    got = ops.head_tail_bwd_weight_fused(cdy, cx, dims, P)
    assert got is not None
    rw, rbf = H.head_bwd_weight(dy, x, dims)
    rep.add("dWb", got[0], rw, "bf16")
    rep.add("dBf (unrounded dy)", got[1], rbf, "both")
    rep.done()


def test_weight_gradient_falls_back_at_wc_48(bf16):
    """Wc = 48 is no multiple of the 32-voxel step: no workspace, no fused kernel, and HeadTailFn.backward takes head_tail_im2col +
    linear_bwd_weight instead.  That GEMM (M = 384 tokens, N = 1728, K = 96: no a2, no a_gelu, N, K >= 48, M >= 64, M % 16 == 0) is
    linear.hip's LDS-DMA core, which rounds both operands at the fragment read: the SAME rounded dy and x, so the bf16 referee."""
    from micformer_amd import _lib
    ops = bf16
    dims, Ci = (1, 2, 4, 48), 96
    x, wb, _, _, dy = inputs(dims, Ci)
    cx, cdy = dev(x), dev(dy)
    assert ops.head_tail_fused_supported(dims, Ci, CO, P)                          # (forward and data gradient do cover it)
    assert int(_lib.lib.micf_head_tail_bwd_weight_fused_workspace(*dims, Ci)) == 0
    assert ops.head_tail_bwd_weight_fused(cdy, cx, dims, P) is None
    rep = Report(f"head weight gradient {dims}, Ci {Ci}: the im2col fallback")
    u = ops.head_tail_im2col(cdy, dims, P)
    assert torch.equal(u.cpu(), H.unfold(dy, dims))
    dwb, dbf = torch.zeros(H.ROWS, Ci, device="cuda"), torch.zeros(H.ROWS, device="cuda")
    ops.linear_bwd_weight(u, cx, dwb, dbf)
    rw, rbf = H.head_bwd_weight(dy, x, dims)
    rep.add("dWb (im2col + linear_bwd_weight)", dwb, rw, "bf16")
    rep.add("dBf", dbf, rbf, "both")
    rep.done()


# ============================================================================= the loss sums in the logits store
@pytest.mark.parametrize("dims,nparts", [((1, 1, 4, 16), 1), ((3, 11, 4, 16), 33), ((2, 13, 4, 80), 130)])
@pytest.mark.parametrize("label", [False, True])
def test_fused_loss(bf16, dims, nparts, label):
    """micf_head_tail_fwd_loss_fused at 1, 33 and 130 partial rows (dice_bce_finish_kernel: lane 0 alone; its tail loop from row 0; one
    round of the four-accumulator loop, then the tail loop from row 128): logits bit-equal to micf_head_tail_fwd_fused, the 32 sums and
    the loss against float64 of loss_terms.h's quantities on the kernel's OWN logits -- the tolerances of
    test_loss_sums_in_the_head_logits_store for unsaturated logits."""
    from micformer_amd import _lib
    ops = bf16
    B, Dc, Hc, Wc = dims
    Ci = 96
    assert int(_lib.lib.micf_head_tail_loss_parts(B, Dc, Hc, Wc)) == nparts
    x, wb, bf, b_out = rnd((B * Dc * Hc * Wc, Ci), 1, 0.5), rnd((H.ROWS, Ci), 2, Ci ** -0.5), rnd((H.ROWS,), 3, 0.2), rnd((CO,), 4)
    lab = torch.randint(0, CO, (B, P * Dc, P * Hc, P * Wc), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    onehot = torch.nn.functional.one_hot(lab.long(), CO).permute(0, 4, 1, 2, 3).float().contiguous()
    pf, _ = ops.head_tail_pack(dev(wb), dev(bf), dev(b_out), P)
    cx = dev(x)
    y0 = ops.head_tail_fwd_fused(cx, pf, dims, CO, P)
    y1, loss, sums = ops.head_tail_fwd_loss_fused(cx, pf, dims, CO, P, dev(lab) if label else dev(onehot))
    assert torch.equal(y0, y1)
    z, t = y1.cpu().double(), onehot.double()
    assert float(z.abs().max()) < 15.0                                             # (unsaturated: 1 - p well inside fp32)
    p = torch.sigmoid(z)
    bce = -(t * torch.log(p).clamp_min(-100.0) + (1.0 - t) * torch.log1p(-p).clamp_min(-100.0))
    want = torch.stack([(p * t).sum((0, 2, 3, 4)), (p * p).sum((0, 2, 3, 4)), (t * t).sum((0, 2, 3, 4)), bce.sum((0, 2, 3, 4))], 1)   # [class][4]
    count = B * 64.0 * Dc * Hc * Wc
    want_loss = float((0.7 * (1.0 - (2.0 * want[:, 0] + 1.0) / (want[:, 1] + want[:, 2] + 1.0)).sum() + 0.3 * (want[:, 3] / count).sum()) / 8.0)
    tol = 2e-5
    err, scale = float((sums.cpu().reshape(CO, 4) - want).abs().max()), float(want.abs().max())
    print(f"\nfused loss {dims}, {'class map' if label else 'one-hot planes'}, {nparts} partial rows: sums max abs err {err:.3e} "
          f"(gate {tol * scale:.3e}), loss {float(loss):.7f} against {want_loss:.7f} (gate {0.1 * tol * max(1.0, abs(want_loss)):.1e})")
    assert err <= tol * scale
    assert abs(float(loss) - want_loss) <= 0.1 * tol * max(1.0, abs(want_loss))


# ============================================================================= the sliding-window form
def test_sliding_window_form(bf16):
    """micf_head_tail_fwd_fused_sw on the three windows of test_fused_head_sliding_window_form (overlapping windows, an origin off every
    alignment, two volume samples): exact visit counts, and the accumulated volume against the referee's per-window logits added in
    float64 -- gate 1, and gate 2 with `terms` doubled where two windows overlap (their two sums and the add that joins them)."""
    ops = bf16
    n, Dc, Hc, Wc, Ci = 3, 4, 8, 16, 96
    dims = (n, Dc, Hc, Wc)
    VB, VD, VH, VW = 2, 24, 40, 72
    origins = [(0, 0, 0, 0), (0, 8, 4, 3), (1, 8, 8, 8)]
    x, wb, bf, b_out, _ = inputs(dims, Ci)
    ref = H.head_fwd(x, wb, bf, b_out, dims)                                       # (a window is a batch entry: its halo stops at its faces)
    vol = [torch.zeros(VB, CO, VD, VH, VW, dtype=torch.float64) for _ in range(3)]
    count = torch.zeros(VB, VD, VH, VW, dtype=torch.float64)
    for w, (s, z0, y0, x0) in enumerate(origins):
        box = (slice(z0, z0 + P * Dc), slice(y0, y0 + P * Hc), slice(x0, x0 + P * Wc))
        for v, src in zip(vol, (ref.want, ref.want32, ref.absdot)):
            v[(s, slice(None)) + box] += src[w]
        count[(s,) + box] += 1.0
    assert float(count.max()) == 2.0
    pf, _ = ops.head_tail_pack(dev(wb), dev(bf), dev(b_out), P)
    out, cnt = torch.zeros(VB, CO, VD, VH, VW, device="cuda"), torch.zeros(VB, VD, VH, VW, device="cuda")
    ops.head_tail_fwd_fused_sw(dev(x), pf, out, cnt, dev(torch.tensor(origins, dtype=torch.int32)), dims, CO, P)
    assert torch.equal(cnt.cpu().double(), count)
    rep = Report(f"head, sliding-window form: {n} windows of {(Dc, Hc, Wc)} into {(VB, VD, VH, VW)}")
    rep.add("accumulated volume", out, R.Ref(vol[0], vol[1], vol[2], ref.terms * count[:, None]), "bf16")
    rep.done()
