"""tests/head_ref.py on the CPU: the referee of the patch-matrix-free head states the right map (the two torch convolutions and their
autograd, float64), its two gates (bf16_ref.check) pass an honest fp32-accumulating evaluation of the rounded operands in another
summation order, and FAIL each fault that head_tail_fused.hip can have without the 6e-3 / 8e-3-of-the-maximum gates of
test_head_tail_without_patch_matrices noticing: a wrong conversion, a dropped neighbour slab, a bias counted for an out-of-volume
neighbour or carried without its lo half, b_out in a second slab, a one-voxel chunk of the dy halo dropped, a reduction step dropped,
a halo that crosses the batch boundary, dBf from the rounded dy, a silent fp32 product.

The emulation evaluates the map on a coarse grid with one ring of PHANTOM voxels (x = 0, bias column 0): the kernel's out-of-volume
halo rows.  A phantom at q = -1 reaches the fine voxels u = 4 q - 1 + f >= 0 only through f = 5, i.e. the neighbour slab d = -1 of the
voxel next to it -- so a neighbour slab d is the set of taps f with f = 5 (d = -1), 1..4 (d = 0), 0 (d = +1) per axis.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import head_ref as H

FACES = (2, 1, 4, 16)          # every coarse voxel on a face, every corner, two samples
INNER = (1, 3, 8, 32)          # interior tiles along all three axes, two 16-wide w tiles, 24 reduction steps of 32 tokens
CI = 16


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def inputs(dims, tie=False, ci=CI):
    B, Dc, Hc, Wc = dims
    T = B * Dc * Hc * Wc
    if tie:
        x, wb, dy = R.ties(T, ci, seed=1), R.ties(H.ROWS, ci, seed=2, scale=ci ** -0.5), R.ties(B, 8, 4 * Dc, 4 * Hc, 4 * Wc, seed=5)
    else:
        x, wb, dy = rnd(T, ci, seed=1), rnd(H.ROWS, ci, seed=2, scale=ci ** -0.5), rnd(B, 8, 4 * Dc, 4 * Hc, 4 * Wc, seed=5)
    return x, wb, rnd(H.ROWS, seed=3, scale=0.2), rnd(8, seed=4), dy


def stacked(dims):
    """The grid with its samples stacked along depth: what a halo that ignores the batch boundary sees."""
    B, Dc, Hc, Wc = dims
    return (1, B * Dc, Hc, Wc)


# ----------------------------------------------------------------------------- the kernels' arithmetic, fp32, with planted faults
def emu_fwd(x, wb, bf, b_out, dims, conv=R.rb, drop_row=None, bias_oov=False, drop_lo=False, b_out_rows=None, leak=False):
    """fp32: [rb(x) | 1 | 1] [rb(Wb) | hi | lo]^T on the grid with its phantom ring, then the overlap-add.  drop_row: a tap f whose rows
    are zeroed;  bias_oov: the phantoms' bias columns left at 1;  b_out_rows: the rows b_out is added to;  leak: samples stacked."""
    if leak:
        B, Dc = dims[0], dims[1]
        y = emu_fwd(x, wb, bf, b_out, stacked(dims), conv, drop_row, bias_oov, drop_lo, b_out_rows)
        return y.reshape(8, B, 4 * Dc, *y.shape[3:]).transpose(0, 1).contiguous()
    B, Dc, Hc, Wc = dims
    ci = x.shape[1]
    rows = H.centre_rows() if b_out_rows is None else b_out_rows
    v32 = bf.float() + torch.where(rows, b_out.float().repeat(216), torch.zeros(H.ROWS))
    hi = v32.bfloat16().float()
    lo = torch.zeros_like(hi) if drop_lo else (v32 - hi).bfloat16().float()
    wa = torch.cat([conv(wb).float(), hi[:, None], lo[:, None]], 1)
    if drop_row is not None:
        wa = wa.reshape(6, 6, 6, 8, ci + 2).clone()
        wa[drop_row] = 0.0
        wa = wa.reshape(H.ROWS, ci + 2)
    xp = torch.zeros(B, Dc + 2, Hc + 2, Wc + 2, ci + 2)
    if bias_oov:
        xp[..., ci:] = 1.0
    xp[:, 1:-1, 1:-1, 1:-1, :ci] = conv(x).float().reshape(B, Dc, Hc, Wc, ci)
    xp[:, 1:-1, 1:-1, 1:-1, ci:] = 1.0
    y = H.fold(xp.reshape(-1, ci + 2) @ wa.t(), (B, Dc + 2, Hc + 2, Wc + 2))
    return y[:, :, 4:-4, 4:-4, 4:-4].contiguous()


def emu_unfold(dy, dims, conv=R.rb, drop_w=None, leak=False):
    """fp32 patch matrix of the converted dy.  drop_w: region voxel 0 (tap fw = 0 of a 16-voxel tile's first coarse voxel) or 65 (tap
    fw = 5 of its last) of the data gradient's 66-voxel halo zeroed;  leak: the depth halo read across the batch boundary."""
    B, Dc, Hc, Wc = dims
    g = conv(dy).float()
    if leak:
        u = H.unfold(g.transpose(0, 1).reshape(1, 8, B * 4 * Dc, 4 * Hc, 4 * Wc), stacked(dims))
    else:
        u = H.unfold(g, dims)
    u = u.reshape(B, Dc, Hc, Wc, 6, 6, 6, 8).clone()
    if drop_w == 0:
        u[:, :, :, 0::16, :, :, 0] = 0.0
    if drop_w == 65:
        u[:, :, :, 15::16, :, :, 5] = 0.0
    return u.reshape(-1, H.ROWS)


def exact(t):
    return t.double()


def report(rows):
    """rows: (name, got, Ref, referee, mutant): an honest `got` must match `referee`, a mutant must NOT (None or the other referee).
    Prints per row the worst ratio to each gate of the bf16 referee."""
    bad = []
    for name, got, ref, expect, mutant in rows:
        which, _ = R.match(got, ref)
        c = R.check(got, ref.want, ref.absdot, ref.terms)
        print(f"  {name:58s} gate 1: {c.worst / R.GATE_MAX:9.2e} x  gate 2: {c.ratio:9.2e} x  rel-L2 {c.l2:8.2e}  matches {which}")
        if mutant and which == expect:
            bad.append(f"{name}: the mutant matches {which}")
        if not mutant and which != expect:
            bad.append(f"{name}: matches {which}, must match {expect} (gate 1 {c.worst / R.GATE_MAX:.2e} x, gate 2 {c.ratio:.2e} x)")
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------- the referee states the right map
def compose(w_up, b_up, w_out):
    """Wb[(f, o), ci] = sum_{cm, p - t + 2 = f} w_out[o, cm, t] w_up[ci, cm, p] and Bf likewise from b_up, in the dtype given."""
    ci, cm = w_up.shape[0], w_up.shape[1]
    wb = F.conv3d(w_up, w_out, padding=2).permute(2, 3, 4, 1, 0).reshape(H.ROWS, ci)
    bf = F.conv3d(b_up.reshape(1, cm, 1, 1, 1).expand(1, cm, 4, 4, 4), w_out, padding=2)[0].permute(1, 2, 3, 0).reshape(H.ROWS)
    return wb, bf


@pytest.mark.parametrize("dims", [FACES, INNER])
def test_referee_states_the_composed_map_and_its_adjoints(dims):
    B, Dc, Hc, Wc = dims
    ci, cm = 6, 3
    g = torch.Generator().manual_seed(7)
    r64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = r64(B * Dc * Hc * Wc, ci).requires_grad_(True)
    w_up, b_up, w_out, b_out = (t.requires_grad_(True) for t in (r64(ci, cm, 4, 4, 4), r64(cm), r64(8, cm, 3, 3, 3), r64(8)))
    dy = r64(B, 8, 4 * Dc, 4 * Hc, 4 * Wc)
    xv = x.reshape(B, Dc, Hc, Wc, ci).permute(0, 4, 1, 2, 3)
    y = F.conv3d(F.conv_transpose3d(xv, w_up, b_up, stride=4), w_out, b_out, padding=1)
    gx, g_up, gb_up, g_out, gb_out = torch.autograd.grad(y, (x, w_up, b_up, w_out, b_out), dy)
    tiny = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())

    wb, bf = compose(w_up, b_up, w_out)
    ref = H.head_fwd(x, wb, bf, b_out, dims)
    assert ref.want32.shape == y.shape and ref.terms == 8 * (ci + 2)
    assert tiny(ref.want32, y.detach())
    assert tiny(H.head_bwd_data(dy, wb, dims).want32, gx)
    rw, rbf = H.head_bwd_weight(dy, x, dims)
    assert torch.equal(rbf.want, rbf.want32) and rw.terms == x.shape[0] + 50
    # the full adjoints, against autograd of torch's own transposed convolution with the composed kernel ...
    wt = wb.detach().reshape(6, 6, 6, 8, ci).permute(4, 3, 0, 1, 2).contiguous().requires_grad_(True)
    vt = torch.zeros(1, 8, 6, 6, 6, dtype=torch.float64, requires_grad=True)
    y2 = F.conv_transpose3d(xv.detach(), wt, stride=4, padding=1) + F.conv_transpose3d(torch.ones(B, 1, Dc, Hc, Wc, dtype=torch.float64), vt, stride=4, padding=1)
    gwt, gvt = torch.autograd.grad(y2, (wt, vt), dy)
    assert tiny(rw.want32, gwt.permute(2, 3, 4, 1, 0).reshape(H.ROWS, ci))
    assert tiny(rbf.want32, gvt[0].permute(1, 2, 3, 0).reshape(H.ROWS))
    # ... and, carried through the composition, against the two layers' own parameter gradients
    p_up, pb_up, p_out = torch.autograd.grad((wb * rw.want32).sum() + (bf * rbf.want32).sum(), (w_up, b_up, w_out))
    assert tiny(p_up, g_up) and tiny(pb_up, gb_up) and tiny(p_out, g_out)
    assert tiny((rbf.want32 * H.centre_rows()).reshape(216, 8).sum(0), gb_out)


def test_fold_and_unfold_are_adjoint_and_the_bias_rows_split_exactly():
    dims = (2, 2, 3, 5)
    t, dy = rnd(60, H.ROWS, seed=1).double(), rnd(2, 8, 8, 12, 20, seed=2).double()
    assert abs(float((H.fold(t, dims) * dy).sum() - (t * H.unfold(dy, dims)).sum())) < 1e-9
    bf, b_out = rnd(H.ROWS, seed=3), rnd(8, seed=4)
    v, hi, lo = H.bias_rows(bf, b_out)
    assert int(H.centre_rows().sum()) == 64 * 8
    assert torch.equal(hi, R.rb(v.float())) and float((v - hi - lo).abs().max()) <= 2.0 ** -17 * float(v.abs().max())
    assert float(lo.abs().max()) > 0
    # every fine voxel has exactly one centre neighbour, and 1, 2, 4 or 8 neighbours in all: b_out once, the pairs per neighbour
    ones = H.fold(torch.ones(60, H.ROWS, dtype=torch.float64) * H.centre_rows(), dims)
    assert torch.equal(ones, torch.ones_like(ones))
    assert sorted(H.fold(torch.ones(60, H.ROWS, dtype=torch.float64), dims).unique().tolist()) == [1.0, 2.0, 4.0, 8.0]


# ----------------------------------------------------------------------------- the gates: honest evaluations pass, mutants fail
@pytest.mark.parametrize("dims", [FACES, INNER])
@pytest.mark.parametrize("tie", [False, True])
def test_an_honest_evaluation_passes_both_gates(dims, tie):
    x, wb, bf, b_out, dy = inputs(dims, tie)
    rw, rbf = H.head_bwd_weight(dy, x, dims)
    print(f"\nhead {dims}, Ci {CI}" + (", ties" if tie else "") + ": honest fp32 evaluation, matmul + fold")
    u = emu_unfold(dy, dims)
    report([("logits", emu_fwd(x, wb, bf, b_out, dims), H.head_fwd(x, wb, bf, b_out, dims), "bf16", False),
            ("dx", u @ R.rb(wb).float(), H.head_bwd_data(dy, wb, dims), "bf16", False),
            ("dWb", u.t() @ R.rb(x).float(), rw, "bf16", False),
            ("dBf (unrounded dy)", emu_unfold(dy, dims, conv=exact).sum(0), rbf, "both", False)])


def test_the_bias_alone_is_the_referees_bias_term():
    """x = 0: the emulation's logits are sums of at most 8 exact hi + lo pairs, within 2^-22 of the maximum of bias_term."""
    x, wb, bf, b_out, _ = inputs(FACES)
    want = H.bias_term(bf, b_out, FACES)
    got = emu_fwd(torch.zeros_like(x), wb, bf, b_out, FACES).double()
    assert float((got - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert torch.equal(H.head_fwd(torch.zeros_like(x), wb, bf, b_out, FACES).want, want)


@pytest.mark.parametrize("dims", [FACES, INNER])
def test_every_mutant_fails_a_gate(dims):
    B, Dc, Hc, Wc = dims
    x, wb, bf, b_out, dy = inputs(dims)
    tx, twb, _, _, tdy = inputs(dims, tie=True)
    fwd, dxr = H.head_fwd(x, wb, bf, b_out, dims), H.head_bwd_data(dy, wb, dims)
    rw, rbf = H.head_bwd_weight(dy, x, dims)
    tfwd, tdx = H.head_fwd(tx, twb, bf, b_out, dims), H.head_bwd_data(tdy, twb, dims)
    trw, _ = H.head_bwd_weight(tdy, tx, dims)
    xr, wr = R.rb(x).float(), R.rb(wb).float()
    rows = []
    for name, conv in (("truncating conversion", R.truncate), ("half-away conversion", R.half_away)):
        u = emu_unfold(tdy, dims, conv=conv)
        rows += [(f"ties, {name}: logits", emu_fwd(tx, twb, bf, b_out, dims, conv=conv), tfwd, "bf16", True),
                 (f"ties, {name}: dx", u @ conv(twb).float(), tdx, "bf16", True),
                 (f"ties, {name}: dWb", u.t() @ conv(tx).float(), trw, "bf16", True)]
    wide = torch.zeros(6, 6, 6, 8, dtype=torch.bool)
    wide[1:5, 1:5, :] = True                                # b_out wherever dd == dh == 0: also the slabs dw = -1, +1
    rows += [("bias column 1 on out-of-volume halo rows", emu_fwd(x, wb, bf, b_out, dims, bias_oov=True), fwd, "bf16", True),
             ("bias without its lo half", emu_fwd(x, wb, bf, b_out, dims, drop_lo=True), fwd, "bf16", True),
             ("b_out in the slabs d = (0, 0, -1) and (0, 0, +1) too", emu_fwd(x, wb, bf, b_out, dims, b_out_rows=wide.reshape(-1)), fwd, "bf16", True),
             ("dBf from the rounded dy", emu_unfold(dy, dims).sum(0), rbf, "both", True)]
    if B > 1:
        rows += [("sample 1's halo reads sample 0: logits", emu_fwd(x, wb, bf, b_out, dims, leak=True), fwd, "bf16", True),
                 ("sample 1's halo reads sample 0: dx", emu_unfold(dy, dims, leak=True) @ wr, dxr, "bf16", True)]
    if Dc > 1:                                              # (a +1 neighbour along every axis exists)
        rows += [("neighbour d = (+1, +1, +1) dropped", emu_fwd(x, wb, bf, b_out, dims, drop_row=(0, 0, 0)), fwd, "bf16", True)]
    if Wc > 16:                                             # (a second 16-voxel tile along w: its halo voxels 0 / 65 are in the volume)
        u = emu_unfold(dy, dims)
        rows += [("dy halo voxel w = 0 dropped: dx", emu_unfold(dy, dims, drop_w=0) @ wr, dxr, "bf16", True),
                 ("dy halo voxel w = 65 dropped: dx", emu_unfold(dy, dims, drop_w=65) @ wr, dxr, "bf16", True),
                 ("last reduction step (32 tokens) dropped: dWb", u[:-32].t() @ xr[:-32], rw, "bf16", True)]
    # the fp32-operand results are the OTHER referee: never confusable with the bf16 one
    u32 = emu_unfold(dy, dims, conv=exact)
    rows += [("fp32 operands: logits", emu_fwd(x, wb, bf, b_out, dims, conv=exact), fwd, "bf16", True),
             ("fp32 operands: dx", u32 @ wb, dxr, "bf16", True), ("fp32 operands: dWb", u32.t() @ x, rw, "bf16", True)]
    print(f"\nhead {dims}, Ci {CI}: mutants against the bf16 referee (ratio to each gate; > 1 fails)")
    report(rows)
    assert R.match(u32 @ wb, dxr)[0] == "fp32" and R.match(u32.t() @ x, rw)[0] == "fp32"
    # (logits: this evaluation keeps the hi + lo pair, 2^-17 of v away from want32's unsplit v: inside both gates)
    assert R.match(emu_fwd(x, wb, bf, b_out, dims, conv=exact), fwd)[0] == "fp32" and R.check(emu_fwd(x, wb, bf, b_out, dims, conv=exact), fwd.want32, fwd.absdot, fwd.terms).ok
