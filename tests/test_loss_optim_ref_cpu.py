"""tests/loss_optim_ref.py on the CPU: the float64 referee of test_gpu_loss_optim_edges.py states the right maps, and its gates
separate right from wrong.

1. The referee against the oracle, outside the two bands of its docstring: the loss (and float64 autograd of a float64
   restatement for the gradient) agrees with R.mdice_loss; dice_metric, argmax / meandice and adam with their oracle
   counterparts; adam also with torch.optim.Adam in float64, cosine_lr with CosineAnnealingLR, bf16_rne with torch's conversion.
2. The gates pass an honest fp32 evaluation -- the fp32 CPU oracle -- on every input set the GPU tests use.  This is the
   condition under which a derived bound may stand.
3. The gates fail wrong results: one dropped element, one dropped float4, a dropped chunk tail, the last chunk not cut at V, a
   label compared with ch + 1; bc2 where sqrt(bc2) belongs, the lr of `step` where `step - 1` belongs, grad_scale applied after the
   moments, a truncating bf16 mirror, a mirror of the old p.  Each wrong result is an honest fp32 evaluation with that one defect.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_optim_ref as L
import test_gpu_loss_optim_edges as E
from oracle import micformer_ref as R


def near(got, want, what, rel):
    err = float((L.f64(got) - L.f64(want)).abs().max())
    scale = float(L.f64(want).abs().max())
    assert err <= rel * scale + 1e-300, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


# ----------------------------------------------------------------------------- 1. the referee against the oracle
def loss64(z, t):
    """R.mdice_loss restated in float64 (p never rounded to fp32: agrees with the referee to fp32 rounding outside the bands)."""
    p = torch.sigmoid(z)
    d = (0, 2)
    dice = 1.0 - (2.0 * (p * t).sum(d) + 1.0) / ((p * p).sum(d) + (t * t).sum(d) + 1.0)
    bce = -(t * torch.log(p).clamp_min(-100.0) + (1 - t) * torch.log(1 - p).clamp_min(-100.0)).mean(d)
    return (0.7 * dice.sum() + 0.3 * bce.sum()) / z.shape[1]


@pytest.mark.parametrize("V", [255, 1028, 32772])
def test_loss_reference_against_the_oracle(V):
    z, lab = L.loss_inputs(2, 3, V, seed=V)
    hot = L.one_hot(lab, 3)
    ref = L.dice_sums(z, lab)
    assert torch.equal(ref.sums, L.dice_sums(z, hot).sums)                       # class map == one-hot planes
    want = float(L.dice_loss(ref.sums, 2 * V))
    assert abs(want - float(R.mdice_loss(z, hot))) <= 1e-6 * want                # fp32 oracle: fp32 rounding
    assert abs(float(L.dice_val_loss(ref.sums)) - float(R.mdice_val_loss(z, hot))) <= 1e-6
    z64 = z.double().requires_grad_(True)
    l64 = loss64(z64, hot.double())
    assert abs(want - float(l64.detach())) <= 1e-7 * want                                 # float64 restatement: the rounding of p32
    for g in (1.0, 0.37):
        g64, = torch.autograd.grad(g * l64, z64, retain_graph=True)
        dz, bound = L.dice_bce_grad(z, hot, ref.sums, g)
        near(dz, g64, f"V={V} g={g}: written-out gradient vs float64 autograd", rel=1e-6)
        assert L.ratio(g64, dz, bound) <= 1.0                                    # ... and well inside its own fp32 bound
    zr = z.clone().requires_grad_(True)
    g32, = torch.autograd.grad(R.mdice_loss(zr, hot), zr)
    near(g32, L.dice_bce_grad(z, hot, ref.sums)[0], f"V={V}: fp32 oracle autograd", rel=1e-5)


def test_loss_reference_at_the_saturation_points():
    """Where p32 is exactly 0 or 1, or safely normal, the terms are 0, |z| or the clamp 100, the fp32 oracle agrees, and the gradient
    is exactly 0 where ATen's is."""
    z = torch.tensor(L.SAT + L.SAT).reshape(1, 1, 20)
    t = torch.cat([torch.zeros(10), torch.ones(10)]).reshape(1, 1, 20)
    term, w = L.bce_terms(L.p32(z), t.double())
    want = torch.tensor([100, 0, 100, 0, 100, 0, 100, 0, 100, 0, 0, 20, 0, 40, 0, 80, 0, 100, 0, 100.0], dtype=torch.float64)
    assert float((term.reshape(-1) - want).abs().max()) <= 1e-7 and bool(torch.isfinite(w).all())
    cpu = F.binary_cross_entropy(torch.sigmoid(z), t, reduction="none").reshape(-1)
    assert float((cpu.double() - want).abs().max()) <= 1e-5
    zr = z.clone().requires_grad_(True)
    g32, = torch.autograd.grad(R.mdice_loss(zr, t), zr)
    dz, bound = L.dice_bce_grad(z, t, L.dice_sums(z, t).sums)
    sat = (L.p32(z) == 0) | (L.p32(z) == 1)
    assert int(sat.sum()) == 14 and bool((dz[sat] == 0).all()) and bool((g32[sat] == 0).all()) and bool((bound[sat] == 0).all())
    assert L.ratio(g32, dz, bound) <= 1.0


def test_bands_are_where_two_fp32_evaluations_part():
    """The reason for the bands: inside them the correctly rounded p32 and ATen's fp32 sigmoid give BCE terms that differ by far more
    than any rounding bound; just outside they agree."""
    zi = torch.tensor([16.5, 16.64, 16.7, 17.0]).reshape(1, 1, -1)
    t0 = torch.zeros_like(zi)
    ref, _ = L.bce_terms(L.p32(zi), t0.double())
    cpu = F.binary_cross_entropy(torch.sigmoid(zi), t0, reduction="none").double()
    print("\nband (13, 17.5), t = 0: referee", ref.reshape(-1).tolist(), "fp32 CPU", cpu.reshape(-1).tolist())
    assert bool(L.in_bands(zi).all()) and bool(L.in_bands(torch.tensor([-95.0, -88.0, -103.0])).all())
    assert not bool(L.in_bands(torch.tensor(L.SAT + (9.0, -9.0, 13.0, 17.5, -87.0, -104.0))).any())
    zo = torch.tensor([12.9, 17.6, 20.0]).reshape(1, 1, -1)
    ref, w = L.bce_terms(L.p32(zo), torch.zeros_like(zo).double())
    cpu = F.binary_cross_entropy(torch.sigmoid(zo), torch.zeros_like(zo), reduction="none").double()
    assert bool(((ref - cpu).abs() <= L.K_ULP * w + 8 * L.U * ref.abs()).all())


@pytest.mark.parametrize("V", [1, 255, 65537])
def test_metric_reference_against_the_oracle(V):
    """Equal to R.dice_metric away from the threshold.  At 0 < z < 1.5 * 2^-24 = 8.9e-8 (ATen's CPU sigmoid; below 1.2e-7 for any
    fp32 sigmoid) the oracle's sigmoid(z) > 0.5 is false and the rule z > 0 -- the kernel's, pinned by the GPU test -- is true: the
    divergence band recorded in ops.dice_metric's docstring."""
    z, lab = E.metric_inputs(2, 3, V, seed=V)
    want = L.dice_metric(z, lab)
    assert torch.equal(want, L.dice_metric(z, L.one_hot(lab, 3)))
    zc = z.clone()
    zc[(zc > 0) & (zc < 1e-6)] = -1.0                       # move the band's points to the side the oracle puts them on
    assert float((L.dice_metric(zc, lab) - R.dice_metric(zc, L.one_hot(lab, 3))).abs().max()) <= 6e-8
    tiny = torch.tensor([1e-30, 2.0 ** -24, 8e-8])
    assert not bool((torch.sigmoid(tiny) > 0.5).any()) and bool((tiny > 0).all())
    assert bool((torch.sigmoid(torch.tensor([2.0 ** -22, 1.3e-7])) > 0.5).all())


@pytest.mark.parametrize("k,V", [(1, 300), (2, 777), (8, 1001), (32, 515)])
def test_argmax_reference_against_the_oracle(k, V):
    z, lab = E.argmax_inputs(2, k, V, seed=k)
    mask, counts, md = L.argmax_counts(z, lab, k)
    assert torch.equal(mask, R.argmax_mask(z))
    assert int(counts[0].sum()) == 2 * V and int(counts[1].sum()) == int((lab < k).sum())
    for c in range(k):
        assert int(counts[2, c]) == int(((mask == c) & (lab.long() == c)).sum())
    if k > 1:
        assert abs(md - float(R.meandice(mask, lab.long(), k))) <= 1e-12


def test_adam_reference_against_torch_optim():
    n, t_max = 257, 10
    p, g, m, v = L.adam_inputs(n, seed=1)
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([w], lr=E.BASE_LR, betas=(0.9, 0.999), eps=1e-8)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=t_max, eta_min=1e-6)
    pp, mm, vv = p.double(), m.double(), v.double()
    for step in range(1, 14):
        gs = (L.rnd(n, seed=step) * 1e-3).double()
        lr = L.cosine_lr(E.BASE_LR, step - 1, t_max, 1e-6)
        assert abs(lr - opt.param_groups[0]["lr"]) <= 1e-15 * E.BASE_LR if step <= t_max + 1 else True
        assert abs(lr - R.cosine_lr(E.BASE_LR, step - 1, t_max, 1e-6)) <= 1e-18
        w.grad = gs.clone()
        if step <= t_max + 1:
            pp, mm, vv = L.adam(pp, gs, mm, vv, step, lr)
            opt.step()
            sched.step()
            near(pp, w.detach(), f"step {step}: p vs torch.optim.Adam", rel=1e-13)
            st = opt.state[w]
            near(mm, st["exp_avg"], "m", rel=1e-13)
            near(vv, st["exp_avg_sq"], "v", rel=1e-13)
    # grad_scale: scaling the gradient first is the same step; the oracle in float64 agrees
    a = L.adam(p, g, m, v, 3, 1e-3, 0.5, 0.9, 1e-8, 0.125)
    b = R.adam_update(p.double(), g.double() * 0.125, m.double(), v.double(), 3, 1e-3, 0.5, 0.9, 1e-8)
    for x, y in zip(a, b):
        near(x, y, "adam vs the oracle in float64", rel=1e-14)


def test_bf16_rne_is_torchs_conversion():
    x = torch.cat([L.rnd(4096, seed=1) * 10 ** L.rnd(4096, seed=2), L.bf16_ties(64, seed=3), torch.tensor([0.0, -0.0, 1.0, 3.0e38])])
    assert torch.equal(L.bf16_rne(x), L.bf16_bits(x.to(torch.bfloat16)))
    ties = L.bf16_ties(64, seed=4)
    bits = ties.view(torch.int32).long() & 0xFFFFFFFF
    assert bool(((bits & 0xFFFF) == 0x8000).all())
    up = ((bits >> 16) & 1) == 1                              # odd kept lsb: up; even: down
    assert torch.equal(L.bf16_rne(ties), (bits >> 16) + up.long()) and 0 < int(up.sum()) < 64


# ----------------------------------------------------------------------------- 2. the gates pass the fp32 oracle
@pytest.mark.parametrize("V", E.FWD_V)
def test_forward_and_backward_gates_pass_the_fp32_oracle(V):
    z, lab, hot, ref, oracle = E.loss_case(V)
    r = L.sums_ratio(oracle, ref, L.fwd_terms(V))
    assert r <= 1.0, f"V={V}: the fp32 oracle's sums are {r:.3g} of the bound"
    lb = L.dice_loss_bound(ref.sums, ref.bound(L.fwd_terms(V)), 2 * V)
    assert abs(float(R.mdice_loss(z, hot)) - float(L.dice_loss(ref.sums, 2 * V))) <= lb
    for g in (1.0, L.f32(0.37)):
        want, bound = L.dice_bce_grad(z, hot, ref.sums, g)
        rg = L.ratio(E.oracle_grad(z, hot, ref.sums, g), want, bound)
        assert rg <= 1.0, f"V={V} g={g}: the fp32 evaluation's dz is {rg:.3g} of the bound"
    print(f"\nV={V}: fp32 oracle sums {r:.3g}, dz {rg:.3g} of the bound")


def test_gates_pass_the_fp32_oracle_at_the_class_count_cases():
    for what, z, target, hot, V in E.class_count_cases():
        ref = L.dice_sums(z, target)
        assert torch.equal(ref.sums, L.dice_sums(z, hot).sums)
        assert L.sums_ratio(E.oracle_sums(z, hot), ref, L.fwd_terms(V)) <= 1.0, what
        want, bound = L.dice_bce_grad(z, hot, ref.sums, 1.0)
        assert L.ratio(E.oracle_grad(z, hot, ref.sums, 1.0), want, bound) <= 1.0, what


def test_backward_gate_passes_fp32_past_the_block_cap():
    V = E.BWD_BIG_V
    z, _ = L.loss_inputs(1, 1, V, seed=11)
    hot = (L.rnd(1, 1, V, seed=12) > 0).float()
    ref = L.dice_sums(z, hot)
    want, bound = L.dice_bce_grad(z, hot, ref.sums, L.f32(0.37))
    assert L.ratio(E.oracle_grad(z, hot, ref.sums, L.f32(0.37)), want, bound) <= 1.0


def adam_sets():
    """(what, inputs, step, betas, grad_scale) of every Adam step the GPU tests take (the second step's state is the referee's)."""
    for n in E.ADAM_N:
        for b1, b2, gs in E.ADAM_CONFIGS:
            yield f"n={n} cold", L.adam_inputs(n, seed=n), 1, L.f32(b1), L.f32(b2), gs
            yield f"n={n} warm", L.adam_inputs(n, seed=n + 20, warm=True), 100001, L.f32(b1), L.f32(b2), gs
    for n in (2052, 1029, 1031):
        yield f"n={n} mirror", L.adam_inputs(n, seed=n, warm=True), 4, L.f32(0.9), L.f32(0.999), 1.0
    for lo in (4, 1028):
        yield f"slice [{lo}:{lo + 1501}]", tuple(t[lo:lo + 1501] for t in L.adam_inputs(4000, seed=lo, warm=True)), 1, L.f32(0.9), L.f32(0.999), 1.0


def adam32(p, g, m, v, step, lr, b1, b2, eps, gscale, defect=None):
    """adam_step_kernel's arithmetic in fp32 on the CPU (the lerp form, bc1 / sqrt(bc2) / lr / bc1 rounded to fp32), with one
    optional defect."""
    f = torch.float32
    bc1 = torch.tensor(1.0 - b1 ** step, dtype=f)
    bc2 = 1.0 - b2 ** step
    bc2s = torch.tensor(bc2 if defect == "bc2" else math.sqrt(bc2), dtype=f)
    ss = torch.tensor(lr / float(bc1), dtype=f)
    gs = g if defect == "gscale_late" else g * torch.tensor(gscale, dtype=f)
    m1 = m + (gs - m) * torch.tensor(1.0 - b1, dtype=f)
    v1 = v * torch.tensor(b2, dtype=f) + torch.tensor(1.0 - b2, dtype=f) * gs * gs
    mh = m1 * torch.tensor(gscale, dtype=f) if defect == "gscale_late" else m1
    return p - ss * (mh / (v1.sqrt() / bc2s + torch.tensor(eps, dtype=f))), m1, v1


def adam_ratios(got, want, bounds):
    return [L.ratio(a, w, b) for a, w, b in zip(got, want, bounds)]


def test_adam_gates_pass_fp32_evaluations():
    worst = 0.0
    for what, (p, g, m, v), step, b1, b2, gs in adam_sets():
        lr = L.cosine_lr(E.BASE_LR, step - 1, E.T_MAX)
        want, bounds = L.adam(p, g, m, v, step, lr, b1, b2, E.EPS, gs, bounds=True)
        for name, got in (("oracle", E.oracle_adam(p, g, m, v, step, lr, b1, b2, gs)),
                          ("kernel form", adam32(p, g, m, v, step, lr, b1, b2, E.EPS, gs))):
            r = adam_ratios(got, want, bounds)
            worst = max(worst, *r)
            assert max(r) <= 1.0, f"{what}: the fp32 {name} is {r} of the bounds (p, m, v)"
    print(f"\nworst fp32 error / bound over the Adam input sets: {worst:.3g}")


def test_adam_gate_passes_fp32_past_the_block_cap():
    p, g, m, v = L.adam_inputs(E.ADAM_BIG_N, seed=41, warm=True)
    lr = L.cosine_lr(E.BASE_LR, 6, E.T_MAX)
    want, bounds = L.adam(p, g, m, v, 7, lr, L.f32(0.9), L.f32(0.999), E.EPS, 0.125, bounds=True)
    assert max(adam_ratios(E.oracle_adam(p, g, m, v, 7, lr, L.f32(0.9), L.f32(0.999), 0.125), want, bounds)) <= 1.0


# ----------------------------------------------------------------------------- 3. the gates fail wrong results
def defective_sums(z, hot, keep=None, extra=None):
    """The fp32 oracle's sums over the elements keep [B, K, V] selects (+ extra [K, 4], what a kernel read that it should not)."""
    p = torch.sigmoid(z)
    k = torch.ones_like(z) if keep is None else keep
    d = (0, 2)
    s = torch.stack([(p * hot * k).sum(d), (p * p * k).sum(d), (hot * hot * k).sum(d),
                     (F.binary_cross_entropy(p, hot, reduction="none") * k).sum(d)], 1).double()
    return s if extra is None else s + extra


def chunk_ends(V):
    chunks, per = L.fwd_launch(V)
    return [(c * per, min((c + 1) * per, V)) for c in range(chunks)], per


@pytest.mark.parametrize("V", E.FWD_V)
def test_forward_gate_fails_a_dropped_element(V):
    """The same voxel dropped in every plane, as a kernel that skips an index does: it carries t = 1 in one plane, so the exact T2
    fails whatever its p; for V <= 1028 the voxel's own terms exceed the rounding bound as well."""
    z, lab, hot, ref, _ = E.loss_case(V)
    for vx in (0, V - 1, V // 2):
        keep = torch.ones_like(z)
        keep[:, :, vx] = 0
        assert L.sums_ratio(defective_sums(z, hot, keep), ref, L.fwd_terms(V)) > 1.0
        if V <= 1028:
            got = defective_sums(z, hot, keep)
            got[:, 2] = ref.sums[:, 2]                           # even with the count repaired
            assert L.sums_ratio(got, ref, L.fwd_terms(V)) > 1.0, f"V={V} voxel {vx}"


@pytest.mark.parametrize("V", [4, 1024, 1028, 32768, 65544])
def test_forward_gate_fails_a_dropped_float4(V):
    z, lab, hot, ref, _ = E.loss_case(V)
    ends, _ = chunk_ends(V)
    for lo, hi in ends:
        keep = torch.ones_like(z)
        keep[:, :, hi - 4:hi] = 0                                # the chunk's last float4
        assert L.sums_ratio(defective_sums(z, hot, keep), ref, L.fwd_terms(V)) > 1.0


@pytest.mark.parametrize("V", [1028, 65544])
def test_forward_gate_fails_a_dropped_chunk_tail(V):
    """The last per % 1024 elements of every chunk (4 at V = 1028, 344 at V = 65544): a double-load loop without its tail loop."""
    z, lab, hot, ref, _ = E.loss_case(V)
    ends, per = chunk_ends(V)
    assert per % 1024 in (4, 344)
    keep = torch.ones_like(z)
    for lo, hi in ends:
        keep[:, :, hi - per % 1024:hi] = 0
    got = defective_sums(z, hot, keep)
    assert L.sums_ratio(got, ref, L.fwd_terms(V)) > 1.0
    got[:, 2] = ref.sums[:, 2]
    assert L.sums_ratio(got, ref, L.fwd_terms(V)) > 1.0          # I, P2, S alone show it too


def test_forward_gate_fails_a_last_chunk_not_cut_at_v():
    """V = 65542: 3 chunks of per = 21848 end at 65544, two elements into the next plane."""
    V = 65542
    z, lab, hot, ref, _ = E.loss_case(V)
    chunks, per = L.fwd_launch(V)
    over = chunks * per - V
    assert over == 2
    zf, tf = z.reshape(-1, V), hot.reshape(-1, V)
    extra = torch.zeros(3, 4, dtype=torch.float64)
    for plane in range(zf.shape[0] - 1):                         # (past the last plane is past the buffer: not modelled)
        s = L.dice_sums(zf[plane + 1, :over].reshape(1, 1, -1), tf[plane + 1, :over].reshape(1, 1, -1)).sums
        extra[plane % 3] += s[0]
    assert L.sums_ratio(defective_sums(z, hot, extra=extra), ref, L.fwd_terms(V)) > 1.0


@pytest.mark.parametrize("V", [255, 32772, 65541])
def test_forward_gate_fails_a_label_compared_with_the_next_class(V):
    z, lab, hot, ref, _ = E.loss_case(V)
    wrong = L.one_hot(lab, 4)[:, 1:]                             # t = (label == ch + 1)
    assert L.sums_ratio(defective_sums(z, wrong), ref, L.fwd_terms(V)) > 1.0


def test_backward_gate_fails_an_unwritten_or_shifted_element():
    z, lab, hot, ref, _ = E.loss_case(1028)
    want, bound = L.dice_bce_grad(z, hot, ref.sums, 1.0)
    got = E.oracle_grad(z, hot, ref.sums, 1.0)
    assert L.ratio(got, want, bound) <= 1.0
    for vx in (21, 1027, 500):                                  # (voxels 0..19 are saturation points: dz = 0 there)
        bad = got.clone()
        bad[1, 2, vx] = 0.0
        assert L.ratio(bad, want, bound) > 1.0
    assert L.ratio(E.oracle_grad(z, L.one_hot(lab, 4)[:, 1:], ref.sums, 1.0), want, bound) > 1.0
    assert L.ratio(got * 0.37, want, bound) > 1.0                # grad_out dropped


@pytest.mark.parametrize("defect", ["bc2", "lr", "gscale_late"])
def test_adam_gates_fail_wrong_updates(defect):
    """On the GPU tests' own input sets: each defect fails the gate at the steps named in the assertion."""
    hits = 0
    for what, (p, g, m, v), step, b1, b2, gs in adam_sets():
        if p.numel() < 3:
            continue
        lr = L.cosine_lr(E.BASE_LR, step - 1, E.T_MAX)
        want, bounds = L.adam(p, g, m, v, step, lr, b1, b2, E.EPS, gs, bounds=True)
        lr_used = L.cosine_lr(E.BASE_LR, step, E.T_MAX) if defect == "lr" else lr
        r = adam_ratios(adam32(p, g, m, v, step, lr_used, b1, b2, E.EPS, gs, defect), want, bounds)
        if defect == "gscale_late" and gs == 1.0:
            assert max(r) <= 1.0                                # (no defect at grad_scale 1: the case needs 0.125)
            continue
        if defect == "bc2" and step > 1000:
            assert max(r) <= 1.0                                # (bc2 = sqrt(bc2) = 1 once beta2^step has vanished: needs step 1, 2)
            continue
        if defect == "lr" and step > 1000:
            continue                                            # (cos has period 2 t_max = 20: steps 100 000 and 100 001 differ, checked below)
        assert max(r) > 1.0, f"{defect} passes on {what}: {r}"
        hits += 1
    assert hits >= 10
    if defect == "lr":                                          # the lr of scheduler epoch 100 001 where 100 000 belongs
        p, g, m, v = L.adam_inputs(1025, seed=1045, warm=True)
        lr, wrong = L.cosine_lr(E.BASE_LR, 100000, E.T_MAX), L.cosine_lr(E.BASE_LR, 100001, E.T_MAX)
        want, bounds = L.adam(p, g, m, v, 100001, lr, L.f32(0.9), L.f32(0.999), E.EPS, 1.0, bounds=True)
        assert max(adam_ratios(adam32(p, g, m, v, 100001, wrong, L.f32(0.9), L.f32(0.999), E.EPS, 1.0), want, bounds)) > 1.0


def test_mirror_gate_fails_truncation_and_the_old_p():
    n = 1031
    p, g, m, v = L.adam_inputs(n, seed=n, warm=True)
    ties = L.bf16_ties(67, seed=n)
    where = torch.cat([torch.arange(64), torch.arange(n - 3, n)])
    p[where] = ties
    g[where], m[where], v[where] = 0.0, 0.0, 0.0
    new = adam32(p, g, m, v, 4, L.cosine_lr(E.BASE_LR, 3, E.T_MAX), L.f32(0.9), L.f32(0.999), E.EPS, 1.0)[0]
    assert torch.equal(new[where], ties)
    right = L.bf16_rne(new)
    trunc = (new.view(torch.int32).long() & 0xFFFFFFFF) >> 16
    assert not torch.equal(trunc, right) and not torch.equal(trunc[where], right[where])   # the odd ties alone show it
    assert not torch.equal(L.bf16_rne(p), right)                                           # a mirror of the old p
    # round-half-up (ties away from even) is caught by the even ties only
    half_up = ((new.view(torch.int32).long() & 0xFFFFFFFF) + 0x8000) >> 16
    assert not torch.equal(half_up[where], right[where])
