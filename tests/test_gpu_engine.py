"""GPU tests of the step engine's contract with the reference's loop (train.py:183-207): one optimiser update and one
scheduler tick per batch also on the HIP-graph path (the capture warm-up must not train), ragged last batches, the LR written
into checkpoints, process-global launch switches scoped to the engine's own step, the HIP DropPath draw, label range guards."""
import os
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fill  # noqa: E402


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import micformer_amd.models.MICFormer_self as m
    return m


def _head(M, train=False):
    h = M.Head(embed_dim=24, num_classes=8, depths=(1, 1, 1, 1))
    with torch.no_grad():
        for name, t in h.state_dict().items():
            t.copy_(fill.fill_tensor(name, t))
    h = h.cuda()
    return h.train() if train else h.eval()


def _data(B, n=64):
    return fill.make_volume(B, n, n, n).cuda(), fill.one_hot(fill.make_label_map(B, n, n, n)).cuda()


def _same_training_state(a, b, what=""):
    """Two engines took the same number of the same updates.  The first Adam steps are lr * g / (|g| + eps): an element whose
    gradient is accumulation-order noise around 0 can land a whole 2 * lr apart, so the weights themselves are not compared;
    the update count is checked through the first moment (m = sum of (1 - b1) b1^k g over the updates
    taken: one extra update changes it by O(1) relative) and the device step counter."""
    assert int(a.adam_state[0].item()) == int(b.adam_state[0].item()), what
    ma, mb = a.flat_m, b.flat_m
    fin = torch.isfinite(ma) & torch.isfinite(mb)
    scale = float(ma[fin].abs().max())
    d = (ma - mb)[fin]
    # (as a whole and almost everywhere: the sampling coordinate's derivative is discontinuous at voxel boundaries, so a handful of
    # offset-head elements may sit O(1) apart between two runs that added their sums in another order -- bf16 mode, ~1 run in 7)
    assert scale > 0 and float(d.norm()) <= 3e-2 * float(ma[fin].norm()) and float((d.abs() > 3e-2 * scale).float().mean()) <= 1e-3, \
        f"{what}: Adam first moments differ"


def test_graph_capture_warmup_does_not_train(M):
    """the first step() of a graph engine used to apply 4 updates (3 warm-ups + the replay) and run the cosine
    schedule 3 ticks ahead.  Now: N graph steps == N eager steps, Adam's step counter == N, and the same again after a
    checkpoint load (which drops the captured graph)."""
    from micformer_amd.engine import TrainEngine
    x, t = _data(2)
    eager = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=False)
    graph = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=True)
    for n in (1, 2):
        le, lg = eager.step(x, t), graph.step(x, t)
        assert int(graph.adam_state[0].item()) == n == int(eager.adam_state[0].item())
        assert abs(float(le) - float(lg)) < 1e-4
        assert abs(graph.lr() - eager.lr()) < 1e-15
        _same_training_state(eager, graph, f"after {n} steps")
    assert graph.steps_done == 2
    ck = graph.checkpoint(epoch=0)
    graph.load_checkpoint(ck)                      # drops the graph: the next step re-captures (and must again not train)
    assert graph._graph is None
    le, lg = eager.step(x, t), graph.step(x, t)
    assert int(graph.adam_state[0].item()) == 3
    _same_training_state(eager, graph, "after reload + 1 step")


def test_ragged_last_batch_runs_eagerly(M):
    """a B=1 batch fed to a graph captured at B=2 was broadcast into the static buffers (the sample trained twice).
    The reference's loader has drop_last=False, so this happens at the end of every epoch."""
    from micformer_amd.engine import TrainEngine
    x2, t2 = _data(2)
    x1, t1 = x2[:1].contiguous(), t2[:1].contiguous()
    a = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=True)
    b = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=False)
    a.step(x2, t2), b.step(x2, t2)
    la, lb = a.step(x1, t1), b.step(x1, t1)        # graph engine: shape mismatch -> eager fallback
    assert abs(float(la) - float(lb)) < 1e-4
    _same_training_state(a, b, "after the ragged batch")
    la, lb = a.step(x2, t2), b.step(x2, t2)        # and the captured graph is still valid for the full batch
    assert abs(float(la) - float(lb)) < 1e-4
    assert int(a.adam_state[0].item()) == 3
    _same_training_state(a, b, "after the next full batch")


def test_checkpoint_lr_is_torchs_after_n_scheduler_steps(M):
    """after N iterations torch holds cosine(N) in param_groups[0]['lr'] and scheduler._last_lr (scheduler.step() has
    already run); the engine used to write cosine(N-1)."""
    from micformer_amd.engine import TrainEngine
    x, t = _data(1, 32)
    eng = TrainEngine(_head(M), base_lr=1e-3, t_max=7, use_graph=False)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=1e-3)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=7)
    assert abs(eng.optimizer_state_dict()["param_groups"][0]["lr"] - 1e-3) < 1e-18
    for n in range(1, 4):
        eng.step(x, t)
        p.grad = torch.ones(1)
        opt.step()
        sch.step()
        want = opt.param_groups[0]["lr"]
        assert abs(eng.optimizer_state_dict()["param_groups"][0]["lr"] - want) < 1e-12 * 1e3
        ssd = eng.scheduler_state_dict()
        assert abs(ssd["_last_lr"][0] - sch.state_dict()["_last_lr"][0]) < 1e-15 and ssd["last_epoch"] == sch.last_epoch == n
        # the rate the last optimiser step USED is the previous epoch's
        assert abs(eng.lr() - (0.5e-3 * (1 + math.cos(math.pi * (n - 1) / 7)))) < 1e-15


def test_engine_switches_are_scoped_to_its_step(M):
    """TrainEngine used to flip the process-global DEFER_WGRAD / PARALLEL_MODALITIES flags for good, so any backward
    outside engine.step() silently lost its linear / LayerNorm parameter gradients."""
    from micformer_amd import functional as Fn
    from micformer_amd.engine import TrainEngine
    import micformer_amd.models.MICFormer_self as ms
    x, t = _data(1, 64)                # (32^3 would give the tiny config a 1^3 stage: NaN gradients, as the reference)
    eng = TrainEngine(_head(M), use_graph=False)
    eng.step(x, t)
    assert Fn.CTX.defer_wgrad is False and ms.PARALLEL_MODALITIES is False
    assert not Fn.CTX.deferred and not Fn.CTX.deferred_ln and not Fn.CTX.queued_dw
    # a manual backward through the SAME (flattened) model: weight gradients are computed in place, nothing is queued
    eng.flat_g.zero_()
    loss = eng.criterion(eng.model(x), t)
    loss.backward()
    assert not Fn.CTX.deferred and not Fn.CTX.deferred_ln
    w = dict(eng.model.named_parameters())["swin.layers.0.self_blocks1.0.mlp.fc1.weight"]
    assert float(w.grad.abs().max()) > 0
    g_manual = eng.flat_g.clone()
    eng._fwd_bwd(x, t)
    scale = float(g_manual[torch.isfinite(g_manual)].abs().max())
    fin = torch.isfinite(g_manual) & torch.isfinite(eng.flat_g)
    assert float((g_manual - eng.flat_g)[fin].abs().max()) <= 2e-3 * scale


def test_two_engines_in_one_process_do_not_share_launch_state(M):
    """the launch plan's queues / mailboxes / switches are a functional.StepContext owned by each TrainEngine.
    Two engines stepping alternately (one eager, one graph-replayed; a validation forward of a third model in between, and a
    manual backward on the module default context) give exactly the losses each gives alone; a step inside another owner's
    step is refused."""
    from micformer_amd import functional as Fn
    from micformer_amd.engine import TrainEngine
    x, t = _data(1, 64)
    x2, t2 = (x * 0.7).contiguous(), t.flip(2).contiguous()
    mk = lambda g: TrainEngine(_head(M), base_lr=1e-3, t_max=20, use_graph=g)
    alone_a = [float(e.step(x, t)) for e in [mk(False)] for _ in range(3)]
    alone_b = [float(e.step(x2, t2)) for e in [mk(True)] for _ in range(3)]
    a, b, other = mk(False), mk(True), _head(M)
    assert a.ctx is not b.ctx and a.ctx is not Fn.CTX
    la, lb = [], []
    for _ in range(3):
        la.append(float(a.step(x, t)))
        with torch.no_grad():
            other(x2)                                         # (a validation forward between two engines' steps)
        lb.append(float(b.step(x2, t2)))
        assert Fn.CTX is Fn._DEFAULT_CTX and not Fn.CTX.deferred and not Fn.CTX.lazy_ln and Fn.CTX.loss_mail["result"] is None
        assert not a.ctx.deferred and not b.ctx.deferred and not a.ctx.pending_flush and not b.ctx.pending_flush
    assert all(abs(u - v) <= 1e-5 for u, v in zip(la, alone_a)), (la, alone_a)
    assert all(abs(u - v) <= 1e-5 for u, v in zip(lb, alone_b)), (lb, alone_b)
    with Fn.use_context(a.ctx):
        with pytest.raises(RuntimeError, match="already in force"):
            b._fwd_bwd(x2, t2)
    assert Fn.CTX is Fn._DEFAULT_CTX
    assert float(a.step(x, t)) == float(a.step(x, t)) or True      # (the refused step left both engines usable)
    float(b.step(x2, t2))


def test_drop_path_draw_kernel():
    from micformer_amd import ops
    dev = torch.device("cuda")
    keep = torch.tensor([1.0, 0.9, 0.5, 0.8182], device=dev)
    rng = ops.drop_path_rng(dev, 1234)
    draws = torch.stack([ops.drop_path_draw(rng, keep, 512) for _ in range(8)])       # [8, 4, 512]
    assert int(rng[1].item()) == 8                                                       # the device counter advanced
    assert torch.all(draws[:, 0] == 1.0)
    for i, k in enumerate(keep.tolist()):
        vals = draws[:, i].unique().tolist()
        assert all(abs(v) < 1e-12 or abs(v - 1.0 / k) < 1e-6 for v in vals)
        frac = float((draws[:, i] > 0).float().mean())
        assert abs(frac - k) < 0.03, (i, frac)
    assert not torch.equal(draws[0], draws[1])                                          # fresh masks per call
    rng2 = ops.drop_path_rng(dev, 1234)
    assert torch.equal(ops.drop_path_draw(rng2, keep, 512), draws[0])                   # reproducible from (seed, counter)
    assert not torch.equal(ops.drop_path_draw(ops.drop_path_rng(dev, 1235), keep, 512), draws[0])
    # a captured graph draws fresh masks at every replay (the counter lives on the device)
    static = ops.drop_path_draw(rng, keep, 512)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = ops.drop_path_draw(rng, keep, 512)
    g.replay()
    a = static.clone()
    g.replay()
    assert not torch.equal(a, static)


def test_label_values_outside_the_class_range_are_ignored():
    """a label >= K (e.g. a 255 ignore index) indexed the shared counters out of bounds."""
    from micformer_amd import ops
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 8, 6, 6, 6, generator=g).cuda()
    lab = torch.randint(0, 8, (2, 6, 6, 6), generator=g, dtype=torch.uint8)
    ign = lab.clone()
    ign[0, :2] = 255
    ign[1, 3] = 40
    mask, md = ops.argmax_meandice(logits, ign.cuda())
    pred = logits.argmax(1).cpu()
    assert torch.equal(mask.cpu().long(), pred)
    s = 0.0
    for c in range(1, 8):
        p, l = pred == c, ign == c
        s += (2.0 * float((p & l).sum()) + 1e-6) / (float(p.sum()) + float(l.sum()) + 1e-6)
    assert abs(float(md) - s / 7) < 1e-9
    # the class-map loss treats such voxels as belonging to no class (t = 0 in every channel)
    loss, _ = ops.dice_bce_fwd(logits, ign.cuda())
    onehot = torch.stack([(ign == c) for c in range(8)], 1).float().cuda()
    ref, _ = ops.dice_bce_fwd(logits, onehot)
    assert abs(float(loss) - float(ref)) < 1e-6


def test_early_adam_over_the_flat_tail_is_the_same_update(M):
    """Adam over [cut, total) launched mid-backward (decoder + last encoder stage are final there) + Adam over [0, cut) at the end
    == one Adam over the whole buffer: same step counter, same moments, and every parameter moved exactly once."""
    from micformer_amd.engine import TrainEngine
    x, t = _data(1)
    engines = []
    for early in (False, True):
        e = TrainEngine(_head(M, train=False), base_lr=1e-3, t_max=10, use_graph=False, early_adam=early)
        assert e._early_cut is not None and 0 < e._early_cut < e.flat_p.numel()
        p0 = e.flat_p.clone()
        for _ in range(2):
            e.step(x, t)
        torch.cuda.synchronize()
        engines.append((e, p0))
    (a, pa), (b, pb) = engines
    _same_training_state(a, b, "early vs single Adam")
    fin = torch.isfinite(a.flat_v) & torch.isfinite(b.flat_v)
    assert float((a.flat_v - b.flat_v)[fin].abs().max()) <= 1e-3 * float(a.flat_v[fin].abs().max()) + 1e-12
    # both halves of the buffer were updated (the 2-step displacement is ~2 lr wherever the gradient is not noise)
    for lo, hi in ((0, b._early_cut), (b._early_cut, b.flat_p.numel())):
        moved = (b.flat_p[lo:hi] - pb[lo:hi]).abs()
        moved = moved[torch.isfinite(moved)]
        assert float(moved.max()) > 1e-3 and float(moved.max()) < 2.5e-3


def test_early_adam_is_not_armed_without_full_flush_points(M):
    """flush_points=False leaves the linear / LayerNorm weight gradients queued until the end of backward: early Adam over the
    flat tail would then run on incomplete gradients (and the late ones would never be applied).  The engine must fall back to
    one Adam at the end: same training state as early_adam=False, and the same as the default layout."""
    from micformer_amd.engine import TrainEngine
    x, t = _data(1)
    engines = []
    for kw in (dict(early_adam=False, flush_points=False), dict(early_adam=True, flush_points=False), dict()):
        e = TrainEngine(_head(M, train=False), base_lr=1e-3, t_max=10, use_graph=False, **kw)
        for _ in range(2):
            e.step(x, t)
        torch.cuda.synchronize()
        engines.append(e)
    _same_training_state(engines[0], engines[1], "early Adam requested without flush points")
    _same_training_state(engines[0], engines[2], "default layout")


def test_graphed_predictor_retires_on_any_parameter_write(M):
    """A captured predictor graph bakes in cached copies of the block weights: load_state_dict (torch version counters) and
    engine.load_checkpoint (PARAM_EPOCH) must retire it -- the next call has to equal a fresh model with the new weights."""
    from micformer_amd.inference import GraphedPredictor

    def head48():                                                # embed 48: the fused block kernels and their cached K16-blocked weights
        h = M.Head(embed_dim=48, num_classes=8, depths=(1, 1, 1, 1))
        with torch.no_grad():
            for name, t in h.state_dict().items():
                t.copy_(fill.fill_tensor(name, t))
        return h.cuda().eval()

    h = head48()
    x = _data(1)[0]
    gp = GraphedPredictor(h)
    with torch.no_grad():
        y0 = gp(x).clone()
        sd = {k: (v * 1.25 if v.dim() >= 2 else v.clone()) for k, v in h.state_dict().items()}   # linear AND conv weights change
        h.load_state_dict(sd)
        y1 = gp(x).clone()
        fresh = head48()
        fresh.load_state_dict(sd)
        want = fresh(x)
    assert float((y1 - y0).abs().max()) > 1e-4
    assert float((y1 - want).abs().max()) <= 1e-5, float((y1 - want).abs().max())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_after_engine_steps_uses_the_updated_weights(M, dtype):
    """The engine's Adam kernel writes the parameters behind torch's back (no version-counter bump).  An engine-less forward
    after training (validation) must not serve weight copies cached or parked before the update: it has to equal the forward
    of a fresh model that loaded the trained state_dict."""
    from micformer_amd import ops
    from micformer_amd.engine import TrainEngine
    ops.set_compute_dtype(dtype)
    try:
        x, t = _data(2)
        model = M.Head(embed_dim=48, num_classes=8, depths=(1, 1, 1, 1)).cuda()     # widths the fused kernels take
        with torch.no_grad():
            model.eval()
            before = model(x).clone()                                               # fills the inference caches
            model.train()
        eng = TrainEngine(model, base_lr=3e-3, t_max=9, use_graph=True)
        for _ in range(3):
            eng.step(x, t)
        fresh = M.Head(embed_dim=48, num_classes=8, depths=(1, 1, 1, 1)).cuda()
        fresh.load_state_dict(model.state_dict())
        with torch.no_grad():
            model.eval(); fresh.eval()
            got, want = model(x), fresh(x)
        assert torch.isfinite(want).all()
        # fp32: the two forwards are the same arithmetic (atomics order aside); bf16 mode amplifies that noise to ~1e-3 through
        # rounding flips.  Three Adam steps at lr 3e-3 move the logits by far more than either tolerance (checked).
        tol = (1e-5 if dtype == "fp32" else 1e-2) * max(1.0, float(want.abs().max()))
        assert float((want - before).abs().max()) > 20 * tol, "the test needs the training steps to change the output"
        assert float((got - want).abs().max()) <= tol, "stale weight copies in the forward"
    finally:
        ops.set_compute_dtype("fp32")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_script_in_miniature(dtype, tmp_path):
    """tools/train_synthetic.py end to end on the fused kernels' widths (embed 48): train with the graph engine, validate by
    sliding-window inference + argmax meandice, save / resume a checkpoint.  Its own assertions: the validation loss falls and
    the resumed model validates exactly like the trained one (this is what caught stale weight copies after engine steps)."""
    import json, subprocess, sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_synthetic.py")
    r = subprocess.run([sys.executable, tool, "--dtype", dtype, "--embed-dim", "48", "--vol", "64", "--steps", "60",
                        "--out", str(tmp_path / f"micf_test_{dtype}.pth.tar")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["val_loss"][1] < out["val_loss"][0] and abs(out["resumed_val_meandice"] - out["val_meandice"][1]) < 1e-3


def test_captured_step_refuses_another_input_kind(M):
    """a graph captured on RawBatch(params=None) replayed a later RawBatch WITH augmentation draws (its flips / scale /
    shift silently dropped under labels that were already flipped), and a plain tensor against a captured RawBatch raised.  The
    engine now replays only for the input kind it captured (same type, same params-is-None state) and steps eagerly otherwise;
    RawBatch.copy_ itself refuses a mismatch."""
    from micformer_amd import data
    from micformer_amd.engine import TrainEngine
    x, t = _data(2)
    img = (x * 40 + 100).half()
    lab = fill.make_label_map(2, 64, 64, 64).to(torch.uint8).cuda()
    params = torch.tensor([[1, 0, 1, 0.07, -0.03], [0, 1, 1, -0.05, 0.09]], dtype=torch.float64).cuda()   # (float64 draws: cast inside)
    raw_plain, _ = data.prepare_raw_batch(img, None, None)
    raw_aug, lab_aug = data.prepare_raw_batch(img, lab, params)
    with pytest.raises(ValueError):
        raw_plain.clone().copy_(raw_aug)
    with pytest.raises(ValueError):
        raw_aug.clone().copy_(raw_plain)
    a = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=True)
    b = TrainEngine(_head(M), base_lr=1e-3, t_max=5, use_graph=False)
    for inp, tgt in ((raw_plain, lab), (raw_aug, lab_aug), (data.prepare_batch(img, None, None)[0], t), (raw_plain, lab)):
        la, lb = a.step(inp, tgt), b.step(inp, tgt)       # graph engine: 1st captures, 2nd / 3rd fall back to eager, 4th replays
        assert abs(float(la) - float(lb)) < 1e-4
    assert int(a.adam_state[0].item()) == 4
    _same_training_state(a, b, "after four input kinds")


def test_bf16_weight_gradient_of_a_layer_too_long_to_queue():
    """bf16-stored operands of a layer with more than DEFER_MAX_TOKENS rows (batch >= 5 at 128^3) fell through to the
    fp32-only per-layer entry point and raised.  Such a layer now launches the grouped kernel at once."""
    from micformer_amd import functional as Fn
    from micformer_amd import ops
    g = torch.Generator().manual_seed(9)
    Mrows, N, K = (1 << 17) + 4096, 48, 192
    dy = (torch.randn(Mrows, N, generator=g) * 0.1).cuda()
    a = torch.randn(Mrows, K, generator=g).cuda()
    dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    prev, prev_defer = ops.compute_dtype(), Fn.CTX.defer_wgrad
    ops.set_compute_dtype("bf16")
    Fn.CTX.defer_wgrad = True
    try:
        Fn._lin_wgrad(True, dy.bfloat16(), a.bfloat16(), dw, db)
        assert not Fn.CTX.deferred                                   # launched, not queued
    finally:
        Fn.CTX.defer_wgrad = prev_defer
        Fn.drop_deferred()
        ops.set_compute_dtype(prev)
    want = dy.bfloat16().float().t() @ a.bfloat16().float()
    assert float((dw - want).abs().max()) <= 2e-3 * float(want.abs().max())
    assert float((db - dy.bfloat16().float().sum(0)).abs().max()) <= 2e-3 * float(dy.sum(0).abs().max()) + 1e-3


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_many_is_the_same_sequence_of_updates(M, dtype):
    """TrainEngine.step_many (k steps in ONE graph, the decoder-side parameter gradients + Adam of step i carried to the head of
    step i + 1: functional.CARRY) against k eager step() calls on the same batches: losses, Adam step counter, first moments --
    twice in a row (the second replay starts from the state the first one left), in train mode (DropPath draws advance per step),
    and a checkpoint round trip drops the captured graph."""
    from micformer_amd import ops
    from micformer_amd.engine import TrainEngine
    ops.set_compute_dtype(dtype)
    try:
        xa, ta = _data(2)
        batches = [(xa, ta), (xa.flip(2).contiguous(), ta.flip(2).contiguous()), ((xa * 0.5).contiguous(), ta)]
        tol = 1e-4 if dtype == "fp32" else 2e-3
        # (the DropPath stream draws its device seed from torch's CPU generator at first use: same seed before each engine's first step)
        torch.manual_seed(5)
        # (bf16 at lr 1e-3: Adam's normalised updates amplify the rounding noise of the fixture's tiny deep-stage gradients into
        # different trajectories -- two RUNS of the same layout then sit 4-44 % apart in the first moments after six steps, measured;
        # at 1e-4 the layouts agree to 3e-3 and an extra / missing update still moves every moment by >= 14 %)
        lr = 1e-3 if dtype == "fp32" else 1e-4
        eager = TrainEngine(_head(M, train=True), base_lr=lr, t_max=20, use_graph=False)
        le = [[float(eager.step(x, t)) for x, t in batches] for _ in range(2)]
        ck_state = eager.flat_m.clone(), int(eager.adam_state[0].item())
        le.append([float(eager.step(x, t)) for x, t in batches])
        torch.manual_seed(5)
        many = TrainEngine(_head(M, train=True), base_lr=lr, t_max=20, use_graph=True)
        for rnd_ in range(2):
            lm = [float(l) for l in many.step_many([b[0] for b in batches], [b[1] for b in batches])]
            assert all(abs(a - b) <= tol for a, b in zip(le[rnd_], lm)), (rnd_, le[rnd_], lm)
            assert int(many.adam_state[0].item()) == 3 * (rnd_ + 1)
        assert int(many.adam_state[0].item()) == ck_state[1]
        fin = torch.isfinite(ck_state[0]) & torch.isfinite(many.flat_m)
        # (the sequence of updates is the same if the moments agree as a whole and almost everywhere: the sampling coordinate's
        # derivative is discontinuous at voxel boundaries, a handful of offset-head elements may differ between two summation orders)
        dm, ref_m = (ck_state[0] - many.flat_m)[fin], ck_state[0][fin]
        assert float(dm.norm()) <= 3e-2 * float(ref_m.norm())
        assert float((dm.abs() > 3e-2 * float(ref_m.abs().max())).float().mean()) <= (0.0 if dtype == "fp32" else 1e-3)
        assert many.steps_done == 6 and many._many is not None and many._many["k"] == 3
        many.load_checkpoint(many.checkpoint(epoch=0))
        assert many._many is None
        lm = [float(l) for l in many.step_many([b[0] for b in batches], [b[1] for b in batches])]
        assert all(abs(a - b) <= tol for a, b in zip(le[2], lm)), (le[2], lm)
        _same_training_state(eager, many, "after 9 steps")
    finally:
        ops.set_compute_dtype("fp32")


def test_step_many_with_three_stages_runs_step_by_step(M):
    """the carried groups are launched at stage entry 3 and waited for at entry n = number of stages; with
    n < 4 that wait would come too late (n = 3: the last encoder stage reads weights Adam is updating; n = 2: it already ran).
    Such models have no carry groups: step_many is k plain step() calls -- same losses as an eager engine, nothing captured."""
    from micformer_amd.engine import TrainEngine

    def head():
        h = M.Head(embed_dim=24, num_classes=8, depths=(1, 1, 1), num_heads=(3, 6, 12))
        with torch.no_grad():
            for name, t in h.state_dict().items():
                t.copy_(fill.fill_tensor(name, t))
        return h.cuda().eval()
    x, t = _data(1)
    eager = TrainEngine(head(), base_lr=1e-3, t_max=20, use_graph=False)
    le = [float(eager.step(x, t)) for _ in range(3)]
    many = TrainEngine(head(), base_lr=1e-3, t_max=20, use_graph=True)
    lm = [float(l) for l in many.step_many([x] * 3, [t] * 3)]
    assert many._carry_groups is False and many._many is None
    assert all(abs(a - b) <= 1e-4 for a, b in zip(le, lm)), (le, lm)
    _same_training_state(eager, many, "after 3 steps")


def test_step_many_without_flush_points_runs_step_by_step(M):
    """an engine whose flush points are off cannot run the carry region (it needs every flush point to launch all that
    is queued): step_many must notice BEFORE it captures, not assert inside the warm-up after k + 1 real updates."""
    from micformer_amd.engine import TrainEngine
    x, t = _data(1)
    ref = TrainEngine(_head(M), base_lr=1e-3, t_max=20, use_graph=True, flush_points=False)
    lr_ = [float(ref.step(x, t)) for _ in range(2)]
    eng = TrainEngine(_head(M), base_lr=1e-3, t_max=20, use_graph=True, flush_points=False)
    lm = [float(l) for l in eng.step_many([x] * 2, [t] * 2)]
    assert eng._many is None and all(abs(a - b) <= 1e-4 for a, b in zip(lr_, lm)), (lr_, lm)


def test_step_many_on_the_fused_kernels_base_model():
    """The same on the kernels the bench runs: base widths (fused block kernels, lazy LayerNorm backward, fused loss), bf16, train
    mode, 64^3: four steps in one graph against four replays of the one-step graph."""
    from micformer_amd import ops
    from micformer_amd.engine import TrainEngine
    import micformer_amd.models.MICFormer_self as MM
    ops.set_compute_dtype("bf16")
    try:
        x, t = _data(2)

        def engine():
            torch.manual_seed(11)
            h = MM.Head(embed_dim=48, num_classes=8).cuda().train()
            torch.manual_seed(12)                       # (the DropPath device seed is drawn at the engine's first step)
            return TrainEngine(h, base_lr=1e-4, t_max=50, use_graph=True)
        one = engine()
        l1 = [float(one.step(x, t)) for _ in range(8)]
        many = engine()
        lm = [float(l) for _ in range(2) for l in many.step_many([x] * 4, [t] * 4)]
        assert all(abs(a - b) <= 2e-3 for a, b in zip(l1, lm)), (l1, lm)
        assert l1[-1] < l1[0]                                                        # (it trains)
        _same_training_state(one, many, "after 8 steps")
        assert float((one.flat_p - many.flat_p).abs().max()) <= 20 * 1e-4           # (a few lr-sized Adam steps apart at most)
    finally:
        ops.set_compute_dtype("fp32")


def test_benched_step_launch_list():
    """What the benched step (bf16, base widths, engine mode) does NOT launch any more (round 4): MDiceLoss's forward reduction
    (folded into the head's logits store), the LayerNorm-1 backward of the cross pairs (prologue of the self pairs' block_bwd), their
    LayerNorm-1 forward (round 6: epilogue of the self pairs' block_fwd), and -- with input_buffers() -- no staging copy; and what it
    launches instead."""
    from micformer_amd import _lib, ops
    from micformer_amd.engine import TrainEngine
    import micformer_amd.models.MICFormer_self as MM
    ops.set_compute_dtype("bf16")
    try:
        x, t = _data(2)
        torch.manual_seed(3)
        eng = TrainEngine(MM.Head(embed_dim=48, num_classes=8).cuda().train(), base_lr=1e-4, t_max=50, use_graph=False)
        eng.step(x, t)
        torch.cuda.synchronize()
        _lib.profile_start()
        loss = eng.step(x, t)
        prof = _lib.profile_stop()
        names = {k.split("|")[0] for k in prof}
        assert float(loss) == float(loss)
        assert "micf_head_tail_fwd_loss_fused" in names and "micf_dice_bce_fwd" not in names and "micf_head_tail_fwd_fused" not in names
        assert "micf_dice_bce_bwd" in names                                   # (the loss backward stays its own launch)
        # (the cross pairs of the tile- / wave-kernel stages: 20 of the 24; the 4 slots of the few-token C = 384 stage keep their
        #  launches.  Round 6: the forward LayerNorm 1 of those 20 is the epilogue of the self pairs' block_fwd)
        assert prof["micf_layernorm_bwd_pair"]["calls"] == 4 and prof["micf_layernorm_fwd_pair"]["calls"] == 4
        assert prof["micf_block_bwd"]["calls"] == prof["micf_block_fwd"]["calls"] == 48 if "micf_block_bwd" in prof else True
        # a graph engine hands out the buffers its captured step reads; passing them back skips the staging copies
        g = TrainEngine(MM.Head(embed_dim=48, num_classes=8).cuda().train(), base_lr=1e-4, t_max=50, use_graph=True)
        assert g.input_buffers() is None
        g.step(x, t)
        bx, bt = g.input_buffers()
        assert bx.data_ptr() != x.data_ptr() and torch.equal(bx, x) and torch.equal(bt, t)
        la = float(g.step(bx, bt))
        assert la == la
    finally:
        ops.set_compute_dtype("fp32")
