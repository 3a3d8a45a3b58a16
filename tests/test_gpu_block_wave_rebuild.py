"""The REBUILD forms of the wave-private block launches at C = 48 (csrc/block_wave_fwd.h / block_wave_bwd.h): the forward stores
neither q, k | v nor the fc1 pre-activation h, the backward rebuilds them in registers from xn / kvs16 / xn2 with the forward's own
fragments, products, bias adds and rounding.  The contract is BIT IDENTITY: every other forward output equals the saving form's, and
the backward returns the same bits whether it reads the saved tensors, rebuilds h, or rebuilds h and q / k / v."""
import pytest
import torch

from test_gpu_block_fused import make_params, rnd

pytestmark = pytest.mark.gpu

C, HEADS, EPS = 48, 3, 1e-5
SCALE = (C // HEADS) ** -0.5
# four tiles + DropPath scales (one of them 0); one window in a 32-token tile (masked rows); three windows (a half-empty second group)
DIMS = [(2, 4, 4, 4), (1, 2, 2, 2), (1, 2, 2, 6)]


@pytest.fixture()
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micformer_amd import ops as o
    o.set_compute_dtype("bf16")
    yield o
    o.set_compute_dtype("fp32")


def _groups(dims, kind, ngroups):
    B, D, H, W = dims
    T = B * D * H * W
    attn = "self_attn" if kind.startswith("self") else "cross_attn"
    gs = []
    for i in range(ngroups):
        P = make_params(C, 4 * C, attn, 20 + 40 * i)
        gd = {"x": rnd((T, C), 3 + i), "kvsrc": None, "P": P, "attn": attn, "s1": None, "s2": None}
        if B > 1:                                       # DropPath: a dropped sample in either residual branch
            gd["s1"] = torch.tensor([0.0, 1.25] if i == 0 else [1.25, 0.8]).cuda()
            gd["s2"] = torch.tensor([1.25, 0.0] if i == 0 else [0.8, 1.25]).cuda()
        if kind.startswith("self"):                     # ... with the epilogue LayerNorm of the next block
            gd["next_ln"] = (1 + rnd((C,), 41 + i, 0.1), rnd((C,), 42 + i, 0.1), None)
        if kind == "cross":
            gd["kvsrc"] = rnd((T, C), 11 + i)
        if kind == "sampled":
            P.update({"conv_offset.1.norm.weight": 1 + rnd((16,), 31 + i, 0.1), "conv_offset.1.norm.bias": rnd((16,), 32 + i, 0.1),
                      "conv_offset.3.weight": rnd((3, 16), 33 + i, 0.3)})
            gd.update(hid=rnd((T, 16), 13 + i), samp_src=rnd((T, C), 15 + i), want_xn=False)
        gs.append(gd)
    return gs


def _fwd(ops, gs, dims, **kw):
    out = ops.block_fwd([dict(g) for g in gs], dims, C, HEADS, EPS, SCALE, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", ["self", "cross", "sampled"])
@pytest.mark.parametrize("ngroups", [1, 2])
def test_forward_without_q_kv_h_writes_the_same_bits_elsewhere(ops, dims, kind, ngroups):
    assert ops.block_rebuilds(dims, C, HEADS, 4 * C)
    gs = _groups(dims, kind, ngroups)
    full = _fwd(ops, gs, dims)
    lean = _fwd(ops, gs, dims, rebuild=True)
    only_h = _fwd(ops, gs, dims, rebuild="h")
    for f, l, oh in zip(full, lean, only_h):
        assert l["q"] is None and l["kv"] is None and l["h"] is None
        assert oh["h"] is None and torch.equal(oh["q"], f["q"]) and torch.equal(oh["kv"], f["kv"])
        assert f["q"] is not None and f["kv"] is not None and f["h"] is not None
        seen = set()
        for k, v in f.items():
            if k in ("q", "kv", "h"):
                continue
            if v is None:
                assert l[k] is None, k
            elif k == "nln":
                assert all(torch.equal(a, b) for a, b in zip(v, l[k])), k
            else:
                assert torch.equal(v, l[k]), k
            seen.add(k)
        want = {"xn", "o", "x1", "xn2", "g", "stats", "y"} | ({"nln"} if kind == "self" else {"kvs16"}) | ({"flow"} if kind == "sampled" else set())
        assert want <= {k for k in seen if f[k] is not None}


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", ["self", "self+pre", "cross", "sampled"])
@pytest.mark.parametrize("ngroups", [1, 2])
def test_backward_returns_the_same_bits_from_saved_and_rebuilt_tensors(ops, dims, kind, ngroups):
    B, D, H, W = dims
    T = B * D * H * W
    cross = kind in ("cross", "sampled")
    gs = _groups(dims, kind, ngroups)
    fw = _fwd(ops, gs, dims)                            # ONE saving forward feeds all three backward forms
    bg = []
    for i, (g, o) in enumerate(zip(gs, fw)):
        gd = {"dy": rnd((T, C), 50 + i), "x": None if cross else g["x"], "x1": o["x1"], "stats": o["stats"], "q": o["q"], "kv": o["kv"],
              "h": o["h"], "xn2": o["xn2"], "xn": o["xn"], "kvs16": o["kvs16"], "P": g["P"], "attn": g["attn"], "s1": g["s1"], "s2": g["s2"],
              "cross": cross, "want_copy": cross}
        if kind == "self+pre":
            px = rnd((T, C), 60 + i)
            gd["pre"] = {"d": rnd((T, C), 62 + i), "x": px, "mean": px.mean(1).contiguous(),
                         "rstd": (px.var(1, unbiased=False) + EPS).rsqrt().contiguous(), "gamma": 1 + rnd((C,), 64 + i, 0.1)}
        bg.append(gd)

    def run(drop):
        out = ops.block_bwd([{k: (None if k in drop else v) for k, v in g.items()} for g in bg], dims, C, HEADS, SCALE)
        torch.cuda.synchronize()
        return out

    saved, reb_h, reb_all = run(()), run(("h",)), run(("h", "q", "kv"))
    keys = ["dx", "dx1", "dh", "dq", "dkv", "dy16", "ln2_part"] + (["dxs", "dx1_copy"] if cross else ["ln1_part"]) \
        + (["pre_part"] if kind == "self+pre" else [])
    for i in range(ngroups):
        for k in keys:
            assert saved[i][k] is not None and torch.isfinite(saved[i][k].float()).all(), k
            assert torch.equal(saved[i][k], reb_h[i][k]), f"group {i} {k}: h rebuilt"
            assert torch.equal(saved[i][k], reb_all[i][k]), f"group {i} {k}: h, q, k | v rebuilt"
        # (not vacuous: dh needs h, dv needs the softmax of q k^T -- dq / dk themselves vanish where every sampled K/V row is the same)
        assert float(saved[i]["dh"].float().abs().max()) > 0 and float(saved[i]["dkv"][:, C:].float().abs().max()) > 0


def test_training_step_saves_no_q_kv_h_at_the_wave_private_stage(ops, monkeypatch):
    """Product path: Head(embed_dim=48) on a 32^3 volume, forward + backward -- the C = 48 stage's block launches store and read no
    q / kv / h, the C = 96 stage's (tile-per-workgroup kernels) still do."""
    from micformer_amd.models.MICFormer_self import Head
    from oracle import fill
    h = Head(embed_dim=48, num_classes=8)
    fill.fill_state_dict(h)
    h = h.cuda().train()
    fwd_seen, bwd_seen = [], []
    real_f, real_b = ops.block_fwd, ops.block_bwd

    def spy_f(groups, dims, c, *a, **kw):
        outs = real_f(groups, dims, c, *a, **kw)
        fwd_seen.extend((c, tuple(o[k] is None for k in ("q", "kv", "h"))) for o in outs)
        return outs

    def spy_b(groups, dims, c, *a, **kw):
        bwd_seen.extend((c, tuple(g[k] is None for k in ("q", "kv", "h"))) for g in groups)
        return real_b(groups, dims, c, *a, **kw)

    monkeypatch.setattr(ops, "block_fwd", spy_f)
    monkeypatch.setattr(ops, "block_bwd", spy_b)
    y = h(fill.make_volume(1, 32, 32, 32).cuda())
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    for seen in (fwd_seen, bwd_seen):
        at48 = [s for c, s in seen if c == 48]
        at96 = [s for c, s in seen if c == 96]
        assert at48 and all(s == (True, True, True) for s in at48), at48
        assert at96 and all(s == (False, False, False) for s in at96), at96
    assert torch.isfinite(y).all() and any(p.grad is not None for p in h.parameters())
