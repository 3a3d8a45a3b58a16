"""GPU parity tests, op level, second generation: every host dispatch arm of csrc/layernorm.hip and csrc/window_attn.hip against the
float64 referee tests/ln_attn_ref.py.  test_gpu_ops.py (test_layernorm, test_layernorm_deferred_parameter_gradients,
test_window_attention) holds the arms the model's common shapes take; this file holds the rest.  Tolerances are that file's:
2e-5 abs + 1e-4 of the tensor's max; 2e-4 of max for atomically accumulated dgamma / dbeta; 3e-4 of max after a deferred finish.

Which arm lives where (test ids name the arm):

layernorm.hip
  ln_fwd_kernel / ln_bwd_kernel (scalar)    test_ln_scalar_arms: C % 4 != 0 (C = 6, 50), c1 % 4 != 0 (c1 = 6 of 10, 46 of 96), a base pointer off
                                            16 bytes, and the rows >= 16384 form (rpb = 32) with a ragged last block; test_gpu_ops has none
  ln_v2_shape / MICF_LN_DISPATCH            <16,1> <32,1> <64,1> <64,2>: test_gpu_ops.test_layernorm (C = 16..48, 96, 192 via the deferred
                                            test, 384) and the pair tests here; <64,4> (C = 516, 768 with vector k = 3 masked, 1024) and
                                            <64,8> (C = 1028, 1536, 2048 = the 64 KiB dynamic-LDS backward): test_ln_vector_arms
  micf_layernorm_bwd_partial_rows           0 on every scalar shape (test_ln_scalar_arms), the backward's grid on the vector ones
  micf_layernorm_fwd_pair                   test_ln_fwd_pair (blockIdx.y set selection, bit-equal to two single calls, the `zero` side job with
                                            one and with two grid-stride trips), test_ln_fwd_pair_single_item (n = 1),
                                            test_ln_fwd_pair_fallback (!ok: two single calls + micf_zero)
  micf_layernorm_bwd_pair                   test_ln_bwd_pair (add, out aliasing add, one / both items deferred, n = 1),
                                            test_ln_bwd_pair_operand_off_16_bytes (!ok with defers: ops.layernorm_bwd_pair must not queue partials)

window_attn.hip
  MICF_WF(8 / 16 / 32), wpb = 1             test_wattn_chunked_backward (N * heads = 192: one window and 64 idle threads per workgroup)
  MICF_BWD4 with nchunks > 1                test_wattn_chunked_backward (the model's stage-3 / stage-4 head counts)
  MICF_BWD4 / MICF_WF over N = 2..8         test_wattn_window_sizes (units that straddle wave boundaries, a partly empty last workgroup)
  MICF_WF(0) / wattn_bwd_kernel<0>          test_wattn_runtime_head_dim (hd = 4, 12, 24: vector-aligned but no instantiation; hd = 5),
                                            test_wattn_hd16_unaligned_through_the_abi (hd = 16 with an odd ldq / a kv pointer off 16 bytes)
  _qkv wrappers (ld = 3C)                   test_wattn_packed_qkv, bit-equal to the split calls
  expf(s - mx) with |s| up to 60            test_wattn_large_scores, bound = 4 x the fp32 CPU reference's own error
"""
import ctypes
import math

import pytest
import torch

import ln_attn_ref as L
import test_gpu_ops as G

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micformer_amd import ops as o
    return o


def dev(t):
    return t.cuda().contiguous() if t is not None else None


def off16(t):
    """Contiguous CUDA copy of t at storage offset 1 float: its base pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def close(got, want, atol=2e-5, rtol=1e-4, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    assert math.isfinite(err), f"{what}: non-finite error"
    assert err <= atol + rtol * scale, f"{what}: max abs err {err:.3e} (scale {scale:.3e})"


# ----------------------------------------------------------------------------- host dispatch, restated
def v2_shape(C):
    """ln_v2_shape: (lanes per row, float4 per lane) or None."""
    if C % 4:
        return None
    nv = C // 4
    lpr = 16 if nv <= 16 else (32 if nv <= 32 else 64)
    vpl = -(-nv // lpr)
    return (lpr, vpl) if vpl <= 8 else None


def v2_arm(C):
    """The MICF_LN_DISPATCH instantiation C takes."""
    lpr, vpl = v2_shape(C)
    return f"<{lpr},{1 if vpl == 1 else 2 if vpl == 2 else 4 if vpl <= 4 else 8}>"


def v2_grid(rows, C, max_blocks):
    """gridDim.x of the vector kernels (ln_v2_rpb; max_blocks = 2048 forward, 512 backward)."""
    step = 4 * (64 // v2_shape(C)[0])
    rpb = max(-(-(-(-rows // max_blocks)) // step) * step, step)
    return -(-rows // rpb)


def unit_map(N, heads, hd):
    """unit_map of the coalesced backward: (heads per unit, chunks per window, threads per workgroup)."""
    lph = hd // 4
    hc = next(d for d in range(heads, 0, -1) if heads % d == 0 and N * d * lph <= 256)
    U = N * hc * lph
    return hc, heads // hc, (256 // U) * U


def partial_rows(rows, C, c1):
    from micformer_amd import _lib
    return _lib.lib.micf_layernorm_bwd_partial_rows(rows, C, c1)


# ----------------------------------------------------------------------------- LayerNorm
def ln_inputs(rows, C, seed=0):
    x = L.rnd(rows, C, seed=seed + 1) * 2 + 0.3
    g, b = 1 + 0.1 * L.rnd(C, seed=seed + 2), 0.1 * L.rnd(C, seed=seed + 3)
    return x, g, b, L.rnd(rows, C, seed=seed + 4), L.rnd(rows, C, seed=seed + 5)


def ln_single(ops, rows, C, c1, misalign=False, vector=True):
    """Forward + backward (with and without add) of one LayerNorm against float64; on vector shapes the deferred form too."""
    x, g, b, dy, add = ln_inputs(rows, C)
    x1, x2 = (x, None) if c1 == C else (x[:, :c1].contiguous(), x[:, c1:].contiguous())
    y64, mean64, rstd64 = L.ln_fwd(x1, g, b, EPS, x2)
    dx1 = off16(x1) if misalign else dev(x1)
    y, mean, rstd = ops.layernorm_fwd(dx1, dev(g), dev(b), EPS, dev(x2))
    close(y, y64, what="y")
    close(mean, mean64, what="mean")
    close(rstd, rstd64, what="rstd")
    dg0, db0 = L.rnd(C, seed=8), L.rnd(C, seed=9)
    for a in (None, add):
        want_dx, want_dg, want_db = L.ln_bwd(dy, x1, g, EPS, x2, add=a)
        dg, db = dev(dg0.clone()), dev(db0.clone())
        r = ops.layernorm_bwd(dev(dy), dx1, mean, rstd, dev(g), dg, db, dev(x2), add=dev(a))
        got = r if c1 == C else torch.cat([r[0], r[1]], 1)
        tag = "add" if a is not None else "no add"
        close(got, want_dx, what=f"dx ({tag})")
        close(dg, dg0.double() + want_dg, rtol=2e-4, what=f"dgamma ({tag})")
        close(db, db0.double() + want_db, rtol=2e-4, what=f"dbeta ({tag})")
    if c1 != C:
        return
    # defer: the partial form where the vector kernel runs, immediate accumulation where it cannot
    queue = []
    dg, db = dev(dg0.clone()), dev(db0.clone())
    got = ops.layernorm_bwd(dev(dy), dx1, mean, rstd, dev(g), dg, db, add=dev(add), defer=queue)
    assert len(queue) == (1 if vector else 0)
    if vector:
        assert torch.equal(dg.cpu(), dg0) and torch.equal(db.cpu(), db0)          # nothing accumulated before the finish
    ops.layernorm_bwd_finish(queue)
    close(got, want_dx, what="dx (defer)")
    close(dg, dg0.double() + want_dg, rtol=3e-4, what="dgamma (defer)")
    close(db, db0.double() + want_db, rtol=3e-4, what="dbeta (defer)")


SCALAR = [pytest.param(37, 6, 6, False, id="scalar-C6"), pytest.param(5, 50, 50, False, id="scalar-C50"),
          pytest.param(33, 10, 6, False, id="scalar-cat-c1=6-of-10"), pytest.param(9, 96, 46, False, id="scalar-cat-c1=46-of-96"),
          pytest.param(37, 48, 48, True, id="scalar-C48-x-off-16-bytes"),
          pytest.param(16384 + 5, 6, 6, False, id="scalar-rpb32-ragged-last-block")]


@pytest.mark.parametrize("rows,C,c1,misalign", SCALAR)
def test_ln_scalar_arms(ops, rows, C, c1, misalign):
    """ln_fwd_kernel / ln_bwd_kernel: every way past ln_v2_shape and the alignment test.  micf_layernorm_bwd_partial_rows must say 0
    wherever the SHAPE rules the vector kernel out; it cannot see a pointer, so for the misaligned x it is ops.layernorm_bwd that must
    not defer (ln_single asserts the queue stays empty and the gradients are accumulated at once)."""
    assert (partial_rows(rows, C, c1) == 0) == (not misalign)
    ln_single(ops, rows, C, c1, misalign=misalign, vector=False)


VECTOR = [pytest.param(rows, C, C, id=f"ln_v2{v2_arm(C)}-C{C}-rows{rows}") for C in (516, 768, 1024, 1028, 1536, 2048) for rows in (9, 70)]
VECTOR += [pytest.param(rows, 768, 384, id=f"ln_v2<64,4>-C768-c1=384-rows{rows}") for rows in (9, 70)]


@pytest.mark.parametrize("rows,C,c1", VECTOR)
def test_ln_vector_arms(ops, rows, C, c1):
    """<64,4> (C in 516..1024; C = 768 masks vector k = 3 of every lane) and <64,8> (C in 1028..2048).  C = 2048 backward launches
    with 8 * C * 4 = 65536 bytes of dynamic LDS, the most a kernel gets without opting in."""
    assert v2_arm(C) == ("<64,4>" if C <= 1024 else "<64,8>")
    assert partial_rows(rows, C, c1) == v2_grid(rows, C, 512)
    ln_single(ops, rows, C, c1)


PAIR_SHAPES = [(37, 48), (130, 24), (9, 384), (70, 768)]


def nan_buffer(n, guard=64):
    buf = torch.full((n + guard,), NAN, device="cuda")
    return buf, buf[:n]


def assert_cleared(buf, n, what):
    host = buf.cpu()
    assert torch.equal(host[:n], torch.zeros(n)), f"{what}: zero buffer not cleared"
    assert bool(torch.isnan(host[n:]).all()), f"{what}: wrote past the zero buffer"


def pair_inputs(rows, C):
    return [ln_inputs(rows, C, seed=100 * i) for i in (0, 1)]


def check_fwd(outs, sets, what):
    for i, ((y, mean, rstd), (x, g, b, _, _)) in enumerate(zip(outs, sets)):
        y64, mean64, rstd64 = L.ln_fwd(x, g, b, EPS)
        close(y, y64, what=f"{what} y[{i}]")
        close(mean, mean64, what=f"{what} mean[{i}]")
        close(rstd, rstd64, what=f"{what} rstd[{i}]")


@pytest.mark.parametrize("rows,C", PAIR_SHAPES, ids=[f"ln_v2{v2_arm(C)}-rows{r}-C{C}" for r, C in PAIR_SHAPES])
def test_ln_fwd_pair(ops, rows, C):
    """micf_layernorm_fwd_pair, n = 2, two different x / gamma / beta sets: blockIdx.y picks the set, body and rows per workgroup are
    those of micf_layernorm_fwd -> bit-equal to two single calls.  The `zero` side job: 4 floats (one float4) and
    (gridDim.x * 256 + 3) float4 (a second trip of the grid-stride loop for three threads); NaN before, exact zeros after, guard intact."""
    sets = pair_inputs(rows, C)
    xs, gs, bs = ([dev(s[k]) for s in sets] for k in (0, 1, 2))
    singles = [ops.layernorm_fwd(xs[i], gs[i], bs[i], EPS) for i in (0, 1)]
    for nfloats in (None, 4, (v2_grid(rows, C, 2048) * 256 + 3) * 4):
        buf, zero = nan_buffer(nfloats) if nfloats else (None, None)
        outs = ops.layernorm_fwd_pair(xs, gs, bs, EPS, zero=zero)
        for i in (0, 1):
            for got, want, name in zip(outs[i], singles[i], ("y", "mean", "rstd")):
                assert torch.equal(got, want), f"pair {name}[{i}] differs from the single call (zero = {nfloats})"
        if nfloats:
            assert_cleared(buf, nfloats, f"zero = {nfloats} floats")
    check_fwd(outs, sets, "pair")


def test_ln_fwd_pair_single_item(ops):
    """n = 1 through the C ABI (the wrapper always builds two items): set 1 mirrors set 0, gridDim.y = 1."""
    from micformer_amd import _lib
    rows, C = 37, 48
    x, g, b, _, _ = ln_inputs(rows, C)
    t = [dev(x), dev(g), dev(b), torch.empty(rows, C, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")]
    arr = (_lib.LnPairItem * 1)()
    for name, v in zip(_lib.LnPairItem.FIELDS, t):
        setattr(arr[0], name, v.data_ptr())
    buf, zero = nan_buffer(4)
    _lib.call("micf_layernorm_fwd_pair", ctypes.cast(arr, ctypes.c_void_p), 1, rows, C, EPS, zero.data_ptr(), 4)
    single = ops.layernorm_fwd(t[0], t[1], t[2], EPS)
    for got, want in zip(t[3:], single):
        assert torch.equal(got, want)
    check_fwd([tuple(t[3:])], [(x, g, b, None, None)], "n = 1")
    assert_cleared(buf, 4, "n = 1")


@pytest.mark.parametrize("C,misalign", [pytest.param(10, False, id="fallback-C10"), pytest.param(48, True, id="fallback-C48-x-off-16-bytes")])
def test_ln_fwd_pair_fallback(ops, C, misalign):
    """!ok in micf_layernorm_fwd_pair: two micf_layernorm_fwd calls (the scalar kernel for C = 10 and for the misaligned item, the
    vector kernel for its aligned partner) plus micf_zero.  Outputs correct, `zero` still cleared."""
    rows = 37
    sets = pair_inputs(rows, C)
    xs, gs, bs = ([dev(s[k]) for s in sets] for k in (0, 1, 2))
    if misalign:
        xs[1] = off16(sets[1][0])
    buf, zero = nan_buffer(3084)
    outs = ops.layernorm_fwd_pair(xs, gs, bs, EPS, zero=zero)
    check_fwd(outs, sets, "fallback")
    assert_cleared(buf, 3084, "fallback")


def bwd_pair_case(ops, rows, C, n=2):
    sets = pair_inputs(rows, C)[:n]
    case = []
    for x, g, b, dy, add in sets:
        t = {"x": dev(x), "gamma": dev(g), "dy": dev(dy)}
        _, t["mean"], t["rstd"] = ops.layernorm_fwd(t["x"], t["gamma"], dev(b), EPS)
        case.append((t, (x, g, dy, add)))
    return case


def run_bwd_pair(ops, case, use_add, alias, defers, C, operands=None):
    """One micf_layernorm_bwd_pair call onto non-zero dgamma / dbeta; checks dx (bit-equal to the single call when `operands` is None),
    that a deferred item accumulates nothing before the finish and the other one everything, and both after the finish."""
    items, want, starts = [], [], []
    for i, (t, (x, g, dy, add)) in enumerate(case):
        dg0, db0 = L.rnd(C, seed=60 + i), L.rnd(C, seed=70 + i)
        d = dict(t, dgamma=dev(dg0), dbeta=dev(db0), add=dev(add) if use_add else None)
        if operands:
            d.update(operands(i, d))
        if alias and i == 0:
            d["out"] = d["add"]                                        # "dx = LN'(dy) + add (out: destination, may alias add)"
        items.append(d)
        starts.append((dg0, db0))
        want.append(L.ln_bwd(dy, x, g, EPS, add=add if use_add else None))
    singles = None
    if operands is None:
        singles = [ops.layernorm_bwd(d["dy"], d["x"], d["mean"], d["rstd"], d["gamma"], torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"),
                                     add=d["add"]) for d in items]
    outs = ops.layernorm_bwd_pair(items, defers)
    for i, (d, (dx64, dg64, db64), (dg0, db0)) in enumerate(zip(items, want, starts)):
        if singles:
            assert torch.equal(outs[i], singles[i]), f"pair dx[{i}] differs from the single call"
        if d.get("out") is not None:
            assert outs[i].data_ptr() == d["out"].data_ptr()
        close(outs[i], dx64, what=f"pair dx[{i}]")
        if operands is None and defers[i] is not None:
            assert torch.equal(d["dgamma"].cpu(), dg0) and torch.equal(d["dbeta"].cpu(), db0), f"item {i} accumulated before the finish"
        elif defers[i] is None:
            close(d["dgamma"], dg0.double() + dg64, rtol=2e-4, what=f"pair dgamma[{i}] (immediate)")
            close(d["dbeta"], db0.double() + db64, rtol=2e-4, what=f"pair dbeta[{i}] (immediate)")
    queued = [q for q in {id(q): q for q in defers if q is not None}.values()]
    for q in queued:
        ops.layernorm_bwd_finish(q)
    for i, (d, (dx64, dg64, db64), (dg0, db0)) in enumerate(zip(items, want, starts)):
        rtol = 3e-4 if defers[i] else 2e-4                             # (an empty queue: nothing was deferred, plain atomics)
        close(d["dgamma"], dg0.double() + dg64, rtol=rtol, what=f"pair dgamma[{i}]")
        close(d["dbeta"], db0.double() + db64, rtol=rtol, what=f"pair dbeta[{i}]")


@pytest.mark.parametrize("rows,C", PAIR_SHAPES, ids=[f"ln_v2{v2_arm(C)}-rows{r}-C{C}" for r, C in PAIR_SHAPES])
def test_ln_bwd_pair(ops, rows, C):
    """micf_layernorm_bwd_pair: plain; `add` with item 0's `out` aliasing its `add` and only item 0 deferred (item 1 accumulates at
    once); both deferred into one queue; n = 1.  dx bit-equal to micf_layernorm_bwd (same body, same rows per workgroup)."""
    case = bwd_pair_case(ops, rows, C)
    run_bwd_pair(ops, case, use_add=False, alias=False, defers=[None, None], C=C)
    q = []
    run_bwd_pair(ops, case, use_add=True, alias=True, defers=[q, None], C=C)
    assert len(q) == 1 and q[0][1] == partial_rows(rows, C, C)
    q = []
    run_bwd_pair(ops, case, use_add=True, alias=False, defers=[q, q], C=C)
    assert len(q) == 2
    run_bwd_pair(ops, case[:1], use_add=True, alias=True, defers=[None], C=C)


@pytest.mark.parametrize("which", ["x", "add", "out"])
def test_ln_bwd_pair_operand_off_16_bytes(ops, which):
    """Regression: one operand of one item 4 bytes off a 16-byte boundary sends micf_layernorm_bwd_pair to its fallback, two
    micf_layernorm_bwd calls, and the misaligned one runs the scalar kernel, which has no partial form.  ops.layernorm_bwd_pair used
    to allocate partials from the shape alone, so the call failed with MICF_EUNSUPPORTED -- for item 1 after item 0 had been written
    and queued.  It must decide from the pointers of both items first; then both items accumulate at once and nothing is queued."""
    rows, C = 37, 48
    case = bwd_pair_case(ops, rows, C)
    if which == "x":                  # item 1, so item 0 has been launched and (before the fix) queued when the call fails
        t = dict(case[1][0], x=off16(case[1][0]["x"]))
        case[1] = (t, case[1][1])
    move = {"x": lambda i, d: {}, "add": lambda i, d: {"add": off16(d["add"])} if i == 0 else {},
            "out": lambda i, d: {"out": off16(torch.zeros(rows, C))} if i == 1 else {}}[which]
    q = []
    run_bwd_pair(ops, case, use_add=True, alias=False, defers=[q, q], C=C, operands=move)
    assert q == []
    if which == "out":                # the single-call wrapper makes the same decision
        t, (x, g, dy, add) = case[0]
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        dx = ops.layernorm_bwd(t["dy"], t["x"], t["mean"], t["rstd"], t["gamma"], dg, db, defer=q, out=off16(torch.zeros(rows, C)))
        dx64, dg64, db64 = L.ln_bwd(dy, x, g, EPS)
        assert q == []
        close(dx, dx64, what="single dx")
        close(dg, dg64, rtol=2e-4, what="single dgamma")
        close(db, db64, rtol=2e-4, what="single dbeta")


# ----------------------------------------------------------------------------- window attention
def attn_want(q, kv, do, dims, heads, ws):
    C = q.shape[1]
    scale = (C // heads) ** -0.5
    o = L.attn_fwd(q, kv[:, :C], kv[:, C:], dims, heads, ws, scale)
    dq, dk, dv = L.attn_bwd(q, kv[:, :C], kv[:, C:], do, dims, heads, ws, scale)
    return scale, o, dq, torch.cat([dk, dv], 1)


def attn_case(ops, dims, C, heads, ws):
    q, kv, do = L.attn_inputs(dims, C)
    scale, o64, dq64, dkv64 = attn_want(q, kv, do, dims, heads, ws)
    o = ops.window_attn_fwd(dev(q), dev(kv), dims, heads, ws, scale)
    close(o, o64, what="attn o")
    dq, dkv = ops.window_attn_bwd(dev(q), dev(kv), dev(do), dims, heads, ws, scale)
    close(dq, dq64, what="attn dq")
    close(dkv, dkv64, what="attn dkv")


CHUNKED = {(192, 12): (6, 2, 192), (384, 24): (8, 3, 256), (192, 24): (12, 2, 192), (384, 12): (4, 3, 256)}


@pytest.mark.parametrize("dims", [(1, 2, 2, 2), (2, 2, 4, 6)], ids=["1-window", "12-windows"])
@pytest.mark.parametrize("C,heads", list(CHUNKED), ids=[f"bwd4-C{C}-heads{h}-nchunks{CHUNKED[C, h][1]}" for C, h in CHUNKED])
def test_wattn_chunked_backward(ops, dims, C, heads):
    """wattn_bwd4_kernel with um.nchunks > 1, the model's stage-3 / stage-4 shapes at window (2,2,2): a window's heads are split over
    2 or 3 units of hc heads, hoff = (chunk * hc + hl) * hd.  The forward at N * heads = 192 (wpb = 1, 64 idle threads) rides along."""
    assert unit_map(8, heads, C // heads) == CHUNKED[C, heads]
    attn_case(ops, dims, C, heads, (2, 2, 2))


WINDOWS = [((1, 1, 2), (2, 1, 3, 4), 2), ((1, 1, 3), (1, 2, 2, 6), 3), ((1, 3, 2), (1, 1, 6, 4), 6), ((7, 1, 1), (1, 7, 2, 3), 7),
           ((7, 1, 1), (1, 7, 2, 2), 7), ((2, 2, 2), (3, 2, 2, 2), 8)]


@pytest.mark.parametrize("ws,dims,N", WINDOWS, ids=[f"N{N}-window{'x'.join(map(str, ws))}-grid{'x'.join(map(str, d))}" for ws, d, N in WINDOWS])
def test_wattn_window_sizes(ops, ws, dims, N):
    """C = 48, heads = 3, hd = 16 over every window size make_geo accepts below the usual 8 (and 8 with three windows).  N = 3 gives
    U = 36 threads per unit, 7 units = 252 threads per workgroup whose units straddle wave boundaries.  The window counts leave the
    last backward workgroup partly empty (N = 7: 4 windows on 3 units per workgroup; the 6-window grid fills two exactly)."""
    assert ws[0] * ws[1] * ws[2] == N
    hc, nchunks, threads = unit_map(N, 3, 16)
    assert (hc, nchunks) == (3, 1) and threads == (256 // (12 * N)) * 12 * N
    attn_case(ops, dims, 48, 3, ws)


@pytest.mark.parametrize("C,heads", [(12, 3), (36, 3), (48, 2), (15, 3)], ids=["hd4", "hd12", "hd24", "hd5-unaligned-rows"])
def test_wattn_runtime_head_dim(ops, C, heads):
    """MICF_WF(0) and wattn_bwd_kernel<0>: hd = 4, 12, 24 pass every vector test but have no instantiation; hd = 5 fails hd % 4."""
    attn_case(ops, (1, 2, 4, 2), C, heads, (2, 2, 2))


@pytest.mark.parametrize("how", ["ldq=C+1", "kv-off-16-bytes"])
def test_wattn_hd16_unaligned_through_the_abi(ops, how):
    """hd = 16 with `vec` false: q (and dq) rows in a [T, C + 1] buffer, or k / v 4 bytes off a 16-byte boundary.  The ops wrappers
    cannot produce either; the C ABI accepts both and must take the runtime-head-dim kernels.  The buffers' spare column is NaN before
    and after: never read into a result, never written."""
    from micformer_amd import _lib
    dims, C, heads, ws = (1, 2, 4, 2), 48, 3, (2, 2, 2)
    T = 16
    q, kv, do = L.attn_inputs(dims, C)
    scale, o64, dq64, dkv64 = attn_want(q, kv, do, dims, heads, ws)
    ldq = C + 1 if how == "ldq=C+1" else C
    qbuf = torch.full((T, ldq), NAN, device="cuda")
    qbuf[:, :C] = q.cuda()
    dqbuf = torch.full((T, ldq), NAN, device="cuda")
    kvd = off16(kv) if how == "kv-off-16-bytes" else dev(kv)
    o, dkv, dod = torch.empty(T, C, device="cuda"), torch.empty(T, 2 * C, device="cuda"), dev(do)
    geo = (dims[0], dims[1], dims[2], dims[3], C, heads, ws[0], ws[1], ws[2], float(scale))
    _lib.call("micf_window_attn_fwd", qbuf.data_ptr(), ldq, kvd.data_ptr(), kvd.data_ptr() + 4 * C, 2 * C, o.data_ptr(), C, *geo)
    _lib.call("micf_window_attn_bwd", qbuf.data_ptr(), ldq, kvd.data_ptr(), kvd.data_ptr() + 4 * C, 2 * C, dod.data_ptr(), C,
              dqbuf.data_ptr(), ldq, dkv.data_ptr(), dkv.data_ptr() + 4 * C, 2 * C, *geo)
    close(o, o64, what="attn o")
    close(dqbuf[:, :C], dq64, what="attn dq")
    close(dkv, dkv64, what="attn dkv")
    if ldq > C:
        assert bool(torch.isnan(dqbuf[:, C]).all()) and bool(torch.isnan(qbuf[:, C]).all())


PACKED = [(48, 3, (2, 4, 6, 4)), (192, 12, (1, 2, 2, 2)), (24, 3, (1, 2, 2, 2)), (12, 3, (1, 2, 2, 2))]


@pytest.mark.parametrize("C,heads,dims", PACKED, ids=[f"qkv-C{C}-heads{h}-hd{C // h}" for C, h, _ in PACKED])
def test_wattn_packed_qkv(ops, C, heads, dims):
    """ops.window_attn_fwd_qkv / _bwd_qkv: q, k, v as three pointers into one [T, 3C] matrix (ld = 3C), dq, dk, dv into one output --
    what the engine runs for every unfused self block.  Same kernel, same summation order as the split call: bit-equal to it."""
    ws = (2, 2, 2)
    q, kv, do = L.attn_inputs(dims, C)
    scale, o64, dq64, dkv64 = attn_want(q, kv, do, dims, heads, ws)
    qkv = dev(torch.cat([q, kv], 1))
    o = ops.window_attn_fwd_qkv(qkv, dims, heads, ws, scale)
    dqkv = ops.window_attn_bwd_qkv(qkv, dev(do), dims, heads, ws, scale)
    close(o, o64, what="qkv o")
    close(dqkv, torch.cat([dq64, dkv64], 1), what="qkv dqkv")
    o_split = ops.window_attn_fwd(dev(q), dev(kv), dims, heads, ws, scale)
    dq, dkv = ops.window_attn_bwd(dev(q), dev(kv), dev(do), dims, heads, ws, scale)
    assert torch.equal(o, o_split)
    assert torch.equal(dqkv, torch.cat([dq, dkv], 1))


@pytest.mark.parametrize("dims,C,heads,ws", L.LARGE_SCORE_CASES, ids=[f"scores60-C{c[1]}-heads{c[2]}" for c in L.LARGE_SCORE_CASES])
def test_wattn_large_scores(ops, dims, C, heads, ws):
    """q and k scaled until the scores reach +-60: expf(s - mx) spans e^-120..1 and the rows are close to one-hot.  Everything stays
    finite, and each tensor's error against float64 is at most 4 x the error of the fp32 CPU reference (`_attn_ref` and its autograd)
    on the same inputs: another summation order plus expf.  test_ln_attn_ref_cpu.py::test_large_score_yardstick prints that yardstick."""
    q, kv, do = L.large_score_inputs(dims, C, heads, ws)
    scale, o64, dq64, dkv64 = attn_want(q, kv, do, dims, heads, ws)
    yard = L.fp32_errors(G._attn_ref, q, kv, do, dims, heads, ws)
    o = ops.window_attn_fwd(dev(q), dev(kv), dims, heads, ws, scale)
    dq, dkv = ops.window_attn_bwd(dev(q), dev(kv), dev(do), dims, heads, ws, scale)
    report = []
    for name, got, want in (("o", o, o64), ("dq", dq, dq64), ("dkv", dkv, dkv64)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()), f"{name}: not finite"
        err = float((got - want).abs().max())
        print(f"large scores C={C} heads={heads} {name}: kernel err {err:.3e}, fp32 CPU err {yard[name]:.3e}, ratio {err / yard[name]:.2f}")
        report.append((name, err, yard[name]))
    for name, err, y in report:
        assert err <= 4 * y, f"{name}: max abs err {err:.3e} > 4 x {y:.3e} (the fp32 CPU reference's)"
