"""Shared by tests/test_gpu_block_oracle.py and tests/test_block_oracle_gates_cpu.py: the inputs of a fused block launch, the oracle's
value of every tensor the launch writes (oracle/micformer_ref.py in bf16-operand mode, any precision), the distance statistics, and
the gates.

TWO kinds of gate live in `Report`:

  add()   absolute gates against the oracle in fp32, calibrated for C = 48 on 2 x 32^3 tokens (and, with `frac_relax`, for C = 384 /
          head_dim 32): the two instantiations that have been pinned since rounds 5 and 6.  Unchanged.
  gate()  gates RELATIVE TO THE ORACLE'S OWN SPREAD, for every other width.  The referee is the oracle evaluated in fp64.  What a
          correct kernel may differ by is fp32 summation order plus the bf16 rounding ties that this noise tips the other way; the
          oracle evaluated in fp32 differs from the fp64 referee by exactly that kind of noise.  `spread()` measures that fp32-vs-fp64
          distance per tensor and statistic -- the maximum over both grids and 8 input seeds -- and the kernel is held to MARGIN = 4
          times it.  Kernel-vs-fp64 and fp32-vs-fp64 are two draws of the same tie noise; the 4 covers the heavy tail of a statistic
          that a handful of ties dominate and the sqrt(128 / 24) between the two grids.  It is a margin over the REFERENCE and is not
          fitted to any kernel's result.  The absolute caps of add() stay on top (relative L2 <= 2e-3 on input gradients, worst
          element <= 2e-2, `exact` quantities <= 1e-5).

Statistics (`stats`): relative L2; its coherent part (the norm of the MEAN error row: what a wrong bias, gain or per-sample factor
leaves in every row alike and tie noise, independent from row to row, does not -- added because a 2 % error of fc2's bias passed the
other statistics at C = 192 / head_dim 32 and C = 384 / head_dim 32); worst element over the scale; fraction of elements beyond 1e-3
of the scale (the 1e-4 fraction of add() is printed but not gated here: ONE tie that falls the other way moves a whole row of K
downstream values by more than 1e-4 of the scale, so the reference alone reaches 26 % at C = 384); for tensors the launch stores as
bf16 the fraction more than one bf16 step away.  A bf16-stored tensor is compared with the referee's value rounded the same way, in
every statistic.

The noise is bimodal.  A launch in which no early operand crossed a tie sits at 1e-6; one tie in q, k or P moves a row of the
attention output by 1e-4, LN2 and the bf16 roundings behind it then tip a few per cent of that row's operands, and the gradients of
the launch end up 1e-3 apart.  The maximum over 16 draws is therefore "a draw with such a cascade", and at C = 384 / head_dim 16
(cross, 24 tokens) the oracle's own spread of the q-path gradient, 2.1e-3, sits AT the absolute 2e-3 cap.

Count floor.  The two fractions are counts k / n, and their spread is the largest of 16 counts.  Where that largest count is 0 or 1,
four times it leaves no room for the Poisson tail of a count whose mean 16 draws bound only by ~0.2 (P(k >= 3 | mean 0.2) = 1e-3,
P(k >= 1) = 18 %), so a count gate is never below COUNT_FLOOR = 2 elements -- and, where the spread saw no element move at all, the
worst-element and relative-L2 gates are never below what those 2 elements would give if each moved by one bf16 step of the scale
(2^-8).  A defect moves a constant share of a tensor, not three of its elements (tests/test_block_oracle_gates_cpu.py).
"""
import math

import torch

EPS = 1e-5
GRIDS = ((1, 2, 6, 2), (2, 4, 4, 4))        # 3 windows: a half-empty last tile for TM 16 and TM 32, no scales | 16 windows, B = 2, DropPath scales
SAMPLER_GRID = (1, 4, 6, 2)
SEEDS = 8
MARGIN = 4.0
COUNT_FLOOR = 2
BF16_STEP = 2.0 ** -8
STATS = ("l2", "colmean", "worst", "far3", "step")


class pinned_threads:
    """The spread, the referee and the stand-ins are evaluated with a FIXED number of CPU threads: the fp32 summation order of a CPU
    GEMM follows the thread count, and with it which ties the fp32 oracle tips -- the gates would otherwise move with the machine."""

    def __enter__(self):
        self.prev = torch.get_num_threads()
        torch.set_num_threads(4)

    def __exit__(self, *exc):
        torch.set_num_threads(self.prev)
        return False


# ----------------------------------------------------------------------------- inputs
def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def make_params(C, hidden, attn, seed):
    """The values of test_gpu_block_fused.make_params, on the CPU."""
    k = 1.0 / math.sqrt(C)
    kh = 1.0 / math.sqrt(hidden)
    return {"norm1.weight": 1 + rnd((C,), seed + 1, 0.1), "norm1.bias": rnd((C,), seed + 2, 0.1),
            f"{attn}.q.weight": rnd((C, C), seed + 3, k), f"{attn}.q.bias": rnd((C,), seed + 4, 0.1),
            f"{attn}.kv.weight": rnd((2 * C, C), seed + 5, k), f"{attn}.kv.bias": rnd((2 * C,), seed + 6, 0.1),
            f"{attn}.proj.weight": rnd((C, C), seed + 7, k), f"{attn}.proj.bias": rnd((C,), seed + 8, 0.1),
            "norm2.weight": 1 + rnd((C,), seed + 9, 0.1), "norm2.bias": rnd((C,), seed + 10, 0.1),
            "mlp.fc1.weight": rnd((hidden, C), seed + 11, k), "mlp.fc1.bias": rnd((hidden,), seed + 12, 0.1),
            "mlp.fc2.weight": rnd((C, hidden), seed + 13, kh), "mlp.fc2.bias": rnd((C,), seed + 14, 0.1)}


def make_group(C, dims, kind, i, seed=0):
    """Group i (0 | 1) of a launch: CPU tensors {x, kvsrc | None, P, attn, s1, s2, dy}.  seed 0 = the inputs the GPU test launches;
    the other seeds exist for the spread.  DropPath scales are given when B > 1."""
    B, D, H, W = dims
    T = B * D * H * W
    o = 1000 * seed
    attn = "self_attn" if kind == "self" else "cross_attn"
    sc = lambda s: torch.rand(B, generator=torch.Generator().manual_seed(s + o)) + 0.5 if B > 1 else None
    return {"x": rnd((T, C), 3 + i + o), "kvsrc": rnd((T, C), 11 + i + o) if kind == "cross" else None,
            "P": make_params(C, 4 * C, attn, 20 + 40 * i + o), "attn": attn, "s1": sc(5 + i), "s2": sc(7 + i), "dy": rnd((T, C), 50 + i + o)}


def make_sampler_group(C, dims, i, seed=0):
    """Group i of a cross launch that samples its K/V source itself: {x, xa, P (with the offset head), attn}."""
    B, D, H, W = dims
    T = B * D * H * W
    o = 1000 * seed
    P = make_params(C, 4 * C, "cross_attn", 20 + 40 * i + o)
    P.update({"conv_offset.0.weight": rnd((16, 2 * C, 3, 3, 3), 41 + i + o, 1.0 / math.sqrt(27 * 2 * C)), "conv_offset.0.bias": rnd((16,), 42 + i + o, 0.1),
              "conv_offset.1.norm.weight": 1 + rnd((16,), 31 + i + o, 0.1), "conv_offset.1.norm.bias": rnd((16,), 32 + i + o, 0.1),
              "conv_offset.3.weight": rnd((3, 16, 1, 1, 1), 33 + i + o, 0.3)})
    return {"x": rnd((T, C), 3 + i + o), "xa": rnd((T, C), 15 + i + o), "P": P, "attn": "cross_attn"}


# ----------------------------------------------------------------------------- the oracle's value of everything a launch writes
def _tok(aux_w, dims, width):
    """(nW, 8, width) window-ordered capture -> [T, width] in token order."""
    from oracle import micformer_ref as R
    B, D, H, W = dims
    return R._from_windows(aux_w, (2, 2, 2), B, D, H, W).reshape(-1, width)


def _mlp_ln2_unrounded(R, x, P, pre):
    """oracle.mlp with ONE rounding point missing (the LN2 output enters fc1 as it is): a mutant for the gate test."""
    import torch.nn.functional as F
    h = R._cap("h", R._rg(F.linear(x, R._r(P[pre + "fc1.weight"]), P[pre + "fc1.bias"])))
    return F.linear(R._r(R._cap("g", R._GeluSavedBF16.apply(h))), R._r(P[pre + "fc2.weight"]), P[pre + "fc2.bias"])


def oracle_block(R, x, kv_given, P, attn, heads, s1, s2, mlp=None):
    """oracle.self_block, generalised to a GIVEN K/V source (the window-local part of a cross block once the sampling is done):
    composed from the oracle's own primitives; with kv_given None it IS oracle.self_block (asserted by both test files)."""
    B, D, H, W, _ = x.shape
    ws = (2, 2, 2)
    xn = R._cap("xn", R.layer_norm(x, P["norm1.weight"], P["norm1.bias"], EPS))
    src = xn if kv_given is None else R._cap("xs", kv_given)
    a = R.window_attention(R._to_windows(xn, ws), R._to_windows(src, ws), P, attn + ".", heads)
    x1 = R._cap("x1", x + R._rg(R._scale_per_sample(R._from_windows(a, ws, B, D, H, W), s1)))
    xn2 = R._cap("xn2", R.layer_norm(x1, P["norm2.weight"], P["norm2.bias"], EPS))
    y = R.mlp(xn2, P, "mlp.") if mlp is None else mlp(R, xn2, P, "mlp.")
    return x1 + R._rg(R._scale_per_sample(y, s2))


class _truncating:
    """Mutant: every bf16 rounding of the oracle truncates (round toward zero) instead of rounding to nearest even."""

    def __init__(self, R):
        self.R = R

    def __enter__(self):
        self.prev = self.R._rb

        def trunc(x):
            f = x.float().contiguous()
            return (f.view(torch.int32) & -65536).view(torch.float32).to(x.dtype)
        self.R._rb = trunc

    def __exit__(self, *exc):
        self.R._rb = self.prev
        return False


MUTANTS = ("truncate", "fc2 bias x 0.98", "s1 ignored on sample 0", "two rows of y swapped", "LN2 output unrounded")


def evaluate(g, dims, heads, dtype=torch.float32, stored_fp32=False, mutant=None):
    """Every tensor block_fwd / block_bwd write for group g, from the oracle in bf16-operand mode evaluated in `dtype`: a dict by the
    names of the report, [T, width] in token order (LayerNorm sums: [C]).  mutant: one of MUTANTS (None: the oracle as it is)."""
    from oracle import micformer_ref as R
    B, D, H, W = dims
    C = g["x"].shape[1]
    T = B * D * H * W
    cross = g["kvsrc"] is not None
    to = lambda t: None if t is None else t.detach().to(dtype)
    P = {k: to(v) for k, v in g["P"].items()}
    s1, s2 = to(g["s1"]), to(g["s2"])
    if mutant == "fc2 bias x 0.98":
        P["mlp.fc2.bias"] = P["mlp.fc2.bias"] * 0.98
    if mutant == "s1 ignored on sample 0":
        assert s1 is not None, "this mutant needs a grid with DropPath scales"
        s1 = s1.clone()
        s1[0] = 1.0
    x = to(g["x"]).reshape(B, D, H, W, C).requires_grad_(True)
    kv_given = to(g["kvsrc"]).reshape(B, D, H, W, C).requires_grad_(True) if cross else None
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items() if k.startswith("norm")}
    Pq = dict(P, **leaves)
    mlp = _mlp_ln2_unrounded if mutant == "LN2 output unrounded" else None
    import contextlib
    with (_truncating(R) if mutant == "truncate" else contextlib.nullcontext()), R.bf16_operands(stored_fp32=stored_fp32), R.capture() as aux:
        y = oracle_block(R, x, kv_given, Pq, g["attn"], heads, s1, s2, mlp)
        (y * to(g["dy"]).reshape(y.shape)).sum().backward()
    y = y.detach().reshape(T, C)
    if mutant == "two rows of y swapped":        # rows 2 and 5 of window 1
        idx = R._to_windows(torch.arange(T).reshape(B, D, H, W, 1), (2, 2, 2))[1, :, 0]
        y = y.clone()
        y[[int(idx[2]), int(idx[5])]] = y[[int(idx[5]), int(idx[2])]]
    xd, x1d = x.detach().reshape(T, C), aux["x1"].detach().reshape(T, C)
    out = {"y": y, "x1": x1d,
           "LN1 mean": xd.mean(1), "LN1 rstd": (xd.var(1, unbiased=False) + EPS).rsqrt(),
           "LN2 mean": x1d.mean(1), "LN2 rstd": (x1d.var(1, unbiased=False) + EPS).rsqrt(),
           "xn": aux["xn"].reshape(T, C), "q": _tok(aux["q_w"], dims, C), "kv": _tok(aux["kv_w"], dims, 2 * C), "o": _tok(aux["o_w"], dims, C),
           "xn2": aux["xn2"].reshape(T, C), "h": aux["h"].reshape(T, 4 * C), "g": aux["g"].reshape(T, 4 * C)}
    if cross:
        out.update({"dxn (q path)": aux["xn"].grad.reshape(T, C), "dxs": kv_given.grad.reshape(T, C), "dx1 copy": aux["x1"].grad.reshape(T, C)})
    else:
        out.update({"dx": x.grad.reshape(T, C), "d ln1 gain": leaves["norm1.weight"].grad, "d ln1 bias": leaves["norm1.bias"].grad})
    out.update({"d ln2 gain": leaves["norm2.weight"].grad, "d ln2 bias": leaves["norm2.bias"].grad,
                "dq": _tok(aux["q_w"].grad, dims, C), "dkv": _tok(aux["kv_w"].grad, dims, 2 * C), "dh": aux["h"].grad.reshape(T, 4 * C),
                "dx1": aux["x1"].grad.reshape(T, C)})
    return {k: v.detach() for k, v in out.items()}


def evaluate_sampler(g, dims, heads, dtype=torch.float32):
    """oracle.cross_block end to end (offset head, reference points, trilinear sampling, block), forward only: the tensors the
    fused-sampling launch writes, plus "hid" (the 3^3 offset convolution's output, which the launch is handed)."""
    from oracle import micformer_ref as R
    B, D, H, W = dims
    C = g["x"].shape[1]
    T = B * D * H * W
    P = {k: v.to(dtype) for k, v in g["P"].items()}
    with torch.no_grad(), R.bf16_operands(), R.capture() as aux:
        y = R.cross_block(g["x"].to(dtype).reshape(B, D, H, W, C), g["xa"].to(dtype).reshape(B, D, H, W, C), P, "", heads, (2, 2, 2), None, None, EPS)
    return {"flow": aux["flow"].reshape(T, 3), "kvs16": aux["xs"].reshape(T, C), "q": _tok(aux["q_w"], dims, C), "kv": _tok(aux["kv_w"], dims, 2 * C),
            "o": _tok(aux["o_w"], dims, C), "x1": aux["x1"].reshape(T, C), "h": aux["h"].reshape(T, 4 * C), "y": y.reshape(T, C),
            "hid": aux["hid"].reshape(T, 16)}


# which tensors a launch stores as bf16: st16 = ops.block_saves_bf16(C, heads).  The fc1 pre-activation is half-width in bf16 mode on
# EVERY path (ops.block_fwd: h_dtype; block_wide.hip stores it through st_h4<true>).
BF16_IF_ST16 = ("xn", "q", "kv", "o", "xn2", "g", "dq", "dkv", "dh", "dx1", "kvs16")
BF16_ALWAYS = ("h",)
EXACT = ("LN1 mean", "LN1 rstd", "flow")                              # fp32 quantities with no rounded operand upstream
INPUT_GRADS = ("dx", "dxn (q path)", "dxs", "dx1 copy", "d ln1 gain", "d ln1 bias", "d ln2 gain", "d ln2 bias")   # relative L2 capped at 2e-3


def stored_bf16(name, st16):
    return name in BF16_ALWAYS or (st16 and name in BF16_IF_ST16)


# ----------------------------------------------------------------------------- statistics
def _rb(t):
    return t.float().bfloat16().double()


def stats(got, want, bf16):
    """Distance statistics of got against want (both brought to fp64); bf16: the tensor is stored as bf16, so want is rounded first."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(got).all(), "non-finite"
    if bf16:
        want = _rb(want)
    scale = max(float(want.abs().max()), 1e-30)
    d = (got - want).abs()
    s = {"scale": scale, "n": got.numel(), "rms": float(want.norm()) / math.sqrt(got.numel()) / scale,
         "l2": float(d.norm() / want.norm().clamp_min(1e-300)), "worst": float(d.max()) / scale,
         "far3": float((d > 1e-3 * scale).double().mean()), "far4": float((d > 1e-4 * scale).double().mean())}
    if got.dim() == 2:
        # the COHERENT part of the error: the norm of the mean error row over the RMS row norm.  Tie noise is independent from row to
        # row, so this is ~ rel-L2 / sqrt(rows); a wrong or missing bias, gain or per-sample factor errs the same way in every row
        s["colmean"] = float((got - want).mean(0).norm() / (want.norm() / math.sqrt(got.shape[0])).clamp_min(1e-300))
    if bf16:
        step = 2.0 ** -7 * torch.maximum(got.abs(), want.abs())
        s["step"] = float((d > step * 1.0001 + 1e-30).double().mean())
    return s


_SPREAD = {}
_REF = {}


def reference(C, heads, kind, dims, st16, seed=0, i=0, dtype=torch.float64):
    """evaluate() of group i of the seed's launch, cached (the fp64 referee of the tests, and the draws of the spread)."""
    key = (C, heads, kind, dims, st16, seed, i, dtype)
    if key not in _REF:
        with pinned_threads():
            _REF[key] = evaluate(make_group(C, dims, kind, i, seed), dims, heads, dtype, stored_fp32=not st16)
    return _REF[key]


def spread(C, heads, kind, st16):
    """{tensor name: {statistic: the oracle's fp32-vs-fp64 distance, maximum over GRIDS and SEEDS input seeds}}, computed once per
    (C, heads, kind).  st16: the launch stores bf16 (ops.block_saves_bf16); False places the roundings where the fp32-storing path
    has them and compares its saved tensors unrounded."""
    key = (C, heads, kind, st16)
    if key not in _SPREAD:
        sp = {}
        for dims in GRIDS:
            for seed in range(SEEDS):
                r64 = reference(C, heads, kind, dims, st16, seed)
                with pinned_threads():
                    r32 = evaluate(make_group(C, dims, kind, 0, seed), dims, heads, torch.float32, stored_fp32=not st16)
                if seed:                                      # (seed 0 is the GPU test's referee: kept)
                    del _REF[(C, heads, kind, dims, st16, seed, 0, torch.float64)]
                for name in r64:
                    bf = stored_bf16(name, st16)
                    s = stats(_rb(r32[name]) if bf else r32[name], r64[name], bf)
                    m = sp.setdefault(name, {})
                    for k in STATS + ("far4",):
                        if k in s:
                            m[k] = max(m.get(k, 0.0), s[k])
        _SPREAD[key] = sp
    return _SPREAD[key]


_SPREAD_S = {}


def spread_sampler(C, heads):
    """The same for the fused-sampling launch (forward, SAMPLER_GRID, SEEDS seeds): these shapes all store bf16."""
    key = (C, heads)
    if key not in _SPREAD_S:
        sp = {}
        for seed in range(SEEDS):
            g = make_sampler_group(C, SAMPLER_GRID, 0, seed)
            with pinned_threads():
                r64, r32 = evaluate_sampler(g, SAMPLER_GRID, heads, torch.float64), evaluate_sampler(g, SAMPLER_GRID, heads, torch.float32)
            for name in r64:
                bf = stored_bf16(name, True)
                s = stats(_rb(r32[name]) if bf else r32[name], r64[name], bf)
                m = sp.setdefault(name, {})
                for k in STATS + ("far4",):
                    if k in s:
                        m[k] = max(m.get(k, 0.0), s[k])
        _SPREAD_S[key] = sp
    return _SPREAD_S[key]


def gates(sp, s):
    """{statistic: gate} for one tensor from its spread sp and the statistics s of the run under test (for n, rms: properties of the
    REFEREE's tensor, not of the value under test): MARGIN x spread, the count floor of the module docstring, the absolute caps."""
    n, floor = s["n"], COUNT_FLOOR / s["n"]
    g = {"l2": MARGIN * sp["l2"], "worst": MARGIN * sp["worst"], "far3": max(MARGIN * sp["far3"], floor)}
    if "colmean" in sp:
        g["colmean"] = MARGIN * sp["colmean"]
    if sp["worst"] == 0.0:                                    # the spread saw no element move: COUNT_FLOOR elements, one bf16 step of the scale each
        g["worst"] = BF16_STEP
        g["l2"] = BF16_STEP * math.sqrt(COUNT_FLOOR / n) / max(s["rms"], 1e-30)
        if "colmean" in sp:
            g["colmean"] = g["l2"]
    if "step" in sp:
        g["step"] = max(MARGIN * sp["step"], floor)
    return g


class Report:
    """Collects (name, statistics) rows and the failed gates; printed in full so a run documents the measured distances."""

    def __init__(self, frac_relax=1.0):
        self.rows, self.bad, self.frac_relax, self.ratios = [], [], frac_relax, {}
        self.cap_within_spread = []     # entries of `bad` where an ABSOLUTE cap failed that the oracle's own fp32-vs-fp64 spread reaches

    # ---- the absolute gates of the C = 48 / C = 384 head_dim 32 runs (fp32 oracle)
    def add(self, name, got, want, frac_gate, bf16=False, far=1e-4, worst=2e-2, exact=False, l2=None):
        got, want = got.detach().double().cpu(), want.detach().double().cpu()
        assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
        assert torch.isfinite(got).all(), f"{name}: non-finite"
        scale = max(float(want.abs().max()), 1e-30)
        d = (got - want).abs()
        if frac_gate is not None and frac_gate > 0:
            # (ONE rounding tie that fell the other way moves up to a window's worth of downstream values -- 8 token rows of the
            # tensor: on a launch of a few dozen tokens that alone is a third of it, whatever the channel count)
            rows = got.numel() // got.shape[-1] if got.dim() > 1 else got.numel()
            frac_gate = min(1.0, max(frac_gate * self.frac_relax, 8.4 * max(1.0, self.frac_relax / 4) / rows))
        l2_ = float(d.norm() / want.norm().clamp_min(1e-300))
        mx = float(d.max()) / scale
        frac_far = float((d > far * scale).double().mean())
        row = f"  {name:12s} scale {scale:9.3e}  rel-L2 {l2_:8.2e}  worst {mx:8.2e}  further than {far:.0e} of the scale: {frac_far:8.2e}"
        if l2 is not None and l2 < l2_:
            self.bad.append(f"{name}: relative L2 distance {l2_:.2e} (gate {l2:.0e})")
        if bf16:
            wb = want.float().bfloat16().double()          # (the kernel stored bf16: compare with the oracle's value rounded the same way)
            step = 2.0 ** -7 * torch.maximum(got.abs(), wb.abs())
            frac_step = float(((got - wb).abs() > step * 1.0001 + 1e-30).double().mean())
            row += f"  more than one bf16 step: {frac_step:8.2e}"
            if frac_gate is not None and frac_step > frac_gate:
                self.bad.append(f"{name}: {frac_step:.2e} of the bf16 values more than one step from the oracle (gate {frac_gate:.0e})")
        elif frac_gate is not None and frac_far > frac_gate:
            self.bad.append(f"{name}: {frac_far:.2e} of the elements further than {far:.0e} of the scale (gate {frac_gate:.0e})")
        if mx > worst:
            self.bad.append(f"{name}: worst element {mx:.2e} of the scale (gate {worst:.0e})")
        if exact and mx > 1e-5:
            self.bad.append(f"{name}: {mx:.2e} (an fp32 quantity with no rounded operand upstream: gate 1e-5)")
        self.rows.append(row)

    # ---- the gates relative to the oracle's spread (fp64 referee)
    def gate(self, name, key, got, want, sp, st16):
        """key: the tensor's name in evaluate() / spread (name carries the group prefix)."""
        bf = stored_bf16(key, st16)
        s = stats(got, want, bf)
        row = f"  {name:15s}{' bf16' if bf else ' fp32'} scale {s['scale']:8.2e} |"
        if key in EXACT:
            row += f" worst {s['worst']:8.2e} (gate 1e-5: an fp32 quantity with no rounded operand upstream)"
            if s["worst"] > 1e-5:
                self.bad.append(f"{name}: {s['worst']:.2e} (an fp32 quantity with no rounded operand upstream: gate 1e-5)")
            self.rows.append(row)
            return
        g = gates(sp[key], s)
        g["worst"] = min(g["worst"], 2e-2)
        caps = {"worst": 2e-2}
        if key in INPUT_GRADS:
            caps["l2"] = 2e-3
            g["l2"] = min(g["l2"], 2e-3)
        label = {"l2": "rel-L2", "colmean": "coherent", "worst": "worst", "far3": ">1e-3", "step": ">1 step"}
        for k in STATS:
            if k not in g:
                continue
            row += f" {label[k]} {sp[key][k]:7.1e}/{g[k]:7.1e}/{s[k]:7.1e} |"
            if s[k] > g[k]:
                self.bad.append(f"{name}: {label[k]} {s[k]:.2e} over the gate {g[k]:.2e} (oracle fp32-vs-fp64 spread {sp[key][k]:.2e})")
                if k in caps and g[k] == caps[k] and sp[key][k] >= caps[k]:
                    self.cap_within_spread.append(self.bad[-1])
            if sp[key][k] > 0:
                self.ratios[k] = max(self.ratios.get(k, 0.0), s[k] / sp[key][k])
        row += f" >1e-4 {sp[key]['far4']:7.1e}/   -   /{s['far4']:7.1e}"
        self.rows.append(row)

    def done(self, title):
        print("\n" + title + "\n" + "\n".join(self.rows))
        if self.ratios:
            print("  largest measured / spread: " + "  ".join(f"{k} {v:.2f}" for k, v in self.ratios.items()))
        assert not self.bad, "\n".join(self.bad)
