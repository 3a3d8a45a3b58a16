"""The bf16-operand referee of the matrix-core entry points (micf_linear_* and micf_conv3_*), in plain torch on the CPU.

The contract of MICF_DTYPE_BF16 (include/micformer_hip.h): both operands of a matrix-core product are rounded to bf16
(round-to-nearest-even) at the fragment read, the products are accumulated in fp32, and everything that is stored stays fp32.
A product of two bf16 values is exact in fp32, so the result is a deterministic function of the ROUNDED operands up to the order of
the fp32 additions.  Every function below therefore returns a `Ref` with

  want    the operation in float64 on the operands rounded with `rb` where the kernels round them: both operands of the product and
          nothing else.  Bias, residual, DropPath scale, GELU', and the accumulate-into term are NOT rounded and are applied after
          the product (the DropPath scale in particular multiplies the finished product: linear.hip's epilogues and block_scale());
  want32  the same with unrounded operands: what the fp32 mode, and every fallback that ignores `dtype`, computes;
  absdot  the same sum with every term replaced by its absolute value (|a| |w|^T + |bias| ...): the scale of the summation error;
  terms   the number of fp32 additions behind one output element.

Bias gradients are fp32 column sums of the UNROUNDED dy in both modes, so their want == want32.  Confirmed in the source:
gemm_dma.h::dma_tile_loop adds `Qb[r * 64 + tid]` -- the fp32 slab image in LDS, before any conversion -- and the workgroup's
DropPath scale multiplies the finished sum (gemm_dma_kernel: `csum * epi.block_scale()`); linear_grouped.hip does the same per
sample segment (`ctot += s * csum`); conv3_wgradx_b16_kernel adds the fp32 `vdy` it fetched, not the bf16 copy it commits to LDS.

`check` holds a result to a referee with two gates, `match` says which of the two referees a result agrees with.
Magnitudes are expected in the normal range (no subnormals, inf, NaN).
"""
import collections
import math

import torch
import torch.nn.functional as F

Ref = collections.namedtuple("Ref", "want want32 absdot terms")
Check = collections.namedtuple("Check", "ok l2 ratio worst")

GATE_MAX = 1e-5          # identical products, fp32 accumulation in another order (test_gpu_bf16.py, grouped weight gradient)
ULP = 2.0 ** -23


# ----------------------------------------------------------------------------- rounding
def rb(x):
    """fp32 -> bf16 (round-to-nearest-even) -> float64."""
    return x.detach().cpu().float().bfloat16().double()


def _exact(x):
    return x.detach().cpu().double()


def _mag(x):
    return x.detach().cpu().double().abs()


def _bits(x):
    return x.detach().cpu().float().contiguous().view(torch.int32).long() & 0xFFFFFFFF


def _from_bits(b):
    b = b & 0xFFFFFFFF
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32)


def rb_int(x):
    """RNE by integer arithmetic on the fp32 bit pattern: add 0x7FFF plus the last kept bit, drop the low half (the emulation that
    gemm_dma.h::pack_bf16's comment describes and that v_cvt_pk_bf16_f32 replaces)."""
    b = _bits(x)
    return _from_bits((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).double()


def truncate(x):
    """A wrong conversion: the low half of the fp32 pattern dropped (round toward zero)."""
    return _from_bits(_bits(x) & 0xFFFF0000).double()


def half_away(x):
    """A wrong conversion: ties rounded away from zero (add 0x8000, drop the low half)."""
    return _from_bits((_bits(x) + 0x8000) & 0xFFFF0000).double()


def ties(*shape, seed=0, scale=1.0):
    """fp32 values exactly halfway between two bf16 neighbours (low half of the pattern = 0x8000), last kept bit odd and even."""
    g = torch.Generator().manual_seed(seed)
    b = _bits((torch.randn(*shape, generator=g) * scale).bfloat16().float())
    return _from_bits(b | 0x8000)


# ----------------------------------------------------------------------------- the gates
def check(got, want, absdot, terms):
    """Gate 1: max|got - want| <= 1e-5 max|want|.  Gate 2, per element: |got - want| <= (terms + 8) 2^-23 absdot -- the worst case of a
    `terms`-long fp32 sum (gamma_n = n u / (1 - n u), u = 2^-24) with a factor 2; it bites on small elements and short sums, where
    gate 1 is slack.  -> Check(ok, relative L2 distance, worst ratio to bound 2, max|got - want| / max|want|)."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, f"shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if not bool(torch.isfinite(got).all()):
        return Check(False, math.inf, math.inf, math.inf)
    d = (got - want).abs()
    scale = max(float(want.abs().max()), 1e-300)
    bound = (terms + 8) * ULP * absdot
    ratio = torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d))
    ratio = float(ratio.max()) if ratio.numel() else 0.0
    worst = float(d.max()) / scale if d.numel() else 0.0
    l2 = float(d.norm() / want.norm().clamp_min(1e-300))
    return Check(worst <= GATE_MAX and ratio <= 1.0, l2, ratio, worst)


def match(got, ref):
    """-> (name of the referee `got` passes: "bf16" | "fp32" | "both" (want == want32, e.g. a bias gradient) | None, Check against it --
    against the nearer one when it passes neither)."""
    c16 = check(got, ref.want, ref.absdot, ref.terms)
    c32 = check(got, ref.want32, ref.absdot, ref.terms)
    if c16.ok and c32.ok:
        return "both", c16
    if c16.ok:
        return "bf16", c16
    if c32.ok:
        return "fp32", c32
    return None, (c16 if c16.worst <= c32.worst else c32)


def _ref(fn, terms):
    """fn(r, u): the operation with r applied to the product's operands and u to every unrounded term."""
    return Ref(fn(rb, _exact), fn(_exact, _exact), fn(_mag, _mag), terms)


# ----------------------------------------------------------------------------- pointwise
def gelu(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _rows(dp_scale, rows_per_sample, M, u):
    if dp_scale is None:
        return torch.ones(M, 1, dtype=torch.float64)
    return u(dp_scale).repeat_interleave(rows_per_sample)[:M, None]


def _cat(a1, a2):
    return a1 if a2 is None else torch.cat([a1.detach().cpu(), a2.detach().cpu()], 1)


# ----------------------------------------------------------------------------- nn.Linear
def linear_fwd(a1, w, bias=None, a2=None, resid=None, dp_scale=None, rows_per_sample=0):
    """lin = [a1|a2] W^T + bias, or resid + s * lin when resid is given.  (act = 1: lin is the pre-activation the kernel hands out;
    y is then held to gelu(that pre-activation) with the fp32 op tests' tolerance: the hardware erf is not part of this referee.)"""
    a = _cat(a1, a2)
    M, K = a.shape

    def fn(r, u):
        lin = r(a) @ r(w).t()
        if bias is not None:
            lin = lin + u(bias)
        if resid is not None:
            lin = u(resid) + _rows(dp_scale, rows_per_sample, M, u) * lin
        return lin

    return _ref(fn, K + (bias is not None) + 2 * (resid is not None))


def linear_bwd_data(dy, w, dp_scale=None, rows_per_sample=0, pre_act=None, base=None):
    """d[a1|a2] [M, K] = base + s * (dy W) * GELU'(pre_act); the caller joins the kernel's da1 | da2."""
    M, N = dy.shape

    def fn(r, u):
        d = _rows(dp_scale, rows_per_sample, M, u) * (r(dy) @ r(w))
        if pre_act is not None:
            d = d * u(gelu_grad(pre_act.detach().cpu()))
        if base is not None:
            d = d + u(base)
        return d

    return _ref(fn, N + (dp_scale is not None) + (pre_act is not None) + (base is not None))


def linear_bwd_weight(dy, a1, a2=None, dp_scale=None, rows_per_sample=0, a_gelu=False):
    """-> (dW [N, K] = sum_m s_m dy[m]^T A[m], dbias [N] = sum_m s_m dy[m]).  A = [a1|a2], or GELU(a1) (fp32 paths only).  The scale
    of a sample multiplies its finished product, so s is outside the rounding; dbias sums the unrounded dy."""
    a = _cat(a1, a2)
    if a_gelu:
        a = gelu(a.detach().cpu())
    M, N = dy.shape

    def fw(r, u):
        return (_rows(dp_scale, rows_per_sample, M, u) * r(dy)).t() @ r(a)

    def fb(r, u):
        return (_rows(dp_scale, rows_per_sample, M, u) * u(dy)).sum(0)

    extra = 1 + (M // rows_per_sample if dp_scale is not None else 0)       # the split / per-sample partial sums
    return _ref(fw, M + extra), _ref(fb, M + extra)


# ----------------------------------------------------------------------------- 3x3x3 convolution, stride 1, zero padding 1
def conv3(x1, x2, w, bias, dy, dims, base=None):
    """Channels-last x1 [T, c1] | x2 [T, c2], w [N, c1 + c2, 3, 3, 3], dy [T, N] -> dict of Ref: y [T, N], dx [T, c1 + c2] (+ base),
    dw, db -- F.conv3d and its autograd adjoints in float64."""
    B, D, H, W = dims
    x = _cat(x1, x2)
    T, Cin = x.shape
    N = w.shape[0]
    vol = lambda t, c: t.reshape(B, D, H, W, c).permute(0, 4, 1, 2, 3)
    tok = lambda t, c: t.permute(0, 2, 3, 4, 1).reshape(T, c)
    out = {k: [] for k in ("y", "dx", "dw", "db")}
    for r, u in ((rb, _exact), (_exact, _exact), (_mag, _mag)):
        xr, wr = vol(r(x), Cin).contiguous().requires_grad_(True), r(w).requires_grad_(True)
        y = F.conv3d(xr, wr, None, padding=1)
        gx, gw = torch.autograd.grad(y, (xr, wr), vol(r(dy), N).contiguous())
        y = tok(y.detach(), N)
        out["y"].append(y + u(bias) if bias is not None else y)
        gx = tok(gx, Cin)
        out["dx"].append(gx + u(base) if base is not None else gx)
        out["dw"].append(gw)
        out["db"].append(u(dy).sum(0))
    terms = {"y": 27 * Cin + 1, "dx": 27 * N + 1, "dw": T + 8, "db": T + 8}
    return {k: Ref(*v, terms[k]) for k, v in out.items()}


def conv_down(x, w, bias, dy):
    """Conv3d(k = s = 2) of PatchMerging on channels-last x [B, D, H, W, C] (odd extents zero-padded at the far side), dy
    [B, D', H', W', N] -> dict of Ref: y, dx, dw, db."""
    B, D, H, W, C = x.shape
    N = w.shape[0]
    pad = (0, W % 2, 0, H % 2, 0, D % 2)
    out = {k: [] for k in ("y", "dx", "dw", "db")}
    for r, u in ((rb, _exact), (_exact, _exact), (_mag, _mag)):
        xr, wr = r(x).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True), r(w).requires_grad_(True)
        y = F.conv3d(F.pad(xr, pad), wr, None, stride=2)
        gx, gw = torch.autograd.grad(y, (xr, wr), r(dy).permute(0, 4, 1, 2, 3).contiguous())
        out["y"].append(y.detach().permute(0, 2, 3, 4, 1) + u(bias))
        out["dx"].append(gx.permute(0, 2, 3, 4, 1))
        out["dw"].append(gw)
        out["db"].append(u(dy).reshape(-1, N).sum(0))
    M = dy.numel() // N
    terms = {"y": 8 * C + 1, "dx": N + 1, "dw": M + 8, "db": M + 8}
    return {k: Ref(*v, terms[k]) for k, v in out.items()}
