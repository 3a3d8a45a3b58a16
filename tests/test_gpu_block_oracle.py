"""The fused block launches DIRECTLY against the oracle: micf_block_fwd / micf_block_bwd in the benched
arithmetic mode, EVERY instantiation the dispatch has (micf_block_tile_tokens / MICF_BF in csrc/block_fwd.hip):

    C / head_dim   kernel                                                gates
    48 / 16        wave-private and tile (TJ 2), 2 x 32^3 tokens         absolute, fp32 oracle (Report.add)
    384 / 32       tile                                                  absolute x FRAC_RELAX 8, fp32 oracle -- and the spread gates
    96 / 16        tile, forward TJ 1, backward TJ 2                     spread of the oracle, fp64 referee (Report.gate)
    192 / 16, 96 / 32, 192 / 32   tile                                   spread
    384 / 16       few-token decomposition (block_wide.hip)              spread, oracle in its "stored in fp32" form

against oracle.self_block / cross_block evaluated with `oracle.bf16_operands()`: the SAME algorithm with the operands of
every matrix product rounded to bf16 at the points the kernels round them (LN outputs, sampled K/V source, weights, q * scale, k, v,
P, attention output, GELU output; the adjoint's dY operands), fp32 everywhere else.

What can still differ is (a) fp32 summation order and the hardware exp / erf forms (1e-6-class) and (b) a bf16 rounding that falls
the other way where (a) moved a value across a tie: ONE operand element off by one bf16 step (2^-8 of its size), which moves a few
downstream values by up to ~1e-2 of the tensor's scale.  Running the oracle itself in fp32 and in fp64 shows exactly that
signature (tools/scratch calibration, 2 x 32^3 tokens): at most 0.3 % of a tensor's elements (1.2 % of a gradient's) further than
1e-4 of the scale apart, at most 0.05 % (0.3 %) of the bf16-stored values more than one bf16 step apart, worst element 4e-3 of the
scale.  The absolute FORWARD gates are those numbers with headroom (measured on MI355X: y 5e-5 relative L2 / 0.1 % of the elements beyond
1e-4 of the scale; at most 0.1 % of any saved bf16 tensor more than one bf16 step from the oracle; LayerNorm statistics and the
sampling flow to 2e-7) -- a kernel that rounds at another point, drops a term or mis-indexes a row moves EVERY element.  The BACKWARD is
held to the same kind of gates: the oracle's adjoint re-reads what the forward stored as bf16 and rounds where the kernels round.

Those fraction gates do not transfer to the other widths (one tie moves a whole row of K downstream values: the oracle in fp32 and in
fp64 already differ beyond 1e-4 of the scale in 26 % of dx at C = 384), so the other widths are held to gates computed IN the test
from the oracle's own fp32-vs-fp64 spread: tests/block_oracle_gates.py, whose teeth tests/test_block_oracle_gates_cpu.py shows.
Two grids per width, two groups per launch: (1, 2, 6, 2) -- 3 windows, a half-empty last tile, no DropPath scales -- and (2, 4, 4, 4)
-- 16 windows, B = 2, a per-sample scale boundary inside the launch.

GPU RUN (MI355X, 43 passed).  Largest measured / spread per launch (gate: 4), statistics l2 = relative L2, colmean = its
coherent part, worst = worst element, far3 = fraction beyond 1e-3 of the scale, step = fraction more than one bf16 step away:

    C  96 /  6 heads  self             (1, 2, 6, 2)  l2 0.34  colmean 0.61  worst 0.36  step 0.21  far3 0.14
    C  96 /  6 heads  cross            (1, 2, 6, 2)  l2 0.65  colmean 0.66  worst 0.77  step 0.44  far3 0.50
    C  96 /  6 heads  self             (2, 4, 4, 4)  l2 0.73  colmean 0.32  worst 1.00  step 0.31  far3 0.28
    C  96 /  6 heads  cross            (2, 4, 4, 4)  l2 1.08  colmean 0.97  worst 2.10  step 0.94  far3 1.50
    C  96 /  3 heads  self             (1, 2, 6, 2)  l2 0.53  colmean 0.45  worst 1.00  far3 0.20  step 0.25
    C  96 /  3 heads  cross            (1, 2, 6, 2)  l2 0.05  colmean 0.05  worst 0.06  far3 0.00  step 0.00
    C  96 /  3 heads  self             (2, 4, 4, 4)  l2 1.02  colmean 0.43  worst 2.29  far3 1.88  step 0.30
    C  96 /  3 heads  cross            (2, 4, 4, 4)  l2 0.97  colmean 0.97  worst 1.00  far3 0.00  step 0.19
    C 192 / 12 heads  self             (1, 2, 6, 2)  l2 0.24  colmean 0.28  worst 0.44  far3 0.07  step 0.11
    C 192 / 12 heads  cross            (1, 2, 6, 2)  l2 1.17  colmean 2.71  worst 1.00  far3 1.20  step 1.13
    C 192 / 12 heads  self             (2, 4, 4, 4)  l2 1.00  colmean 0.73  worst 1.10  far3 1.00  step 0.80
    C 192 / 12 heads  cross            (2, 4, 4, 4)  l2 1.18  colmean 1.09  worst 1.34  far3 1.15  step 1.15
    C 192 /  6 heads  self             (1, 2, 6, 2)  l2 0.16  colmean 0.15  worst 0.34  far3 0.02  step 0.04
    C 192 /  6 heads  cross            (1, 2, 6, 2)  l2 1.17  colmean 2.71  worst 0.66  far3 0.13  step 0.23
    C 192 /  6 heads  self             (2, 4, 4, 4)  l2 0.98  colmean 0.73  worst 1.30  far3 1.67  step 0.75
    C 192 /  6 heads  cross            (2, 4, 4, 4)  l2 1.01  colmean 1.01  worst 1.56  far3 1.06  step 1.00
    C 384 / 24 heads  self             (1, 2, 6, 2)  l2 1.04  colmean 1.35  worst 1.14  far3 2.88  step 0.49
    C 384 / 24 heads  cross            (1, 2, 6, 2)  l2 1.04  colmean 1.11  worst 0.95  far3 0.40  step 0.03
    C 384 / 24 heads  self             (2, 4, 4, 4)  l2 0.96  colmean 0.42  worst 1.11  far3 0.39  step 0.24
    C 384 / 24 heads  cross            (2, 4, 4, 4)  l2 0.96  colmean 0.49  worst 1.12  far3 0.75  step 0.07
    C 384 / 12 heads  self             (1, 2, 6, 2)  l2 0.41  colmean 0.83  worst 0.77  far3 0.56  step 0.42
    C 384 / 12 heads  cross            (1, 2, 6, 2)  l2 1.10  colmean 1.18  worst 1.00  far3 1.29  step 1.28
    C 384 / 12 heads  self             (2, 4, 4, 4)  l2 0.53  colmean 0.42  worst 0.92  far3 0.71  step 0.45
    C 384 / 12 heads  cross            (2, 4, 4, 4)  l2 0.94  colmean 0.68  worst 1.68  far3 0.69  step 0.79
    C  96 /  6 heads  cross + sampling (1, 4, 6, 2)  l2 1.00  colmean 1.00  worst 1.24  step 1.00  far3 1.00
    C  96 /  3 heads  cross + sampling (1, 4, 6, 2)  l2 1.00  colmean 1.00  worst 1.11  step 1.00  far3 0.00
    C 192 / 12 heads  cross + sampling (1, 4, 6, 2)  l2 1.00  colmean 1.00  worst 1.00  step 1.00  far3 1.00
    C 192 /  6 heads  cross + sampling (1, 4, 6, 2)  l2 1.00  colmean 1.00  worst 1.00  step 1.00  far3 1.00
    C 384 / 12 heads  cross + sampling (1, 4, 6, 2)  l2 0.29  colmean 0.28  worst 0.90  step 0.08  far3 0.09

The whole report of one of them (group 0; per statistic: oracle fp32-vs-fp64 spread / gate / measured):

C 96, 6 heads, cross pair, dims (2, 4, 4, 4): distance to the oracle in fp64; per statistic: oracle fp32-vs-fp64 spread / gate / measured
  g0.y            fp32 scale 5.30e+00 | rel-L2 1.9e-04/7.4e-04/6.6e-05 | coherent 3.8e-05/1.5e-04/6.3e-06 | worst 6.1e-04/2.5e-03/4.6e-04 | >1e-3 0.0e+00/1.6e-04/0.0e+00 | >1e-4 2.9e-02/   -   /6.0e-03
  g0.x1           fp32 scale 4.44e+00 | rel-L2 3.9e-05/1.5e-04/2.4e-05 | coherent 5.2e-06/2.1e-05/2.7e-06 | worst 2.3e-04/9.1e-04/1.8e-04 | >1e-3 0.0e+00/1.6e-04/0.0e+00 | >1e-4 2.3e-03/   -   /9.8e-04
  g0.LN1 mean     fp32 scale 3.74e-01 | worst 1.27e-07 (gate 1e-5: an fp32 quantity with no rounded operand upstream)
  g0.LN1 rstd     fp32 scale 1.16e+00 | worst 1.25e-07 (gate 1e-5: an fp32 quantity with no rounded operand upstream)
  g0.LN2 mean     fp32 scale 3.22e-01 | rel-L2 1.6e-05/6.2e-05/1.4e-05 | worst 4.7e-05/1.9e-04/4.7e-05 | >1e-3 0.0e+00/1.6e-02/0.0e+00 | >1e-4 0.0e+00/   -   /0.0e+00
  g0.LN2 rstd     fp32 scale 1.13e+00 | rel-L2 3.2e-06/1.3e-05/1.6e-06 | worst 2.2e-05/8.9e-05/1.3e-05 | >1e-3 0.0e+00/1.6e-02/0.0e+00 | >1e-4 0.0e+00/   -   /0.0e+00
  g0.xn           bf16 scale 3.94e+00 | rel-L2 1.0e-05/4.1e-05/0.0e+00 | coherent 2.1e-06/8.4e-06/0.0e+00 | worst 1.3e-04/5.3e-04/0.0e+00 | >1e-3 0.0e+00/1.6e-04/0.0e+00 | >1 step 8.1e-05/3.3e-04/0.0e+00 | >1e-4 4.3e-04/   -   /0.0e+00
  g0.q            bf16 scale 3.94e+00 | rel-L2 4.6e-05/1.9e-04/1.1e-09 | coherent 9.5e-06/3.8e-05/9.4e-11 | worst 5.1e-04/2.1e-03/3.0e-08 | >1e-3 0.0e+00/1.6e-04/0.0e+00 | >1 step 4.3e-04/1.7e-03/8.1e-05 | >1e-4 8.7e-04/   -   /0.0e+00
  g0.kv           bf16 scale 4.97e+00 | rel-L2 2.5e-05/1.0e-04/2.5e-05 | coherent 2.3e-06/9.0e-06/2.2e-06 | worst 7.9e-04/3.1e-03/7.9e-04 | >1e-3 0.0e+00/8.1e-05/0.0e+00 | >1 step 0.0e+00/8.1e-05/0.0e+00 | >1e-4 8.1e-05/   -   /4.1e-05
  g0.o            bf16 scale 2.55e+00 | rel-L2 9.8e-05/3.9e-04/8.8e-05 | coherent 1.1e-05/4.5e-05/9.4e-06 | worst 1.2e-03/4.6e-03/1.2e-03 | >1e-3 8.1e-05/3.3e-04/8.1e-05 | >1 step 4.3e-04/1.7e-03/4.1e-04 | >1e-4 1.7e-03/   -   /9.0e-04
  g0.xn2          bf16 scale 3.81e+00 | rel-L2 1.7e-04/6.7e-04/7.2e-05 | coherent 3.4e-05/1.4e-04/6.4e-06 | worst 2.1e-03/8.4e-03/1.0e-03 | >1e-3 5.7e-04/2.3e-03/2.4e-04 | >1 step 8.7e-04/3.5e-03/1.6e-04 | >1e-4 2.2e-03/   -   /1.1e-03
  g0.h            bf16 scale 4.09e+00 | rel-L2 3.2e-04/1.3e-03/1.8e-04 | coherent 6.6e-05/2.6e-04/1.5e-05 | worst 3.8e-03/1.5e-02/1.9e-03 | >1e-3 2.5e-03/1.0e-02/3.5e-04 | >1 step 2.8e-03/1.1e-02/7.1e-04 | >1e-4 9.9e-03/   -   /2.5e-03
  g0.g            bf16 scale 4.09e+00 | rel-L2 3.5e-04/1.4e-03/1.7e-04 | coherent 7.1e-05/2.8e-04/1.6e-05 | worst 3.8e-03/1.5e-02/1.9e-03 | >1e-3 1.6e-03/6.5e-03/1.2e-04 | >1 step 2.2e-03/8.7e-03/6.3e-04 | >1e-4 8.6e-03/   -   /1.9e-03
  g0.dxn (q path) fp32 scale 2.72e+00 | rel-L2 7.8e-04/2.0e-03/3.9e-04 | coherent 1.4e-04/5.7e-04/3.4e-05 | worst 2.4e-03/9.8e-03/1.5e-03 | >1e-3 7.4e-03/3.0e-02/4.9e-04 | >1e-4 3.7e-02/   -   /2.3e-02
  g0.dxs          fp32 scale 3.91e+00 | rel-L2 8.1e-04/2.0e-03/3.7e-04 | coherent 2.0e-04/7.9e-04/4.0e-05 | worst 2.1e-03/8.3e-03/7.2e-04 | >1e-3 3.4e-03/1.4e-02/0.0e+00 | >1e-4 2.4e-01/   -   /7.3e-02
  g0.dx1 copy     fp32 scale 4.64e+00 | rel-L2 1.3e-04/5.3e-04/4.0e-05 | coherent 2.7e-05/1.1e-04/3.4e-06 | worst 4.3e-04/1.7e-03/2.5e-04 | >1e-3 0.0e+00/1.6e-04/0.0e+00 | >1e-4 2.3e-02/   -   /2.5e-03
  g0.d ln2 gain   fp32 scale 1.62e+01 | rel-L2 3.0e-04/1.2e-03/9.1e-05 | worst 4.7e-04/1.9e-03/1.2e-04 | >1e-3 0.0e+00/2.1e-02/0.0e+00 | >1e-4 2.4e-01/   -   /3.1e-02
  g0.d ln2 bias   fp32 scale 1.70e+01 | rel-L2 2.5e-04/1.0e-03/7.2e-05 | worst 2.4e-04/9.7e-04/9.1e-05 | >1e-3 0.0e+00/2.1e-02/0.0e+00 | >1e-4 2.5e-01/   -   /0.0e+00
  g0.dq           bf16 scale 4.19e+00 | rel-L2 7.2e-04/2.9e-03/4.1e-04 | coherent 1.5e-04/5.9e-04/3.7e-05 | worst 1.9e-03/7.5e-03/1.9e-03 | >1e-3 3.5e-03/1.4e-02/1.6e-04 | >1 step 1.2e-02/4.7e-02/6.9e-03 | >1e-4 2.7e-02/   -   /1.1e-02
  g0.dkv          bf16 scale 5.28e+00 | rel-L2 8.7e-04/3.5e-03/3.8e-04 | coherent 2.1e-04/8.5e-04/4.4e-05 | worst 3.0e-03/1.2e-02/1.5e-03 | >1e-3 6.5e-03/2.6e-02/8.1e-05 | >1 step 2.1e-02/8.6e-02/7.1e-03 | >1e-4 5.4e-02/   -   /1.1e-02
  g0.dh           bf16 scale 2.19e+00 | rel-L2 2.5e-04/9.9e-04/9.0e-05 | coherent 5.1e-05/2.0e-04/7.8e-06 | worst 1.8e-03/7.2e-03/1.3e-03 | >1e-3 1.1e-04/4.3e-04/2.0e-05 | >1 step 1.8e-03/7.4e-03/3.7e-04 | >1e-4 4.3e-03/   -   /8.7e-04
  g0.dx1          bf16 scale 4.62e+00 | rel-L2 3.3e-04/1.3e-03/1.9e-04 | coherent 6.7e-05/2.7e-04/1.7e-05 | worst 3.4e-03/1.4e-02/3.4e-03 | >1e-3 1.7e-03/6.9e-03/3.3e-04 | >1 step 3.5e-03/1.4e-02/1.6e-04 | >1e-4 1.1e-02/   -   /2.0e-03
  g0.dy16      scale 4.020e+00  rel-L2 1.66e-03  worst 2.71e-03  further than 1e-04 of the scale: 6.52e-01  more than one bf16 step: 0.00e+00
  g0.kvs16     scale 3.797e+00  rel-L2 1.69e-03  worst 2.05e-03  further than 1e-04 of the scale: 6.69e-01  more than one bf16 step: 0.00e+00
"""
import pytest
import torch

import block_oracle_gates as G
from block_oracle_gates import EPS, Report

pytestmark = pytest.mark.gpu

NEW_WIDTHS = [(96, 6), (96, 3), (192, 12), (192, 6), (384, 24), (384, 12)]
# (forward, backward) tokens per tile: the instantiation each width must reach (micf_block_tile_tokens)
TILE_TOKENS = {(48, 3): (32, 32), (96, 6): (16, 32), (96, 3): (16, 16), (192, 12): (16, 16), (192, 6): (16, 16), (384, 24): (16, 16),
               (384, 12): (16, 16)}
# The "fraction of elements further than 1e-4 of the scale" gates of Report.add are calibrated on C = 48 (sums over 48 ... 192 operands).  A value is
# off by more than fp32 noise only downstream of a bf16 rounding TIE that fell the other way in the kernel's summation order; both the
# chance of a tie (fp32 noise of a sum ~ sqrt(K) ulp against a fixed bf16 step) and the number of values downstream of one (K operands
# per output) grow with the channel count, so the C = 384 / head_dim 32 run multiplies the FRACTION gates by 8 (the "more than one bf16 step" fractions too).  The rel-L2 (2e-3) and
# worst-element gates are unchanged: measured there 1.4-1.7e-3 / 3e-3.
FRAC_RELAX = {(48, 3): 1.0, (384, 12): 8.0}


@pytest.fixture()
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micformer_amd import ops as o
    o.set_compute_dtype("bf16")
    yield o
    o.set_compute_dtype("fp32")


def _cuda(g):
    return {k: ({n: t.cuda() for n, t in v.items()} if k == "P" else v.cuda() if torch.is_tensor(v) else v) for k, v in g.items()}


# the absolute gates (Report.add), by tensor.  Backward: the kernel ran on ITS OWN saved tensors, as in a step.  The oracle's adjoint
# follows the kernels' (oracle _AttnCoreBF16 / _GeluSavedBF16 / _rg): q, k, v and h are re-read as the forward STORED them (bf16), S and
# P rebuilt from those, dY operands rounded where they enter a product, the DropPath scale applied after the product.  Measured on
# MI355X: input gradients 2e-4 relative L2 with 1 % of the elements beyond 1e-4 of the scale (the oracle against itself in fp64:
# 0.9-1.2 %), 0.03-0.23 % of the stored bf16 gradients more than one bf16 step off (fp64 self-check: 0.03-0.16 %), LayerNorm sums 1-4e-4.
_S16 = dict(frac_gate=3e-3, bf16=True)
_G2 = dict(frac_gate=5e-2, l2=2e-3, worst=2e-2)
_G16 = dict(frac_gate=1e-2, worst=2e-2, bf16=True)
_GS = dict(frac_gate=None, l2=2e-3, worst=5e-3)
ABSOLUTE = {"y": dict(frac_gate=1e-2), "x1": dict(frac_gate=1e-2), "LN1 mean": dict(frac_gate=0.0, exact=True), "LN1 rstd": dict(frac_gate=0.0, exact=True),
            "LN2 mean": dict(frac_gate=1e-2), "LN2 rstd": dict(frac_gate=1e-2), "xn": dict(frac_gate=1e-4, bf16=True),
            "q": _S16, "kv": _S16, "o": _S16, "xn2": _S16, "h": _S16, "g": _S16,
            "dxn (q path)": _G2, "dxs": _G2, "dx1 copy": _G2, "dx": _G2, "d ln1 gain": _GS, "d ln1 bias": _GS, "d ln2 gain": _GS, "d ln2 bias": _GS,
            "dq": _G16, "dkv": _G16, "dh": _G16, "dx1": _G16}


def _launch_outputs(o, b, C, cross):
    """What one group of block_fwd / block_bwd wrote, by the names of block_oracle_gates.evaluate, in the order of the report."""
    got = {"y": o["y"], "x1": o["x1"], "LN1 mean": o["stats"][0], "LN1 rstd": o["stats"][1], "LN2 mean": o["stats"][2], "LN2 rstd": o["stats"][3]}
    if o.get("xn") is not None:
        got["xn"] = o["xn"]
    got.update({k: o[k] for k in ("q", "kv", "o", "xn2", "h", "g")})
    if cross:
        got.update({"dxn (q path)": b["dx"], "dxs": b["dxs"], "dx1 copy": b["dx1_copy"]})
    else:
        part = b["ln1_part"].double().sum(0)
        got.update({"dx": b["dx"], "d ln1 gain": part[:C], "d ln1 bias": part[C:]})
    part = b["ln2_part"].double().sum(0)
    got.update({"d ln2 gain": part[:C], "d ln2 bias": part[C:], "dq": b["dq"], "dkv": b["dkv"], "dh": b["dh"], "dx1": b["dx1"]})
    return got


def _launches_against_the_oracle(ops, hook, C, heads, dims, kind, wave, absolute):
    """Forward (y + every saved tensor + LayerNorm statistics) and backward (dx, the K/V-source gradient, the second dx1 copy, the
    five weight-gradient operands dq / dkv / dh / dx1 / dy16, LayerNorm gain / bias sums) of a self pair and of a cross pair with a
    given K/V source; two groups per launch.  absolute: the gates of Report.add against the oracle in fp32; otherwise the gates of
    Report.gate (4 x the oracle's own fp32-vs-fp64 spread, absolute caps on top) against the oracle in fp64."""
    if C == 48:
        hook("block_wave", 1 if wave else 0)
    B, D, H, W = dims
    scale = (C // heads) ** -0.5
    cross = kind == "cross"
    st16 = ops.block_saves_bf16(C, heads)
    assert (ops.block_tile_tokens(dims, C, heads, 4 * C), ops.block_tile_tokens(dims, C, heads, 4 * C, backward=True)) == TILE_TOKENS[(C, heads)]
    cpu = [G.make_group(C, dims, kind, i) for i in range(2)]
    gs = [_cuda(g) for g in cpu]
    fw = ops.block_fwd([dict(g) for g in gs], dims, C, heads, EPS, scale)
    bg = [{"dy": g["dy"], "x": None if cross else g["x"], "x1": o["x1"], "stats": o["stats"], "q": o["q"], "kv": o["kv"], "h": o["h"],
           "xn2": o["xn2"], "P": g["P"], "attn": g["attn"], "s1": g["s1"], "s2": g["s2"], "cross": cross, "want_copy": cross}
          for g, o in zip(gs, fw)]
    bw = ops.block_bwd([dict(g) for g in bg], dims, C, heads, scale)
    torch.cuda.synchronize()
    rep = Report(FRAC_RELAX.get((C, heads), 1.0))
    sp = None if absolute else G.spread(C, heads, kind, st16)
    for i, (g, o, b) in enumerate(zip(cpu, fw, bw)):
        if not cross and i == 0:
            from oracle import micformer_ref as R
            x = g["x"].reshape(B, D, H, W, C)
            with R.bf16_operands(), torch.no_grad():
                assert torch.equal(G.oracle_block(R, x, None, g["P"], g["attn"], heads, g["s1"], g["s2"]),
                                   R.self_block(x, g["P"], "", heads, (2, 2, 2), g["s1"], g["s2"], EPS)), "helper != oracle.self_block"
        got = _launch_outputs(o, b, C, cross)
        n = f"g{i}."
        for k in ("q", "kv", "o", "xn2", "g", "dq", "dkv", "dh", "dx1"):
            assert (got[k].dtype == torch.bfloat16) == st16, f"{k}: stored as {got[k].dtype}, block_saves_bf16 says {st16}"
        assert got["h"].dtype == torch.bfloat16
        if absolute:
            want = G.evaluate(g, dims, heads, torch.float32)
            for k, t in got.items():
                rep.add(n + k, t.float() if t.dtype == torch.bfloat16 else t, want[k], **ABSOLUTE[k])
        else:
            want = G.reference(C, heads, kind, dims, st16, 0, i)
            for k, t in got.items():
                rep.gate(n + k, k, t, want[k], sp, st16)
        # the bf16 copies of the launch's own inputs: exactly the rounded input
        if b["dy16"] is not None:
            rep.add(n + "dy16", b["dy16"].float(), g["dy"], 0.0, bf16=True, worst=4e-3)
        if cross and o["kvs16"] is not None:
            rep.add(n + "kvs16", o["kvs16"].float(), g["kvsrc"], 0.0, bf16=True, worst=4e-3)
    how = "the oracle (fp32)" if absolute else "the oracle in fp64; per statistic: oracle fp32-vs-fp64 spread / gate / measured"
    rep.done(f"C {C}, {heads} heads{', wave-private' if C == 48 and wave else ''}, {kind} pair, dims {dims}: distance to {how}")


def _launch_cases():
    # (the C = 48 cases keep the ids they had before the widths were parametrised)
    cases = [pytest.param(48, 3, dims, kind, wave, True, id=f"dims{di}-{kind}-{wave}")
             for di, dims in enumerate([(2, 32, 32, 32), (1, 2, 6, 2)]) for kind in ("self", "cross") for wave in (True, False)]
    cases += [pytest.param(C, heads, dims, kind, False, False, id=f"c{C}h{heads}-grid{di}-{kind}")
              for C, heads in NEW_WIDTHS for di, dims in enumerate(G.GRIDS) for kind in ("self", "cross")]
    return cases


@pytest.mark.parametrize("C,heads,dims,kind,wave,absolute", _launch_cases())
def test_block_launches_against_the_oracle(ops, hook, C, heads, dims, kind, wave, absolute):
    """Every instantiation, self and cross: C = 48 (wave-private and tile kernels, on a real 2 x 32^3-token launch and on an odd
    window count) by the absolute gates; every other width on the two grids of block_oracle_gates.GRIDS by the spread gates."""
    _launches_against_the_oracle(ops, hook, C, heads, dims, kind, wave, absolute)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_c384_head_dim_32_tile_kernels_against_the_oracle(ops, hook, kind):
    """The instantiation round 6 added for the large model's third stage (C = 384, head_dim 32: `block_fwd_kernel<384, 32, 1, 8>`,
    `block_bwd_kernel<384, 32, 1, 8>` -- hidden chunk 2C, K = 384 products in two k chunks, inputs requested in two waves): the same
    absolute forward and backward gates as the benched kernels (fractions x 8: FRAC_RELAX), on a grid with a half-empty last tile (3
    windows) and on 12 full tiles."""
    assert ops.block_fuses_sampler(384, 12) and ops.block_tile_tokens((1, 4, 6, 8), 384, 12, 1536) == 16
    for dims in ((1, 2, 6, 2), (1, 4, 6, 8)):
        _launches_against_the_oracle(ops, hook, 384, 12, dims, kind, False, True)


def _sampler_cases():
    cases = [pytest.param(48, 3, dims, wave, True, id=f"dims{di}-{wave}") for di, dims in enumerate([(2, 32, 32, 32), (1, 4, 6, 2)]) for wave in (True, False)]
    return cases + [pytest.param(C, heads, G.SAMPLER_GRID, False, False, id=f"c{C}h{heads}") for C, heads in NEW_WIDTHS if (C, heads) != (384, 24)]


@pytest.mark.parametrize("C,heads,dims,wave,absolute", _sampler_cases())
def test_cross_launch_with_fused_sampling_against_the_oracle(ops, hook, C, heads, dims, wave, absolute):
    """The cross pair as the step launches it: the conv_offset[0] output in, LayerNorm(16) -> GELU -> 1^3 conv -> reference points
    (permuted divisors) -> trilinear sampling of the raw other modality INSIDE the block launch, then the block.  oracle.cross_block
    (MS.py:339-426) end to end; the kernel is handed the oracle's own conv output (the 3^3 conv is a separate launch).  Every width
    whose launch samples (ops.block_fuses_sampler: all but the few-token decomposition); forward only."""
    if C == 48:
        hook("block_wave", 1 if wave else 0)
    assert ops.block_fuses_sampler(C, heads) and ops.block_saves_bf16(C, heads)
    scale = (C // heads) ** -0.5
    cpu = [G.make_sampler_group(C, dims, i) for i in range(2)]
    ref32 = [G.evaluate_sampler(g, dims, heads, torch.float32) for g in cpu]
    gs = []
    for g, r in zip(cpu, ref32):
        Pk = {k: v.cuda() for k, v in g["P"].items()}
        Pk["conv_offset.3.weight"] = Pk["conv_offset.3.weight"].reshape(3, 16).contiguous()
        gs.append({"x": g["x"].cuda(), "kvsrc": None, "P": Pk, "attn": "cross_attn", "s1": None, "s2": None, "want_xn": False,
                   "hid": r["hid"].contiguous().cuda(), "samp_src": g["xa"].cuda()})
    fw = ops.block_fwd([dict(g) for g in gs], dims, C, heads, EPS, scale)
    torch.cuda.synchronize()
    rep = Report()
    sp = None if absolute else G.spread_sampler(C, heads)
    for i, (o, g, r32) in enumerate(zip(fw, cpu, ref32)):
        n = f"g{i}."
        if absolute:
            rep.add(n + "flow", o["flow"], r32["flow"], 0.0, exact=True)
            rep.add(n + "kvs16", o["kvs16"].float(), r32["kvs16"], 1e-3, bf16=True)
            rep.add(n + "q", o["q"].float(), r32["q"], 3e-3, bf16=True)
            rep.add(n + "kv", o["kv"].float(), r32["kv"], 3e-3, bf16=True)
            rep.add(n + "o", o["o"].float(), r32["o"], 3e-3, bf16=True)
            rep.add(n + "x1", o["x1"], r32["x1"], 1e-2)
            rep.add(n + "h", o["h"].float(), r32["h"], 3e-3, bf16=True)
            rep.add(n + "y", o["y"], r32["y"], 3e-2)        # (measured 7e-3: the gathered rows carry fp32 interpolation noise into more ties)
        else:
            with G.pinned_threads():
                want = G.evaluate_sampler(g, dims, heads, torch.float64)
            for k in ("flow", "kvs16", "q", "kv", "o", "x1", "h", "y"):
                rep.gate(n + k, k, o[k], want[k], sp, True)
    rep.done(f"C {C}, {heads} heads{', wave-private' if C == 48 and wave else ''}, cross pair with the sampling fused in, dims {dims}")
