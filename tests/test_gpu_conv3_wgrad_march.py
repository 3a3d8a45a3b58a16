"""The plane-marching weight gradient of the offset convolution (csrc/conv3_wgradx.hip: conv3_wgradx_b16_kernel + the streaming
reduce) through ops.conv3_bwd_weight / ops.conv3_bwd_weight_grouped in the benched bf16 mode, against the bf16-operand referee
(tests/bf16_ref.conv3) through the gates of test_gpu_bf16_referee.py: dw must match the bf16 referee, dbias (the unrounded dy)
both.  No tolerance of its own.  The shapes are the smallest at which the walk can go wrong: the ring's start and end with both
zero planes at once (D = 1, 2, 3), a sample boundary between two planes, a d range that starts inside a sample (two primed planes,
ranges of unequal length), the 16-wide ragged footprint over two channel slabs, and the masked W = 4."""
import math

import pytest
import torch

import bf16_ref as R
from test_gpu_bf16_referee import Report, bf16, dev, rnd  # noqa: F401  (bf16: the fixture that sets the compute mode)

pytestmark = pytest.mark.gpu

SLAB_FLOATS = 4 * 21 * 256          # csrc/conv3_wgrad_plan.h: kSlabFloats
_REF = {}


def layer(dims, C, seed=0, tie=False):
    """(dy, x1, x2) of one layer and its referee with a zero weight (only dw and db are read), computed once and shared."""
    key = (dims, C, seed, tie)
    if key not in _REF:
        B, D, H, W = dims
        T = B * D * H * W
        x1 = R.ties(T, C, seed=10 * seed + 1) if tie else rnd((T, C), 10 * seed + 1)
        x2 = rnd((T, C), 10 * seed + 2)
        dy = R.ties(T, 16, seed=10 * seed + 5) if tie else rnd((T, 16), 10 * seed + 5)
        ref = R.conv3(x1, x2, torch.zeros(16, 2 * C, 3, 3, 3), None, dy, dims)
        _REF[key] = ((dy, x1, x2), ref)
    return _REF[key]


def outputs(C, base=None):
    if base is None:
        return torch.zeros(16, 2 * C, 3, 3, 3, device="cuda"), torch.zeros(16, device="cuda")
    return dev(base[0]).clone(), dev(base[1]).clone()


def run_one(ops, dims, C, ins, base=None):
    dy, x1, x2 = ins
    dw, db = outputs(C, base)
    ops.conv3_bwd_weight(dev(dy), dev(x1), dw, db, dims, x2=dev(x2))
    return dw, db


def d_ranges(dims, C):
    """d ranges per (sample, footprint) of the plan, read off the workspace size: parts x (slabs x slab + 16 bias floats)."""
    from micformer_amd import _lib
    B, D, H, W = dims
    floats = _lib.lib.micf_conv3_bwd_weight_workspace(B, D, H, W, 16, C, C)
    slabs = -(-2 * C // 48)
    parts, rest = divmod(floats, slabs * SLAB_FLOATS + 16)
    assert floats > 0 and rest == 0
    tw = 16 if W >= 12 else 8
    nranges, rest = divmod(parts, B * -(-H // (64 // tw)) * -(-W // tw))
    assert rest == 0
    return nranges


# ring start and end at once (D = 1: both zero planes in the one step), C = 24: a 16-channel tile across the x1 | x2 seam;
# sample 1's first plane after sample 0's last;  TW = 16, ragged, two slabs;  the masked W = 4
@pytest.mark.parametrize("dims,C", [((1, 1, 5, 9), 24), ((1, 2, 5, 9), 24), ((1, 3, 5, 9), 24), ((2, 2, 4, 12), 48),
                                    ((1, 3, 6, 19), 96), ((1, 4, 4, 4), 24)], ids=str)
def test_march(bf16, dims, C):
    rep = Report(f"marching conv3 weight gradient {dims}, 2 x {C} -> 16")
    ins, ref = layer(dims, C)
    assert d_ranges(dims, C) == 1                 # D < 8: no split over d
    dw, db = run_one(bf16, dims, C, ins)
    rep.add("dw", dw, ref["dw"], "bf16")
    rep.add("dbias (unrounded dy)", db, ref["db"], "both")
    rep.done()


def test_march_splits_d_inside_a_sample(bf16):
    """(1, 9, 5, 9): two footprints cannot fill the chip, so D = 9 is split into the ranges [0, 4) and [4, 9) -- the second starts
    inside the sample and primes planes 3 and 4; 9 is no multiple of either length."""
    dims, C = (1, 9, 5, 9), 24
    assert d_ranges(dims, C) == 2 and dims[1] % 2 != 0
    rep = Report(f"marching conv3 weight gradient {dims}, 2 x {C} -> 16, two d ranges")
    ins, ref = layer(dims, C)
    dw, db = run_one(bf16, dims, C, ins)
    rep.add("dw", dw, ref["dw"], "bf16")
    rep.add("dbias (unrounded dy)", db, ref["db"], "both")
    rep.done()


def test_march_ties(bf16):
    """x1 and dy made of exact rounding ties: RNE at the LDS write, nothing else."""
    dims, C = (1, 3, 5, 9), 24
    rep = Report(f"marching conv3 weight gradient {dims}, 2 x {C} -> 16, ties")
    ins, ref = layer(dims, C, tie=True)
    dw, db = run_one(bf16, dims, C, ins)
    rep.add("dw", dw, ref["dw"], "bf16")
    rep.add("dbias (unrounded dy)", db, ref["db"], "both")
    rep.done()


def test_march_accumulates_onto_a_base(bf16):
    """dw and dbias start from random values: the reduce adds (+=), compared with referee + base."""
    dims, C = (1, 9, 5, 9), 24
    rep = Report(f"marching conv3 weight gradient {dims}, 2 x {C} -> 16, += onto a base")
    ins, ref = layer(dims, C)
    base = (rnd((16, 2 * C, 3, 3, 3), 71), rnd((16,), 72))
    dw, db = run_one(bf16, dims, C, ins, base)
    for name, got, r, b, expect in (("dw", dw, ref["dw"], base[0], "bf16"), ("dbias", db, ref["db"], base[1], "both")):
        rep.add(name + " + base", got, R.Ref(r.want + b.double(), r.want32 + b.double(), r.absdot + b.double().abs(), r.terms + 1), expect)
    rep.done()


def test_march_ignores_what_the_workspace_held(bf16):
    """The workspace filled with NaN before the call: every float the reduce reads was written by the call itself."""
    from micformer_amd import _lib
    ops = bf16
    dims, C = (1, 3, 6, 19), 96
    B, D, H, W = dims
    rep = Report(f"marching conv3 weight gradient {dims}, 2 x {C} -> 16, NaN workspace")
    ins, ref = layer(dims, C)
    need = _lib.lib.micf_conv3_bwd_weight_workspace(B, D, H, W, 16, C, C)
    ws = ops.scratch(torch.device("cuda", torch.cuda.current_device()), need)
    ws.fill_(math.nan)
    dw, db = run_one(ops, dims, C, ins)
    assert ops.scratch(ws.device, need) is ws     # the call used the poisoned buffer
    rep.add("dw", dw, ref["dw"], "bf16")
    rep.add("dbias", db, ref["db"], "both")
    rep.done()
    ws.zero_()


def test_march_twice_is_bit_identical(bf16):
    """No atomics and a fixed order of summation: the same call on fresh outputs gives the same bits (one and three layers)."""
    ops = bf16
    dims, C = (1, 9, 5, 9), 24
    ins, _ = layer(dims, C)
    a, b = run_one(ops, dims, C, ins), run_one(ops, dims, C, ins)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    runs = []
    for _ in range(2):
        items = [tuple(dev(t) for t in layer(dims, C, seed=k)[0]) + outputs(C) for k in range(3)]
        ops.conv3_bwd_weight_grouped(items, dims)
        runs.append(items)
    for x, y in zip(*runs):
        assert torch.equal(x[3], y[3]) and torch.equal(x[4], y[4])


# 13 layers: more than one launch takes (12), so a launch of 12 and one of 1
@pytest.mark.parametrize("n", [3, 12, 13])
def test_march_grouped(bf16, n):
    ops = bf16
    dims, C = (1, 3, 5, 9), 24
    rep = Report(f"grouped marching conv3 weight gradient {dims}, 2 x {C} -> 16, {n} layers")
    layers = [layer(dims, C, seed=k) for k in range(n)]
    items = [tuple(dev(t) for t in ins) + outputs(C) for ins, _ in layers]
    ops.conv3_bwd_weight_grouped(items, dims)
    for k, ((_, ref), it) in enumerate(zip(layers, items)):
        rep.add(f"layer {k}: dw", it[3], ref["dw"], "bf16")
        rep.add(f"layer {k}: dbias", it[4], ref["db"], "both")
    rep.done()
