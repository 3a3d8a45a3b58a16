"""The spread-relative gates of tests/block_oracle_gates.py have teeth -- without a GPU.  The "kernel output" is a stand-in: the oracle
itself, evaluated in fp32 on inputs of a seed the spread has NOT seen (seed 8; the spread takes seeds 0 .. 7), held against the
fp64 referee of the same inputs exactly as tests/test_gpu_block_oracle.py holds a launch.

  - the unmodified oracle passes every gate: at every width, both kinds, both grids;
  - five defects of the kind a kernel change introduces are each REJECTED at every width, both kinds, on every grid they apply to:
    bf16 truncation instead of round-to-nearest-even, fc2's bias scaled by 0.98, s1 ignored on sample 0 (the grid with DropPath
    scales), two token rows of one window swapped in y, LN2's output entering fc1 unrounded.

The table printed per width lists, for every mutant, the tensor and statistic that stands furthest over its gate: spread, gate,
mutant distance.
"""
import pytest
import torch

import block_oracle_gates as G

WIDTHS = [(48, 3), (96, 6), (96, 3), (192, 12), (192, 6), (384, 24), (384, 12)]
HELD_OUT = G.SEEDS


def _st16(C, heads):
    """ops.block_saves_bf16 in bf16 mode: the library's own predicate (a host function: no GPU involved)."""
    from micformer_amd import _lib
    return bool(_lib.lib.micf_block_saves_bf16(C, heads, 1))


def test_only_the_few_token_path_stores_fp32():
    assert [w for w in WIDTHS if not _st16(*w)] == [(384, 24)]


def _verdict(C, heads, kind, dims, mutant):
    """(failed gates, row of the worst offender) of the stand-in against the fp64 referee."""
    st16 = _st16(C, heads)
    sp = G.spread(C, heads, kind, st16)
    g = G.make_group(C, dims, kind, 0, HELD_OUT)
    want = G.reference(C, heads, kind, dims, st16, HELD_OUT)
    with G.pinned_threads():
        got = G.evaluate(g, dims, heads, torch.float32, stored_fp32=not st16, mutant=mutant)
    rep = G.Report()
    for key in want:
        bf = G.stored_bf16(key, st16)
        rep.gate(key, key, got[key].float().bfloat16() if bf else got[key], want[key], sp, st16)
    return rep


def test_helper_is_the_oracles_self_block():
    from oracle import micformer_ref as R
    g = G.make_group(96, (2, 4, 4, 4), "self", 0)
    x = g["x"].reshape(2, 4, 4, 4, 96)
    with R.bf16_operands(), torch.no_grad():
        assert torch.equal(G.oracle_block(R, x, None, g["P"], g["attn"], 6, g["s1"], g["s2"]),
                           R.self_block(x, g["P"], "", 6, (2, 2, 2), g["s1"], g["s2"], G.EPS))


def test_stored_fp32_switch_moves_only_the_attention_adjoint():
    """bf16_operands(stored_fp32=True): the forward and everything downstream of dh are the default mode's bit for bit; with head_dim
    32 (scale not a power of two) the q / k gradients differ, with head_dim 16 (scale 2^-2) nothing does."""
    for heads, differs in ((12, True), (24, False)):
        g = G.make_group(384, (1, 2, 6, 2), "self", 0)
        a = G.evaluate(g, (1, 2, 6, 2), heads, stored_fp32=False)
        b = G.evaluate(g, (1, 2, 6, 2), heads, stored_fp32=True)
        for k in ("y", "x1", "q", "kv", "o", "h", "g", "dh", "dx1", "d ln2 gain"):
            assert torch.equal(a[k], b[k]), k
        assert (not torch.equal(a["dq"], b["dq"])) == differs
        assert float((a["dq"] - b["dq"]).norm() / a["dq"].norm()) < 2.0 ** -7      # (an operand one bf16 step off is 2^-8 of its size)


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("width", WIDTHS, ids=lambda w: f"c{w[0]}h{w[1]}")
def test_gates_pass_the_oracle_and_reject_the_mutants(width, kind):
    C, heads = width
    errs, table = [], []
    for dims in G.GRIDS:
        rep = _verdict(C, heads, kind, dims, None)
        # An absolute cap that the REFERENCE's own fp32-vs-fp64 spread reaches cannot be asked of this fp32 stand-in (C = 384 /
        # head_dim 16, cross, 24 tokens: the q-path gradient, spread 2.1e-3 against the 2e-3 cap).  It still binds a launch.
        bad = [b for b in rep.bad if b not in rep.cap_within_spread]
        table.append(f"  {str(dims):14s} {'unmodified oracle':26s} {'passes' if not bad else 'REJECTED'}   largest measured / spread: "
                     + "  ".join(f"{k} {v:.2f}" for k, v in rep.ratios.items()))
        table += [f"  {str(dims):14s}   (absolute cap within the reference's own spread) {b}" for b in rep.cap_within_spread]
        errs += [f"{dims} unmodified oracle: {b}" for b in bad]
        for mutant in G.MUTANTS:
            if mutant == "s1 ignored on sample 0" and dims[0] == 1:
                continue                                      # (no DropPath scales on this grid)
            rep = _verdict(C, heads, kind, dims, mutant)
            table.append(f"  {str(dims):14s} {mutant:26s} {'rejected' if rep.bad else 'NOT REJECTED'} ({len(rep.bad)} gates)   "
                         + (rep.bad[0] if rep.bad else ""))
            if not rep.bad:
                errs.append(f"{dims} mutant '{mutant}' passes every gate")
    print(f"\nC = {C}, heads = {heads}, {kind}: stand-ins (the oracle in fp32, seed {HELD_OUT}) against the fp64 referee\n" + "\n".join(table))
    assert not errs, "\n".join(errs)
