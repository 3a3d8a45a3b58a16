"""micf_block_fwd / micf_block_bwd with q == NULL (the backward rebuilds q, k | v and the fc1 pre-activation: wave-private kernels
only): what the library refuses, before any launch -- so this runs without a GPU: every pointer below is a made-up, 16-byte aligned
address that a refused call never reads -- and that ops.block_rebuilds says the same about shape, mode and hook."""
import ctypes as C

import pytest

from micformer_amd import _lib, ops

EINVAL = -1
DIMS, HEADS48 = (2, 4, 4, 4), 3
F32, BF16 = 0, 1


def _fake(struct, null=()):
    """Every field a distinct aligned non-NULL address, except the ones named in `null`."""
    g = (struct * 2)()
    for i in range(2):
        for k, name in enumerate(struct.FIELDS):
            setattr(g[i], name, None if name in null else 0x100000 * (i + 1) + 0x1000 * (k + 1))
    return g


def _fwd(null, c=48, heads=HEADS48, dtype=BF16, ngroups=2):
    # (a self block without the fused sampler, the next-LayerNorm epilogue or the fp32-only xs32: valid but for what is under test)
    off = ("kvsrc", "kvs16", "hid", "samp_src", "ln16_g", "ln16_b", "w1c", "flow", "xs32", "nln_g", "nln_b", "nln_y", "nln_mean",
           "nln_rstd", "zero16")
    g = _fake(_lib.BlockFwdGroup, null=off + tuple(null))
    return _lib.lib.micf_block_fwd(C.cast(g, C.c_void_p), ngroups, *DIMS, c, heads, 4 * c, C.c_float(1e-5), C.c_float(0.25), dtype, None)


def _bwd(null, c=48, heads=HEADS48, dtype=BF16, ngroups=2):
    off = ("dxs", "kvs16", "pre_d", "pre_x", "pre_mean", "pre_rstd", "pre_g", "pre_part")       # a self block without the prologue
    g = _fake(_lib.BlockBwdGroup, null=off + tuple(null))
    return _lib.lib.micf_block_bwd(C.cast(g, C.c_void_p), ngroups, *DIMS, c, heads, 4 * c, C.c_float(0.25), dtype, None)


@pytest.fixture()
def bf16():
    ops.set_compute_dtype("bf16")
    yield
    ops.set_compute_dtype("fp32")


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_q_null_needs_kv_and_h_null(call, bf16):
    assert ops.block_rebuilds(DIMS, 48, HEADS48, 192)          # the shape and mode are the wave-private ones: the mix is what is refused
    assert call(("q",)) == EINVAL                              # kv given
    assert call(("q", "h")) == EINVAL
    assert call(("kv", "h")) == EINVAL                         # ... and q given without kv
    assert call(("q", "kv")) == EINVAL                         # h given


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_q_null_is_refused_off_the_wave_private_kernels(call, bf16, hook):
    null = ("q", "kv", "h")
    assert call(null, c=96, heads=6) == EINVAL                 # tile-per-workgroup kernel
    assert not ops.block_rebuilds(DIMS, 96, 6, 384)
    assert call(null, dtype=F32) == EINVAL                     # fp32 parity mode
    ops.set_compute_dtype("fp32")
    assert not ops.block_rebuilds(DIMS, 48, HEADS48, 192)
    ops.set_compute_dtype("bf16")
    hook("block_wave", 0)
    assert call(null) == EINVAL                                # the tile kernel at C = 48
    assert not ops.block_rebuilds(DIMS, 48, HEADS48, 192)


def test_backward_refuses_q_null_without_its_sources_or_with_unlike_groups(bf16):
    for miss in ("xn", "wq", "wkv", "bq", "bkv", "xn2", "w1", "b1"):
        assert _bwd(("q", "kv", "h", miss)) == EINVAL, miss
    g = _fake(_lib.BlockBwdGroup, null=("dxs", "kvs16", "pre_d", "pre_x", "pre_mean", "pre_rstd", "pre_g", "pre_part"))
    g[1].q = g[1].kv = g[1].h = None                           # group 0 reads its saved tensors, group 1 would rebuild
    assert _lib.lib.micf_block_bwd(C.cast(g, C.c_void_p), 2, *DIMS, 48, HEADS48, 192, C.c_float(0.25), BF16, None) == EINVAL
