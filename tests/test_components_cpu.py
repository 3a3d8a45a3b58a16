"""CPU checks of the connected components: the referee (tests/components_ref.py) against a flood fill, the ctypes struct and constants against
include/micformer_components.h (tests/test_abi.py has the entry points), argument errors caught before any launch, the workspace
query, and the Python front end's validation."""
import ctypes

import numpy as np
import pytest
import torch

import abi_header
import components_ref as C

HEADER = "micformer_components.h"
EINVAL, EUNSUP = -1, -2


# ---- the referee ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_referee_matches_a_flood_fill(connectivity, K):
    g = np.random.default_rng(100 * K + connectivity)
    for trial in range(12):
        shape = tuple(int(s) for s in g.integers(1, 7, size=3))
        vol = g.integers(0, K, size=shape).astype(np.uint8)
        labels, sizes = C.components(vol, K, None, connectivity)
        want_labels, want_sizes = C.brute_force_components(vol, K, None, connectivity)
        assert np.array_equal(labels, want_labels), (shape, trial)
        assert np.array_equal(sizes, want_sizes), (shape, trial)
    # label values instead of class indices, with a value that names no class: it belongs to no component
    vol = C.to_values(g.integers(0, 8, size=(6, 6, 6)).astype(np.uint8), C.MMWHS_LABEL_VALUES, np.int16)
    vol[2, 3, 4] = 77
    if K == 8:
        labels, sizes = C.components(vol, 8, C.MMWHS_LABEL_VALUES, connectivity)
        want_labels, want_sizes = C.brute_force_components(vol, 8, C.MMWHS_LABEL_VALUES, connectivity)
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
        assert labels[2, 3, 4] == 0 and sizes[2, 3, 4] == 0


def test_referee_filters_and_scenes():
    vol = np.zeros((4, 5, 9), np.uint8)
    vol[0, 0, 0:2] = 1                                    # two components of class 1, sizes 2 and 2: the first one stays
    vol[3, 4, 7:9] = 1
    vol[1, 1, 1:4] = 2                                    # class 2: sizes 3 and 1
    vol[3, 0, 0] = 2
    kept = C.keep_largest(vol, 3)
    assert kept[0, 0, 0] == 1 and kept[3, 4, 8] == 0 and kept[1, 1, 2] == 2 and kept[3, 0, 0] == 0
    assert np.array_equal(C.keep_largest(vol, 3, classes=[2])[3, 4, 7:9], [1, 1])
    assert np.array_equal(C.remove_small(vol, 1, 3), vol)
    assert int((C.remove_small(vol, 3, 3) > 0).sum()) == 3
    assert int((C.remove_small(vol, 4, 3) > 0).sum()) == 0
    for shape in [(17, 33, 130), (5, 4, 3), (6, 7, 1)]:
        for conn in (6, 26):
            s = C.snake(shape)
            labels, sizes = C.components(s, 2, None, conn)
            assert set(np.unique(labels)) == {0, 1} and int(sizes.max()) == int(s.sum())
    cb = C.checkerboard((4, 5, 6))
    assert len(np.unique(C.components(cb, 2, None, 6)[0])) == 1 + int(cb.sum())
    assert len(np.unique(C.components(cb, 2, None, 26)[0])) == 2


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_sample_struct_and_constants_match_the_header():
    from micformer_amd import postprocess as P
    assert abi_header.struct_decls(HEADER, "micf_component_sample") == ["const void* in", "void* out", "int32_t shape[3]"]
    assert [t for _, t in P.ComponentSample._fields_] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32 * 3]
    assert ctypes.sizeof(P.ComponentSample) == 32
    consts = abi_header.defines(HEADER, "MICF_COMPONENTS_")
    assert (consts["MICF_COMPONENTS_U8"], consts["MICF_COMPONENTS_I16"], consts["MICF_COMPONENTS_I32"]) == (P.IN_U8, P.IN_I16, P.IN_I32)
    assert (consts["MICF_COMPONENTS_KEEP_LARGEST"], consts["MICF_COMPONENTS_REMOVE_SMALL"]) == (P.KEEP_LARGEST, P.REMOVE_SMALL)
    assert consts["MICF_COMPONENTS_MAX_CLASSES"] == P.MAX_CLASSES == 32


def _samples(shapes, in_=1 << 20, out=1 << 21):
    from micformer_amd import postprocess as P
    items = (P.ComponentSample * len(shapes))()
    for it, s in zip(items, shapes):
        it.in_, it.out = in_, out
        it.shape[:] = s
    return items


def test_workspace_query_is_pure_additive_and_negative_for_bad_arguments():
    from micformer_amd import postprocess as P
    q = P.lib.micf_components_workspace

    def one(*shape):
        return q(ctypes.addressof(_samples([shape])), 1)

    def rounded(n):
        return (n + 255) // 256 * 256

    assert one(1, 1, 1) == 2 * 256 + 256 == one(1, 1, 1)                                    # pure
    assert one(3, 5, 7) == 2 * rounded(3 * 5 * 7 * 4) + 256
    assert one(363, 512, 512) == 2 * 363 * 512 * 512 * 4 + 256                              # 761 MB: 8 bytes per voxel
    shapes = [(3, 5, 7), (40, 70, 130), (1, 1, 70), (9, 17, 65)]
    assert q(ctypes.addressof(_samples(shapes)), 4) == sum(one(*s) for s in shapes)          # additive over the samples
    assert P.workspace_bytes(shapes) == sum(one(*s) for s in shapes)
    assert q(None, 1) == EINVAL and q(ctypes.addressof(_samples(shapes)), 0) == EINVAL and q(ctypes.addressof(_samples(shapes)), -3) == EINVAL
    assert one(0, 5, 7) == EINVAL and one(3, -1, 7) == EINVAL
    assert one(2049, 5, 7) == EUNSUP and one(3, 5, 2049) == EUNSUP
    assert one(2048, 1024, 1024) == EUNSUP                                                   # 2^31 voxels
    assert one(2047, 1024, 1024) > 0 and one(2048, 2048, 511) > 0
    assert q(ctypes.addressof(_samples([(3, 5, 7), (2049, 1, 1)])), 2) == EUNSUP
    assert q(ctypes.addressof(_samples([(2049, 1, 1), (3, 0, 7)])), 2) == EINVAL


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd import postprocess as P
    lib = P.lib
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    vals7 = (ctypes.c_int32 * 7)(*P.MMWHS_LABEL_VALUES)
    BIG = 1 << 40

    def call(fn="filter", B=1, K=8, in_=fake, out=fake, shape=(20, 24, 28), dtype=P.IN_I16, values=vals7, nvals=7, conn=26,
             mask=0xFE, mode=P.KEEP_LARGEST, min_size=1, ws=fake, ws_bytes=BIG, samples_ptr=True, sizes=None):
        s = _samples([shape], in_, out)
        sp = ctypes.addressof(s) if samples_ptr else None
        vp = None if values is None else ctypes.addressof(values)
        if fn == "filter":
            return lib.micf_filter_components(sp, B, dtype, K, vp, nvals, conn, mask, mode, min_size, ws, ws_bytes, None)
        return lib.micf_connected_components(sp, B, dtype, K, vp, nvals, conn, sizes, ws, ws_bytes, None)

    for fn in ("filter", "labels"):
        assert call(fn, samples_ptr=False) == EINVAL
        assert call(fn, B=0) == EINVAL and call(fn, B=-1) == EINVAL
        assert call(fn, conn=7) == EINVAL and call(fn, conn=0) == EINVAL
        assert call(fn, dtype=3) == EINVAL
        assert call(fn, K=1, values=None, nvals=0, dtype=P.IN_U8, mask=2) == EUNSUP
        assert call(fn, K=33, values=(ctypes.c_int32 * 32)(*range(1, 33)), nvals=32) == EUNSUP
        assert call(fn, shape=(20, 0, 28)) == EINVAL                   # an extent of 0
        assert call(fn, shape=(20, 2049, 28)) == EUNSUP                # an extent of 2049
        assert call(fn, shape=(2048, 1024, 1024)) == EUNSUP            # 2^31 voxels
        assert call(fn, shape=(2048, 2048, 512)) == EUNSUP             # 2^31 voxels: one more than the limit allows
        assert call(fn, nvals=6) == EINVAL                             # num_label_values != K - 1
        assert call(fn, K=7, mask=0x7E) == EINVAL
        assert call(fn, values=None) == EINVAL                         # an int16 volume needs the table ...
        assert call(fn, dtype=P.IN_U8) == EINVAL                       # ... and a uint8 class map takes none
        assert call(fn, values=(ctypes.c_int32 * 7)(1, 2, 3, 4, 5, 6, 40000)) == EINVAL        # does not fit int16
        assert call(fn, values=(ctypes.c_int32 * 7)(1, 2, 3, 4, 5, 6, 0)) == EINVAL            # zero is the background
        assert call(fn, values=(ctypes.c_int32 * 7)(1, 2, 3, 4, 5, 6, 3)) == EINVAL            # twice the same value
        assert call(fn, in_=None) == EINVAL and call(fn, out=None) == EINVAL
        assert call(fn, in_=fake + 1) == EINVAL                        # int16 needs 2-byte alignment
        assert call(fn, ws=None) == EINVAL
        assert call(fn, ws=fake + 4) == EINVAL                         # the workspace needs 256-byte alignment
        need = P.workspace_bytes([(20, 24, 28)])
        assert call(fn, ws_bytes=need - 1) == EINVAL                   # a short workspace
    assert call("labels", out=fake + 2) == EINVAL                      # int32 labels need 4-byte alignment
    assert call("filter", out=fake + 1) == EINVAL
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL          # an unknown mode
    assert call(mode=P.REMOVE_SMALL, min_size=0) == EINVAL and call(mode=P.REMOVE_SMALL, min_size=-5) == EINVAL
    assert call(min_size=0) == EINVAL
    assert call(mask=0) == EINVAL and call(mask=1) == EINVAL and call(mask=0x1FE) == EINVAL      # no class, class 0, class 8 of 8


# ---- the Python front end ---------------------------------------------------------------------------------------------------

def test_python_front_end_rejects_before_the_device():
    from micformer_amd import postprocess as P
    cpu16 = torch.zeros(4, 5, 6, dtype=torch.int16)
    cpu8 = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for fn in (P.connected_components, P.keep_largest_components, lambda v, **kw: P.remove_small_components(v, 3, **kw)):
        with pytest.raises(ValueError, match="CUDA"):
            fn(cpu16)                                                  # a CPU tensor
        with pytest.raises(ValueError, match="CUDA"):
            fn([cpu8, cpu8], label_values=None, num_classes=4)
        with pytest.raises(ValueError, match="CUDA"):
            fn(cpu16.unsqueeze(0))
        for bad in (cpu16.float(), cpu16.long(), cpu16.bool()):
            with pytest.raises(TypeError):
                fn(bad)                                                # wrong dtype: TypeError before the device ValueError
        with pytest.raises(TypeError):
            fn(cpu16.numpy())
        with pytest.raises(TypeError):
            fn([cpu16, cpu8])                                          # mixed dtypes
        with pytest.raises(TypeError):
            fn([])
        with pytest.raises(ValueError, match="shape"):
            fn(torch.zeros(5, 6, dtype=torch.int16))
        with pytest.raises(ValueError, match="shape"):
            fn(torch.zeros(4, 0, 6, dtype=torch.int16))
        with pytest.raises(ValueError, match="shape"):
            fn(torch.zeros(1, 1, 2049, dtype=torch.uint8), label_values=None, num_classes=2)
        for values in [(1, 2, 2), (1, 0, 3), (1, 2, 40000), "abc", (1.5, "x")]:   # duplicate, zero, beyond int16, no integers
            with pytest.raises(ValueError, match="label"):
                fn(cpu16, label_values=values)
        with pytest.raises(ValueError, match="label"):
            fn(cpu16, label_values=None)
        with pytest.raises(ValueError, match="label"):
            fn(cpu16, label_values=(1, 2, 3), num_classes=8)
        with pytest.raises(ValueError, match="CUDA"):
            fn(cpu16.int(), label_values=(1, 2, 40000))                # fits int32: the next complaint is the device
        for K in (1, 33, 0, 2.0, True):
            with pytest.raises(ValueError, match="num_classes"):
                fn(cpu8, label_values=None, num_classes=K)
        with pytest.raises(ValueError, match="num_classes"):
            fn(cpu8, label_values=None)
        for conn in (7, 0, 4, 8, "26", None):
            with pytest.raises(ValueError, match="connectivity"):
                fn(cpu16, connectivity=conn)
    for fn in (P.keep_largest_components, lambda v, **kw: P.remove_small_components(v, 3, **kw)):
        for classes in [(0,), (8,), (1, 9), (), (1.0,), 3, (True,)]:
            with pytest.raises(ValueError, match="classes"):
                fn(cpu16, classes=classes)
        with pytest.raises(ValueError, match="CUDA"):
            fn(cpu16, classes=(1, 7))
    for m in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="min_size"):
            P.remove_small_components(cpu16, m)
    with pytest.raises(ValueError, match="CUDA"):
        P.KeepLargestConnectedComponent(applied_labels=[1, 2])(cpu16)
    with pytest.raises(ValueError, match="CUDA"):
        P.RemoveSmallObjects(min_size=8)(cpu16)
    with pytest.raises(ValueError, match="connectivity"):
        P.RemoveSmallObjects(min_size=8, connectivity=5)(cpu16)


def test_non_contiguous_is_rejected_before_the_device():
    """Contiguity needs no device: a transposed, a strided and a sliced volume are refused as such by every public entry point,
    alone, in a list and as a [B, d, h, w] batch, before the complaint about the device that a contiguous CPU tensor gets."""
    from micformer_amd import postprocess as P
    base = torch.zeros(6, 6, 12, dtype=torch.int16)
    bad = [base.transpose(1, 2), base.transpose(0, 1), base[:, :, ::2], base[:, 1:5, :], base.unsqueeze(0).expand(3, 6, 6, 12)[:, :, :, 1:]]
    assert not any(t.is_contiguous() for t in bad)
    fns = (P.connected_components, P.keep_largest_components, lambda v, **kw: P.remove_small_components(v, 3, **kw),
           P.KeepLargestConnectedComponent(), P.RemoveSmallObjects(min_size=4))
    for fn in fns:
        for t in bad:
            with pytest.raises(ValueError, match="contiguous"):
                fn(t)
        with pytest.raises(ValueError, match=r"volume\[1\] must be contiguous"):
            fn([base, bad[0]])
        with pytest.raises(ValueError, match="CUDA"):
            fn(base)
        with pytest.raises(ValueError, match="CUDA"):
            fn(base[1:4])                                  # a slice along z alone is contiguous: the next complaint is the device


def test_segment_pair_has_the_keyword_and_defaults_to_off():
    import inspect
    from micformer_amd import restore
    p = inspect.signature(restore.segment_pair).parameters["keep_largest"]
    assert p.default is False
