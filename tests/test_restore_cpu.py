"""CPU checks of the volume restore: the referee (tests/restore_ref.py) against a float64 brute force of the coordinate rule, the
ctypes struct and constants against include/micformer_restore.h (tests/test_abi.py has the entry points), argument errors caught before any launch, the
workspace query, and the compiled device code's scratch use."""
import ctypes
import numpy as np
import pytest
import torch

import abi_header
import restore_ref as R

HEADER = "micformer_restore.h"


# ---- the referee ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("probabilities", [False, True])
@pytest.mark.parametrize("src,shape", [((9, 14, 11), (20, 33, 27)), ((1, 20, 7), (5, 31, 13)), ((23, 17, 31), (8, 12, 10))])
def test_referee_matches_float64_brute_force(src, shape, probabilities):
    """Three small shapes, one with an extent of 1, one that downsamples: torch's fp32 operator against the rule in float64."""
    logits = R.make_logits(src, K=8, seed=sum(src))[0]
    labels, margin, up = R.restore(logits, shape, R.MMWHS_LABEL_VALUES, probabilities)
    x = torch.softmax(logits.double(), 0) if probabilities else logits.double()
    want = R.brute_force_upsample(x.numpy(), shape)
    err = float(np.abs(up.numpy().astype(np.float64) - want).max())
    tau = R.TAU[probabilities]
    print(f"{src} -> {shape} probabilities={probabilities}: max |torch fp32 - float64| = {err:.2e} (tau {tau:g})")
    assert err <= tau / 5
    table = R.label_table(R.MMWHS_LABEL_VALUES, 8).numpy()
    clear = margin.numpy() >= tau
    assert clear.mean() > 0.99
    assert np.array_equal(labels.numpy()[clear], table[want.argmax(0)][clear])


def test_referee_rule_details():
    # output shape = source shape: every tap weight is 0 or 1
    logits = R.make_logits((7, 6, 5), K=4)[0]
    labels, margin, up = R.restore(logits, (7, 6, 5), (11, 22, 33))
    assert torch.equal(up, logits)
    assert torch.equal(labels, torch.tensor([0, 11, 22, 33])[logits.argmax(0)])
    assert torch.equal(R.restore(logits, (7, 6, 5), None)[0], logits.argmax(0))
    # an exact tie: the lowest class index wins; one class: the margin is infinite
    tie = torch.zeros(3, 2, 2, 2)
    assert int(R.restore(tie, (3, 3, 3), (5, 6))[0].abs().sum()) == 0
    assert torch.isinf(R.restore(tie[:1], (3, 3, 3), ())[1]).all()
    # the judge accepts any class within tau at a near tie and nothing else
    up = torch.tensor([0.0, 5e-5, -1.0]).reshape(3, 1, 1, 1)
    for lab, ok in ((0, True), (7, True), (9, False), (8, False)):
        assert R.judge(torch.full((1, 1, 1), lab), up, (7, 9), False)["ok"] is ok, lab
    up = torch.tensor([0.0, 5e-4, -1.0]).reshape(3, 1, 1, 1)
    for lab, ok in ((0, False), (7, True), (9, False)):
        assert R.judge(torch.full((1, 1, 1), lab), up, (7, 9), False)["ok"] is ok, lab


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------

def test_sample_struct_and_constants_match_the_header():
    from micformer_amd import restore
    assert abi_header.struct_decls(HEADER, "micf_restore_sample") == ["void* out", "int32_t out_shape[3]"]
    assert [(n, t) for n, t in restore.RestoreSample._fields_] == [("out", ctypes.c_void_p), ("out_shape", ctypes.c_int32 * 3)]
    assert ctypes.sizeof(restore.RestoreSample) == 24
    consts = abi_header.defines(HEADER, "MICF_RESTORE_")
    assert (consts["MICF_RESTORE_U8"], consts["MICF_RESTORE_I16"], consts["MICF_RESTORE_I32"]) == (
        restore.OUT_U8, restore.OUT_I16, restore.OUT_I32)
    assert (consts["MICF_RESTORE_LOGITS"], consts["MICF_RESTORE_PROBS"]) == (restore.LOGITS, restore.PROBS)
    assert consts["MICF_RESTORE_MAX_CLASSES"] == restore.MAX_CLASSES == 32


def test_workspace_query_is_pure_and_sized_as_documented():
    from micformer_amd.restore import LOGITS, PROBS, lib
    q = lib.micf_volume_restore_workspace
    assert q(1, 8, 128, 128, 128, LOGITS) == 0 and q(5, 32, 16, 16, 16, LOGITS) == 0
    assert q(1, 8, 128, 128, 128, PROBS) == 8 * 128 ** 3 * 4 == q(1, 8, 128, 128, 128, PROBS)        # 64 MB, and pure
    assert q(3, 5, 7, 9, 11, PROBS) == 3 * 5 * 7 * 9 * 11 * 4
    assert q(1, 1, 512, 512, 512, PROBS) == 512 ** 3 * 4
    EINVAL, EUNSUP = -1, -2
    assert q(0, 8, 8, 8, 8, PROBS) == EINVAL and q(1, 8, 8, 0, 8, LOGITS) == EINVAL and q(1, 8, 8, 8, -2, LOGITS) == EINVAL
    assert q(1, 8, 8, 8, 8, 2) == EINVAL and q(1, 8, 8, 8, 8, -1) == EINVAL
    assert q(1, 0, 8, 8, 8, LOGITS) == EUNSUP and q(1, 33, 8, 8, 8, PROBS) == EUNSUP
    assert q(1, 8, 512, 512, 513, LOGITS) == EUNSUP


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd import restore
    lib = restore.lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    vals7 = (ctypes.c_int32 * 7)(*restore.MMWHS_LABEL_VALUES)

    def call(logits=fake, B=1, K=8, src=(16, 16, 16), out=fake, shape=(20, 24, 28), out_dtype=restore.OUT_I16,
             interpoland=restore.LOGITS, values=vals7, nvals=7, workspace=None, ws_bytes=0, samples_ptr=True):
        s = restore.RestoreSample()
        s.out = out
        s.out_shape[:] = shape
        return lib.micf_volume_restore(logits, B, K, *src, ctypes.addressof(s) if samples_ptr else None, out_dtype, interpoland,
                                       None if values is None else ctypes.addressof(values), nvals, workspace, ws_bytes, None)

    assert call(logits=None) == EINVAL
    assert call(logits=fake + 2) == EINVAL                            # float32 needs 4-byte alignment
    assert call(samples_ptr=False) == EINVAL
    assert call(B=0) == EINVAL
    assert call(src=(16, 0, 16)) == EINVAL
    assert call(out=None) == EINVAL
    assert call(out=fake + 1) == EINVAL                               # int16 needs 2-byte alignment
    assert call(out_dtype=3) == EINVAL
    assert call(interpoland=2) == EINVAL
    assert call(shape=(20, 0, 28)) == EINVAL                          # an extent of 0
    assert call(shape=(20, 2049, 28)) == EUNSUP                       # an extent of 2049
    assert call(shape=(2048, 1024, 1024)) == EUNSUP                   # 2^31 output voxels
    assert call(K=0, values=None, nvals=0, out_dtype=restore.OUT_U8) == EUNSUP
    assert call(K=33, values=(ctypes.c_int32 * 32)(*range(1, 33)), nvals=32) == EUNSUP
    assert call(src=(512, 512, 513)) == EUNSUP
    assert call(nvals=6) == EINVAL                                    # num_label_values != K - 1
    assert call(K=7) == EINVAL
    assert call(values=None) == EINVAL                                # an int16 volume needs the table ...
    assert call(out_dtype=restore.OUT_U8) == EINVAL                   # ... and a uint8 class map takes none
    assert call(values=(ctypes.c_int32 * 7)(1, 2, 3, 4, 5, 6, 40000)) == EINVAL          # does not fit int16
    need = lib.micf_volume_restore_workspace(1, 8, 16, 16, 16, restore.PROBS)
    assert call(interpoland=restore.PROBS) == EINVAL                  # no workspace
    assert call(interpoland=restore.PROBS, workspace=fake, ws_bytes=need - 1) == EINVAL  # a short workspace
    assert call(interpoland=restore.PROBS, workspace=fake + 2, ws_bytes=need) == EINVAL


def test_python_front_end_rejects_before_the_device():
    from micformer_amd import restore
    cpu = torch.zeros(1, 8, 4, 5, 6)
    with pytest.raises(ValueError, match="CUDA"):
        restore.restore_batch(cpu, [(8, 8, 8)])                        # a CPU tensor
    with pytest.raises(ValueError, match="CUDA"):
        restore.restore_labels(cpu[0], (8, 8, 8))
    with pytest.raises(TypeError):
        restore.restore_batch(cpu.double(), [(8, 8, 8)])               # wrong dtype: TypeError before the device ValueError
    with pytest.raises(TypeError):
        restore.restore_batch(cpu.half(), [(8, 8, 8)])
    with pytest.raises(TypeError):
        restore.restore_batch(cpu.numpy(), [(8, 8, 8)])
    with pytest.raises(TypeError):
        restore.restore_batch(cpu, [(8, 8, 8)], dtype=torch.int64)
    with pytest.raises(TypeError):
        restore.restore_batch(cpu, [(8, 8, 8)], out=torch.zeros(8, 8, 8, dtype=torch.int16))       # not a list
    # shape, class count, output shapes and label values are checked before the device: a CPU tensor reaches every one of them
    for bad in [torch.zeros(1, 0, 4, 5, 6), torch.zeros(1, 33, 4, 5, 6), torch.zeros(8, 4, 5, 6), torch.zeros(1, 8, 0, 5, 6)]:
        with pytest.raises(ValueError, match="classes|non-empty"):
            restore.restore_batch(bad, [(8, 8, 8)], label_values=None)
    with pytest.raises(ValueError, match="one sample"):
        restore.restore_labels(torch.zeros(2, 8, 4, 5, 6), (8, 8, 8))
    for shapes in [[(8, 0, 8)], [(8, 2049, 8)], [(2048, 1024, 1024)], [(8, 8)], [], [(8, 8, 8), (8, 8, 8)], None, [None]]:
        with pytest.raises(ValueError, match="shape"):
            restore.restore_batch(cpu, shapes)
    for values in [(1, 2, 3), range(1, 9), (), (1, 2, 3, 4, 5, 6, 40000), "abcdefg"]:      # len != K - 1, beyond int16, no integers
        with pytest.raises(ValueError, match="label"):
            restore.restore_batch(cpu, [(8, 8, 8)], label_values=values)
    restore_int32 = dict(label_values=(1, 2, 3, 4, 5, 6, 40000), dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        restore.restore_batch(cpu, [(8, 8, 8)], **restore_int32)       # fits int32: the next complaint is the device
    with pytest.raises(ValueError, match="CUDA"):
        restore.restore_batch(cpu.transpose(3, 4), [(8, 8, 6)])        # (contiguity is a matter of the device tensor: after it)


# ---- the device code ----------------------------------------------------------------------------------------------------------

def test_volume_restore_device_code_uses_no_scratch():
    kernels, asm, flags = abi_header.device_asm("volume_restore.hip")
    assert not any("fast-math" in f or "-Ofast" in f for f in flags)     # the softmax pre-pass needs the IEEE divide
    fused = [k for k in kernels if "restore_fused_kernel" in k]
    assert len(kernels) == 4 and len(fused) == 3, sorted(kernels)          # softmax + the fused kernel for uint8 / int16 / int32
    assert all(v == 0 for v in kernels.values()), kernels
    assert "scratch_" not in asm and "flat_load" not in asm                # the taps are global loads, nothing spills
    assert "atomic" not in asm                                             # bit-identical from run to run
