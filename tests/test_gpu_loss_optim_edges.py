"""GPU parity tests, op level, second generation: every launch edge of csrc/loss_optim.hip (MDiceLoss forward / backward, argmax +
meandice, the thresholded Dice metric, the fused Adam + cosine-LR step with its bf16 mirror) against the float64 referee
tests/loss_optim_ref.py.  test_gpu_ops.py holds each kernel at one or two training shapes against the fp32 oracle; this file holds
the host-side arms those shapes never take.  Every bound is derived in loss_optim_ref.py's docstring (none is tuned), and
tests/test_loss_optim_ref_cpu.py shows on the CPU that the fp32 oracle passes each of them on the inputs used here and that the listed
wrong kernels fail them.  Every case prints (-s) the kernel's worst error / bound and the fp32 CPU oracle's on the same input.

Inputs: z = 3 randn clipped to |z| <= 9, plus (`saturate`) the exact saturation points +-20, +-40, +-80, +-110, +-inf with both target
values, where p is exactly 0 or 1 or safely normal and the BCE term is 0, |z| or the clamp 100.  No input enters (13, 17.5), where
q = 1 - p is quantised in steps of 2^-24 and then jumps to 0, or (-104, -87), where sigmoid(z) is an fp32 denormal on the CPU and
the hardware exp overflows: there two honest fp32 evaluations of the reference's own formula (BCELoss on the sigmoid's output)
disagree by up to 84 per element, which is a property of that formula and not an error of the kernel.  test_loss_cliff_report
prints what the kernel gives at z = 16.0, 16.7 and -95 and asserts only that it is finite.  NaN logits are outside every contract.

Which arm lives where (chunks = ceil(V / 32768), per = ceil(V / chunks); grid caps 4096 / 8192 / 256):

dice_bce_partial_kernel (test_loss_forward, one-hot and uint8 targets, B = 2, K = 3; sums I, P2, S within the bound, T2 exact)
  one chunk, scalar loads, partly filled wave      V = 1, 3, 255
  one chunk, 16-byte loads                         V = 4, 1024, 1028 (one 1024-stride tail trip), 32768 (16 double-load trips)
  two chunks, per = 16386: scalar although V % 4 == 0                    V = 32772
  three chunks, per = 21848: ten double-load trips, tail of 1024 + 344   V = 65544
  three chunks, scalar                             V = 65541; V = 65542 (3 per > V: the last chunk is cut at V)
  a pointer off 16 bytes with V % 4 == 0           test_loss_forward_pointer_off_16_bytes (logits, then target)
  K = 1; K = 255 with labels; label 255            test_loss_forward_class_counts
  K = 256 with labels                              test_loss_label_k256_rejected (MICF_EUNSUPPORTED before any launch)
  dice_bce_final_kernel, MDiceLoss_Val             every forward case: the scalar from the kernel's own sums, and from the referee's
dice_bce_bwd_kernel (test_loss_backward: the REFEREE's float64 sums go in, so the forward kernel is not part of the test)
  one trip                                         the forward's V list, grad_out 1 and 0.37, both target kinds
  saturated p                                      the `saturate` cases: exactly 0
  the 4096-block cap, a ragged second trip         test_loss_backward_past_block_cap (V = 8 388 608 + 2048 + 5)
argmax_count_kernel (test_argmax_*)
  K = 1 (mask only), 2, 8, 32; K = 33              test_argmax_meandice_classes, test_argmax_k33_rejected
  ties, -inf, all-equal voxels, labels >= K, want_mask=False, label=None, V % 256 != 0     test_argmax_meandice_classes
  the 8192-block cap: several trips per block, one flush of the 32-bit LDS counters into the 64-bit totals
                                                   test_argmax_past_block_cap (B V = 8192 * 2048 + 2048 + 7, K = 2)
dice_metric_partial_kernel (test_dice_metric_*)
  one chunk / two chunks                           V = 1, 255, 65536 / 65537; empty target planes; z = +-0, +-2^-22, +-1e-30
  the 256-chunk cap                                test_dice_metric_past_chunk_cap (V = 256 * 65536 + 65536 + 3)
adam_tick_kernel                                   test_adam_tick: step - 1 in {0, t_max / 2, t_max, t_max + 1}, eta_min 0 and 1e-6
adam_step_kernel (p, m, v one step from the device's own state, against float64)
  first float4 / scalar tail, one block            n = 1, 3, 4, 5, 1023, 1024
  several blocks, tail in the last                 n = 1025, 1027, 2049, 8 * 1024 + 6
  the 4096-block cap: second float4 (i1), second grid-stride trip, tail in the first half      test_adam_past_block_cap
  steps 1, 2, 100 001; betas; grad_scale           test_adam_step
  bf16 mirror, float4 store and scalar tail        test_adam_mirror (n % 4 = 0, 1, 3; exact rounding ties), test_adam_past_block_cap
  sliced views (what the engine passes)            test_adam_sliced_views (offsets 4, 1028), test_adam_slice_off_16_bytes_rejected,
                                                   test_adam_empty_range, test_adam_split_ranges_bit_equal
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import loss_optim_ref as L
from oracle import micformer_ref as R

pytestmark = pytest.mark.gpu

B, K = 2, 3
FWD_V = (1, 3, 4, 255, 1024, 1028, 32768, 32772, 65544, 65541, 65542)
SATURATE_V = (255, 1028, 65544)
BWD_BIG_V = 8388608 + 2048 + 5
ARGMAX_BIG = 8192 * 2048 + 2048 + 7
METRIC_V = (1, 255, 65536, 65537)
METRIC_BIG_V = 256 * 65536 + 65536 + 3
ADAM_N = (1, 3, 4, 5, 1023, 1024, 1025, 1027, 2049, 8 * 1024 + 6)
ADAM_BIG_N = 2 * 4096 * 1024 + 1024 + 3
ADAM_CONFIGS = ((0.9, 0.999, 1.0), (0.5, 0.9, 0.125))         # beta1, beta2, grad_scale
EPS = L.f32(1e-8)
BASE_LR, T_MAX = 1e-3, 10                                     # a short schedule: the lr of neighbouring steps differs by percents


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from micformer_amd import ops as o
    return o


def off16(t):
    """Contiguous CUDA copy of t at storage offset 1 element of float32: its base pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ----------------------------------------------------------------------------- loss: inputs and references, computed once
@functools.lru_cache(maxsize=None)
def loss_case(V, b=B, k=K):
    """-> z, label, one-hot planes, the referee's Sums, the fp32 oracle's sums on the same input."""
    z, lab = L.loss_inputs(b, k, V, seed=V, saturate=V in SATURATE_V and k >= 2)
    hot = L.one_hot(lab, k)
    return z, lab, hot, L.dice_sums(z, lab), oracle_sums(z, hot)


def oracle_sums(z, hot):
    """The four sums as the fp32 CPU oracle forms them (R.mdice_loss's expressions, before the final scalar)."""
    p = torch.sigmoid(z)
    d = (0, 2)
    return torch.stack([(p * hot).sum(d), (p * p).sum(d), (hot * hot).sum(d),
                        F.binary_cross_entropy(p, hot, reduction="none").sum(d)], 1)


def oracle_grad(z, hot, sums, g):
    """An honest fp32 evaluation of the backward from given sums: ATen's sigmoid and the kernel's documented formula in fp32."""
    k = z.shape[1]
    s = sums.reshape(k, 4)
    I2 = (2.0 * s[:, 0] + 1.0).float().reshape(1, k, 1)
    den = (s[:, 1] + s[:, 2] + 1.0).float().reshape(1, k, 1)
    cd = torch.tensor(g).float() * 0.7 / k
    cb = torch.tensor(g).float() * 0.3 / k / float(z.shape[0] * z.shape[2])
    p = torch.sigmoid(z)
    pq = (1.0 - p) * p
    ddice = -(2.0 * hot * den - I2 * 2.0 * p) / (den * den)
    return (cd * ddice + cb * (p - hot) / pq.clamp_min(1e-12)) * pq


def check_forward(ops, z, target, ref, V, what, oracle=None):
    """sums, the loss scalar and MDiceLoss_Val of one forward call against the referee."""
    from micformer_amd.loss.dice import MDiceLoss_Val
    b, k = z.shape[:2]
    loss, sums = ops.dice_bce_fwd(z, target)
    val = MDiceLoss_Val()(z, target)
    terms = L.fwd_terms(V)
    sums, loss, val = sums.cpu().reshape(k, 4), float(loss.cpu()), float(val.cpu())
    r = L.sums_ratio(sums, ref, terms)
    ro = L.sums_ratio(oracle, ref, terms) if oracle is not None else float("nan")
    print(f"\n{what}: sums error / bound {r:.3g} (fp32 CPU oracle {ro:.3g}); T2 {sums[:, 2].tolist()}")
    assert torch.equal(sums[:, 2], ref.sums[:, 2]), f"{what}: T2 {sums[:, 2].tolist()} is not the count {ref.sums[:, 2].tolist()}"
    assert r <= 1.0, f"{what}: I / P2 / S error is {r:.3g} of the bound: {sums.tolist()} vs {ref.sums.tolist()}"
    # the scalars: from the kernel's own sums (one fp32 rounding of a float64 expression), and against the referee's
    own, ref_loss = float(L.dice_loss(sums, b * V)), float(L.dice_loss(ref.sums, b * V))
    assert abs(loss - own) <= 2 * L.U * abs(own), f"{what}: loss {loss!r} vs {own!r} from its own sums"
    lb = L.dice_loss_bound(ref.sums, ref.bound(terms), b * V)
    assert abs(loss - ref_loss) <= lb, f"{what}: loss {loss!r} vs {ref_loss!r} (bound {lb:.3g})"
    own_val = float(L.dice_val_loss(sums))
    assert abs(val - own_val) <= 2 * L.U * abs(own_val), f"{what}: val loss {val!r} vs {own_val!r} from its own sums"
    vb = L.dice_loss_bound(ref.sums, ref.bound(terms), math.inf) / 0.7
    assert abs(val - float(L.dice_val_loss(ref.sums))) <= vb + 2 * L.U, f"{what}: val loss {val!r} vs the referee (bound {vb:.3g})"


@pytest.mark.parametrize("kind", ["onehot", "label"])
@pytest.mark.parametrize("V", FWD_V)
def test_loss_forward(ops, V, kind):
    z, lab, hot, ref, oracle = loss_case(V)
    check_forward(ops, z.cuda(), (hot if kind == "onehot" else lab).cuda(), ref, V, f"fwd V={V} {kind}", oracle)


@pytest.mark.parametrize("which", ["logits", "target"])
def test_loss_forward_pointer_off_16_bytes(ops, which):
    V = 1028
    z, lab, hot, ref, oracle = loss_case(V)
    zz, tt = (off16(z), hot.cuda()) if which == "logits" else (z.cuda(), off16(hot))
    check_forward(ops, zz, tt, ref, V, f"fwd V={V} {which} off 16 bytes", oracle)
    for g in (1.0, L.f32(0.37)):
        check_backward(ops, z, hot, zz, tt, ref, g, f"bwd V={V} {which} off 16 bytes g={g:.2f}")


def class_count_cases():
    """(what, z, target, one-hot planes, V): K = 1 with one-hot planes of both target values and with a class map whose label 1
    belongs to no plane; K = 255 with labels 0..255, where 255 is no class."""
    z, _ = L.loss_inputs(2, 1, 1028, seed=5)
    t = (L.rnd(2, 1, 1028, seed=6) > 0).float()
    lab = (L.rnd(2, 1028, seed=7) > 0).to(torch.uint8)
    z255, _ = L.loss_inputs(1, 255, 70, seed=8)
    lab255 = torch.randint(0, 256, (1, 70), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    lab255[0, :3] = torch.tensor([255, 254, 0], dtype=torch.uint8)
    return [("K=1 one-hot", z, t, t, 1028), ("K=1 label", z, lab, L.one_hot(lab, 1), 1028),
            ("K=255 label", z255, lab255, L.one_hot(lab255, 255), 70)]


def test_loss_forward_class_counts(ops):
    for what, z, target, hot, V in class_count_cases():
        ref = L.dice_sums(z, target)
        check_forward(ops, z.cuda(), target.cuda(), ref, V, "fwd " + what, oracle_sums(z, hot))
        check_backward(ops, z, hot, z.cuda(), target.cuda(), ref, 1.0, "bwd " + what)


def test_loss_label_k256_rejected(ops):
    """A uint8 class map cannot name 256 classes and a 256th plane: MICF_EUNSUPPORTED on the host, nothing launched or written."""
    from micformer_amd import _lib
    z = torch.zeros(1, 256, 8, device="cuda")
    lab = torch.zeros(1, 8, dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    sums = torch.full((4 * 256,), 5.0, dtype=torch.float64, device="cuda")
    dz = torch.full((1, 256, 8), 3.0, device="cuda")
    with pytest.raises(_lib.MicfError, match=r"code -2"):
        _lib.call("micf_dice_bce_label_fwd", _lib.f32(z), _lib.ptr(lab), _lib.ptr(sums), _lib.f32(loss), 1, 256, 8)
    with pytest.raises(_lib.MicfError, match=r"code -2"):
        _lib.call("micf_dice_bce_label_bwd", _lib.f32(z), _lib.ptr(lab), _lib.ptr(sums), None, _lib.f32(dz), 1, 256, 8)
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((sums == 5.0).all()) and bool((dz == 3.0).all())
    with pytest.raises(_lib.MicfError, match=r"code -2"):
        ops.dice_bce_fwd(z, lab)
    with pytest.raises(_lib.MicfError, match=r"code -2"):
        ops.dice_bce_bwd(z, lab, sums, loss)


def test_loss_cliff_report(ops):
    """Report only: the kernel inside the two bands the reference's formula leaves open (module docstring)."""
    z = torch.tensor([16.0, 16.7, -95.0]).reshape(3, 1, 1)
    t = torch.tensor([0.0, 0.0, 1.0]).reshape(3, 1, 1)
    cpu = F.binary_cross_entropy(torch.sigmoid(z), t, reduction="none").reshape(-1).tolist()
    ref = [float(L.dice_sums(z[i:i + 1], t[i:i + 1]).sums[0, 3]) for i in range(3)]
    got = []
    for i in range(3):
        loss, sums = ops.dice_bce_fwd(z[i:i + 1].cuda(), t[i:i + 1].cuda())
        got.append(float(sums.cpu()[3]))
        assert math.isfinite(got[-1]) and math.isfinite(float(loss.cpu()))
    print(f"\ncliff report: BCE term at z = 16.0 (t=0), 16.7 (t=0), -95 (t=1): kernel {got}, fp32 CPU {cpu}, referee {ref}")


# ----------------------------------------------------------------------------- loss backward
def check_backward(ops, z, hot, z_dev, target_dev, ref, g, what):
    """dz from the REFEREE's sums, element-wise within the derived bound (exactly 0 where p saturates)."""
    want, bound = L.dice_bce_grad(z, hot, ref.sums, g)
    sums = ref.sums.reshape(-1).contiguous().cuda()
    dz = ops.dice_bce_bwd(z_dev, target_dev, sums, torch.full((1,), g, device="cuda")).cpu().reshape(want.shape)
    r, ro = L.ratio(dz, want, bound), L.ratio(oracle_grad(z, hot, ref.sums, g), want, bound)
    print(f"\n{what}: dz error / bound {r:.3g} (fp32 CPU {ro:.3g}); {int((bound == 0).sum())} saturated elements")
    assert r <= 1.0, f"{what}: dz error is {r:.3g} of the bound"


@pytest.mark.parametrize("kind", ["onehot", "label"])
@pytest.mark.parametrize("V", FWD_V)
def test_loss_backward(ops, V, kind):
    z, lab, hot, ref, _ = loss_case(V)
    for g in (1.0, L.f32(0.37)):
        check_backward(ops, z, hot, z.cuda(), (hot if kind == "onehot" else lab).cuda(), ref, g, f"bwd V={V} {kind} g={g:.2f}")


def test_loss_backward_past_block_cap(ops):
    """ceil(V / 2048) = 4098 > 4096 blocks: every block makes 8 grid-stride trips, blocks 0..8 a ninth, block 8's over 5 elements."""
    V = BWD_BIG_V
    z, _ = L.loss_inputs(1, 1, V, seed=11)
    hot = (L.rnd(1, 1, V, seed=12) > 0).float()
    ref = L.dice_sums(z, hot)
    check_backward(ops, z, hot, z.cuda(), hot.cuda(), ref, L.f32(0.37), f"bwd V={V}")


# ----------------------------------------------------------------------------- argmax + meandice
def argmax_raw(z, label, want_mask=True):
    """micf_argmax_meandice with the counts kept: -> mask, counts [3, K] int64, meandice."""
    from micformer_amd import _lib
    b, k = z.shape[:2]
    V = z[0, 0].numel()
    mask = torch.full((b, V), 77, dtype=torch.uint8, device="cuda") if want_mask else None
    counts = torch.full((3 * k,), -1, dtype=torch.int64, device="cuda") if label is not None else None
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda") if label is not None else None
    _lib.call("micf_argmax_meandice", _lib.f32(z), _lib.ptr(label), _lib.ptr(mask), _lib.ptr(counts), _lib.ptr(out), b, k, V)
    return (mask.cpu() if want_mask else None, counts.cpu().reshape(3, k) if label is not None else None,
            float(out.cpu()) if label is not None else None)


def argmax_inputs(b, k, V, seed):
    """Logits on a grid of 0.25 (ties are common), with ties of the maximum at the first, last and middle voxels between every pair
    of neighbouring channels, a -inf channel, a voxel of all -inf and a voxel of all-equal logits; labels 0..K+1 and 255."""
    z = (L.rnd(b, k, V, seed=seed) * 4).round() / 4
    for j, vx in enumerate((0, V - 1, V // 2, V // 3)):
        c = j % k
        z[:, c, vx] = z[:, (c + 1) % k, vx] = 9.0
        if k > 2:
            z[:, k - 1, vx] = 9.0
    z[:, k - 1, 1 % V] = -math.inf
    z[:, :, 2 % V] = -math.inf
    z[:, :, 5 % V] = 0.5
    lab = torch.randint(0, k + 2, (b, V), generator=torch.Generator().manual_seed(seed + 1)).to(torch.uint8)
    lab[:, 3 % V] = 255
    return z, lab


@pytest.mark.parametrize("k,V", [(1, 300), (2, 777), (8, 1001), (32, 515)])
def test_argmax_meandice_classes(ops, k, V):
    z, lab = argmax_inputs(2, k, V, seed=k)
    want_mask, want_counts, want_md = L.argmax_counts(z, lab if k > 1 else None, k)
    assert torch.equal(want_mask, torch.argmax(z, 1))
    zd, ld = z.cuda(), lab.cuda()
    mask, md = ops.argmax_meandice(zd, None)                         # label=None: the mask alone
    assert md is None and torch.equal(mask.cpu().long(), want_mask)
    if k == 1:
        return
    mask, counts, md = argmax_raw(zd, ld)
    assert torch.equal(mask.long(), want_mask), "mask differs from torch.argmax (the first maximum wins)"
    assert torch.equal(counts, want_counts), f"counts {counts.tolist()} vs {want_counts.tolist()}"
    assert abs(md - want_md) <= 1e-12
    assert abs(md - float(R.meandice(want_mask, lab.long(), k))) <= 1e-12
    mask, counts, md2 = argmax_raw(zd, ld, want_mask=False)          # want_mask=False: the same counts, no mask store
    assert mask is None and torch.equal(counts, want_counts) and md2 == md
    mask, md3 = ops.argmax_meandice(zd, ld, want_mask=False)
    assert mask is None and float(md3.cpu()) == md
    mask, md4 = ops.argmax_meandice(zd, ld)
    assert torch.equal(mask.cpu().long(), want_mask) and float(md4.cpu()) == md


def test_argmax_k33_rejected(ops):
    from micformer_amd import _lib
    z = torch.zeros(1, 33, 8, device="cuda")
    with pytest.raises(_lib.MicfError, match=r"code -1"):
        ops.argmax_meandice(z, torch.zeros(1, 8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.MicfError, match=r"code -1"):
        ops.argmax_meandice(z, None)


def test_argmax_past_block_cap(ops):
    """ceil(B V / 2048) = 8194 > 8192 blocks: every block makes 8 trips, blocks 0..8 a ninth (block 8's over 7 voxels); the LDS
    counters of a block hold ~2048 voxels and are flushed once into the 64-bit totals (16.8 M voxels in all)."""
    V = ARGMAX_BIG
    g = torch.Generator().manual_seed(21)
    z = torch.randint(-8, 9, (1, 2, V), generator=g).float() / 4            # a coarse grid: one voxel in 17 is a tie
    z[0, :, V - 1] = 1.0
    lab = torch.randint(0, 4, (1, V), generator=g).to(torch.uint8)          # labels 2, 3 >= K: counted nowhere
    want_mask, want_counts, want_md = L.argmax_counts(z, lab, 2)
    mask, counts, md = argmax_raw(z.cuda(), lab.cuda())
    assert torch.equal(mask.long(), want_mask)
    assert torch.equal(counts, want_counts), f"counts {counts.tolist()} vs {want_counts.tolist()}"
    assert int(counts[0].sum()) == V and abs(md - want_md) <= 1e-12


# ----------------------------------------------------------------------------- Dice metric
def metric_inputs(b, k, V, seed):
    """randn logits whose first voxels hold the threshold's neighbours (the kernel's rule is z > 0: +0, -0 and every negative are
    background, 2^-22 and 1e-30 are foreground); sample 0 has no voxel of class k-1 and predicts none there (metric 1), sample 1 has
    none of class 1 but predicts some (metric 0)."""
    z = L.rnd(b, k, V, seed=seed)
    edge = torch.tensor([0.0, -0.0, 2.0 ** -22, -2.0 ** -22, 1e-30, -1e-30])[:V]
    z[:, :, :edge.numel()] = edge
    lab = torch.randint(0, k, (b, V), generator=torch.Generator().manual_seed(seed + 1)).to(torch.uint8)
    if k >= 3 and b >= 2:
        lab[0][lab[0] == k - 1] = 0
        z[0, k - 1] = -z[0, k - 1].abs()
        lab[1][lab[1] == 1] = 0
        z[1, 1, V - 1] = 1.0
    return z, lab


@pytest.mark.parametrize("V", METRIC_V)
def test_dice_metric_edges(ops, V):
    z, lab = metric_inputs(2, 3, V, seed=V)
    want = L.dice_metric(z, lab)
    assert float(want[0, 2]) == 1.0 and float(want[1, 1]) == 0.0
    for target in (lab, L.one_hot(lab, 3)):
        got = ops.dice_metric(z.cuda(), target.cuda()).cpu()
        assert torch.equal(got, want), f"V={V} {target.dtype}: {got.tolist()} vs {want.tolist()}"


def test_dice_metric_past_chunk_cap(ops):
    """ceil(V / 65536) = 258 > 256 chunks: per = 65793, 257 or 258 voxels per thread."""
    V = METRIC_BIG_V
    z, lab = metric_inputs(1, 1, V, seed=31)
    lab = (L.rnd(1, V, seed=32) > 0.5).to(torch.uint8)                      # label 1 >= K: no plane; label 0: the target
    want = L.dice_metric(z, lab)
    got = ops.dice_metric(z.cuda(), lab.cuda()).cpu()
    assert torch.equal(got, want), f"{got.tolist()} vs {want.tolist()}"


# ----------------------------------------------------------------------------- Adam
def state_of(st):
    """(step, lr) read back from the device state {int64 step; double lr}."""
    c = st.cpu()
    return int(c[0]), float(c.view(torch.float64)[1])


def oracle_adam(p, g, m, v, step, lr, b1, b2, gscale):
    """The fp32 CPU oracle's step on the same inputs (the gradient scaled first)."""
    return R.adam_update(p, g * gscale, m, v, step, lr, b1, b2, EPS)


def adam_one_step(ops, dev, g, st, b1, b2, gscale, what, mirror=None):
    """One tick + one step on the device buffers dev = [P, M, V]; the referee starts from the device's own state before the step.
    -> the device's updated p on the host."""
    p0, m0, v0 = (t.cpu() for t in dev)
    g, g_dev = g.cpu(), (g if g.is_cuda else g.cuda())
    ops.adam_tick(st, BASE_LR, 0.0, T_MAX)
    step, lr_dev = state_of(st)
    lr = L.cosine_lr(BASE_LR, step - 1, T_MAX)
    assert abs(lr_dev - lr) <= 8 * 2.0 ** -53 * BASE_LR
    ops.adam_step(dev[0], g_dev, dev[1], dev[2], st, b1, b2, EPS, grad_scale=gscale, mirror=mirror)
    want, bounds = L.adam(p0, g, m0, v0, step, lr, b1, b2, EPS, gscale, bounds=True)
    orc = oracle_adam(p0, g, m0, v0, step, lr, b1, b2, gscale)
    got = [t.cpu() for t in dev]
    for name, a, w, bd, o in zip("pmv", got, want, bounds, orc):
        r, ro = L.ratio(a, w, bd), L.ratio(o, w, bd)
        print(f"\n{what} step {step}: {name} error / bound {r:.3g} (fp32 CPU oracle {ro:.3g})")
        assert r <= 1.0, f"{what} step {step}: {name} error is {r:.3g} of the bound"
    still = (g == 0) & (m0 == 0) & (v0 == 0)
    assert torch.equal(got[0][still], p0[still]), f"{what}: a parameter with g = m = v = 0 moved"
    return got[0]


@pytest.mark.parametrize("b1,b2,gscale", ADAM_CONFIGS)
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step(ops, n, b1, b2, gscale):
    """Steps 1 and 2 from a zero state, then step 100 001 from a warm one (the counter preset by writing the int64)."""
    b1, b2 = L.f32(b1), L.f32(b2)                  # the ABI takes float betas: the referee gets the numbers the kernel gets
    p, g, m, v = L.adam_inputs(n, seed=n)
    dev = [p.cuda(), m.cuda(), v.cuda()]
    st = ops.adam_state("cuda")
    what = f"adam n={n} betas=({b1:.3f},{b2:.3f}) gscale={gscale}"
    adam_one_step(ops, dev, g, st, b1, b2, gscale, what)
    adam_one_step(ops, dev, L.rnd(n, seed=n + 9) * 1e-3, st, b1, b2, gscale, what)
    assert state_of(st)[0] == 2
    p, g, m, v = L.adam_inputs(n, seed=n + 20, warm=True)
    dev = [p.cuda(), m.cuda(), v.cuda()]
    st[0] = 100000
    adam_one_step(ops, dev, g, st, b1, b2, gscale, what)
    assert state_of(st)[0] == 100001


def test_adam_past_block_cap(ops):
    """ceil(n / 1024) = 8194 > 4096 blocks: every thread's second float4 (i1 = i0 + 4096 * 1024) runs, blocks 0..1 take a second
    grid-stride trip whose first half ends in a 3-element scalar tail and whose second half is past n.  With the bf16 mirror."""
    n = ADAM_BIG_N
    b1, b2 = L.f32(0.9), L.f32(0.999)
    p, g, m, v = L.adam_inputs(n, seed=41, warm=True)
    dev = [p.cuda(), m.cuda(), v.cuda()]
    mirror = torch.ones(n, dtype=torch.bfloat16, device="cuda")
    st = ops.adam_state("cuda")
    st[0] = 6
    got_p = adam_one_step(ops, dev, g, st, b1, b2, 0.125, f"adam n={n}", mirror=mirror)
    assert torch.equal(L.bf16_bits(mirror), L.bf16_rne(got_p)), "the mirror is not the RNE bf16 of the updated parameters"


@pytest.mark.parametrize("s", [0, T_MAX // 2, T_MAX, T_MAX + 1])
@pytest.mark.parametrize("eta_min", [0.0, 1e-6])
def test_adam_tick(ops, s, eta_min):
    """The tick takes the counter from s to s + 1 and leaves the lr of scheduler epoch s, as a double.  Tolerance: 1 + cos carries a
    few roundings of 2^-53 relative to 1 and is scaled by (base - eta_min) / 2: 8 * 2^-53 * base_lr absolute."""
    st = ops.adam_state("cuda")
    st[0] = s
    ops.adam_tick(st, BASE_LR, eta_min, T_MAX)
    step, lr = state_of(st)
    want = L.cosine_lr(BASE_LR, s, T_MAX, eta_min)
    print(f"\nadam_tick s={s} eta_min={eta_min}: lr {lr!r} vs {want!r}")
    assert step == s + 1
    assert abs(lr - want) <= 8 * 2.0 ** -53 * BASE_LR


@pytest.mark.parametrize("n", [2052, 1029, 1031])
def test_adam_mirror(ops, n):
    """The bf16 mirror is bit-equal to the round-to-nearest-even bf16 of the DEVICE's updated p, through the float4 store and the
    scalar tail (n % 4 = 0, 1, 3).  The first 64 and the last 3 parameters are exact rounding ties with g = m = v = 0, which the
    update leaves as they are."""
    b1, b2 = L.f32(0.9), L.f32(0.999)
    p, g, m, v = L.adam_inputs(n, seed=n, warm=True)
    ties = L.bf16_ties(67, seed=n)
    where = torch.cat([torch.arange(64), torch.arange(n - 3, n)])
    p[where] = ties
    g[where], m[where], v[where] = 0.0, 0.0, 0.0
    dev = [p.cuda(), m.cuda(), v.cuda()]
    mirror = torch.ones(n, dtype=torch.bfloat16, device="cuda")
    st = ops.adam_state("cuda")
    st[0] = 3
    got_p = adam_one_step(ops, dev, g, st, b1, b2, 1.0, f"adam mirror n={n}", mirror=mirror)
    assert torch.equal(got_p[where].view(torch.int32), ties.view(torch.int32)), "the tie-valued parameters moved"
    assert torch.equal(L.bf16_bits(mirror), L.bf16_rne(got_p)), "the mirror is not the RNE bf16 of the updated parameters"
    from micformer_amd import _lib
    before = [t.clone() for t in dev]
    with pytest.raises(_lib.MicfError):
        ops.adam_step(dev[0], g.cuda(), dev[1], dev[2], st, mirror=torch.ones(n, dtype=torch.float16, device="cuda"))
    with pytest.raises(_lib.MicfError):
        ops.adam_step(dev[0], g.cuda(), dev[1], dev[2], st, mirror=torch.ones(n + 1, dtype=torch.bfloat16, device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


def sliced(n_total, lo, hi, seed):
    """Full device buffers [P, G, M, V, mirror] and their [lo:hi] views, as the engine slices its flat buffers."""
    p, g, m, v = L.adam_inputs(n_total, seed=seed, warm=True)
    full = [p.cuda(), g.cuda(), m.cuda(), v.cuda(), torch.ones(n_total, dtype=torch.bfloat16, device="cuda")]
    return full, [t[lo:hi] for t in full]


@pytest.mark.parametrize("lo", [4, 1028])
def test_adam_sliced_views(ops, lo):
    n_total, hi = 4000, lo + 1501
    b1, b2 = L.f32(0.9), L.f32(0.999)
    full, (p, g, m, v, mir) = sliced(n_total, lo, hi, seed=lo)
    before = [t.clone() for t in full]
    st = ops.adam_state("cuda")
    got_p = adam_one_step(ops, [p, m, v], g, st, b1, b2, 1.0, f"adam slice [{lo}:{hi}]", mirror=mir)
    assert torch.equal(L.bf16_bits(mir), L.bf16_rne(got_p))
    outside = torch.ones(n_total, dtype=torch.bool)
    outside[lo:hi] = False
    for a, b0 in zip(full, before):
        assert torch.equal(a.cpu()[outside].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                           b0.cpu()[outside].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32))


def test_adam_slice_off_16_bytes_rejected(ops):
    from micformer_amd import _lib
    full, (p, g, m, v, mir) = sliced(2000, 1, 1001, seed=3)
    before = [t.clone() for t in full]
    st = ops.adam_state("cuda")
    ops.adam_tick(st, BASE_LR, 0.0, T_MAX)
    with pytest.raises(_lib.MicfError, match=r"code -1"):
        ops.adam_step(p, g, m, v, st)
    with pytest.raises(_lib.MicfError, match=r"code -1"):
        ops.adam_step(full[0][4:1004], full[1][4:1004], full[2][4:1004], full[3][4:1004], st, mirror=full[4][1:1001])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b0) for a, b0 in zip(full, before))


def test_adam_empty_range(ops):
    """n = 0 (an empty slice of the flat buffers, whose pointer torch reports as NULL) is a no-op, not an error."""
    full, (p, g, m, v, mir) = sliced(64, 32, 32, seed=4)
    before = [t.clone() for t in full]
    st = ops.adam_state("cuda")
    ops.adam_tick(st, BASE_LR, 0.0, T_MAX)
    ops.adam_step(p, g, m, v, st)
    ops.adam_step(p, g, m, v, st, mirror=mir)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b0) for a, b0 in zip(full, before)) and state_of(st)[0] == 1


def test_adam_split_ranges_bit_equal(ops):
    """[cut, n) then [0, cut) on one tick (the engine's early tail update) = one call over [0, n), bit for bit."""
    n, cut = 3003, 1028
    one, _ = sliced(n, 0, n, seed=5)
    two, _ = sliced(n, 0, n, seed=5)
    st = ops.adam_state("cuda")
    ops.adam_tick(st, BASE_LR, 0.0, T_MAX)
    ops.adam_step(one[0], one[1], one[2], one[3], st, grad_scale=0.125, mirror=one[4])
    for lo, hi in ((cut, n), (0, cut)):
        ops.adam_step(two[0][lo:hi], two[1][lo:hi], two[2][lo:hi], two[3][lo:hi], st, grad_scale=0.125, mirror=two[4][lo:hi])
    assert state_of(st)[0] == 1
    for a, b0 in zip(one, two):
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), b0.view(bits))
