"""The bf16-operand referee of the patch-matrix-free head (micformer_amd/csrc/head_tail_fused.hip: micf_head_tail_pack, _fwd_fused
with its _loss_fused and _sw forms, _bwd_data_fused, _bwd_weight_fused), in plain torch on the CPU, with tests/bf16_ref.py's gates.

The composed map is a transposed convolution with kernel 6, stride 4, padding 1 on the coarse grid (u: fine voxel, q: coarse voxel):

  y[u, o] = sum_q Wb[(f, o), :] . x[q, :] + sum_{q in the volume} v[(f, o)]        f = u - 4 q + 1 in [0, 6)^3,
  row (f, o) = ((fd * 6 + fh) * 6 + fw) * 8 + o   (tail_pack_kernel),     v = bf + (b_out where f in [1, 5)^3: the centre slab).

Inputs are the kernels' own: x [B Dc Hc Wc, Ci], wb [1728, Ci], bf [1728], b_out [8], dy [B, 8, 4 Dc, 4 Hc, 4 Wc]; wb and bf are FREE
tensors here (the composition kernel has its own fp32 test).  Where the head rounds (read off head_tail_fused.hip):
  * x at the LDS write of the forward's halo and of the weight gradient's stretch (pack_bf16), dy at the LDS write of the data
    gradient's region and of the weight gradient's de-interleave, Wb in tail_pack_kernel -- all round-to-nearest-even;
  * the composite bias rides in the GEMM as a hi + lo bf16 pair of the fp32 value v against a 1.0 column that is 0 for out-of-volume
    halo rows: want carries rb(v) + rb(fp32(v - rb(v))) per in-volume neighbour, want32 the unsplit v;
  * dBf sums the fp32 values the weight-gradient kernel de-interleaves, BEFORE their conversion: want == want32, it matches "both".
Every function returns bf16_ref.Ref(want, want32, absdot, terms).  The overlap-add is a matmul + 216 strided slice adds (`fold`), its
adjoint 216 strided slices (`unfold`): test_head_ref_cpu.py holds both to torch's own convolutions and their autograd.
"""
import torch
import torch.nn.functional as F

from bf16_ref import Ref, rb, _exact, _mag, _ref

ROWS = 216 * 8
TAPS = [(fd, fh, fw) for fd in range(6) for fh in range(6) for fw in range(6)]


def fold(t, dims):
    """Patch matrix t [tokens, 1728] -> its overlap-add [B, 8, 4 Dc, 4 Hc, 4 Wc] (in t's dtype): fine voxel 4 q - 1 + f += t[q, (f, o)]."""
    B, Dc, Hc, Wc = dims
    t = t.reshape(B, Dc, Hc, Wc, 6, 6, 6, 8)
    out = t.new_zeros(B, 8, 4 * Dc + 2, 4 * Hc + 2, 4 * Wc + 2)                  # (index = fine voxel + 1)
    for fd, fh, fw in TAPS:
        out[:, :, fd:fd + 4 * Dc:4, fh:fh + 4 * Hc:4, fw:fw + 4 * Wc:4] += t[:, :, :, :, fd, fh, fw].permute(0, 4, 1, 2, 3)
    return out[:, :, 1:-1, 1:-1, 1:-1].contiguous()


def unfold(dy, dims):
    """The adjoint of `fold`: dy [B, 8, 4 Dc, 4 Hc, 4 Wc] -> u [tokens, 1728], u[q, (f, o)] = dy[o, 4 q - 1 + f] (0 outside the volume)."""
    B, Dc, Hc, Wc = dims
    p = F.pad(dy, (1, 1, 1, 1, 1, 1))
    u = dy.new_empty(B, Dc, Hc, Wc, 6, 6, 6, 8)
    for fd, fh, fw in TAPS:
        u[:, :, :, :, fd, fh, fw] = p[:, :, fd:fd + 4 * Dc:4, fh:fh + 4 * Hc:4, fw:fw + 4 * Wc:4].permute(0, 2, 3, 4, 1)
    return u.reshape(B * Dc * Hc * Wc, ROWS)


def centre_rows():
    """[1728] bool: the rows (f, o) with f in [1, 5)^3 -- the slab d = 0, the only one b_out is folded into."""
    m = torch.zeros(6, 6, 6, 8, dtype=torch.bool)
    m[1:5, 1:5, 1:5] = True
    return m.reshape(ROWS)


def bias_rows(bf, b_out):
    """-> (v, hi, lo), float64 [1728] each: v = bf + b_out on the centre rows (exact), and the bf16 pair the pack stores for fp32(v):
    hi = rb(fp32 v), lo = rb(fp32(fp32 v - hi)) -- the subtraction is exact in fp32 (the difference has at most 16 significant bits)."""
    add = torch.where(centre_rows(), b_out.detach().cpu().float().repeat(216), torch.zeros(ROWS))
    v32 = bf.detach().cpu().float() + add
    hi = v32.bfloat16().float()
    lo = (v32 - hi).bfloat16().float()
    v = bf.detach().cpu().double() + torch.where(centre_rows(), b_out.detach().cpu().double().repeat(216), torch.zeros(ROWS, dtype=torch.float64))
    return v, hi.double(), lo.double()


def _bias_volume(row, dims):
    B, Dc, Hc, Wc = dims
    return fold(row[None, :].expand(B * Dc * Hc * Wc, ROWS), dims)


def bias_term(bf, b_out, dims):
    """The composite bias as the kernel carries it (float64): per fine voxel the hi + lo pairs of its in-volume coarse neighbours."""
    _, hi, lo = bias_rows(bf, b_out)
    return _bias_volume(hi + lo, dims)


def head_fwd(x, wb, bf, b_out, dims):
    """Logits [B, 8, 4 Dc, 4 Hc, 4 Wc].  terms: a fine voxel has at most 8 coarse neighbours, each a (Ci + 2)-long product."""
    v, hi, lo = bias_rows(bf, b_out)
    want = fold(rb(x) @ rb(wb).t(), dims) + _bias_volume(hi + lo, dims)
    want32 = fold(_exact(x) @ _exact(wb).t(), dims) + _bias_volume(v, dims)
    absdot = fold(_mag(x) @ _mag(wb).t(), dims) + _bias_volume(hi.abs() + lo.abs(), dims)
    return Ref(want, want32, absdot, 8 * (x.shape[1] + 2))


def head_bwd_data(dy, wb, dims):
    """dx [tokens, Ci] = sum_{f, o} dy[o, 4 q - 1 + f] Wb[(f, o), :]."""
    return _ref(lambda r, u: unfold(r(dy), dims) @ r(wb), ROWS)


def head_bwd_weight(dy, x, dims):
    """-> (dWb [1728, Ci] on the rounded dy and x, dBf [1728] on the UNROUNDED dy).  terms: the tokens, the sum over the at most 42
    workgroup groups' partial slabs, the folds of the dBf lanes."""
    terms = x.shape[0] + 42 + 8
    return _ref(lambda r, u: unfold(r(dy), dims).t() @ r(x), terms), _ref(lambda r, u: unfold(u(dy), dims).sum(0), terms)
