"""Float64 referee of csrc/loss_optim.hip (MDiceLoss forward / backward, argmax + meandice, the thresholded Dice metric, the fused
Adam + cosine-LR step and its bf16 mirror): plain torch on the CPU, no kernel, no oracle import.  tests/test_loss_optim_ref_cpu.py
holds this file to the fp32 oracle, float64 autograd and torch.optim; tests/test_gpu_loss_optim_edges.py holds the kernels to it.

The one rounding the loss reference models
------------------------------------------
The operation is nn.BCELoss on the fp32 OUTPUT of a sigmoid (dice.py:158-166), so p is an fp32 number before any log is taken:
p = float32(sigmoid(z)), q = 1 - p, logs clamped at -100.  That map is discontinuous in z: 1 + exp(-z) rounds to 1 for z > 16.64,
q becomes exactly 0 and -log(q) jumps from about 16 to the clamp 100.  A reference that keeps p in float64 never saturates and is
a reference for another operation.  Here p32 = float32(sigmoid(float64 z)) -- the correctly rounded sigmoid -- and everything after
it (q = 1 - p32, the logs, the sums) is float64.

Two bands of z are outside any fp32 contract and no test input may enter them:
  (13, 17.5)    q = 1 - p is quantised in steps of 2^-24 (a 1-ulp difference in p is a 2^-24 / q relative difference in q) and then
                jumps to 0: two honest fp32 evaluations disagree by up to 84 per element.
  (-104, -87)   sigmoid(z) is an fp32 denormal: libm keeps it, exp(-z) = inf on the hardware exp gives p = 0 and the clamp 100.
Outside them p32 is exactly 0 or 1, or a normal number that every honest fp32 evaluation hits to a few ulp.

Bounds (derived, never tuned)
-----------------------------
Every gate has the form  |got - want| <= K_ULP * cond + (terms + 8) * 2^-24 * absdot + TINY:
  cond     first-order effect of an error of one ulp in p (and of the rounding of q = 1 - p) on the sum: the condition weights
           t/p + (1-t)/q of the BCE term, t for sum p t, 2 p for sum p^2, each times the ulp of the number it multiplies;
  K_ULP    4: the kernel states p "to 2-3 ulp" (loss_terms.h), plus the rounding of p32 itself;
  terms    length of the longest fp32 accumulation chain (per thread, plus the 6 levels of the wave reduction); + 8 for the
           roundings inside one term (log, the two products, 1 - t, the subtraction, ...);
  absdot   sum of |term|: the classic bound of a sum of `terms` roundings in any order;
  TINY     2^-126 per result: an fp32 operation whose result is below the normal range may lose that much.
Adam's p, m, v use the same form element-wise with terms = 2 (each is a two-term sum) and cond the first-order propagation of the
bounds of m and v through the update.
"""
import math

import torch

U = 2.0 ** -24          # unit roundoff of fp32
K_ULP = 4
TINY = 2.0 ** -126
BANDS = ((13.0, 17.5), (-104.0, -87.0))


def f64(t):
    if t is None or (t.dtype == torch.float64 and not t.is_cuda):
        return t
    return t.detach().cpu().double()


def f32(x):
    """A Python float rounded to fp32 (what a `float` argument of the C ABI receives)."""
    return float(torch.tensor(x, dtype=torch.float32))


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (x float64; 2^-149 below the normal range)."""
    _, e = torch.frexp(x.abs().clamp_min(TINY))
    return torch.ldexp(torch.ones_like(x), e - 24)


def in_bands(z):
    z = f64(z)
    bad = torch.zeros_like(z, dtype=torch.bool)
    for lo, hi in BANDS:
        bad |= (z > lo) & (z < hi)
    return bad


def p32(z):
    """The correctly rounded fp32 sigmoid, as float64."""
    return torch.sigmoid(f64(z)).float().double()


def planes(z, target):
    """-> z [B, K, V] float64, t [B, K, V] float64 (one-hot planes as given; a uint8 class map [B, ...] expanded: labels >= K
    belong to no plane)."""
    z = f64(z)
    B, K = z.shape[:2]
    z = z.reshape(B, K, -1)
    if target.dtype == torch.uint8:
        lab = target.detach().cpu().reshape(B, 1, -1).long()
        t = (lab == torch.arange(K).reshape(1, K, 1)).double()
    else:
        t = f64(target).reshape(B, K, -1)
    return z, t


# ----------------------------------------------------------------------------- loss forward
class Sums:
    """sums [K, 4] = I, P2, T2, S per class; cond / absdot [K, 4]: the two data-dependent factors of the bound (module docstring)."""

    def __init__(self, sums, cond, absdot):
        self.sums, self.cond, self.absdot = sums, cond, absdot

    def bound(self, terms):
        return K_ULP * self.cond + (terms + 8) * U * self.absdot + TINY


def bce_terms(p, t):
    """-> (term, weight): term = -(t max(log p, -100) + (1-t) max(log q, -100)) with q = 1 - p in float64; weight = the change of
    the term for an fp32 evaluation whose p is off by one ulp: t ulp(p)/p + (1-t) max(ulp(p), ulp(q))/q (q = 1 - p is rounded once
    more in fp32, to half an ulp of q).  Where p32 is exactly 0 or 1 the clamp gives the term exactly and the weight is 0."""
    q = 1.0 - p
    lp = torch.log(p).clamp_min(-100.0)
    lq = torch.log(q).clamp_min(-100.0)
    term = -(t * lp + (1.0 - t) * lq)
    wp = torch.where(p > 0, ulp32(p) / p.clamp_min(TINY), torch.zeros_like(p))
    wq = torch.where(q > 0, torch.maximum(ulp32(p), ulp32(q)) / q.clamp_min(TINY), torch.zeros_like(p))
    return term, t * wp + (1.0 - t) * wq


def dice_sums(z, target):
    z, t = planes(z, target)
    p = p32(z)
    term, w = bce_terms(p, t)
    up = ulp32(p)
    d = (0, 2)
    sums = torch.stack([(p * t).sum(d), (p * p).sum(d), (t * t).sum(d), term.sum(d)], 1)
    cond = torch.stack([(t * up).sum(d), (2 * p * up).sum(d), torch.zeros(z.shape[1], dtype=torch.float64), w.sum(d)], 1)
    absdot = torch.stack([(p * t).sum(d), (p * p).sum(d), torch.zeros(z.shape[1], dtype=torch.float64), term.abs().sum(d)], 1)
    return Sums(sums, cond, absdot)


def fwd_launch(V):
    """(chunks, per) of dice_fwd's launch."""
    chunks = -(-V // 32768)
    return chunks, -(-V // chunks)


def fwd_vector(V, label, aligned=True):
    """Does dice_bce_partial_kernel take its 16-byte loads?"""
    return (not label) and V % 4 == 0 and fwd_launch(V)[1] % 4 == 0 and aligned


def fwd_terms(V):
    """Longest fp32 accumulation chain of dice_bce_partial_kernel: 4 elements per 1024-stride trip of a thread (the scalar loop's
    ceil(per / 256) is never longer) + the 6 levels of the 64-lane reduction.  The workgroup's 4 wave partials and the chunks meet
    in double."""
    return 4 * -(-fwd_launch(V)[1] // 1024) + 6


def dice_loss(sums, count):
    s = f64(sums).reshape(-1, 4)
    dice = 1.0 - (2.0 * s[:, 0] + 1.0) / (s[:, 1] + s[:, 2] + 1.0)
    return (0.7 * dice.sum() + 0.3 * (s[:, 3] / count).sum()) / s.shape[0]


def dice_val_loss(sums):
    s = f64(sums).reshape(-1, 4)
    return (1.0 - (2.0 * s[:, 0] + 1.0) / (s[:, 1] + s[:, 2] + 1.0)).sum() / s.shape[0]


def dice_loss_bound(sums, bound, count):
    """First-order propagation of the bounds of the sums to the loss, + one fp32 rounding of the result."""
    s, b = f64(sums).reshape(-1, 4), bound
    den = s[:, 1] + s[:, 2] + 1.0
    d = 2.0 * b[:, 0] / den + (2.0 * s[:, 0] + 1.0) / den ** 2 * (b[:, 1] + b[:, 2])
    return float((0.7 * d.sum() + 0.3 * (b[:, 3] / count).sum()) / s.shape[0] + 2 * U * abs(float(dice_loss(s, count))))


# ----------------------------------------------------------------------------- loss backward
BWD_ROUNDINGS = 16      # fp32 roundings on the way from p to dz (I2, den, 1/den^2 : 4; ddice: 3; cd, cb: 5; dbce, p q, the sum: 4)


def dice_bce_grad(z, target, sums, g=1.0):
    """dz = (cd ddice + cb (p - t) / max(p q, 1e-12)) p q with p = p32(z) and everything else float64; cd = 0.7 g / K,
    cb = 0.3 g / (K B V); exactly 0 where p saturates (p q = 0), as ATen's binary_cross_entropy_backward gives.
    -> (dz [B, K, V], bound [B, K, V]): bound = K_ULP ulp(p) |d dz / d p| + BWD_ROUNDINGS 2^-24 (|dice part| + |bce part|) + TINY."""
    z, t = planes(z, target)
    B, K, V = z.shape
    s = f64(sums).reshape(K, 4)
    I2 = (2.0 * s[:, 0] + 1.0).reshape(1, K, 1)
    den = (s[:, 1] + s[:, 2] + 1.0).reshape(1, K, 1)
    cd, cb = 0.7 * g / K, 0.3 * g / K / (B * V)
    p = p32(z)
    pq = p * (1.0 - p)
    A = -(2.0 * t * den - I2 * 2.0 * p) / den ** 2
    clamp = pq.clamp_min(1e-12)
    dz = (cd * A + cb * (p - t) / clamp) * pq
    part_d = abs(cd) * (2.0 * t * den + 2.0 * I2 * p) / den ** 2 * pq
    part_b = abs(cb) * (p - t).abs() / clamp * pq
    slope = (1.0 - 2.0 * p).abs()
    d_dice = abs(cd) * (2.0 * I2 / den ** 2 * pq + A.abs() * slope)
    d_bce = abs(cb) * torch.where(pq >= 1e-12, torch.ones_like(p), (pq + (p - t).abs() * slope) / 1e-12)
    bound = K_ULP * ulp32(p) * (d_dice + d_bce) + BWD_ROUNDINGS * U * (part_d + part_b) + TINY
    return dz, torch.where(pq == 0, torch.zeros_like(bound), bound)


# ----------------------------------------------------------------------------- argmax / meandice, metric
def argmax_counts(z, label, K):
    """-> mask int64 [B, ...] (the first maximum wins), counts int64 [3, K] = voxels predicted / labelled / both per class (labels
    >= K are counted nowhere; None without a label), meandice (smooth 1e-6 over classes 1..K-1; None without a label or K = 1)."""
    z = z.detach().cpu()                 # comparisons of fp32 numbers are exact: no need to widen
    best, arg = z[:, 0].clone(), torch.zeros(z[:, 0].shape, dtype=torch.int64)
    for c in range(1, K):
        better = z[:, c] > best
        best = torch.where(better, z[:, c], best)
        arg = torch.where(better, torch.full_like(arg, c), arg)
    if label is None:
        return arg, None, None
    lab = label.detach().cpu().long().reshape(arg.shape)
    counts = torch.stack([torch.bincount(arg.reshape(-1), minlength=K)[:K],
                          torch.bincount(lab[lab < K].reshape(-1), minlength=K)[:K],
                          torch.bincount(arg[lab == arg].reshape(-1), minlength=K)[:K]])
    md = None
    if K > 1:
        c = counts.double()
        md = float(((2.0 * c[2, 1:] + 1e-6) / (c[0, 1:] + c[1, 1:] + 1e-6)).sum() / (K - 1))
    return arg, counts, md


def dice_metric(z, target):
    """[B, K] float32: Dice of the prediction z > 0 (the kernel's documented rule) per plane, 2 I / (P + T) rounded to fp32; 1 / 0
    for an empty target plane without / with predictions."""
    z, t = planes(z, target)
    pr = (z > 0).double()
    I, P, T = (pr * t).sum(2), pr.sum(2), t.sum(2)
    ratio = (2.0 * I / (P + T).clamp_min(1.0)).float()
    return torch.where(T == 0, (P == 0).float(), ratio)


# ----------------------------------------------------------------------------- Adam
def cosine_lr(base_lr, step, t_max, eta_min=0.0):
    """CosineAnnealingLR's closed form at scheduler epoch `step` (the optimizer's 1-based step n runs at epoch n - 1)."""
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * step / t_max)) / 2.0


def adam(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, bounds=False):
    """torch.optim.Adam's single-tensor step (no weight decay, no amsgrad) on float64 copies; step is 1-based, g is scaled by
    gscale BEFORE the moments.  -> (p, m, v), with bounds=True also (bound_p, bound_m, bound_v) for an fp32 evaluation FROM THE
    SAME INPUTS with bc1, sqrt(bc2) and lr / bc1 rounded to fp32 (module docstring; terms = 2)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    gs = g * gscale
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = m + (gs - m) * c1
    v1 = v * b2 + c2 * gs * gs
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    ss = lr / bc1
    s = v1.sqrt()
    denom = s / bc2s + eps
    upd = ss * m1 / denom
    p1 = p - upd
    if not bounds:
        return p1, m1, v1
    k = (2 + 8) * U
    bm = k * (m.abs() + c1 * (gs.abs() + m.abs())) + TINY
    bv = k * v1 + TINY
    ds = torch.minimum(bv / (2.0 * s).clamp_min(TINY), bv.sqrt())          # |sqrt(a) - sqrt(b)| <= min(|a-b| / 2 sqrt(a), sqrt|a-b|)
    dden = ds / bc2s + 4 * U * denom
    cond = abs(ss) * (bm / denom + m1.abs() * dden / denom ** 2)
    bp = cond + k * (p.abs() + upd.abs()) + TINY
    return (p1, m1, v1), (bp, bm, bv)


def bf16_rne(x):
    """fp32 tensor -> its bfloat16 bit patterns (int64 in [0, 65535]), round to nearest, ties to even, by integer arithmetic on the
    bits: add 0x7FFF plus the lowest kept bit, drop 16 bits.  (Finite inputs: a NaN payload is not preserved.)"""
    bits = x.detach().cpu().contiguous().view(torch.int32).long() & 0xFFFFFFFF
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF


def bf16_bits(t):
    """Bit patterns of a bfloat16 tensor, as bf16_rne returns them."""
    return t.detach().cpu().contiguous().view(torch.int16).long() & 0xFFFF


# ----------------------------------------------------------------------------- gates and inputs shared by the CPU and the GPU tests
def ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 the result must be exact; a NaN anywhere gives inf."""
    err = (f64(got).reshape(-1) - f64(want).reshape(-1)).abs()
    bound = bound.reshape(-1) if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(err), torch.full_like(err, math.inf), r)
    return float(r.max()) if r.numel() else 0.0


def sums_ratio(got, ref, terms):
    """Gate of the forward sums: T2 (an integer count) exact, I / P2 / S within ref.bound(terms).  -> worst error / bound (inf
    when T2 differs)."""
    got = f64(got).reshape(-1, 4)
    if not torch.equal(got[:, 2], ref.sums[:, 2]):
        return math.inf
    keep = [0, 1, 3]
    return ratio(got[:, keep], ref.sums[:, keep], ref.bound(terms)[:, keep])


SAT = (20.0, -20.0, 40.0, -40.0, 80.0, -80.0, 110.0, -110.0, math.inf, -math.inf)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def loss_inputs(B, K, V, seed=0, saturate=False):
    """-> z [B, K, V] fp32 = 3 randn clipped to |z| <= 9, label [B, V] uint8 uniform over the K classes.  saturate (V >= 20, K >= 2):
    the first 20 voxels of every plane hold the 10 saturation points SAT twice, labelled 0 the first time and 1 the second, so every
    point meets both target values in planes 0 and 1."""
    z = (3.0 * rnd(B, K, V, seed=seed)).clamp(-9.0, 9.0)
    lab = torch.randint(0, K, (B, V), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.uint8)
    if saturate:
        z[:, :, :20] = torch.tensor(SAT + SAT)
        lab[:, :10], lab[:, 10:20] = 0, 1
    assert not bool(in_bands(z).any())
    return z, lab


def one_hot(lab, K):
    """uint8 class map [B, V] -> float planes [B, K, V] (labels >= K: no plane)."""
    return (lab.long().unsqueeze(1) == torch.arange(K).reshape(1, K, 1)).float()


def adam_inputs(n, seed=0, warm=False):
    """p: randn, every odd element scaled by 1e-3 (so that an error of 1e-8 shows against the parameter's own ulp); g: 1e-3 randn
    with every 7th element 0 and every 11th 1e-30; m, v: zeros (the first step) or, warm, a plausible running state that is zero
    on every 5th element."""
    p = rnd(n, seed=seed + 1)
    p[1::2] *= 1e-3
    g = rnd(n, seed=seed + 2) * 1e-3
    g[::7] = 0.0
    g[3::11] = 1e-30
    m, v = torch.zeros(n), torch.zeros(n)
    if warm:
        m, v = rnd(n, seed=seed + 3) * 1e-3, (rnd(n, seed=seed + 4) * 1e-3) ** 2
        m[::5] = 0.0
        v[::5] = 0.0
    return p, g, m, v


def bf16_ties(count, seed=0):
    """fp32 numbers exactly half way between two bfloat16 neighbours (low half 0x8000), normal, both parities of the kept lsb."""
    g = torch.Generator().manual_seed(seed)
    hi = torch.randint(0x3000, 0x4800, (count,), generator=g)           # exponents 2^-31 .. 2^17, sign +
    hi[1::2] |= 0x8000                                                  # every other one negative
    hi[: count // 2] &= ~1                                              # even kept lsb: ties round down in magnitude
    hi[count // 2:] |= 1                                                # odd: up
    bits = (hi << 16) | 0x8000
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
