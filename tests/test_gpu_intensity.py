"""GPU checks of the intensity augmentation (micformer_amd.intensity, csrc/volume_intensity.hip) against the float64 referee of
tests/intensity_ref.py on its cases: shapes (5, 9, 70) (two axes shorter than the radius, W crossing a tile edge), (33, 34, 35)
and (64, 64, 64), B = 3, C = 2, z-score-like and min-max-like inputs with a zero background, and two sets of six parameter rows
(each step alone, sigma 0.1 and 2.0, contrast below and above 1, gamma 0.7 and 1.5 plain and inverted with and without
retain_stats, every step together, every step off).  The tolerance E = 1.72e-6 of the channel's max - min is 4 x the float32
referee's own distance from the float64 referee (tests/test_intensity_cpu.py::test_fp32_gate).

`stats`: the statistics are float64 fixed-order sums over float32 voxels, and a float32 voxel is within E x range of the referee's,
not within 1e-9.  So the 1e-9 relative bound is held where it can be: against the referee's float64 formulas applied to the very
float32 field the device summed, which further calls with the later steps switched off return exactly (the blurred field; the
field before the power law; the field after it).  Against the referee's own statistics the bound is what E allows the voxels.

Measured on an MI355X: fp32 I/O at most 3.6e-7 of the range from the referee, fp16 I/O at most 2.2e-7 beyond half a float16 step;
stats within 3.4e-16 relative of the float64 sums over the device's fields (min and max equal), within 1.8e-7 of the range of the
referee's own."""
import numpy as np
import pytest
import torch

import intensity_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [f"{'x'.join(map(str, s))}-{k}-{n}" for s, k, n in CASES]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                      # (a copy: the cached references are read-only)


def _augment(x, params, seeds, dtype=torch.float32, **kw):
    from micformer_amd.intensity import augment_intensity
    return augment_intensity(_dev(x).to(dtype), _dev(params), _dev(seeds), **kw)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_io_is_within_e_of_the_referee(case):
    x, p, s, want, _ = R.reference(*case)
    got = _augment(x, p, s).cpu().numpy().astype(np.float64)
    err = (np.abs(got - want) / R.span(want)).max(axis=(2, 3, 4))
    print(f"{case}: |gpu - referee| / range per (sample, channel): {np.array2string(err.ravel(), precision=2)}; E {R.E:.2e}")
    assert np.isfinite(got).all() and (err <= R.E).all()


def _half_step(v):
    """half the float16 spacing at |v| (normal range: 2^(e - 10), 2^-24 below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp16_io_is_within_e_and_half_a_step(case):
    x, p, s, want, _ = R.reference(*case, half=True)
    out = _augment(x, p, s, torch.float16)
    assert out.dtype == torch.float16
    got = out.float().cpu().numpy().astype(np.float64)
    excess = np.abs(got - want) - _half_step(want)
    err = (excess / R.span(want)).max(axis=(2, 3, 4))
    print(f"{case}: (|gpu - referee| - half a float16 step) / range: {np.array2string(err.ravel(), precision=2)}; E {R.E:.2e}")
    assert np.isfinite(got).all() and (err <= R.E).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stats(case):
    x, p, s, _, ref_stats = R.reference(*case)
    out, stats = _augment(x, p, s, return_stats=True)
    stats = stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (R.B, R.C, 8) and not stats[:, :, 7].any()

    def field(neutral_from):                                         # the device's own float32 field with the later steps off
        q = p.copy()
        q[:, :, neutral_from:7] = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0], np.float32)[neutral_from:7]
        return _augment(x, q, s).cpu().numpy().astype(np.float64)
    blurred, before = field(2), field(4)
    q = p.copy()
    q[:, :, 6] = 0.0
    after = _augment(x, q, s).cpu().numpy().astype(np.float64)
    want = np.zeros_like(stats)
    want[:, :, 0], want[:, :, 1], want[:, :, 2] = blurred.mean(axis=(2, 3, 4)), blurred.min(axis=(2, 3, 4)), blurred.max(axis=(2, 3, 4))
    retain = (p[:, :, 5] != 0) & (p[:, :, 6] != 0)
    sign = np.where(p[:, :, 5] == 2, -1.0, 1.0)
    want[:, :, 3] = np.where(retain, sign * before.mean(axis=(2, 3, 4)), 0.0)
    want[:, :, 4] = np.where(retain, before.std(axis=(2, 3, 4)), 0.0)
    want[:, :, 5] = np.where(retain, sign * after.mean(axis=(2, 3, 4)), 0.0)
    want[:, :, 6] = np.where(retain, after.std(axis=(2, 3, 4)), 0.0)
    rel = np.abs(stats - want) / np.where(want != 0, np.abs(want), 1.0)
    print(f"{case}: stats vs float64 sums over the device's fields, worst relative difference per slot: "
          f"{np.array2string(rel.max(axis=(0, 1)), precision=2)}")
    assert np.array_equal(stats[:, :, 1:3], want[:, :, 1:3])         # min and max: exact
    assert (rel <= 1e-9).all()
    # ... and against the referee's own statistics: what E allows every voxel, it allows their mean, min and max; a standard
    # deviation moves by at most twice that.  Brightness and contrast stretch the range by at most their factors.
    rng = (ref_stats[:, :, 2] - ref_stats[:, :, 1]) * np.maximum(p[:, :, 2], 1.0) * np.maximum(p[:, :, 3], 1.0)
    err = np.abs(stats - ref_stats) / rng[:, :, None]
    print(f"{case}: stats vs the referee's, worst |diff| / range per slot: {np.array2string(err.max(axis=(0, 1)), precision=2)}")
    assert (err <= R.E * np.array([1, 1, 1, 1, 2, 1, 2, 1])).all()
    assert torch.equal(out, _augment(x, p, s))                       # the record changes nothing


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_neutral_parameters_return_the_input_bit_for_bit(dtype):
    from micformer_amd.intensity import NEUTRAL, augment_intensity
    x = _dev(R.volume((5, 9, 70), "zscore")).to(dtype)
    x[0, 0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")], dtype=dtype)
    x[1, 1, 2, 3, 5] = 6.0e-8 if dtype == torch.float16 else 1.0e-40                                  # a subnormal
    p = torch.tensor(NEUTRAL, dtype=torch.float32).expand(R.B, R.C, 8).contiguous().cuda()
    out = augment_intensity(x, p, _dev(R.SEEDS))
    assert out.data_ptr() != x.data_ptr() and torch.equal(_bits(out), _bits(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", sorted(R.ROWS))
def test_in_place_equals_out_of_place_and_out_is_written(name, dtype):
    from micformer_amd.intensity import augment_intensity
    x, p, s, _, _ = R.reference((33, 34, 35), "minmax", name)
    xd, pd, sd = _dev(x).to(dtype), _dev(p), _dev(s)
    want = augment_intensity(xd, pd, sd)
    out = torch.full_like(xd, 7.0)
    back = augment_intensity(xd, pd, sd, out=out)
    assert back is out and torch.equal(_bits(out), _bits(want))
    again = xd.clone()
    assert augment_intensity(again, pd, sd, out=again) is again and torch.equal(_bits(again), _bits(want))
    with pytest.raises(ValueError, match="out"):
        augment_intensity(xd, pd, sd, out=out.float() if dtype == torch.float16 else out.half())
    with pytest.raises(ValueError, match="out"):
        augment_intensity(xd, pd, sd, out=out[:, :1])


@pytest.mark.parametrize("name", sorted(R.ROWS))
def test_runs_are_bit_equal_and_samples_independent(name):
    x, p, s, _, _ = R.reference((33, 34, 35), "zscore", name)
    a, sa = _augment(x, p, s, return_stats=True)
    b, sb = _augment(x, p, s, return_stats=True)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(sa, sb)
    for i in range(R.B):                                              # a sample alone is the sample inside the batch
        alone, st = _augment(x[i:i + 1], p[i:i + 1], s[i:i + 1], return_stats=True)
        assert torch.equal(_bits(alone[0]), _bits(a[i])) and torch.equal(st[0], sa[i])
    order = [2, 0, 1]                                                 # ... and wherever it stands in the batch
    c = _augment(x[order], p[order], s[order])
    assert torch.equal(_bits(c), _bits(a[order]))


def test_noise_depends_on_the_seed_and_the_channel_not_on_the_batch():
    x = np.zeros((4, 2, 5, 9, 70), np.float32)
    p = np.tile(np.array([0.0, 0.5, 1.0, 1.0, 1.0, 0, 0, 0], np.float32), (4, 2, 1))
    s = np.array([11, 12, 11, -(2 ** 63)], np.int64)
    z = _augment(x, p, s)
    assert torch.equal(z[0], z[2]) and not torch.equal(z[0], z[1]) and not torch.equal(z[0, 0], z[0, 1])
    assert torch.equal(_augment(x[:1], p[:1], s[2:3])[0], z[2])       # B = 1
    flat = z.cpu().numpy().astype(np.float64).reshape(4, 2, -1) / 0.5
    assert np.abs(flat.mean(axis=2)).max() < 0.1 and np.abs(flat.std(axis=2) - 1).max() < 0.1
    want = np.stack([[R.normal(R.words(s[b], c, flat.shape[2])) for c in range(2)] for b in range(4)])
    assert np.abs(flat - want).max() < 5e-6                           # the referee's draw (float32 Box-Muller: test_intensity_cpu)
    p[:, :, 1] = 0.0
    assert not _augment(x, p, s).any()


def test_a_captured_graph_replays_and_reads_new_parameters():
    from micformer_amd.intensity import augment_intensity
    x, p, s, _, _ = R.reference((33, 34, 35), "zscore", "gamma")
    p2 = R.rows("steps")
    s2 = np.array([5, 6, 7], np.int64)
    xd, pd, sd = _dev(x).half(), _dev(p), _dev(s)
    out = torch.empty_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        augment_intensity(xd, pd, sd, out=out)                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment_intensity(xd, pd, sd, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(augment_intensity(xd, pd, sd)))
    pd.copy_(_dev(p2))
    sd.copy_(_dev(s2))
    graph.replay()
    torch.cuda.synchronize()
    want = augment_intensity(xd, _dev(p2), _dev(s2))
    assert torch.equal(_bits(out), _bits(want)) and not torch.equal(_bits(out), _bits(augment_intensity(xd, _dev(p), _dev(s))))


@pytest.mark.parametrize("value", [0.0, 0.7, -3.0])
@pytest.mark.parametrize("name", sorted(R.ROWS))
def test_a_constant_channel_comes_out_finite(name, value):
    x = np.full((R.B, R.C, 5, 9, 70), value, np.float32)
    p = R.rows(name)
    out, stats = _augment(x, p, R.SEEDS, return_stats=True)
    assert torch.isfinite(out).all() and torch.isfinite(stats).all()
    quiet = p[:, :, 1] == 0                                           # without noise: constant in, the same constant out ...
    got = out.cpu().numpy()
    bright = np.float32(value) * p[:, :, 2]
    assert np.abs(got[quiet] - bright[quiet][:, None, None, None]).max() <= 1e-6 * max(abs(value), 1.0)


def test_non_finite_voxels_and_parameters_stay_in_their_channel():
    x, p, s, _, _ = R.reference((33, 34, 35), "zscore", "gamma")
    clean = _augment(x, p, s)
    bad_x, bad_p = x.copy(), p.copy()
    bad_x[0, 0, 3, 4, 5], bad_x[0, 0, 20, 30, 1], bad_x[0, 0, 32, 33, 34] = np.nan, np.inf, -np.inf
    bad_p[1, 1] = np.array([np.nan, np.nan, np.inf, np.nan, np.nan, 2, 1, 0], np.float32)
    bad_p[2, 0] = np.array([np.inf, np.inf, -np.inf, -2.0, -np.inf, np.nan, np.nan, np.nan], np.float32)
    got = _augment(bad_x, bad_p, s)                                   # returns MICF_OK: no exception
    torch.cuda.synchronize()
    touched = {(0, 0), (1, 1), (2, 0)}
    for b in range(R.B):
        for c in range(R.C):
            if (b, c) not in touched:
                assert torch.equal(_bits(got[b, c]), _bits(clean[b, c])), (b, c)
    assert not torch.isfinite(got[0, 0]).all() and not torch.isfinite(got[1, 1]).all()
    again = _augment(x, p, s)                                         # the library is in order afterwards
    assert torch.equal(_bits(again), _bits(clean))
