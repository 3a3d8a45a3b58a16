"""GPU checks of the low-resolution simulation (micformer_amd.lowres, csrc/volume_lowres.hip) against the float64 referee of
tests/lowres_ref.py on its cases: shapes (5, 9, 70) (W crossing a tile edge, D short enough for t = 1..3), (33, 34, 35) and
(64, 64, 64), B = 3, C = 2, z-score-like and min-max-like inputs with a zero background, and two sets of six targets per shape
(exact halves, t = 1, t = n on one or two axes, t = n - 1, odd ratios, one channel off).  The tolerance E = 2.4e-6 of the input
channel's max - min is 4 x the float32 referee's own distance from the float64 referee (tests/test_lowres_cpu.py::test_fp32_gate).
(128, 8, 136) is added for what the three shapes do not reach: D above one wave of lines per block, W above two tiles and a
multiple of 8, so that the 16-byte store path runs next to the scalar one of W = 70 and 35.

Measured on an MI355X: fp32 I/O at most 5.7e-7 of the range from the referee, fp16 I/O at most 2.4e-7 beyond half a float16 step;
augment_moreda at most 0.12 of the sum of the two tolerances from the composed referees."""
import numpy as np
import pytest
import torch

import intensity_ref as IR
import lowres_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
IDS = [f"{'x'.join(map(str, s))}-{k}-{n}" for s, k, n in CASES]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                      # (a copy: the cached references are read-only)


def _simulate(x, target, dtype=torch.float32, **kw):
    from micformer_amd.lowres import simulate_low_resolution
    return simulate_low_resolution(_dev(x).to(dtype), _dev(target), **kw)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _half_step(v):
    """half the float16 spacing at |v| (normal range: 2^(e - 10), 2^-24 below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_io_is_within_e_of_the_referee(case):
    x, t, want = R.reference(*case)
    out = _simulate(x, t)
    got = out.cpu().numpy().astype(np.float64)
    err = (np.abs(got - want) / R.span(x)).max(axis=(2, 3, 4))
    print(f"{case}: |gpu - referee| / range per (sample, channel): {np.array2string(err.ravel(), precision=2)}; E {R.E:.2e}")
    assert np.isfinite(got).all() and (err <= R.E).all()
    off = R.is_off(case[0], t)
    assert off.any() and np.array_equal(out.cpu().numpy()[off].view(np.int32), x[off].view(np.int32))   # off: bit for bit


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp16_io_is_within_e_and_half_a_step(case):
    x, t, want = R.reference(*case, half=True)
    out = _simulate(x, t, torch.float16)
    assert out.dtype == torch.float16
    got = out.float().cpu().numpy().astype(np.float64)
    excess = np.abs(got - want) - _half_step(want)
    err = (excess / R.span(x)).max(axis=(2, 3, 4))
    print(f"{case}: (|gpu - referee| - half a float16 step) / range: {np.array2string(err.ravel(), precision=2)}; E {R.E:.2e}")
    assert np.isfinite(got).all() and (err <= R.E).all()
    off = R.is_off(case[0], t)
    assert np.array_equal(out.cpu().numpy()[off].view(np.int16), x.astype(np.float16)[off].view(np.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_wide_volume_takes_the_vector_store_and_many_lines(dtype):
    """(128, 8, 136): 16-byte stores (W a multiple of 8, torch's allocation aligned), three W tiles, more lines than one block."""
    shape = (128, 8, 136)
    g = np.random.default_rng(77)
    x = g.standard_normal((2, 2) + shape).astype(np.float32)
    if dtype == torch.float16:
        x = x.astype(np.float16).astype(np.float32)
    t = np.array([[(64, 4, 68), (128, 8, 136)], [(127, 7, 101), (77, 8, 136)]], np.int32)
    want = R.simulate(x, t)
    out = _simulate(x, t, dtype)
    got = out.float().cpu().numpy().astype(np.float64)
    slack = _half_step(want) if dtype == torch.float16 else 0.0
    err = ((np.abs(got - want) - slack) / R.span(x)).max(axis=(2, 3, 4))
    print(f"{shape} {dtype}: {np.array2string(err.ravel(), precision=2)}; E {R.E:.2e}")
    assert (err <= R.E).all()
    assert torch.equal(_bits(out[0, 1]), _bits(_dev(x).to(dtype)[0, 1]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", R.NAMES)
def test_in_place_equals_out_of_place_and_off_is_untouched(name, dtype):
    from micformer_amd.lowres import simulate_low_resolution
    shape = (33, 34, 35)
    x, t, _ = R.reference(shape, "minmax", name)
    xd, td = _dev(x).to(dtype), _dev(t)
    want = simulate_low_resolution(xd, td)
    out = torch.full_like(xd, 7.0)
    back = simulate_low_resolution(xd, td, out=out)
    assert back is out and torch.equal(_bits(out), _bits(want))
    again = xd.clone()
    assert simulate_low_resolution(again, td, out=again) is again and torch.equal(_bits(again), _bits(want))
    off = torch.from_numpy(R.is_off(shape, t)).cuda()
    assert off.any() and torch.equal(_bits(again[off]), _bits(xd[off])) and not torch.equal(_bits(again[~off]), _bits(xd[~off]))
    with pytest.raises(ValueError, match="out"):
        simulate_low_resolution(xd, td, out=out.float() if dtype == torch.float16 else out.half())
    with pytest.raises(ValueError, match="out"):
        simulate_low_resolution(xd, td, out=out[:, :1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_all_targets_off_return_the_input_bit_for_bit(dtype):
    from micformer_amd.lowres import simulate_low_resolution
    shape = (5, 9, 70)
    x = _dev(R.volume(shape, "zscore")).to(dtype)
    x[0, 0, 0, 0, :4] = torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")], dtype=dtype)
    x[1, 1, 2, 3, 5] = 6.0e-8 if dtype == torch.float16 else 1.0e-40                                  # a subnormal
    t = torch.tensor(shape, dtype=torch.int32).expand(R.B, R.C, 3).contiguous().cuda()
    out = simulate_low_resolution(x, t)
    assert out.data_ptr() != x.data_ptr() and torch.equal(_bits(out), _bits(x))
    keep = x.clone()
    simulate_low_resolution(x, t, out=x)
    assert torch.equal(_bits(x), _bits(keep))


@pytest.mark.parametrize("name", R.NAMES)
def test_runs_are_bit_equal_and_samples_independent(name):
    x, t, _ = R.reference((33, 34, 35), "zscore", name)
    a = _simulate(x, t)
    b = _simulate(x, t)
    assert torch.equal(_bits(a), _bits(b))
    for i in range(R.B):                                              # a sample alone is the sample inside the batch
        alone = _simulate(x[i:i + 1], t[i:i + 1])
        assert torch.equal(_bits(alone[0]), _bits(a[i]))
    order = [2, 0, 1]                                                 # ... and wherever it stands in the batch
    c = _simulate(x[order], t[order])
    assert torch.equal(_bits(c), _bits(a[order]))


def test_non_finite_voxels_stay_in_their_channel():
    x, t, _ = R.reference((33, 34, 35), "zscore", "a")
    clean = _simulate(x, t)
    bad = x.copy()
    bad[0, 0, 3, 4, 5], bad[0, 0, 20, 30, 1], bad[0, 0, 32, 33, 34] = np.nan, np.inf, -np.inf
    for b, c in ((0, 0), (2, 1)):                                     # ... and a NaN at a voxel the nearest gather does pick
        bad[(b, c) + tuple(R.gather_index(n, v)[v // 2] for n, v in zip(x.shape[2:], t[b, c]))] = np.nan
    got = _simulate(bad, t)
    torch.cuda.synchronize()
    for b in range(R.B):
        for c in range(R.C):
            if (b, c) not in {(0, 0), (2, 1)}:
                assert torch.equal(_bits(got[b, c]), _bits(clean[b, c])), (b, c)
    assert not torch.isfinite(got[0, 0]).all() and not torch.isfinite(got[2, 1]).all()
    assert torch.equal(_bits(_simulate(x, t)), _bits(clean))          # the library is in order afterwards


def test_targets_out_of_range_are_clamped_on_the_device():
    shape = (33, 34, 35)
    x = R.volume(shape, "minmax")
    wild = np.array([[(0, 17, 40), (-5, 34, 35)], [(38, 39, 40), (33, 0, 23)], [(16, 17, -2147483648), (2147483647, 34, 18)]], np.int32)
    tame = np.array([[(1, 17, 35), (1, 34, 35)], [(33, 34, 35), (33, 1, 23)], [(16, 17, 1), (33, 34, 18)]], np.int32)
    a, b = _simulate(x, wild), _simulate(x, tame)
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(a[1, 0]), _bits(_dev(x)[1, 0]))          # n + 5 on every axis: off


def test_a_captured_graph_replays_and_reads_new_targets():
    from micformer_amd.lowres import simulate_low_resolution
    shape = (33, 34, 35)
    x, t, _ = R.reference(shape, "zscore", "a")
    t2 = R.targets(shape, "b")
    flip = R.is_off(shape, t) & ~R.is_off(shape, t2)
    assert flip.any() and (~R.is_off(shape, t) & R.is_off(shape, t2)).any()      # a channel goes off -> on, another on -> off
    xd, td = _dev(x).half(), _dev(t)
    out = torch.empty_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        simulate_low_resolution(xd, td, out=out)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        simulate_low_resolution(xd, td, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(simulate_low_resolution(xd, td)))
    td.copy_(_dev(t2))
    graph.replay()
    torch.cuda.synchronize()
    want = simulate_low_resolution(xd, _dev(t2))
    assert torch.equal(_bits(out), _bits(want)) and not torch.equal(_bits(out), _bits(simulate_low_resolution(xd, _dev(t))))


# ---- augment_moreda -------------------------------------------------------------------------------------------------------------

#               sigma noise bright contrast gamma mode retain 0
MOREDA_ROWS = [(0.8, 0.05, 0.9, 1.15, 1.5, 1, 0, 0), (0.0, 0.0, 1.0, 1.0, 1.3, 2, 0, 0), (0.5, 0.0, 1.2, 0.8, 1.0, 0, 0, 0),
               (0.0, 0.08, 1.0, 1.0, 1.5, 1, 0, 0), (1.0, 0.0, 1.0, 1.2, 1.4, 2, 0, 0), (0.0, 0.0, 1.0, 1.0, 1.0, 0, 0, 0)]


def _split(params):
    first, last = params.copy(), np.tile(np.array(IR.ROWS["gamma"][-1], np.float32), params.shape[:2] + (1,))
    first[:, :, 4:7] = last[:, :, 4:7]
    last[:, :, 4:7] = params[:, :, 4:7]
    return first, last


def test_augment_moreda_is_the_two_referees_composed():
    """float32 image: the intensity referee up to the contrast, the low-resolution referee, the intensity referee's gamma step,
    all in float64, against the device's three calls, within the sum of the two tolerances.  The exponents are above 1 and
    retain_stats is off: the power law's slope is bounded (by the exponent, at most 1.5), where an exponent below 1 has an
    unbounded slope at the channel's minimum and would turn a voxel's error before the step into any multiple of it."""
    from micformer_amd.lowres import augment_moreda
    shape = (33, 34, 35)
    x = R.volume(shape, "minmax")
    params = np.array(MOREDA_ROWS, np.float32).reshape(R.B, R.C, 8)
    t = R.targets(shape, "a")
    first, last = _split(params)
    mid, _ = IR.augment(x, first, IR.SEEDS)
    low = R.simulate(mid, t)
    want, _ = IR.augment(low, last, IR.SEEDS)
    got = augment_moreda(_dev(x), _dev(params), _dev(IR.SEEDS), _dev(t)).cpu().numpy().astype(np.float64)
    tol = IR.E * IR.span(want) + R.E * R.span(mid)
    err = (np.abs(got - want) / tol).max(axis=(2, 3, 4))
    print(f"|gpu - composed referees| / (E_intensity x range + E_lowres x range): {np.array2string(err.ravel(), precision=2)}")
    assert np.isfinite(got).all() and (err <= 1.0).all()
    assert np.abs(want - IR.augment(mid, last, IR.SEEDS)[0]).max() > 0.1          # the step in the middle matters


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_augment_moreda_with_every_target_off_is_the_split_chain(dtype):
    from micformer_amd.intensity import augment_intensity
    from micformer_amd.lowres import augment_moreda
    shape = (33, 34, 35)
    x, p, s, _, _ = IR.reference(shape, "zscore", "gamma")
    xd, pd, sd = _dev(x).to(dtype), _dev(p), _dev(s)
    off = torch.tensor(shape, dtype=torch.int32).expand(R.B, R.C, 3).contiguous().cuda()
    first, last = _split(p)
    want = augment_intensity(augment_intensity(xd, _dev(first), sd), _dev(last), sd)
    got = augment_moreda(xd, pd, sd, off)
    assert torch.equal(_bits(got), _bits(want))
    inplace = xd.clone()
    assert augment_moreda(inplace, pd, sd, off, out=inplace) is inplace and torch.equal(_bits(inplace), _bits(want))
    on = _dev(R.targets(shape, "a"))
    assert not torch.equal(_bits(augment_moreda(xd, pd, sd, on)), _bits(want))


def test_python_argument_checks_on_device_tensors():
    """TypeErrors before ValueErrors; a tensor on the wrong device, a non-contiguous one and a wrong target are refused before any
    launch (the output tensor keeps its sentinel)."""
    from micformer_amd.lowres import simulate_low_resolution
    x = torch.zeros(1, 2, 4, 6, 8, device="cuda")
    t = torch.ones(1, 2, 3, dtype=torch.int32, device="cuda")
    out = torch.full_like(x, 7.0)
    with pytest.raises(TypeError, match="target"):                    # a TypeError of a later argument before a ValueError of an earlier
        simulate_low_resolution(x[:, :, :, :, ::2], t.long(), out=out)
    with pytest.raises(ValueError, match="image must be contiguous"):
        simulate_low_resolution(x[:, :, :, :, ::2], t, out=out)
    with pytest.raises(ValueError, match="target must be contiguous"):
        simulate_low_resolution(x, torch.ones(1, 2, 6, dtype=torch.int32, device="cuda")[:, :, ::2], out=out)
    with pytest.raises(ValueError, match="target must be a CUDA"):
        simulate_low_resolution(x, t.cpu(), out=out)
    with pytest.raises(ValueError, match="image must be a CUDA"):
        simulate_low_resolution(x.cpu(), t, out=out)
    with pytest.raises(ValueError, match="target must have shape"):
        simulate_low_resolution(x, torch.ones(1, 2, 4, dtype=torch.int32, device="cuda"), out=out)
    with pytest.raises(TypeError, match="target"):
        simulate_low_resolution(x, t.float(), out=out)
    with pytest.raises(ValueError, match="out"):
        simulate_low_resolution(x, t, out=out.cpu())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
