"""GPU tests of the volume restore (micformer_amd/restore.py, csrc/volume_restore.hip) against the referee tests/restore_ref.py.

Acceptance rule (restore_ref.judge): where the referee's top-1 minus top-2 margin is >= tau the device label equals the referee's;
where it is < tau the device label is a class whose referee value is within tau of the maximum.  tau = 1e-4 (logits) / 1e-5
(probabilities).  The near-tie share of every case is a condition, <= 5e-4, asserted on the referee alone before the device runs.
Exact cases (output shape = source shape, where every tap weight is 0 or 1) take no tolerance."""
import numpy as np
import pytest
import torch

import restore_ref as R
from tiny_model import tiny_head

pytestmark = pytest.mark.gpu

SRC32 = (32, 32, 32)
CASES = {
    # name: (source grid, output shape, K)
    "up_45x64x50": (SRC32, (45, 64, 50), 8),
    "down_23x40x31": (SRC32, (23, 40, 31), 8),
    "16x20x24_to_61x33x50": ((16, 20, 24), (61, 33, 50), 8),
    "K1": (SRC32, (45, 64, 50), 1),
    "K2": (SRC32, (45, 64, 50), 2),
    "K32": (SRC32, (45, 64, 50), 32),
}


def _values(K):
    """K - 1 distinct non-zero label values that fit int16 (MM-WHS's own for 8 classes)."""
    return R.MMWHS_LABEL_VALUES if K == 8 else tuple(100 + 37 * k for k in range(K - 1))


def _referee_condition(logits, shape, probabilities, tag):
    """The referee alone: its near-tie share stays within the cap.  -> the referee's interpoland [K, d, h, w] on the CPU."""
    up = R.upsample(logits, shape, probabilities)
    share = R.near_tie_share(R.margin_of(up), probabilities)
    print(f"{tag}: referee near-tie share {share:.2e} (tau {R.TAU[probabilities]:g})")
    assert share <= R.MAX_NEAR_TIE_SHARE, (tag, share)
    return up


def _judge(labels, up, values, probabilities, tag):
    res = R.judge(labels.cpu(), up, values, probabilities)
    print(f"{tag}: {res}")
    assert res["ok"], (tag, res)
    return res


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("name", list(CASES))
def test_restore_meets_the_acceptance_rule(name, probabilities):
    from micformer_amd import restore
    src, shape, K = CASES[name]
    logits = R.make_logits(src, K)
    up = _referee_condition(logits[0], shape, probabilities, name)
    dev = logits.cuda()
    values = _values(K)
    got16 = restore.restore_labels(dev[0], shape, label_values=values, probabilities=probabilities)
    got32 = restore.restore_labels(dev, shape, label_values=values, probabilities=probabilities, dtype=torch.int32)
    got8 = restore.restore_labels(dev[0], shape, label_values=None, probabilities=probabilities)
    assert got16.dtype == torch.int16 and got32.dtype == torch.int32 and got8.dtype == torch.uint8
    assert got16.shape == got32.shape == got8.shape == shape and got16.is_contiguous()
    _judge(got16, up, values, probabilities, f"{name} int16")
    _judge(got32, up, values, probabilities, f"{name} int32")
    _judge(got8, up, None, probabilities, f"{name} uint8")
    # the three outputs are one argmax seen through three tables
    assert torch.equal(got16.int(), got32)
    assert torch.equal(R.label_table(values, K, "cuda")[got8.long()].int(), got32)


def test_interpolands_differ_and_are_not_swapped():
    """The two interpolands give different labels on about 1.4 % of the voxels of this input: each must fail the other's referee."""
    from micformer_amd import restore
    src, shape, K = CASES["up_45x64x50"]
    logits = R.make_logits(src, K)
    up = {p: _referee_condition(logits[0], shape, p, "swap") for p in (False, True)}
    got = {p: restore.restore_labels(logits.cuda()[0], shape, probabilities=p) for p in (False, True)}
    differ = float((got[False] != got[True]).float().mean())
    print(f"labels that differ between the interpolands: {differ:.3%}")
    assert 0.005 < differ < 0.03
    for p in (False, True):
        assert R.judge(got[p].cpu(), up[p], R.MMWHS_LABEL_VALUES, p)["ok"]
        assert not R.judge(got[p].cpu(), up[not p], R.MMWHS_LABEL_VALUES, not p)["ok"]


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
def test_batch_of_three_shapes_equals_the_single_calls(probabilities):
    from micformer_amd import restore
    shapes = [(45, 64, 50), (23, 40, 31), (61, 33, 70)]
    logits = R.make_logits((20, 24, 28), 8, batch=3)
    ups = [_referee_condition(logits[b], shapes[b], probabilities, f"batch sample {b}") for b in range(3)]
    dev = logits.cuda()
    got = restore.restore_batch(dev, shapes, probabilities=probabilities)
    assert isinstance(got, list) and len(got) == 3
    for b in range(3):
        assert got[b].shape == shapes[b] and got[b].dtype == torch.int16
        _judge(got[b], ups[b], R.MMWHS_LABEL_VALUES, probabilities, f"batch sample {b}")
        single = restore.restore_labels(dev[b].contiguous(), shapes[b], probabilities=probabilities)
        assert torch.equal(single, got[b]), b                          # bit for bit


def test_batch_beyond_one_launch_chunk():
    """11 samples (the descriptors travel 8 per launch), uint8 class maps, every sample against its single call."""
    from micformer_amd import restore
    logits = R.make_logits((10, 12, 14), 5, batch=11).cuda()
    shapes = [(9 + 3 * b, 40 - 2 * b, 17 + 5 * b) for b in range(11)]
    for p in (False, True):
        got = restore.restore_batch(logits, shapes, label_values=None, probabilities=p)
        for b in range(11):
            assert torch.equal(got[b], restore.restore_labels(logits[b].contiguous(), shapes[b], label_values=None, probabilities=p)), b


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
@pytest.mark.parametrize("shape", [(32, 32, 32), (16, 20, 24), (1, 7, 130)])
def test_identity_shape_is_the_plain_argmax(shape, probabilities):
    """Output shape = source shape: every tap weight is 0 or 1, the labels are logits.argmax(1) through the lookup, no tolerance
    (softmax is monotone; the recipe has no two logits of a voxel close enough for their probabilities to round together)."""
    from micformer_amd import restore
    logits = R.make_logits(shape, 8)
    want = R.label_table(R.MMWHS_LABEL_VALUES, 8)[logits[0].argmax(0)]
    if probabilities:
        assert torch.equal(torch.softmax(logits[0], 0).argmax(0), logits[0].argmax(0))
    got = restore.restore_labels(logits.cuda()[0], shape, probabilities=probabilities)
    assert torch.equal(got.cpu().long(), want)
    got8 = restore.restore_labels(logits.cuda()[0], shape, label_values=None, probabilities=probabilities)
    assert torch.equal(got8.cpu().long(), logits[0].argmax(0))


def test_exact_ties_go_to_the_lowest_class():
    from micformer_amd import restore
    logits = torch.zeros(1, 4, 5, 6, 7)
    logits[0, 2, :, :3] = 1.0
    logits[0, 3, :, :3] = 1.0                                          # classes 2 and 3 tie where they win: class 2 it is
    for p in (False, True):
        got = restore.restore_labels(logits.cuda()[0], (5, 6, 7), label_values=None, probabilities=p)
        assert torch.equal(got.cpu().long(), logits[0].argmax(0)) and set(got.unique().tolist()) == {0, 2}
    up = restore.restore_labels(torch.zeros(3, 4, 4, 4).cuda(), (9, 10, 11), label_values=(5, 6))
    assert int(up.abs().sum()) == 0


def test_round_trip_of_a_loaded_class_map():
    """loader.load_pair's class map -> one-hot logits -> restore at the same grid gives the class map back, both interpolands."""
    from micformer_amd import loader, restore
    g = np.random.default_rng(3)
    shape, size = (41, 50, 37), (32, 32, 32)
    ct = torch.from_numpy(g.integers(-1000, 3000, size=shape, dtype=np.int16)).cuda()
    mr = torch.from_numpy(g.random(shape, dtype=np.float32)).cuda()
    values = np.array((0,) + R.MMWHS_LABEL_VALUES, np.int16)
    lab = torch.from_numpy(values[g.integers(0, 8, size=shape)]).cuda()
    _, cmap, _ = loader.load_pair(ct, mr, lab, size=size)
    assert int(cmap.max()) == 7 and len(cmap.unique()) == 8
    onehot = torch.nn.functional.one_hot(cmap.long(), 8).permute(3, 0, 1, 2).float().contiguous()
    for p in (False, True):
        assert torch.equal(restore.restore_labels(onehot, size, label_values=None, probabilities=p), cmap)
        back = restore.restore_labels(onehot, size, probabilities=p)
        assert torch.equal(back.long(), R.label_table(R.MMWHS_LABEL_VALUES, 8, "cuda")[cmap.long()])


def test_two_calls_are_bit_identical_and_out_is_written_in_place():
    from micformer_amd import restore
    logits = R.make_logits(SRC32, 8, batch=2).cuda()
    shapes = [(45, 64, 50), (70, 31, 129)]
    for p in (False, True):
        first = restore.restore_batch(logits, shapes, probabilities=p)
        out = [torch.full(s, -7, dtype=torch.int16, device="cuda") for s in shapes]
        res = restore.restore_batch(logits, shapes, probabilities=p, out=out)
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert all(torch.equal(a, b) for a, b in zip(first, out))
    with pytest.raises(ValueError, match="contiguous"):
        restore.restore_batch(logits.transpose(3, 4), shapes)          # a CUDA tensor, but not contiguous
    with pytest.raises(ValueError):
        restore.restore_batch(logits, shapes, out=[out[0], out[1].int()])
    with pytest.raises(ValueError):
        restore.restore_batch(logits, shapes, out=[out[0]])
    with pytest.raises(ValueError):
        restore.restore_batch(logits, shapes, out=[out[1], out[0]])
    with pytest.raises(ValueError):
        restore.restore_batch(logits, shapes, label_values=None, out=out)      # a class map is uint8


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
def test_capture_and_replay_under_a_graph(probabilities):
    from micformer_amd import restore
    shapes = [(45, 64, 50), (23, 40, 31)]
    logits = R.make_logits(SRC32, 8, batch=2).cuda()
    eager = restore.restore_batch(logits, shapes, probabilities=probabilities)
    out = [torch.zeros_like(t) for t in eager]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            restore.restore_batch(logits, shapes, probabilities=probabilities, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    # fresh logits in the same buffer: the replay reads them
    logits.copy_(R.make_logits(SRC32, 8, batch=2, seed=1))
    graph.replay()
    torch.cuda.synchronize()
    fresh = restore.restore_batch(logits, shapes, probabilities=probabilities)
    assert all(torch.equal(a, b) for a, b in zip(out, fresh))
    assert not any(torch.equal(a, b) for a, b in zip(out, eager))


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
def test_full_size_against_the_aten_composition(probabilities):
    """8 x 128^3 -> 363 x 512 x 512 against F.interpolate + argmax + lookup on the GPU, under the same rule; the near-tie share is
    taken from the ATen result's margin.  Noise term of the recipe: 0.3, as in the small cases."""
    from micformer_amd import restore
    shape = (363, 512, 512)
    logits = R.make_logits((128, 128, 128), 8).cuda()
    up = R.upsample(logits[0], shape, probabilities)                   # the 3 GB tensor the fused call never writes
    share = R.near_tie_share(R.margin_of(up), probabilities)
    print(f"full size probabilities={probabilities}: ATen near-tie share {share:.2e}")
    assert share <= R.MAX_NEAR_TIE_SHARE, share
    got = restore.restore_labels(logits[0], shape, probabilities=probabilities)
    assert got.shape == shape and got.dtype == torch.int16
    res = R.judge(got, up, R.MMWHS_LABEL_VALUES, probabilities)
    print(f"full size probabilities={probabilities}: {res}")
    assert res["ok"], res


@pytest.mark.parametrize("probabilities", [False, True], ids=["logits", "probs"])
def test_segment_pair_end_to_end(probabilities):
    from micformer_amd import data, loader, restore
    g = np.random.default_rng(41)
    shape, size = (41, 50, 37), (32, 32, 32)
    ct = torch.from_numpy(g.integers(-1000, 3000, size=shape, dtype=np.int16)).cuda()
    mr = torch.from_numpy(g.integers(0, 1500, size=shape, dtype=np.int16)).cuda()
    model = tiny_head()
    # the model's own logits, copied to the host for the referee
    image, _, _ = loader.load_pair(ct, mr, None, size=size)
    x, _ = data.prepare_raw_batch(image.unsqueeze(0), None, None)
    with torch.no_grad():
        logits = model(x)
    assert logits.shape == (1, 8) + size and logits.dtype == torch.float32
    print(f"end to end: max |logit| {float(logits.abs().max()):.2f}")
    up = _referee_condition(logits[0].cpu(), shape, probabilities, "end to end")
    got = restore.segment_pair(model, ct, mr, size=size, probabilities=probabilities)
    assert got.shape == shape and got.dtype == torch.int16 and got.is_cuda
    assert set(got.unique().tolist()) <= {0} | set(R.MMWHS_LABEL_VALUES)
    assert len(got.unique()) >= 4
    _judge(got, up, R.MMWHS_LABEL_VALUES, probabilities, "end to end")
