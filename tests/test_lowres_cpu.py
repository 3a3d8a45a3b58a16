"""CPU checks of the low-resolution simulation: the float64 referee (tests/lowres_ref.py) against scipy.ndimage.zoom (the nearest
gather off the ties, the full 3-D result to 1e-12), the fp32 gate that fixes the GPU tests' tolerance E and the mutations it must
catch, draw_low_resolution, include/micformer_lowres.h against the ctypes table of micformer_amd/lowres.py and the built library,
argument errors caught before any launch, and the host program tests/lowres_index_main.cpp (csrc/lowres_coords.h under the address
and undefined-behaviour sanitizers: a stand-alone program, nothing is preloaded).

The fp32 gate, measured here on the cases of the GPU tests (3 shapes x 2 inputs x 2 target sets of 6 channels): the float32 referee
differs from the float64 referee by at most 5.92e-7 of the input channel's max - min; lowres_ref.MEASURED_FP32 = 6.0e-7 and
E = 4 x that = 2.4e-6.  The smallest error a mutation makes is 0.13 of the range (reflect instead of edge), 55 000 x E."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_header
import lowres_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_lowres.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "elastic", "intensity", "restore", "postprocess", "surface")
NAMES = {"micf_lowres_workspace", "micf_lowres_simulate"}


# ---- the referee ------------------------------------------------------------------------------------------------------------

def test_nearest_rule_is_scipy_off_the_ties():
    """The integer rule equals scipy's order-0 zoom (grid_mode, mode="nearest") at every position that is not an exact tie, for
    every n in 2..199 and t in n // 2 - 1 .. n, and is within one index of it at the ties."""
    ndimage = pytest.importorskip("scipy.ndimage")
    pairs = positions = ties = tie_misses = 0
    for n in range(2, 200):
        ramp = np.arange(n, dtype=np.float64)
        for t in range(max(n // 2 - 1, 1), n + 1):
            got = R.gather_index(n, t)
            want = ndimage.zoom(ramp, t / n, order=0, mode="nearest", grid_mode=True)
            assert want.shape == (t,), (n, t)
            want = want.astype(np.int64)
            tie = R.is_tie(n, t)
            assert np.array_equal(got[~tie], want[~tie]), (n, t)
            assert (np.abs(got - want) <= 1).all(), (n, t)
            assert (got >= 0).all() and (got < n).all() and (np.diff(got) >= 0).all()
            pairs += 1
            positions += t
            ties += int(tie.sum())
            tie_misses += int((got != want).sum())
    print(f"{pairs} (n, t) pairs, {positions} positions, {ties} ties, scipy differs at {tie_misses} of them")
    assert ties > 0


@pytest.mark.parametrize("case", R.cases(), ids=str)
def test_referee_is_scipy_zoom(case):
    """The float64 referee is within 1e-12 of ndi.zoom(low, n / t, order=3, mode="nearest", grid_mode=True) on every channel of
    every case, `low` being the referee's own gather."""
    ndimage = pytest.importorskip("scipy.ndimage")
    shape = case[0]
    x, t, out = R.reference(*case)
    off = R.is_off(shape, t)
    worst = 0.0
    for b in range(R.B):
        for c in range(R.C):
            if off[b, c]:
                assert np.array_equal(out[b, c], x[b, c].astype(np.float64))
                continue
            low = R.downsample(x[b, c], t[b, c]).astype(np.float64)
            want = ndimage.zoom(low, [shape[a] / low.shape[a] for a in range(3)], order=3, mode="nearest", grid_mode=True)
            assert want.shape == tuple(shape)
            worst = max(worst, float(np.abs(out[b, c] - want).max()))
    print(f"{case}: max |referee - scipy zoom| {worst:.2e}")
    assert worst <= 1e-12


def test_cases_cover_what_they_claim():
    seen = set()
    for shape in R.SHAPES:
        for name in R.NAMES:
            t = R.targets(shape, name).reshape(-1, 3)
            assert ((t >= 1) & (t <= np.array(shape))).all()
            for row in t:
                same = [int(row[a]) == shape[a] for a in range(3)]
                seen.add("off" if all(same) else f"keep{sum(same)}")
                for a in range(3):
                    n, v = shape[a], int(row[a])
                    seen.update(k for k, hit in (("one", v == 1 and n > 1), ("minus1", v == n - 1), ("half", 2 * v == n),
                                                 ("odd", v < n and n % v != 0 and v != n - 1)) if hit)
    assert seen >= {"off", "keep1", "keep2", "keep0", "one", "minus1", "half", "odd"}, seen
    assert R.is_tie(64, 32).all() and R.is_tie(70, 35).all()       # exact halves: every position is a tie


def test_an_axis_at_full_size_is_not_an_identity():
    """t == n on one axis still prefilters and interpolates it (weights 1/6, 4/6, 1/6, 0): samples come back up to rounding only,
    and only the all-axes case is the input itself."""
    fl, f = R.taps(9, 9)
    assert np.array_equal(fl, np.arange(9)) and not f.any()
    assert np.allclose([w[0] for w in R.bspline_weights(f)], [1 / 6, 4 / 6, 1 / 6, 0])
    x = R.volume((5, 9, 70), "zscore")[0, 0]
    same = R.channel(x, (5, 9, 70))
    assert np.array_equal(same, x.astype(np.float64))
    low = R.downsample(x, (5, 9, 35))
    back = R.upsample(low, low.shape)                                 # every axis at full size, through the arithmetic
    assert np.abs(back - low).max() < 1e-14


# ---- the fp32 gate ------------------------------------------------------------------------------------------------------------

def _relative_error(got, want, x):
    return float((np.abs(got.astype(np.float64) - want) / R.span(x)).max())


def test_fp32_gate():
    """The referee in float32 against the referee in float64 on every case of the GPU tests: the worst |diff| / (input channel's
    max - min) is what MEASURED_FP32 records (not exceeded, and not overstated by more than a quarter); E is 4 x MEASURED_FP32."""
    worst, where = 0.0, None
    for case in R.cases():
        x, t, out = R.reference(*case)
        e = _relative_error(R.simulate(x, t, np.float32), out, x)
        if e > worst:
            worst, where = e, case
    print(f"fp32 referee vs fp64 referee: worst |diff| / range {worst:.3e} at {where}; MEASURED_FP32 {R.MEASURED_FP32:.3e}, E {R.E:.3e}")
    assert 0.75 * R.MEASURED_FP32 <= worst <= R.MEASURED_FP32
    assert R.E == 4.0 * R.MEASURED_FP32


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_breaks_the_gate(mutation):
    """Each slip applied to the float64 referee moves some voxel of the cases (the two smaller shapes) by at least 10 E x range."""
    worst = 0.0
    for case in R.cases():
        if case[0] == R.SHAPES[-1]:
            continue
        x, t, out = R.reference(*case)
        worst = max(worst, _relative_error(R.simulate(x, t, np.float64, mutation), out, x))
    print(f"{mutation}: worst |diff| / range {worst:.3e} = {worst / R.E:.0f} E")
    assert worst >= 10 * R.E


# ---- draw_low_resolution --------------------------------------------------------------------------------------------------------

def test_draw_low_resolution():
    from micformer_amd.lowres import draw_low_resolution
    n, size = 20000, (128, 96, 50)
    t = draw_low_resolution(n, size, generator=torch.Generator().manual_seed(5))
    t2 = draw_low_resolution(n, size, generator=torch.Generator().manual_seed(5))
    t3 = draw_low_resolution(n, size, generator=torch.Generator().manual_seed(6))
    assert t.dtype == torch.int32 and tuple(t.shape) == (n, 2, 3) and t.is_contiguous() and t.device.type == "cpu"
    assert torch.equal(t, t2) and not torch.equal(t, t3)
    t = t.numpy()
    full = np.array(size)
    on = (t != full).any(axis=2)

    def rate(mask, want):                                             # within 5 standard deviations of a binomial
        got = float(mask.mean())
        assert abs(got - want) <= 5 * np.sqrt(want * (1 - want) / mask.size), (got, want)

    assert ((t >= 1) & (t <= full)).all()
    rate(on.any(axis=1), 0.25 * 0.75)                                 # per sample 0.25, then per channel 0.5
    rate(on, 0.125)
    assert (t[on] >= np.round(full * 0.5)).all() and t[on][:, 0].min() <= 66 and t[on][:, 0].max() >= 126
    zoom = t[on] / full                                               # one zoom per channel: the three axes agree within rounding
    assert (np.abs(zoom - zoom[:, :1]) <= 0.5 / full.min() + 0.5 / full[0]).all()
    both = on.all(axis=1)
    assert both.any() and (t[both, 0, 0] != t[both, 1, 0]).mean() > 0.9   # ... and a zoom of its own per channel
    # keywords
    off = draw_low_resolution(64, size, channels=3, p_per_sample=0)
    assert tuple(off.shape) == (64, 3, 3) and (off.numpy() == full).all()
    assert (draw_low_resolution(64, size, p_per_sample=1, p_per_channel=0).numpy() == full).all()
    every = draw_low_resolution(64, size, p_per_sample=1, p_per_channel=1, zoom_range=(0.5, 0.9)).numpy()
    assert (every < full).all()
    kept = draw_low_resolution(64, size, p_per_sample=1, p_per_channel=1, zoom_range=(0.5, 0.9), ignore_axes=(0,)).numpy()
    assert (kept[:, :, 0] == 128).all() and (kept[:, :, 1:] < full[1:]).all()
    kept = draw_low_resolution(64, size, p_per_sample=1, p_per_channel=1, zoom_range=(0.5, 0.9), ignore_axes=[2, 1]).numpy()
    assert (kept[:, :, 1:] == full[1:]).all() and (kept[:, :, 0] < 128).all()
    # np.round at a half: to even, 2.5 -> 2 and 3.5 -> 4; clamped to at least 1
    half = draw_low_resolution(8, (5, 7, 1), p_per_sample=1, p_per_channel=1, zoom_range=(0.5, 0.5)).numpy()
    assert (half == np.array([2, 4, 1])).all()
    tiny = draw_low_resolution(8, (2, 3, 1), p_per_sample=1, p_per_channel=1, zoom_range=(0.1, 0.1)).numpy()
    assert (tiny == 1).all()
    assert draw_low_resolution(2, [8, 8, 8], device=torch.device("cpu")).shape == (2, 2, 3)
    doc = draw_low_resolution.__doc__
    assert "unpinned" in doc and "batchgenerators" in doc
    for bad in (dict(batch=0), dict(batch=2, channels=5), dict(batch=2, channels=0), dict(batch=2, p_per_sample=1.5),
                dict(batch=2, p_per_channel=-0.1), dict(batch=2, zoom_range=(1.0, 0.5)), dict(batch=2, zoom_range=(0.0, 1.0)),
                dict(batch=2, ignore_axes=(3,)), dict(batch=2, ignore_axes=(-1,)), dict(batch=2, size=(8, 8)),
                dict(batch=2, size=(0, 8, 8)), dict(batch=2, size=(8, 8, 4096))):
        with pytest.raises(ValueError):
            draw_low_resolution(**{"size": size, **bad})
    for bad in (dict(batch=2.0), dict(batch=True), dict(batch=2, channels=2.0), dict(batch=2, p_per_sample="often"),
                dict(batch=2, zoom_range=0.5), dict(batch=2, zoom_range=("a", "b")), dict(batch=2, ignore_axes=1),
                dict(batch=2, ignore_axes=(0.0,))):
        with pytest.raises(TypeError):
            draw_low_resolution(**{"size": size, **bad})
    with pytest.raises(TypeError):                                    # TypeError before ValueError
        draw_low_resolution(0, size, channels=2.0)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, lowres
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(lowres.SIGNATURES) == NAMES
    assert lowres.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert lowres.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {lowres.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in lowres.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert abi_header.defines(HEADER, "MICF_LOWRES_") == {
        "MICF_LOWRES_F32": lowres.F32, "MICF_LOWRES_F16": lowres.F16, "MICF_LOWRES_MAX_CHANNELS": lowres.MAX_CHANNELS,
        "MICF_LOWRES_MAX_EXTENT": 2048, "MICF_LOWRES_MAX_VOLUMES": lowres.MAX_VOLUMES}
    assert lowres.DTYPES == {torch.float32: 0, torch.float16: 1}
    build = abi_header.build_module()
    assert "volume_lowres.hip" in build.SOURCES


def test_table_is_disjoint_from_the_others():
    from micformer_amd import lowres
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(lowres.SIGNATURES) & set(other), module


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.lowres import lib
    q = lib.micf_lowres_workspace
    a = q(1, 2, 128, 128, 128)
    assert a == q(1, 2, 128, 128, 128) and a % 256 == 0
    assert 2 * 132 ** 3 * 4 <= a < 2 * 132 ** 3 * 4 + 256            # the worst case t = n: two entries beyond either end
    assert q(8, 2, 128, 128, 128) >= 8 * 2 * 132 ** 3 * 4 and q(3, 2, 5, 9, 70) >= 6 * 9 * 13 * 74 * 4
    for bad in [(0, 2, 8, 8, 8), (1, 0, 8, 8, 8), (1, 2, 0, 8, 8), (1, 2, 8, -1, 8), (1, 2, 8, 8, 0), (-1, 5, 8, 8, 8)]:
        assert q(*bad) == -1, bad
    for unsupported in [(1, 5, 8, 8, 8), (1, 2, 2049, 8, 8), (1, 2, 8, 2049, 8), (1, 2, 8, 8, 2049), (16384, 4, 8, 8, 8)]:
        assert q(*unsupported) == -2, unsupported
    assert q(1, 4, 2048, 2048, 2048) >= 4 * 2052 ** 3 * 4 > 1 << 32    # no 32-bit overflow


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd.lowres import lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    ws = lib.micf_lowres_workspace(1, 2, 8, 8, 8)

    def call(src=fake, dst=fake, dtype=0, shape=(1, 2, 8, 8, 8), target=fake, workspace=fake, ws_bytes=ws):
        return lib.micf_lowres_simulate(src, dst, dtype, *shape, target, workspace, ws_bytes, None)

    for kw in ("src", "dst", "target", "workspace"):
        assert call(**{kw: None}) == EINVAL, kw
    assert call(src=fake + 2) == EINVAL and call(dst=fake + 1) == EINVAL          # float32 alignment
    assert call(src=fake + 1, dtype=1) == EINVAL and call(dst=fake + 3, dtype=1) == EINVAL
    assert call(target=fake + 2) == EINVAL
    assert call(workspace=fake + 64) == EINVAL and call(ws_bytes=ws - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    for dtype in (-1, 2, 7):
        assert call(dtype=dtype) == EINVAL
    for shape in [(0, 2, 8, 8, 8), (1, 0, 8, 8, 8), (1, 2, 0, 8, 8), (1, 2, 8, -4, 8), (1, 2, 8, 8, 0), (1, 9, 0, 8, 8)]:
        assert call(shape=shape) == EINVAL, shape                     # (EINVAL before EUNSUPPORTED)
    big = 1 << 62
    for shape in [(1, 5, 8, 8, 8), (1, 2, 2049, 8, 8), (1, 2, 8, 4096, 8), (1, 2, 8, 8, 2049), (65536, 1, 8, 8, 8)]:
        assert call(shape=shape, ws_bytes=big) == EUNSUP, shape
    assert call(shape=(1, 5, 8, 8, 8), src=None) == EINVAL


def test_python_front_end_rejects_before_the_device():
    """Every argument error raised with CPU tensors in hand; a correct call with CPU tensors fails last, on the device check."""
    from micformer_amd.lowres import augment_moreda, simulate_low_resolution
    x = torch.zeros(1, 2, 4, 5, 6)
    t = torch.ones(1, 2, 3, dtype=torch.int32)
    p = torch.zeros(1, 2, 8)
    s = torch.zeros(1, dtype=torch.int64)
    for bad in [np.zeros((1, 2, 4, 5, 6), np.float32), None, 1.0, x.double(), x.to(torch.bfloat16), x.to(torch.int16)]:
        with pytest.raises(TypeError, match="image"):
            simulate_low_resolution(bad, t)
        with pytest.raises(TypeError, match="image"):                 # TypeError before ValueError
            simulate_low_resolution(bad, torch.ones(7, dtype=torch.int32))
    for bad in [None, [4, 5, 6], t.long(), t.float(), t.to(torch.int16)]:
        with pytest.raises(TypeError, match="target"):
            simulate_low_resolution(x, bad)
        with pytest.raises(TypeError, match="target"):
            simulate_low_resolution(torch.zeros(3), bad)
        with pytest.raises(TypeError, match="target"):
            augment_moreda(x, p, s, bad)
    for bad in [np.zeros(3), 0, "image"]:
        with pytest.raises(TypeError, match="out"):
            simulate_low_resolution(x, t, out=bad)
    for bad in [torch.zeros(2, 4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(1, 1, 2, 4, 5, 6)]:
        with pytest.raises(ValueError, match="image must have shape"):
            simulate_low_resolution(bad, t)
    for bad in [torch.zeros(1, 5, 4, 5, 6), torch.zeros(0, 2, 4, 5, 6), torch.zeros(1, 0, 4, 5, 6)]:
        with pytest.raises(ValueError, match="channels"):
            simulate_low_resolution(bad, t)
    with pytest.raises(ValueError, match="extents"):
        simulate_low_resolution(torch.zeros(1, 2, 0, 5, 6), t)
    with pytest.raises(ValueError, match="extents"):
        simulate_low_resolution(torch.zeros(1, 1, 1, 1, 2049), torch.ones(1, 1, 3, dtype=torch.int32))
    for bad in [torch.ones(1, 2, 2, dtype=torch.int32), torch.ones(2, 2, 3, dtype=torch.int32), torch.ones(1, 1, 3, dtype=torch.int32),
                torch.ones(6, dtype=torch.int32)]:
        with pytest.raises(ValueError, match="target must have shape"):
            simulate_low_resolution(x, bad)
    with pytest.raises(ValueError, match="image must be a CUDA"):     # a correct call: the device check is the last one standing
        simulate_low_resolution(x, t)
    with pytest.raises(ValueError, match="image must be a CUDA"):
        simulate_low_resolution(x.half(), t, out=x.half())
    # augment_moreda: the TypeErrors of all its arguments before any ValueError, the ValueErrors before the device
    with pytest.raises(TypeError, match="params"):
        augment_moreda(torch.zeros(3), p.double(), s, t)
    with pytest.raises(TypeError, match="seeds"):
        augment_moreda(torch.zeros(3), p, s.int(), t)
    with pytest.raises(ValueError, match="params must have shape"):
        augment_moreda(x, torch.zeros(1, 2, 7), s, t)
    with pytest.raises(ValueError, match="seeds must have shape"):
        augment_moreda(x, p, torch.zeros(2, dtype=torch.int64), t)
    with pytest.raises(ValueError, match="image must be a CUDA"):
        augment_moreda(x, p, s, t)


def test_placement_checks_use_metadata_only():
    from micformer_amd import lowres

    class Fake:                                                       # the metadata of a device tensor
        is_cuda, device = True, torch.device("cuda", 0)

        @staticmethod
        def is_contiguous():
            return False
    with pytest.raises(ValueError, match="contiguous"):
        lowres._placed(Fake, "target", torch.device("cuda", 0))
    with pytest.raises(ValueError, match="target must be on"):
        lowres._placed(Fake, "target", torch.device("cuda", 1))
    Fake.is_contiguous = staticmethod(lambda: True)
    lowres._placed(Fake, "target", torch.device("cuda", 0))


# ---- the host program -----------------------------------------------------------------------------------------------------------

def test_index_weight_and_prefilter_functions_on_the_host(tmp_path):
    """tests/lowres_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lowres_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "lowres_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:], r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "every index in range" in r.stdout
