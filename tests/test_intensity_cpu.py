"""CPU checks of the intensity augmentation: the float64 referee (tests/intensity_ref.py) against scipy.ndimage.gaussian_filter,
the fp32 gate that fixes the GPU tests' tolerance E and the mutations it must catch, include/micformer_intensity.h against the
ctypes table of micformer_amd/intensity.py and the built library, argument errors caught before any launch, draw_intensity, and the
host program tests/intensity_index_main.cpp (csrc/intensity_coords.h under the address and undefined-behaviour sanitizers: a
stand-alone program, nothing is preloaded).

The fp32 gate, measured here on the cases of the GPU tests (3 shapes x 2 inputs x 12 parameter rows): the float32 referee differs
from the float64 referee by at most 4.25e-7 of the channel's max - min (the worst case is the row with every step together, 64^3,
min-max-like input); intensity_ref.MEASURED_FP32 = 4.3e-7 and E = 4 x that = 1.72e-6.  The smallest error a mutation makes is
1.06e-4 (ddof 1), 60 x E."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_header
import intensity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "micformer_intensity.h"
OTHER_TABLES = ("_lib", "metrics", "loader", "normalise", "affine", "elastic", "restore", "postprocess", "surface")
NAMES = {"micf_intensity_augment_workspace", "micf_intensity_augment"}


# ---- the referee ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 9, 70), (3, 2, 1), (1, 1, 40), (20, 17, 19)], ids=str)
@pytest.mark.parametrize("sigma", [0.1, 0.13, 0.5, 0.8, 1.0, 1.37, 2.0])
def test_explicit_blur_is_gaussian_filter(sigma, shape):
    """Explicit reflect + weights equals scipy's filter to 1e-12, on axes shorter than the radius too (5, 3, 2 and 1 against 8)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    x = np.random.default_rng(9001).standard_normal(shape)
    want = ndimage.gaussian_filter(x, sigma, order=0, mode="reflect", truncate=4.0)
    err = float(np.abs(R.blur(x, sigma) - want).max())
    print(f"sigma {sigma} shape {shape}: radius {R.weights(sigma)[0]}, max |explicit - gaussian_filter| {err:.2e}")
    assert err <= 1e-12
    assert R.weights(sigma)[0] == int(4 * sigma + 0.5) <= 8 and abs(R.weights(sigma)[1].sum() - 1) < 1e-15


def test_reflect_is_numpy_symmetric_padding():
    for n in range(1, 12):
        data = np.arange(n)
        assert np.array_equal(data[R.reflect(np.arange(-30, n + 30), n)], np.pad(data, 30, mode="symmetric"))


def test_noise_is_standard_normal_and_keyed():
    h = R.words(R.SEEDS[0], 1, 1 << 18)
    z = R.normal(h)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01 and np.isfinite(z).all() and np.abs(z).max() < 6
    assert not np.array_equal(h, R.words(R.SEEDS[0], 0, 1 << 18)) and not np.array_equal(h, R.words(R.SEEDS[1], 1, 1 << 18))
    assert np.array_equal(h[:100], R.words(R.SEEDS[0], 1, 100))                   # the key depends on the voxel alone
    z32 = R.normal(h, np.float32)
    # float32: the angle 2 pi u2 carries up to 6e-7 (the constant 1.8e-7, the product's rounding 2.4e-7, u2's 1.9e-7), times a
    # radius of at most 5.9, plus a few roundings of z itself
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 5e-6
    u1, u2 = R.uniforms(h)
    assert 0 < u1.min() and u1.max() < 1 and 0 < u2.min() and u2.max() < 1


def test_neutral_rows_return_the_input():
    x, p, s, out, stats = R.reference((5, 9, 70), "zscore", "gamma")
    assert np.array_equal(out[2, 1], x[2, 1].astype(np.float64))
    assert np.array_equal(stats[2, 1, 3:], np.zeros(5))


# ---- the fp32 gate ------------------------------------------------------------------------------------------------------------

def _relative_error(got, want):
    return float((np.abs(got.astype(np.float64) - want) / R.span(want)).max())


def test_fp32_gate():
    """The referee in float32 against the referee in float64 on every case of the GPU tests: the worst |diff| / (channel max -
    min) is what MEASURED_FP32 records (not exceeded, and not overstated by more than a quarter); E is 4 x MEASURED_FP32."""
    worst, where = 0.0, None
    for shape, kind, name in R.cases():
        x, p, s, out, _ = R.reference(shape, kind, name)
        e = _relative_error(R.augment(x, p, s, np.float32)[0], out)
        if e > worst:
            worst, where = e, (shape, kind, name)
    print(f"fp32 referee vs fp64 referee: worst |diff| / range {worst:.3e} at {where}; MEASURED_FP32 {R.MEASURED_FP32:.3e}, E {R.E:.3e}")
    assert 0.75 * R.MEASURED_FP32 <= worst <= R.MEASURED_FP32
    assert R.E == 4.0 * R.MEASURED_FP32


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_breaks_the_gate(mutation):
    """Each slip applied to the float64 referee moves some voxel of the cases (the two smaller shapes) by more than E x range."""
    worst = 0.0
    for shape, kind, name in R.cases():
        if shape == R.SHAPES[-1]:
            continue
        x, p, s, out, _ = R.reference(shape, kind, name)
        worst = max(worst, _relative_error(R.augment(x, p, s, np.float64, mutation)[0], out))
    print(f"{mutation}: worst |diff| / range {worst:.3e} = {worst / R.E:.0f} E")
    assert worst > R.E


def test_ddof_in_both_deviations_cancels():
    """Why the ddof mutation is applied to s0 alone: with ddof 1 in s0 AND in the deviation after the power law the factor
    sqrt(N / (N - 1)) cancels in the output."""
    x = R.volume((5, 9, 70), "zscore")[0, 0].astype(np.float64)
    lo, rng = x.min(), x.max() - x.min()
    y = np.power((x - lo) / (rng + 1e-7), 0.7) * rng + lo
    a = (y - y.mean()) / y.std() * x.std() + x.mean()
    b = (y - y.mean()) / y.std(ddof=1) * x.std(ddof=1) + x.mean()
    assert np.abs(a - b).max() / rng < 1e-12


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------

def test_header_table_binding_and_library_agree():
    from micformer_amd import _lib, intensity
    d = abi_header.parse_header(HEADER)
    assert set(d) == set(intensity.SIGNATURES) == NAMES
    assert intensity.lib is _lib.lib
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, sig) in d.items():
        assert intensity.SIGNATURES[name] == sig, f"{name}: header {sig} vs ctypes {intensity.SIGNATURES[name]}"
        assert ret in ("int", "int64_t") and (name in intensity.INT64_RETURNS) == (ret == "int64_t"), name
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == [abi_header.CTYPES[c] for c in sig], name
        assert fn.restype is abi_header.RETURNS[ret], name
        assert hasattr(exported, name), f"{name} declared but not exported"
    assert abi_header.defines(HEADER, "MICF_INTENSITY_") == {
        "MICF_INTENSITY_F32": intensity.F32, "MICF_INTENSITY_F16": intensity.F16, "MICF_INTENSITY_MAX_CHANNELS": intensity.MAX_CHANNELS,
        "MICF_INTENSITY_MAX_EXTENT": 2048, "MICF_INTENSITY_MAX_VOLUMES": intensity.MAX_VOLUMES}
    assert intensity.DTYPES == {torch.float32: 0, torch.float16: 1}
    build = abi_header.build_module()
    assert "volume_intensity.hip" in build.SOURCES
    assert len(intensity.SLOTS) == len(intensity.NEUTRAL) == len(intensity.STATS) == R.SLOTS


def test_table_is_disjoint_from_the_others():
    from micformer_amd import intensity
    for module in OTHER_TABLES:
        other = importlib.import_module(f"micformer_amd.{module}").SIGNATURES
        assert not set(intensity.SIGNATURES) & set(other), module


def test_workspace_query_is_pure_and_validates():
    from micformer_amd.intensity import lib
    q = lib.micf_intensity_augment_workspace
    a = q(1, 2, 128, 128, 128)
    assert a == q(1, 2, 128, 128, 128) and a % 256 == 0
    field = 2 * 128 ** 3 * 4
    assert field < a < field + (1 << 20)                            # the float32 copy plus the partials and the records
    assert q(8, 2, 128, 128, 128) > 8 * field and q(3, 2, 5, 9, 70) >= 6 * 5 * 9 * 70 * 4
    for bad in [(0, 2, 8, 8, 8), (1, 0, 8, 8, 8), (1, 2, 0, 8, 8), (1, 2, 8, -1, 8), (1, 2, 8, 8, 0), (-1, 5, 8, 8, 8)]:
        assert q(*bad) == -1, bad
    for unsupported in [(1, 5, 8, 8, 8), (1, 2, 2049, 8, 8), (1, 2, 8, 2049, 8), (1, 2, 8, 8, 2049), (16384, 4, 8, 8, 8)]:
        assert q(*unsupported) == -2, unsupported
    assert q(1, 4, 2048, 2048, 2048) > 4 * 2048 ** 3 * 4               # no 32-bit overflow


def test_bad_arguments_return_codes_before_any_launch():
    from micformer_amd.intensity import lib
    EINVAL, EUNSUP = -1, -2
    fake = 1 << 20                          # never dereferenced: every call below fails validation first
    ws = lib.micf_intensity_augment_workspace(1, 2, 8, 8, 8)

    def call(src=fake, dst=fake, dtype=0, shape=(1, 2, 8, 8, 8), params=fake, seeds=fake, workspace=fake, ws_bytes=ws, stats=None):
        return lib.micf_intensity_augment(src, dst, dtype, *shape, params, seeds, workspace, ws_bytes, stats, None)

    for kw in ("src", "dst", "params", "seeds", "workspace"):
        assert call(**{kw: None}) == EINVAL, kw
    assert call(src=fake + 2) == EINVAL and call(dst=fake + 1) == EINVAL          # float32 alignment
    assert call(src=fake + 1, dtype=1) == EINVAL and call(dst=fake + 3, dtype=1) == EINVAL
    assert call(params=fake + 2) == EINVAL and call(seeds=fake + 4) == EINVAL and call(stats=fake + 4) == EINVAL
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
    from micformer_amd.intensity import augment_intensity
    x = torch.zeros(1, 2, 4, 5, 6)
    p = torch.zeros(1, 2, 8)
    s = torch.zeros(1, dtype=torch.int64)
    for bad in [np.zeros((1, 2, 4, 5, 6), np.float32), None, 1.0, x.double(), x.to(torch.bfloat16), x.to(torch.int16)]:
        with pytest.raises(TypeError, match="image"):
            augment_intensity(bad, p, s)
        with pytest.raises(TypeError, match="image"):                 # TypeError before ValueError
            augment_intensity(bad, torch.zeros(3), torch.zeros(7, dtype=torch.int64))
    for bad in [None, [0.0] * 8, p.double(), p.half(), p.to(torch.int32)]:
        with pytest.raises(TypeError, match="params"):
            augment_intensity(x, bad, s)
        with pytest.raises(TypeError, match="params"):
            augment_intensity(torch.zeros(3), bad, s)
    for bad in [None, [1], 3, s.to(torch.int32), s.float(), s.to(torch.uint8)]:
        with pytest.raises(TypeError, match="seeds"):
            augment_intensity(x, p, bad)
        with pytest.raises(TypeError, match="seeds"):
            augment_intensity(x, torch.zeros(1, 3, 8), bad)
    for bad in [np.zeros(3), 0, "image"]:
        with pytest.raises(TypeError, match="out"):
            augment_intensity(x, p, s, out=bad)
    for bad in [torch.zeros(2, 4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(1, 1, 2, 4, 5, 6)]:
        with pytest.raises(ValueError, match="image must have shape"):
            augment_intensity(bad, p, s)
    for bad in [torch.zeros(1, 5, 4, 5, 6), torch.zeros(0, 2, 4, 5, 6), torch.zeros(1, 0, 4, 5, 6)]:
        with pytest.raises(ValueError, match="channels"):
            augment_intensity(bad, p, s)
    with pytest.raises(ValueError, match="extents"):
        augment_intensity(torch.zeros(1, 2, 0, 5, 6), p, s)
    with pytest.raises(ValueError, match="extents"):
        augment_intensity(torch.zeros(1, 1, 1, 1, 2049), torch.zeros(1, 1, 8), s)
    for bad in [torch.zeros(1, 2, 7), torch.zeros(2, 2, 8), torch.zeros(1, 1, 8), torch.zeros(16)]:
        with pytest.raises(ValueError, match="params must have shape"):
            augment_intensity(x, bad, s)
    for bad in [torch.zeros(2, dtype=torch.int64), torch.zeros(1, 1, dtype=torch.int64), torch.zeros((), dtype=torch.int64)]:
        with pytest.raises(ValueError, match="seeds must have shape"):
            augment_intensity(x, p, bad)
    with pytest.raises(ValueError, match="image must be a CUDA"):     # a correct call: the device check is the last one standing
        augment_intensity(x, p, s)
    with pytest.raises(ValueError, match="image must be a CUDA"):
        augment_intensity(x.half(), p, s, out=x.half(), return_stats=True)


def test_placement_checks_use_metadata_only():
    from micformer_amd import intensity

    class Fake:                                                       # the metadata of a device tensor
        is_cuda, device = True, torch.device("cuda", 0)

        @staticmethod
        def is_contiguous():
            return False
    with pytest.raises(ValueError, match="contiguous"):
        intensity._placed(Fake, "params", torch.device("cuda", 0))
    with pytest.raises(ValueError, match="params must be on"):
        intensity._placed(Fake, "params", torch.device("cuda", 1))
    Fake.is_contiguous = staticmethod(lambda: True)
    intensity._placed(Fake, "params", torch.device("cuda", 0))


# ---- draw_intensity -----------------------------------------------------------------------------------------------------------

def test_draw_intensity():
    from micformer_amd.intensity import NEUTRAL, draw_intensity
    n = 20000
    p, s = draw_intensity(n, generator=torch.Generator().manual_seed(5))
    p2, s2 = draw_intensity(n, generator=torch.Generator().manual_seed(5))
    p3, s3 = draw_intensity(n, generator=torch.Generator().manual_seed(6))
    assert p.dtype == torch.float32 and tuple(p.shape) == (n, 2, 8) and p.is_contiguous() and p.device.type == "cpu"
    assert s.dtype == torch.int64 and tuple(s.shape) == (n,) and len(set(s.tolist())) == n
    assert torch.equal(p, p2) and torch.equal(s, s2) and not torch.equal(p, p3) and not torch.equal(s, s3)
    p = p.numpy().astype(np.float64)
    sigma, std, bright, contrast, gamma, mode, retain, reserved = (p[:, :, j] for j in range(8))

    def rate(mask, want):                                             # within 5 standard deviations of a binomial of `n` draws
        got = float(mask.mean())
        assert abs(got - want) <= 5 * np.sqrt(want * (1 - want) / mask.size), (got, want)

    assert not reserved.any()
    # noise: per sample, shared by the channels
    assert np.array_equal(std[:, 0], std[:, 1]) and std.min() >= 0 and std.max() <= 0.1 and std.max() > 0.09
    rate(std[:, 0] > 0, 0.1)
    # blur: per sample 0.2, then per channel 0.5; a sigma per channel
    on = sigma > 0
    assert ((sigma[on] >= 0.5) & (sigma[on] <= 1.0)).all() and (sigma[~on] == 0).all()
    rate(on.any(axis=1), 0.2 * 0.75)
    rate(on, 0.1)
    both = on.all(axis=1)
    assert (sigma[both, 0] != sigma[both, 1]).all()
    # brightness: per sample, a factor per channel
    on = bright != 1
    assert ((bright >= 0.75) & (bright <= 1.25)).all() and np.array_equal(on[:, 0], on[:, 1])
    rate(on[:, 0], 0.15)
    assert (bright[on[:, 0], 0] != bright[on[:, 0], 1]).all()
    # contrast: two-sided, half below 1 and half above
    on = contrast != 1
    assert ((contrast >= 0.75) & (contrast <= 1.25)).all()
    rate(on[:, 0], 0.15)
    rate(contrast[on] < 1, 0.5)
    assert abs(contrast[on & (contrast < 1)].mean() - 0.875) < 0.01 and abs(contrast[on & (contrast > 1)].mean() - 1.125) < 0.01
    # gamma: inverted 0.1, else plain 0.3, retain_stats on, the two-sided draw
    assert set(np.unique(mode)) == {0.0, 1.0, 2.0} and np.array_equal(mode[:, 0], mode[:, 1])
    rate(mode[:, 0] == 2, 0.1)
    rate(mode[:, 0] == 1, 0.9 * 0.3)
    assert np.array_equal(retain, (mode != 0).astype(np.float64))
    assert (gamma[mode == 0] == 1).all() and ((gamma >= 0.7) & (gamma <= 1.5)).all()
    rate(gamma[mode != 0] < 1, 0.5)
    assert abs(gamma[(mode != 0) & (gamma < 1)].mean() - 0.85) < 0.01 and abs(gamma[(mode != 0) & (gamma > 1)].mean() - 1.25) < 0.01
    # a sample with nothing drawn is the neutral row, exactly
    quiet = (std[:, 0] == 0) & (sigma == 0).all(axis=1) & (bright == 1).all(axis=1) & (contrast == 1).all(axis=1) & (mode[:, 0] == 0)
    assert quiet.sum() > n // 4 and np.array_equal(p[quiet], np.broadcast_to(np.array(NEUTRAL), (int(quiet.sum()), 2, 8)))
    # keywords
    off = draw_intensity(64, channels=3, p_noise=0, p_blur=0, p_brightness=0, p_contrast=0, p_gamma=0, p_gamma_inverted=0)[0]
    assert tuple(off.shape) == (64, 3, 8) and np.array_equal(off.numpy(), np.broadcast_to(np.array(NEUTRAL, np.float32), (64, 3, 8)))
    full = draw_intensity(64, p_noise=1, p_blur=1, p_blur_channel=1, p_brightness=1, p_contrast=1, p_gamma=1, p_gamma_inverted=0,
                          sigma=(0.1, 2.0), retain_stats=False)[0].numpy()
    assert (full[:, :, 0] >= 0.1).all() and (full[:, :, 0] <= 2.0).all() and (full[:, :, 1] > 0).all()
    assert (full[:, :, 5] == 1).all() and not full[:, :, 6].any()
    doc = draw_intensity.__doc__
    assert "unpinned" in doc and "batchgenerators" in doc and "ONE" in doc and "replaces its two" in doc
    for bad in (dict(batch=0), dict(batch=2, channels=5), dict(batch=2, channels=0), dict(batch=2, p_noise=1.5), dict(batch=2, sigma=(0.05, 1.0)),
                dict(batch=2, sigma=(0.5, 2.5)), dict(batch=2, sigma=(1.0, 0.5)), dict(batch=2, brightness=(0.0, 1.0)),
                dict(batch=2, contrast=(-1.0, 1.0)), dict(batch=2, gamma=(0.0, 1.5)), dict(batch=2, noise_std=(-0.1, 0.1))):
        with pytest.raises(ValueError):
            draw_intensity(**bad)
    for bad in (dict(batch=2.0), dict(batch=True), dict(batch=2, channels=2.0), dict(batch=2, p_blur="often"), dict(batch=2, sigma=1.0),
                dict(batch=2, gamma=("a", "b"))):
        with pytest.raises(TypeError):
            draw_intensity(**bad)


# ---- the host program -----------------------------------------------------------------------------------------------------------

def test_index_weight_and_hash_functions_on_the_host(tmp_path):
    """tests/intensity_index_main.cpp under the address and undefined-behaviour sanitizers: a host program of its own.  Its 4 096
    hash words and both uniforms (float32 bit patterns) equal the numpy referee's bit for bit; its normal draws are the referee's
    within float32 rounding."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "intensity_index_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fsanitize=float-cast-overflow", os.path.join(ROOT, "tests", "intensity_index_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-300:], r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "every index in range" in r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("word ")]
    assert len(lines) == 4096
    got = np.array([[int(v, 16) for v in ln[1:]] for ln in lines], dtype=np.uint64)
    h = R.words(R.SEEDS[0], 1, 4096)
    assert np.array_equal(got[:, 0], h)
    u1, u2 = R.uniforms(h, np.float32)
    assert u1.dtype == np.float32
    assert np.array_equal(got[:, 1].astype(np.uint32), u1.view(np.uint32)) and np.array_equal(got[:, 2].astype(np.uint32), u2.view(np.uint32))
    z = got[:, 3].astype(np.uint32).view(np.float32)
    assert np.abs(z.astype(np.float64) - R.normal(h)).max() < 5e-6        # (the bound of test_noise_is_standard_normal_and_keyed)
