"""Time micformer_amd.patches on a resident full-resolution scan next to what a user composes today; one JSON line per batch size.

    python tools/bench_patches.py [--batches 1,2,8] [--shape 363,512,512] [--patch 128] [--min-seconds 0.5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_patches.py --profile-only 8      # the crop kernel's own time

The scan is an int16 CT / MR pair with an int16 label (blocks of the MM-WHS values on a background of zeros); a batch holds the same
scan B times, every sample forced onto a foreground voxel (the costly branch) with its own draws.
  index_ms             patches.index_scans of one scan (statistics, class counts, per-segment counts), per scan
  load_batch_ms        the plain loader.load_batch call (min-max statistics + resize to 128^3) on the same scan, same session: the
                       same statistics work as the index, for scale
  sample_ms            patches.sample_patches per call with a preallocated `out` (per chunk of 8: locate + crop)
  aten_ms              an ATen composition of the same rule on the same GPU, per call: (label == v).nonzero() and a host read of
                       the chosen row for the pick, slices, F.pad, the class lookup, normalisation with the stored statistics,
                       .half(); it is handed the class counts, so it skips the search for the present classes
  numpy_ms             the numpy restatement on the host arrays (np.flatnonzero pick, crop, np.pad), per call, one repetition
  crop_bytes           what the crop kernel must move per call: per output voxel two source elements, one label element, 4 bytes
                       of float16 and 1 byte of class
  ratio_aten / ratio_numpy = theirs / ours (above 1: the kernels are faster).

    python tools/bench_patches.py --warp [--batches 1,2,8]                                      # the crop through a map / a field
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_patches.py --warp --profile-only 8

--warp times patches.sample_patches(..., affine=theta) and (..., affine=theta, displacement=field, field_interpolation="cubic") with
affine.draw_affine / elastic.draw_elastic's default draws on the patch grid (a (7, 7, 7) field), per call with a preallocated `out`:
  sample_ms            the plain sample_patches of the same session
  warp_map_ms / warp_map_field_ms      the call through a map / through a map and the field
  aten_map_ms / aten_map_field_ms      the ATen composition on the same GPU (aten_warp below), handed the origins
  ratio_aten_* = theirs / ours; ratio_plain_map = warp_map_ms / sample_ms.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, min_seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, ms = 0, 0.0
    while ms < min_seconds * 1e3:
        n = max(1, calls or 4)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
        calls += n
    return ms / calls


def make_scan(shape, values, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ct = torch.randint(-1000, 2000, shape, generator=g, device="cuda", dtype=torch.int16)
    mr = torch.randint(0, 1500, shape, generator=g, device="cuda", dtype=torch.int16)
    coarse = [-(-s // 8) for s in shape]
    pick = torch.randint(0, 4 * (len(values) + 1), coarse, generator=g, device="cuda")         # three quarters background
    table = torch.tensor([0] + list(values) + [0] * (3 * (len(values) + 1)), device="cuda", dtype=torch.int16)
    lab = table[pick]
    for ax in range(3):
        lab = lab.repeat_interleave(8, dim=ax)
    return ct, mr, lab[:shape[0], :shape[1], :shape[2]].contiguous()


def index_of(u, n):
    return min(int(float(u) * n), n - 1)


def bounds(L, P):
    need = max(P - L, 0)
    return -((need + 1) // 2), L + need // 2 + need % 2 - P


def aten_sample(scan, stats, counts, draws_host, values, patch):
    ct, mr, lab = scan
    images, labels = [], []
    for u in draws_host:
        present = [k for k in range(1, len(values) + 1) if counts[k]]
        c = present[index_of(u[1], len(present))]
        where = (lab == values[c - 1]).nonzero()
        v = where[index_of(u[2], where.shape[0])].tolist()                                  # the host round trip
        sl, pad = [], []
        for ax in range(3):
            lb, ub = bounds(lab.shape[ax], patch[ax])
            o = min(max(v[ax] - patch[ax] // 2, lb), ub)
            lo, hi = max(o, 0), min(o + patch[ax], lab.shape[ax])
            sl.append(slice(lo, hi))
            pad = [lo - o, o + patch[ax] - hi] + pad
        chans = []
        for vol, (mn, mx) in zip((ct, mr), stats):
            chans.append(F.pad((vol[tuple(sl)].float() - mn) / (mx - mn), pad))
        images.append(torch.stack(chans).half())
        raw = lab[tuple(sl)]
        cls = torch.full(raw.shape, 255, dtype=torch.uint8, device=raw.device)
        cls[raw == 0] = 0
        for k, val in enumerate(values):
            cls[raw == val] = k + 1
        labels.append(F.pad(cls, pad))
    return torch.stack(images), torch.stack(labels)


def numpy_sample(host, stats, counts, draws_host, values, patch):
    ct, mr, lab = host
    out = []
    for u in draws_host:
        present = [k for k in range(1, len(values) + 1) if counts[k]]
        c = present[index_of(u[1], len(present))]
        where = np.flatnonzero(lab.ravel() == values[c - 1])
        v = np.unravel_index(where[index_of(u[2], len(where))], lab.shape)
        sl, pad = [], []
        for ax in range(3):
            lb, ub = bounds(lab.shape[ax], patch[ax])
            o = min(max(int(v[ax]) - patch[ax] // 2, lb), ub)
            lo, hi = max(o, 0), min(o + patch[ax], lab.shape[ax])
            sl.append(slice(lo, hi))
            pad.append((lo - o, o + patch[ax] - hi))
        image = np.stack([np.pad((vol[tuple(sl)].astype(np.float32) - np.float32(mn)) / np.float32(mx - mn), pad)
                          for vol, (mn, mx) in zip((ct, mr), stats)]).astype(np.float16)
        raw = lab[tuple(sl)]
        cls = np.full(raw.shape, 255, np.uint8)
        cls[raw == 0] = 0
        for k, val in enumerate(values):
            cls[raw == val] = k + 1
        out.append((image, np.pad(cls, pad)))
    return out


def aten_warp(scan, stats, origins_host, theta, field, values, patch):
    """What a user composes from ATen for a warped patch: per sample a crop of a window enlarged by half a patch on every side
    (zero-padded where it leaves the scan), normalised in float32, and F.grid_sample of that window and of the one-hot label at
    F.affine_grid's coordinates (plus the field, resized trilinearly: ATen has no cubic B-spline), argmax for the class."""
    ct, mr, lab = scan
    images, labels = [], []
    K = len(values)
    for b, o in enumerate(origins_host):
        m = [p // 2 for p in patch]
        sl, pad = [], []
        for ax in range(3):
            lo_w, hi_w = o[ax] - m[ax], o[ax] + patch[ax] + m[ax]
            lo, hi = max(lo_w, 0), min(hi_w, lab.shape[ax])
            sl.append(slice(lo, hi))
            pad = [lo - lo_w, hi_w - hi] + pad
        window = torch.stack([F.pad((vol[tuple(sl)].float() - mn) / (mx - mn), pad) for vol, (mn, mx) in zip((ct, mr), stats)])
        raw = F.pad(lab[tuple(sl)], pad)
        cls = torch.full(raw.shape, K + 1, dtype=torch.int64, device=raw.device)
        cls[raw == 0] = 0
        for k, val in enumerate(values):
            cls[raw == val] = k + 1
        onehot = F.one_hot(cls, K + 2).permute(3, 0, 1, 2).float()
        n = F.affine_grid(torch.eye(3, 4, device=ct.device)[None], (1, 1) + tuple(patch), align_corners=False)
        if field is not None:
            n = n + F.interpolate(field[b:b + 1], size=patch, mode="trilinear", align_corners=True).permute(0, 2, 3, 4, 1)
        grid = n @ theta[b, :, :3].T + theta[b, :, 3]
        grid = grid * torch.tensor([patch[2] / window.shape[3], patch[1] / window.shape[2], patch[0] / window.shape[1]], device=ct.device)
        images.append(F.grid_sample(window[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0].half())
        labels.append(F.grid_sample(onehot[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0].argmax(0).to(torch.uint8))
    return torch.stack(images), torch.stack(labels)


def bench_warp(a, scan, index, shape, patch, values):
    """--warp: sample_patches through a map, and through a map and a (7, 7, 7) cubic field, next to the plain sample_patches of the
    same session and to aten_warp; one JSON line per batch size.  The image is compared with the ATen composition's where no tap
    leaves the enlarged window (share of elements within 2 fp16 steps), the label as the share of equal voxels."""
    from micformer_amd import affine, elastic, patches
    V = patch[0] * patch[1] * patch[2]
    stats = index[0].stats.cpu().tolist()
    if a.profile_only:
        B = a.profile_only
        g = torch.Generator().manual_seed(1)
        draws = patches.draw_patches(B, oversample_foreground_percent=1.0, generator=g, device="cuda")
        theta = affine.draw_affine(B, size=patch, generator=g, device="cuda")
        field = elastic.draw_elastic(B, size=patch, generator=g, device="cuda")
        for _ in range(20):
            patches.sample_patches([scan] * B, index * B, draws, patch_size=patch, affine=theta)
        for _ in range(20):
            patches.sample_patches([scan] * B, index * B, draws, patch_size=patch, affine=theta, displacement=field,
                                   field_interpolation="cubic")
        torch.cuda.synchronize()
        print(json.dumps({"profile_only": True, "warp": True, "B": B, "calls": "20 with a map, then 20 with a map and a cubic field"}))
        return
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        draws = patches.draw_patches(B, oversample_foreground_percent=1.0, generator=g, device="cuda")
        theta = affine.draw_affine(B, size=patch, generator=g, device="cuda")
        field = elastic.draw_elastic(B, size=patch, generator=g, device="cuda")
        samples, idx = [scan] * B, index * B
        out = patches.sample_patches(samples, idx, draws, patch_size=patch)
        plain = timed(lambda: patches.sample_patches(samples, idx, draws, patch_size=patch, out=out), a.min_seconds)
        ours_map = timed(lambda: patches.sample_patches(samples, idx, draws, patch_size=patch, out=out, affine=theta), a.min_seconds)
        kw = dict(affine=theta, displacement=field, field_interpolation="cubic")
        ours_field = timed(lambda: patches.sample_patches(samples, idx, draws, patch_size=patch, out=out, **kw), a.min_seconds)
        got = [t.clone() for t in patches.sample_patches(samples, idx, draws, patch_size=patch, affine=theta)]
        origins_host = got[2].cpu().tolist()
        aten_map = timed(lambda: aten_warp(scan, stats, origins_host, theta, None, values, patch), a.min_seconds)
        aten_field = timed(lambda: aten_warp(scan, stats, origins_host, theta, field, values, patch), a.min_seconds)
        ref_image, ref_label = aten_warp(scan, stats, origins_host, theta, None, values, patch)
        close = (got[0].float() - ref_image.float()).abs() <= 2.0 ** -9 * ref_image.float().abs().clamp(min=2.0 ** -5)
        row = {"case": f"{B} x warped patch {a.patch}^3 of " + "x".join(map(str, shape)) + " int16 pair + label", "B": B,
               "sample_ms": round(plain, 4), "warp_map_ms": round(ours_map, 4), "warp_map_field_ms": round(ours_field, 4),
               "aten_map_ms": round(aten_map, 4), "aten_map_field_ms": round(aten_field, 4),
               "ratio_aten_map": round(aten_map / ours_map, 2), "ratio_aten_map_field": round(aten_field / ours_field, 2),
               "ratio_plain_map": round(ours_map / plain, 2), "voxels": B * V,
               "image_close_aten": round(float(close.float().mean()), 5),
               "label_equal_aten": round(float((got[1] == ref_label).float().mean()), 5)}
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--shape", default="363,512,512")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--profile-only", type=int, default=0, metavar="B",
                    help="20 sample_patches calls of batch B and nothing else (for rocprofv3)")
    ap.add_argument("--warp", action="store_true",
                    help="time the crop through a map, and through a map and a (7, 7, 7) cubic field, next to the plain crop and an "
                         "ATen composition (a crop of an enlarged window + F.grid_sample on image and one-hot label)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patches.py needs the GPU")
    from micformer_amd import loader, patches
    shape = tuple(int(s) for s in a.shape.split(","))
    patch = (a.patch,) * 3
    values = patches.MMWHS_LABEL_VALUES
    scan = make_scan(shape, values, 7)
    index = patches.index_scans([scan])
    if a.warp:
        return bench_warp(a, scan, index, shape, patch, values)
    V = patch[0] * patch[1] * patch[2]
    crop_bytes_per_sample = V * (2 * 2 + 2 + 4 + 1)
    if a.profile_only:
        B = a.profile_only
        draws = patches.draw_patches(B, oversample_foreground_percent=1.0, generator=torch.Generator().manual_seed(1), device="cuda")
        for _ in range(20):
            patches.sample_patches([scan] * B, index * B, draws, patch_size=patch)
        torch.cuda.synchronize()
        print(json.dumps({"profile_only": True, "B": B, "calls": 20, "crop_bytes_per_call": B * crop_bytes_per_sample}))
        return
    index_ms = timed(lambda: patches.index_scans([scan]), a.min_seconds)
    load_ms = timed(lambda: loader.load_batch([scan]), a.min_seconds)
    stats = index[0].stats.cpu().tolist()
    counts = index[0].class_counts.cpu().tolist()
    host = tuple(t.cpu().numpy() for t in scan)
    for B in [int(b) for b in a.batches.split(",")]:
        draws = patches.draw_patches(B, oversample_foreground_percent=1.0, generator=torch.Generator().manual_seed(B), device="cuda")
        draws_host = draws.cpu().tolist()
        samples, idx = [scan] * B, index * B
        out = patches.sample_patches(samples, idx, draws, patch_size=patch)
        ours = timed(lambda: patches.sample_patches(samples, idx, draws, patch_size=patch, out=out), a.min_seconds)
        aten = timed(lambda: aten_sample(scan, stats, counts, draws_host, values, patch), a.min_seconds)
        ref_image, ref_label = aten_sample(scan, stats, counts, draws_host, values, patch)
        t0 = time.perf_counter()
        numpy_sample(host, stats, counts, draws_host, values, patch)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        row = {"case": f"{B} x patch {a.patch}^3 of " + "x".join(map(str, shape)) + " int16 pair + label", "B": B,
               "index_ms": round(index_ms, 4), "load_batch_ms": round(load_ms, 4), "sample_ms": round(ours, 4),
               "aten_ms": round(aten, 4), "numpy_ms": round(numpy_ms, 1), "ratio_aten": round(aten / ours, 2),
               "ratio_numpy": round(numpy_ms / ours, 1), "crop_bytes": B * crop_bytes_per_sample,
               "call_GBps": round(B * crop_bytes_per_sample / ours / 1e6, 1),
               "label_equal_aten": bool(torch.equal(out[1], ref_label)),
               "image_equal_aten": bool(torch.equal(out[0].view(torch.int16), ref_image.view(torch.int16)))}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
