"""Time micformer_amd.restore.restore_batch on full-size MM-WHS-like predictions (8 x 128^3 float32 logits -> 363x512x512 int16
labels) against the ATen composition it replaces, in the same process with the same timing method; one JSON line per batch size
and interpoland.

    python tools/bench_restore.py [--batches 1,2] [--min-seconds 0.5]

fused_ms: device events around >= min-seconds of calls after warm-up (the whole call with preallocated outputs: for the probability
interpoland the softmax pre-pass at 128^3 plus its workspace allocation, then the fused upsample + argmax + label pass).
aten_ms: F.interpolate(trilinear) [+ softmax before it] + argmax(1) + an int16 table lookup on the GPU, timed the same way.
ratio = aten_ms / fused_ms; the tool fails when the fused call is slower than the composition.
fused_GBps: the bytes the fused call must move (one read of the logits, one write of the labels) over fused_ms -- an end-to-end
figure of the call, not a kernel's share of peak.  Per-kernel times proper come from a kernel trace of this script
(restore_softmax_kernel / restore_fused_kernel).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SRC = (128, 128, 128)
SHAPE = (363, 512, 512)
CLASSES = 8


def make_logits(batch, seed=0):
    """Smooth class fields plus noise, |logits| <= about 12 (the recipe of tests/restore_ref.py, generated on the device)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn(batch, CLASSES, 6, 6, 6, generator=g, device="cuda")
    noise = torch.randn(batch, CLASSES, *SRC, generator=g, device="cuda")
    return (3 * F.interpolate(base, size=SRC, mode="trilinear") + 0.3 * noise).contiguous()


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
    return ms / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore.py needs the GPU")
    from micformer_amd import restore
    table = torch.tensor((0,) + tuple(restore.MMWHS_LABEL_VALUES), dtype=torch.int16, device="cuda")
    slower = []
    for B in [int(b) for b in a.batches.split(",")]:
        logits = make_logits(B)
        shapes = [SHAPE] * B
        out = [torch.empty(SHAPE, dtype=torch.int16, device="cuda") for _ in range(B)]
        nbytes = logits.numel() * 4 + sum(t.numel() * 2 for t in out)
        for probabilities in (False, True):
            def fused():
                restore.restore_batch(logits, shapes, probabilities=probabilities, out=out)

            def aten():
                x = torch.softmax(logits, 1) if probabilities else logits
                return table[F.interpolate(x, size=SHAPE, mode="trilinear", align_corners=False).argmax(1)]

            fused_ms, calls = timed(fused, a.min_seconds)
            aten_ms, aten_calls = timed(aten, a.min_seconds)
            differ = sum(int((o != r).sum()) for o, r in zip(out, aten()))
            torch.cuda.empty_cache()
            print(json.dumps({"case": f"{CLASSES}x" + "x".join(map(str, SRC)) + " -> " + "x".join(map(str, SHAPE)), "B": B,
                              "interpoland": "probabilities" if probabilities else "logits",
                              "fused_ms": round(fused_ms, 4), "fused_ms_per_sample": round(fused_ms / B, 4), "calls": calls,
                              "aten_ms": round(aten_ms, 4), "aten_calls": aten_calls, "ratio": round(aten_ms / fused_ms, 2),
                              "fused_GBps": round(nbytes / fused_ms / 1e6, 1), "bytes_per_call": nbytes,
                              "labels_differing_from_aten": differ, "voxels": B * SHAPE[0] * SHAPE[1] * SHAPE[2]}), flush=True)
            if fused_ms > aten_ms:
                slower.append((B, probabilities, fused_ms, aten_ms))
    assert not slower, f"the fused call is slower than the ATen composition: {slower}"


if __name__ == "__main__":
    main()
