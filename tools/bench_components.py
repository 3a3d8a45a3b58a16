"""Time micformer_amd.postprocess.keep_largest_components on MM-WHS-like label volumes against the composition it replaces
(scipy.ndimage.label once per class on the host), in the same run; one JSON line per case and connectivity.

    python tools/bench_components.py [--cases a,b,c] [--min-seconds 0.5] [--no-referee]

Cases:
  a  128^3 uint8 class map: 8 smooth classes with planted islands
  b  the same kind of scene at 363 x 512 x 512, int16 label values
  c  363 x 512 x 512 uint8 binary noise of density 0.5 (about 8.6e5 components with 6 neighbours): the adversarial input
a and b run with 26 and 6 neighbours, c with 6.

device_ms: device events around >= min-seconds of replays of a captured graph of the call, after warm-up (the whole call with a
preallocated output and workspace: five launches; 16 calls per graph below 2^24 voxels, so that launch cost does not fill the
window).  eager_ms: the same call issued from Python, host launch cost included.  referee_ms: the host composition, one run (its
result must equal the device's: `differing` is asserted 0).  floor_ms: (input + output bytes) / 6.3 TB/s, the copy rate of the
chip; x_floor = device_ms / floor_ms.  An end-to-end figure of the call, not a kernel's share of peak: per-kernel times come from a
kernel trace of this script (components_*_kernel).
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

COPY_RATE = 6.3e12
CLASSES = 8
FULL = (363, 512, 512)


def blob_scene(shape, seed=0, islands=2e-5):
    """A class map on the device: argmax of 8 smooth fields, plus isolated voxels of random class (`islands` of the voxels)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn(1, CLASSES, 7, 9, 9, generator=g, device="cuda")
    base[:, 0] += 0.8                                     # more background than anything else
    cmap = F.interpolate(base, size=shape, mode="trilinear", align_corners=False)[0].argmax(0).to(torch.uint8)
    speck = torch.rand(shape, generator=g, device="cuda") < islands
    cls = torch.randint(1, CLASSES, shape, generator=g, device="cuda", dtype=torch.uint8)
    return torch.where(speck, cls, cmap).contiguous()


def _window(run, per_run, min_seconds):
    """ms per call and calls: device events around windows of `run()` (per_run calls each) until min_seconds have been timed."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs, ms = 0, 0.0
    while ms < min_seconds * 1e3:
        n = max(1, runs or 4)
        e0.record()
        for _ in range(n):
            run()
        e1.record()
        e1.synchronize()
        ms += e0.elapsed_time(e1)
        runs += n
    return ms / (runs * per_run), runs * per_run


def timed(fn, per_graph, min_seconds):
    """-> (device ms per call, calls, eager ms per call).  The device figure replays a captured graph of `per_graph` calls back to
    back, so the host's five launches per call are not in it; the eager figure is the same call issued from Python (ctypes and
    the launches included), which is what a caller without a graph sees."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(per_graph):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    ms, calls = _window(graph.replay, per_graph, min_seconds)
    eager_ms, _ = _window(fn, 1, min_seconds / 4)
    return ms, calls, eager_ms


def referee(vol, values, conn):
    """scipy per class: keep the largest component (argmax of bincount).  -> (result, seconds, components)."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
    t0 = time.perf_counter()
    out = vol.copy()
    total = 0
    for value in values:
        lab, n = ndimage.label(vol == value, st)
        total += n
        if n > 1:
            out[(lab > 0) & (lab != int(np.argmax(np.bincount(lab.ravel())[1:])) + 1)] = 0
    return out, time.perf_counter() - t0, total


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-referee", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_components.py needs the GPU")
    from micformer_amd import postprocess as P
    table = torch.tensor((0,) + tuple(P.MMWHS_LABEL_VALUES), dtype=torch.int16, device="cuda")
    host = cpu_name()
    for case in a.cases.split(","):
        if case == "a":
            vol, kw, values, conns = blob_scene((128, 128, 128)), dict(num_classes=CLASSES, label_values=None), range(1, CLASSES), (26, 6)
        elif case == "b":
            vol, kw, values, conns = table[blob_scene(FULL).long()].contiguous(), {}, P.MMWHS_LABEL_VALUES, (26, 6)
        elif case == "c":
            g = torch.Generator(device="cuda").manual_seed(0)
            vol = (torch.rand(FULL, generator=g, device="cuda") < 0.5).to(torch.uint8)
            kw, values, conns = dict(num_classes=2, label_values=None), (1,), (6,)
        else:
            raise SystemExit(f"unknown case {case!r}")
        out = torch.empty_like(vol)
        ws = torch.empty(P.workspace_bytes([tuple(vol.shape)]), dtype=torch.uint8, device="cuda")
        nbytes = 2 * vol.numel() * vol.element_size()
        for conn in conns:
            per_graph = 16 if vol.numel() < 1 << 24 else 1
            ms, calls, eager_ms = timed(lambda: P.keep_largest_components(vol, connectivity=conn, out=out, workspace=ws, **kw),
                                        per_graph, a.min_seconds)
            floor_ms = nbytes / COPY_RATE * 1e3
            rec = {"case": case, "shape": "x".join(map(str, vol.shape)), "dtype": str(vol.dtype).replace("torch.", ""),
                   "connectivity": conn, "device_ms": round(ms, 4), "timing": f"graph replay, {per_graph} calls per graph",
                   "eager_ms": round(eager_ms, 4), "calls": calls, "bytes_in_out": nbytes,
                   "floor_ms": round(floor_ms, 4), "x_floor": round(ms / floor_ms, 1), "workspace_bytes": ws.numel(),
                   "voxels_removed": int((out != vol).sum())}
            if not a.no_referee:
                want, seconds, n = referee(vol.cpu().numpy(), values, conn)
                differing = int((out.cpu().numpy() != want).sum())
                rec.update({"referee_ms": round(seconds * 1e3, 1), "referee_over_device": round(seconds * 1e3 / ms, 1),
                            "components": n, "differing": differing, "host_cpu": host})
                print(json.dumps(rec), flush=True)
                assert differing == 0, f"case {case} connectivity {conn}: {differing} voxels differ from the referee"
            else:
                print(json.dumps(rec), flush=True)
        del vol, out, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
