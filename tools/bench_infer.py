#!/usr/bin/env python3
"""BASELINE config 5: sliding-window inference of MicFormer base on a synthetic 512 x 512 x 256 two-modality volume
(roi 128^3, overlap 0.5 -> 147 windows), one MI355X.  Prints seconds per volume and windows/s for a few sw_batch_size values.
usage: python tools/bench_infer.py [D H W] [--autocast] [--mode constant|gaussian] [--mirror-axes 0,1,2 [--trivial] [--rounds N]]
(--autocast: bf16 matrix-core mode for the predictor, utils.py:236-238; --mode: the blending of overlapping windows, default constant)
--mirror-axes: test-time mirroring.  Times three things with device events, graph replay, 7 items per call, alternating them for
--rounds rounds (default 3) after a warm-up of each: the call without mirroring, the call with mirror_axes, and the composition a
user writes without it -- one call of the inferer per flip with a torch.flip-wrapped predictor, the outputs averaged.  --trivial
swaps the network for a predictor that only copies channels, so that the data movement of the three shows on its own."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from micformer_amd.models.MICFormer_self import Head
from micformer_amd.inference import sliding_window_inference, sliding_window_starts

AUTOCAST = "--autocast" in sys.argv
TRIVIAL = "--trivial" in sys.argv
MODE = "constant"
args = sys.argv[1:]


def _option(name, default=None):
    if name not in args:
        return default
    at = args.index(name)
    if at + 1 >= len(args):
        sys.exit(f"{name} takes a value")
    value = args[at + 1]
    del args[at:at + 2]
    return value


MODE = _option("--mode", "constant")
if MODE not in ("constant", "gaussian"):
    sys.exit("--mode takes constant or gaussian")
MIRROR = _option("--mirror-axes")
ROUNDS = int(_option("--rounds", "3"))
if MIRROR is not None:
    from micformer_amd import mirror
    try:
        MIRROR = tuple(int(a) for a in MIRROR.split(",") if a != "")
        CODES = mirror.flip_codes(MIRROR)
    except ValueError:
        sys.exit("--mirror-axes takes distinct axes from 0,1,2 separated by commas")
argv = [a for a in args if not a.startswith("--")]
dims = tuple(int(a) for a in argv[:3]) if len(argv) >= 3 else (512, 512, 256)
torch.manual_seed(0)
model = Head(embed_dim=48, num_classes=8).cuda().eval()
x = torch.randn((1, 2) + dims, device="cuda")
nwin = 1
for L in dims:
    nwin *= len(sliding_window_starts(L, 128))
from micformer_amd.inference import GraphedPredictor
WORKLOAD = f"sliding-window inference, MicFormer base, volume {dims}, roi 128^3, overlap 0.5, {nwin} windows, {'bf16 mode' if AUTOCAST else 'fp32 kernels'}, mode {MODE}"


def bench_mirror():
    sw = 7
    if TRIVIAL:
        def pred(win):                                   # [n, 2, roi] -> [n, 8, roi]: one copy, no network
            return win.repeat(1, 4, 1, 1, 1)
    else:
        pred = GraphedPredictor(model)
    kw = dict(overlap=0.5, mode=MODE, autocast=AUTOCAST and not TRIVIAL)

    def plain():
        return sliding_window_inference(x, (128, 128, 128), sw, pred, **kw)

    def mirrored():
        return sliding_window_inference(x, (128, 128, 128), sw, pred, mirror_axes=MIRROR, **kw)

    def composed():
        total = None
        for f in CODES:
            flip_dims = [a + 2 for a in range(3) if f >> a & 1]
            wrapped = pred if not flip_dims else (lambda win: torch.flip(pred(torch.flip(win, flip_dims)), flip_dims))
            out = sliding_window_inference(x, (128, 128, 128), sw, wrapped, **kw)
            total = out if total is None else total.add_(out)
        return total.div_(len(CODES))

    runs = {"no_mirroring": plain, "mirror_axes": mirrored, "composition": composed}
    times = {k: [] for k in runs}
    with torch.no_grad():
        outs = {k: fn() for k, fn in runs.items()}        # warm-up of every shape and graph; the outputs are compared below
        apart = float((outs["mirror_axes"] - outs["composition"]).abs().max())
        checksum = float(outs["mirror_axes"].double().mean())
        del outs
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / 1e3)
    res = {k: {"s_per_volume": round(min(v), 4), "spread_s": round(max(v) - min(v), 4), "runs": [round(t, 4) for t in v]}
           for k, v in times.items()}
    print(json.dumps({"workload": WORKLOAD + f", mirror axes {list(MIRROR)} ({len(CODES)} flips), graph replay, {sw} items per call"
                      + (", trivial predictor" if TRIVIAL else ""),
                      "results": res, "max_abs_mirror_minus_composition": apart, "checksum": checksum}))


if MIRROR is not None:
    bench_mirror()
    sys.exit(0)
res = {}
for graphed in (False, True):
    for sw in (1, 3, 7):
        pred = GraphedPredictor(model) if graphed else model
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            # warm-up on the SAME volume and overlap (graph capture incl. the volume accumulators it bakes in), then the better of two runs
            sliding_window_inference(x, (128, 128, 128), sw, pred, overlap=0.5, mode=MODE, autocast=AUTOCAST)
            dt = 1e9
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = sliding_window_inference(x, (128, 128, 128), sw, pred, overlap=0.5, mode=MODE, autocast=AUTOCAST)
                torch.cuda.synchronize()
                dt = min(dt, time.perf_counter() - t0)
        res[f"{'graph' if graphed else 'eager'}_sw_batch_{sw}"] = {"s_per_volume": round(dt, 3), "windows_per_s": round(nwin / dt, 1)}
print(json.dumps({"workload": WORKLOAD, "results": res, "checksum": float(out.double().mean())}))
