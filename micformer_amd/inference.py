"""Sliding-window inference on the device -- the counterpart of `monai.inferers.sliding_window_inference` as the reference
calls it (utils.py:226-240: roi 128^3, sw_batch_size 1, overlap 0.5, default mode "constant", under autocast / no_grad).

MONAI is not vendored under /root/reference (un-pinned dependency), so the algorithm is restated from its documentation:
scan interval int(roi * (1 - overlap)) per axis, ceil((L - roi) / interval) + 1 windows with starts min(k * interval, L - roi),
symmetric zero padding when the image is smaller than the ROI, constant importance map, output = sum(pred) / count in fp32.
The referee is oracle/micformer_ref.py::sliding_window_inference (parity with MONAI itself is UNPINNED).

mode="gaussian" (nnU-Net's default blending) weights every window with the separable Gaussian importance map of blend.py:
out[b, k, v] = sum_i w_i(v) p_i[k, v] / sum_i w_i(v) over the windows i that cover v, in the order they are enumerated here (z, y, x,
then b).  It always takes the generic path -- predictor(win), then one plain read-modify-write launch per window
(csrc/sliding_window.hip, no float atomics) -- so for the same predictions its result is bit-identical from run to run and for every
sw_batch_size.  The map is
this library's definition (blend.py); parity with MONAI's compute_importance_map is UNPINNED as well, the referee is
tests/sw_blend_ref.py.

mirror_axes=(0, 1, 2) (nnU-Net's test-time mirroring, mirror.py) predicts every window under each flip of the chosen axes and
averages the predictions flipped back: out[b, k, v] = sum_i sum_f w_i(v) p_{i,f}[k, M_f(v - o_i)] / sum_i sum_f w_i(v), the terms in
(window, flip code) order.  Both flips are index arithmetic inside the crop and the accumulate (csrc/sliding_window.hip), so it adds no
pass and no buffer; in either mode it takes the generic path with the store-and-sum accumulate, and is bit-identical for the same
predictions from run to run and for every sw_batch_size.  The referee is tests/sw_mirror_ref.py.

The full-volume fp32 accumulator (8 x 512 x 512 x 256 = 2.1 GB for BASELINE config 5) and the visit counts stay in HBM; window
crops, the accumulate and the final divide are HIP kernels (csrc/sliding_window.hip); the predictor sees `sw_batch_size` windows per
call -- the network is batch-independent, so any sw_batch_size gives the same result and large ones fill the GPU better.
"""
import contextlib
import functools
import math

import torch

from . import blend, mirror
from .blend import importance_map  # noqa: F401  (public: the map sliding_window_inference applies)


FUSE_ACCUMULATE = True


def sliding_window_starts(L, roi, overlap=0.5):
    if L <= roi:
        return [0]
    interval = max(int(roi * (1 - overlap)), 1)
    n = int(math.ceil((L - roi) / interval)) + 1
    return [min(k * interval, L - roi) for k in range(n)]


class GraphedPredictor:
    """Replays the predictor's forward from one HIP graph per input shape (the eager forward of the base model is ~1000 launches
    and host-bound: 16 ms per 128^3 window eager, a few ms replayed).  The returned tensor is the graph's static output: it is
    consumed (accumulated) on the same stream before the next replay overwrites it."""

    def __init__(self, predictor, warmup=2):
        self.predictor, self.warmup, self.graphs = predictor, warmup, {}

    def _param_versions(self):
        params = getattr(self.predictor, "parameters", None)
        if params is None:
            return 0
        return sum(p._version for p in params())

    def __call__(self, x):
        from . import ops
        # The arithmetic mode and the cached K16-blocked / re-laid-out weight copies are baked into a captured graph (biases,
        # LayerNorm parameters and head weights are read live): ANY parameter write retires it -- an engine step or checkpoint
        # load (PARAM_EPOCH), or torch code such as load_state_dict / an optimizer step (the tensors' version counters).
        stamp = (ops.PARAM_EPOCH[0], self._param_versions())
        if getattr(self, "_epoch", None) != stamp:
            self.graphs.clear()
            self._epoch = stamp
        key = (tuple(x.shape), x.dtype, ops.arith_mode())
        entry = self.graphs.get(key)
        if entry is None:
            static_in = x.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(self.warmup):
                    self.predictor(static_in)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                static_out = self.predictor(static_in)
            entry = self.graphs[key] = (graph, static_in, static_out)
        graph, static_in, static_out = entry
        static_in.copy_(x)
        graph.replay()
        return static_out

    def accumulators(self, shape, device):
        """Persistent (out, count) volume accumulators per volume shape: the captured accumulate graphs bake their addresses in,
        so re-using them across volumes avoids a re-capture per volume.  sliding_window_inference returns a copy of `out`."""
        acc = self.__dict__.setdefault("_acc", {})
        key = (tuple(shape), str(device))
        if key not in acc:
            # ONE accumulator pair is kept (validation sets with varying volume sizes would otherwise grow device memory without
            # bound: 2.4 GB per 512x512x256 shape at 8 classes); a new shape evicts the old pair and the graphs that baked it in
            for old in list(acc):
                o, c = acc.pop(old)
                for k in [k for k in self.graphs if k[0] == "acc" and k[-2:] == (o.data_ptr(), c.data_ptr())]:
                    del self.graphs[k]
            B, K, D, H, W = shape
            acc[key] = (torch.empty(shape, dtype=torch.float32, device=device), torch.empty((B, D, H, W), dtype=torch.float32, device=device))
        return acc[key]

    def accumulate(self, x, out, count, coords):
        """The predictor's `forward_accumulate` (windows -> ADDED into the volume accumulator at `coords`, see
        MICFormer_self.Head.forward_accumulate) replayed from one HIP graph per (window batch shape, accumulator): the accumulator
        addresses are baked in, the coordinates are a static device tensor refreshed before every replay."""
        from . import ops
        stamp = (ops.PARAM_EPOCH[0], self._param_versions())
        if getattr(self, "_epoch", None) != stamp:
            self.graphs.clear()
            self._epoch = stamp
        key = ("acc", tuple(x.shape), x.dtype, ops.arith_mode(), out.data_ptr(), count.data_ptr())
        entry = self.graphs.get(key)
        if entry is None:
            static_in, static_c = x.clone(), coords.clone()
            keep_out, keep_cnt = out.clone(), count.clone()             # the eager warm-up runs accumulate for real: undone below
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(self.warmup):
                    self.predictor.forward_accumulate(static_in, out, count, static_c)
            torch.cuda.current_stream().wait_stream(side)
            out.copy_(keep_out)
            count.copy_(keep_cnt)
            del keep_out, keep_cnt
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                self.predictor.forward_accumulate(static_in, out, count, static_c)
            entry = self.graphs[key] = (graph, static_in, static_c)
        graph, static_in, static_c = entry
        static_in.copy_(x)
        static_c.copy_(coords)
        graph.replay()


@contextlib.contextmanager
def _bf16_predictor(on):
    """The predictor runs in bf16 mode inside (`on`; else in the mode that is set); the mode is restored after."""
    from . import ops
    prev = ops.arith_mode()
    if on:
        ops.set_compute_dtype("bf16")
    try:
        yield
    finally:
        ops.set_compute_dtype(prev)


def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.5, mode="constant", sigma_scale=0.125, *,
                             graph=False, autocast=False, mirror_axes=()):
    """inputs (B, C, D, H, W) on the GPU -> (B, K, D, H, W) fp32, K = the predictor's output channels.
    mode "constant" (MONAI's default: every voxel of a window weighs 1) or "gaussian" (blend.importance_map: sigma_scale, a positive
    float or one per axis, times the roi size is the Gaussian's sigma; ignored for "constant").  The Gaussian mode calls
    `predictor(win)` also for a Head that offers the fused accumulate epilogue, and for the same predictions it is bit-identical from
    run to run and for every sw_batch_size; parity of its map with MONAI's is UNPINNED (blend.py states the definition).
    graph=True wraps the predictor in a GraphedPredictor (pass your own instance as `predictor` to reuse it across volumes).
    autocast=True runs the predictor with bf16 matrix-core operands -- this library's counterpart of the
    `torch.cuda.amp.autocast()` the reference wraps the call in (utils.py:236-238; fp16 there).
    mirror_axes: a subset of (0, 1, 2) = (D, H, W); every window is predicted under each of the 2^k flips of these axes and the
    predictions, flipped back, are averaged (mirror.py).  In either mode this calls `predictor(win)` on `sw_batch_size` (window,
    flip) pairs at a time and is bit-identical for every sw_batch_size; () is the call without mirroring, launch for launch."""
    if graph and not isinstance(predictor, GraphedPredictor):
        predictor = GraphedPredictor(predictor)
    gaussian = blend.check_mode(mode) == "gaussian"
    codes = mirror.flip_codes(mirror_axes)
    mirrored = len(codes) > 1
    if gaussian:
        blend.sigma_scales(sigma_scale)
    if inputs.dim() != 5 or not inputs.is_cuda:
        raise ValueError("sliding_window_inference expects a (B, C, D, H, W) CUDA (ROCm) tensor")
    if isinstance(roi_size, int):
        roi_size = (roi_size,) * 3
    roi = rd, rh, rw = tuple(int(r) for r in roi_size)
    x = inputs.float().contiguous()
    B, C, D, H, W = x.shape
    pd, ph, pw = max(rd - D, 0), max(rh - H, 0), max(rw - W, 0)
    if pd or ph or pw:       # image smaller than the ROI: symmetric zero padding, cropped away again at the end
        x = torch.nn.functional.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2, pd // 2, pd - pd // 2)).contiguous()
    Dp, Hp, Wp = x.shape[2:]
    slices = [(b, z, y, xx) for z in sliding_window_starts(Dp, rd, overlap) for y in sliding_window_starts(Hp, rh, overlap)
              for xx in sliding_window_starts(Wp, rw, overlap) for b in range(B)]
    if mirrored:       # items (b, z0, y0, x0, flip), window-major: a voxel's terms arrive in (window, flip code) order for every sw
        slices = [s + (f,) for s in slices for f in codes]
    sw = min(max(int(sw_batch_size), 1), 64)
    out = count = None
    from . import ops
    # Fused epilogue: a predictor that offers `forward_accumulate` (MICFormer_self.Head with the composed head)
    # adds its logits straight into the volume accumulator at the window origins and bumps the visit counts in its last launch --
    # no [n, K, roi] prediction tensor, no accumulate launch.  Needs roi dims that the patch size divides (else the model pads).
    base = predictor.predictor if isinstance(predictor, GraphedPredictor) else predictor
    fused = not gaussian and not mirrored and FUSE_ACCUMULATE and hasattr(base, "forward_accumulate") and hasattr(base, "out_conv") \
        and getattr(base, "can_accumulate", lambda roi: False)(roi)      # (else: the generic crop / predict / accumulate path)
    with torch.no_grad():
        if fused:
            K = base.out_conv.out_channels
            cached = isinstance(predictor, GraphedPredictor)
            out, count = blend.new_sums(B, K, Dp, Hp, Wp, x.device,
                                        reuse=predictor.accumulators((B, K, Dp, Hp, Wp), x.device) if cached else None)
            accumulate = predictor.accumulate if cached else base.forward_accumulate
            with _bf16_predictor(autocast):
                for i in range(0, len(slices), sw):
                    chunk = slices[i:i + sw]
                    win = ops.sw_window_batch(x, chunk, roi)
                    accumulate(win, out, count, torch.tensor(chunk, dtype=torch.int32).to(x.device, non_blocking=True))
        else:
            # ONE launch crops the whole batch of windows (mirrored: each under its item's flip); then one accumulate launch per
            # item in order, flipped back (mirrored), one per window in order with `count` = sum(w) (Gaussian), or ONE that adds
            # the batch into the volume accumulator with atomics
            crop = mirror.window_batch if mirrored else ops.sw_window_batch
            if mirrored or gaussian:
                taps, floor = blend.device_taps(roi, sigma_scale, x.device) if gaussian else (None, 1.0)
                accumulate = functools.partial(mirror.accumulate if mirrored else blend.accumulate, taps=taps, floor=floor)
            else:
                accumulate = ops.sw_accumulate_batch
            for i in range(0, len(slices), sw):
                chunk = slices[i:i + sw]
                win = crop(x, chunk, roi)
                with _bf16_predictor(autocast):
                    pred = predictor(win).float().contiguous()
                if pred.shape[0] != len(chunk) or tuple(pred.shape[2:]) != roi:
                    raise ValueError(f"predictor returned {tuple(pred.shape)} for windows {tuple(win.shape)}")
                if out is None:
                    out, count = blend.new_sums(B, pred.shape[1], Dp, Hp, Wp, x.device)
                accumulate(pred, out, count, chunk)
        blend.normalize(out, count)
        if fused and cached:
            out = out.clone()                             # (the accumulator itself stays with the predictor's graphs)
    if pd or ph or pw:
        out = out[:, :, pd // 2:pd // 2 + D, ph // 2:ph // 2 + H, pw // 2:pw // 2 + W].contiguous()
    return out
