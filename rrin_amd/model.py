"""Drop-in ``Net`` for RRIN inference on MI355X.

Boundary: same class name, no-arg constructor, submodules
``Mask``/``Flow``/``refine_flow``/``final`` (reference `model.py:24-30`), the
same 162 state_dict keys, and ``forward(input0, input1, t=0.5)`` returning a
fresh ``[N,3,H,W]`` tensor on the inputs' device (`model.py:59-65`).

Unlike the reference, the arithmetic of ``forward`` is done entirely by the
hand-written HIP kernels of ``librrin_hip.so`` (see ``rrin_amd.engine``); there
is no PyTorch-operator path.  The HIP path requires:

* inputs on a ROCm device, fp32 (the metric's dtype), NCHW, H % 16 == W % 16 == 0
  (the reference raises at `model.py:41` otherwise — we raise earlier);
* autograd off (``torch.no_grad()`` / ``inference_mode``), as in the production
  caller `convert.py:117`.

With autograd on (the training caller `train.py:98`) ``forward``
runs the reference graph (`model.py:32-65`) on the HIP training kernels: on a
ROCm device every conv3x3 (+ leaky), avg-pool, upsample and backwarp is an
autograd Function whose forward and backward are HIP kernels
(``rrin_amd.autograd``, ``csrc/train.hip``), the elementwise glue is PyTorch
autograd; on a CPU device the same graph runs with PyTorch operators
(``_forward_autograd``).  That path is never taken for inference, and a
missing or failing HIP library raises.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .unet import UNet


def _plane_kw(plane):
    """The ``plane=`` keyword of a frame method for the engine: absent unless given, so a call without
    it is the call it always was."""
    return {} if plane is None else {"plane": plane}


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        # model.py:27-30 — construction order fixes the state_dict key order.
        self.Mask = UNet(16, 2, 4)
        self.Flow = UNet(6, 4, 5)
        self.refine_flow = UNet(10, 4, 4)
        self.final = UNet(9, 3, 4)
        self._engine = None
        self._engine_fp = None
        self._engine_version = -1
        self._weights_version = 0
        # Arithmetic of the HIP path (not part of the reference contract):
        #   "fp32"         exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
        #   "fp32_split16" fp32 values as fp16 hi+lo pairs, 3 f16 MFMA products, fp32 accumulate
        #   "fp16"         fp16 storage and products, fp32 accumulate (BASELINE fp16 configs)
        self.precision = "fp32"
        # fp32_split16 / fp16: up convs whose output level is <= this run as
        # sub-pixel convs on the low-res input (upsample folded into the weights,
        # no upsample pass); -1 = always an explicit upsample pass
        self.subpixel_max_level = 2
        # HIP streams a batch of N >= 2 pairs is split over (pairs are
        # independent: the output is bitwise that of one stream; the parts'
        # kernels fill each other's launch gaps and tails); None: by precision
        # and batch (engine.default_streams: 2)
        self.streams = None
        self.register_load_state_dict_post_hook(Net._on_load)

    # Packed weights are rebuilt after load_state_dict / .to() (version bump) and
    # after any in-place parameter edit (optimizer.step, p.copy_, nn.init, a
    # sub-UNet's load_state_dict): engine() compares each parameter's storage
    # pointer and autograd version counter with those the packing was built from.
    @staticmethod
    def _on_load(module, incompatible_keys):
        module._weights_version += 1

    def invalidate_packed_weights(self):
        self._weights_version += 1

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._weights_version += 1
        return out

    def _weights_fingerprint(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def engine(self):
        from .engine import RRINEngine
        fp = self._weights_fingerprint()
        if (self._engine is None or self._engine_version != self._weights_version
                or self._engine_fp != fp
                or self._engine.precision != self.precision
                or self._engine.subpixel_max_level != self.subpixel_max_level):
            self._engine = None  # free the previous packed weights first
            self._engine = RRINEngine(self, self.precision, self.subpixel_max_level)
            self._engine_version = self._weights_version
            self._engine_fp = fp
        return self._engine

    def check_range(self, wait: bool = True):
        """fp32_split16 / fp16: raise if an activation overflowed fp16 in a
        forward issued so far (those outputs are NaN-poisoned on the device).
        ``wait=False`` only looks at the forwards that have already finished.
        A no-op for the fp32 precisions."""
        if self._engine is not None:
            self._engine._poll_range(wait=wait)

    def interpolate(self, input0, input1, ts, flow_scale=1):
        """All intermediate frames of one (batch of) pair(s): ``[forward(I0, I1, t) for t in ts]``
        with the t-independent Flow U-Net computed once (the
        reference recomputes it per t, convert.py:127-130).

        ``flow_scale`` 2 or 4, here and on every frame method below: the Flow U-Net runs at 1/s of
        the size and its flow is scaled up (:mod:`rrin_amd.flowscale`, which is the definition);
        the frame paths then pad to a multiple of 16 * s.  Record precisions, inference only."""
        from .flowscale import check_flow_scale
        check_flow_scale(flow_scale)
        if torch.is_grad_enabled():
            raise RuntimeError("rrin_amd.Net.interpolate is inference-only: use torch.no_grad()")
        eng = self.engine()
        return [eng.forward(input0, input1, t, reuse_flow=(k > 0), streams=self.streams, flow_scale=flow_scale)
                for k, t in enumerate(ts)]

    def _frames(self, path, f0, f1, t, many, **kw):  # kw may carry plane=: every result is then (frames, plane)
        """``forward_<path>`` (one ``t``) or, ``many``, ``interpolate_<path>`` (a list ``t``) of the frame
        paths: the engine's ``forward_<path>`` once, or for every t of the list with the Flow U-Net (and
        the gate's sums) of the first call reused by the others."""
        if torch.is_grad_enabled():
            what = ("interpolate_" if many else "forward_") + path
            raise RuntimeError(f"rrin_amd.Net.{what} is inference-only: use torch.no_grad()")
        fwd = getattr(self.engine(), "forward_" + path)
        if not many:
            return fwd(f0, f1, t, streams=self.streams, **kw)
        return [fwd(f0, f1, v, reuse_flow=(k > 0), streams=self.streams, **kw) for k, v in enumerate(t)]

    def forward_u8(self, f0, f1, t=0.5, scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """``forward`` on 8-bit frames of any size: uint8 ``[N,H0,W0,3]`` in and out, on the
        device; bit for bit ``convert.load_frame`` -> ``forward`` -> ``convert.to_uint8_image``
        (``RRINEngine.forward_u8``).  Inference-only; not for ``precision='fp32_planar'``.

        The scene gate is off unless ``scene_threshold`` (a mean absolute byte difference in
        [0, 255]) or ``gate`` (an int32 device tensor ``[N]`` of codes) is given, never both: a
        repeated frame returns ``f0``, a shot change the nearer input frame (``f1`` from t = 0.5
        on), decided and applied on the device (``RRINEngine.forward_u8``).  The network still
        runs for a gated pair: skipping it would need a host sync.  No threshold has been
        validated on real footage; :attr:`last_gate` reports what a call decided.

        ``plane=(a0, a1)``, here and on every frame method below: one extra single-channel image per
        input frame, uint8 (uint16 on the 16-bit paths) ``[N,H0,W0]`` -- an alpha matte, a depth or an
        ID plane -- carried to time t by the picture's own refined flows and mask weights
        (:mod:`rrin_amd.plane` is the definition).  The call then returns ``(frames, plane)``; the
        ``interpolate_*`` methods a list of such pairs, one per t; the ``interpolate_items_*`` methods
        take one ``[P+1,H0,W0]`` stack.  RGB is taken as stored (no premultiply).  Without the keyword
        nothing changes."""
        return self._frames("u8", f0, f1, t, False, scene_threshold=scene_threshold, gate=gate,
                            flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_u8(self, f0, f1, ts, scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """``[forward_u8(f0, f1, t) for t in ts]`` with the Flow U-Net computed once, as
        :meth:`interpolate`; with ``scene_threshold`` the pairs' sums of absolute differences are
        computed once too (the cut code depends on t, so :attr:`last_gate` is that of ``ts[-1]``)."""
        return self._frames("u8", f0, f1, ts, True, scene_threshold=scene_threshold, gate=gate,
                            flow_scale=flow_scale, **_plane_kw(plane))

    def pair_stats_u8(self, f0, f1):
        """int64 device tensor ``[N]``: the sum of absolute byte differences of every pair of two
        uint8 ``[N,H0,W0,3]`` stacks, exact (rrin_pair_sad_u8_len) -- what ``scene_threshold`` compares
        with ``floor(threshold * H0*W0*3)``, for callers who pass their own ``gate``."""
        return self.engine().pair_stats_u8(f0, f1)

    def forward_yuv(self, f0, f1, t=0.5, layout="nv12", coef=None, scene_threshold=None, gate=None, flow_scale=1,
                    plane=None):
        """``forward`` on 8-bit YUV 4:2:0 frames, as decoders and video pipes deliver them: uint8
        ``[N, 3*H0//2, W0]`` in and out on the device (H0, W0 even; ``layout`` "nv12" or "i420") -- or
        4:2:2 (``layout`` "nv16" / "i422": ``[N, 2*H0, W0]``, W0 even) and 4:4:4 ("i444": ``[N, 3*H0,
        W0]``, any size), defined by ``yuv.rgb_to_yuv`` / ``yuv.yuv_to_rgb`` with that layout.
        By definition, and bit for bit, ``yuv.rgb_to_yuv420(forward_u8(yuv.yuv420_to_rgb(f0),
        yuv.yuv420_to_rgb(f1), t))`` with the integer conversions of :mod:`rrin_amd.yuv` (``coef``:
        ``yuv.coefficients(...)`` or any 15 ints; None is BT.709 limited range), computed inside
        the input pack and the last head's store: no RGB frame exists on the device
        (``RRINEngine.forward_yuv``).  Inference-only; not for ``precision='fp32_planar'``.

        The scene gate is ``forward_u8``'s, on the frames' bytes: a gated pair returns its input
        frame's YUV bytes unchanged.  ``scene_threshold`` is a mean absolute difference over luma
        and chroma bytes, so not the same number as the RGB path's; no value has been validated
        on real footage."""
        return self._frames("yuv", f0, f1, t, False, layout=layout, coef=coef,
                            scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_yuv(self, f0, f1, ts, layout="nv12", coef=None, scene_threshold=None, gate=None, flow_scale=1,
                        plane=None):
        """``[forward_yuv(f0, f1, t) for t in ts]`` with the Flow U-Net (and, with
        ``scene_threshold``, the pairs' sums of absolute differences) computed once, as
        :meth:`interpolate_u8`."""
        return self._frames("yuv", f0, f1, ts, True, layout=layout, coef=coef,
                            scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def pair_stats_yuv(self, f0, f1, layout="nv12"):
        """int64 device tensor ``[N]``: the sum of absolute byte differences, luma and chroma, of
        every pair of two 4:2:0 stacks -- what ``forward_yuv``'s ``scene_threshold`` compares with
        ``floor(threshold * H0*W0*3/2)`` (a 4:2:2 / 4:4:4 ``layout``: ``2*H0*W0`` / ``3*H0*W0`` bytes)."""
        return self.engine().pair_stats_yuv(f0, f1, layout=layout)

    def forward_u16(self, f0, f1, t=0.5, depth=10, scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """``forward_u8`` on 16-bit frames: uint16 ``[N,H0,W0,3]`` RGB samples of ``depth`` 9..16 (in
        the words' low bits; a word above ``maxval = 2**depth - 1`` is read as maxval) in and out on
        the device; bit for bit ``convert.frames_u16_to_float`` -> ``forward`` ->
        ``convert.frames_float_to_u16`` (``RRINEngine.forward_u16``).  Inference-only; not for
        ``precision='fp32_planar'``.  The scene gate is ``forward_u8``'s with ``scene_threshold`` a
        mean absolute sample difference in [0, maxval]."""
        return self._frames("u16", f0, f1, t, False, depth=depth, scene_threshold=scene_threshold, gate=gate,
                            flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_u16(self, f0, f1, ts, depth=10, scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """``[forward_u16(f0, f1, t, depth) for t in ts]`` with the Flow U-Net (and the pairs' sums
        of absolute differences) computed once, as :meth:`interpolate_u8`."""
        return self._frames("u16", f0, f1, ts, True, depth=depth, scene_threshold=scene_threshold, gate=gate,
                            flow_scale=flow_scale, **_plane_kw(plane))

    def pair_stats_u16(self, f0, f1, depth=10):
        """int64 device tensor ``[N]``: the exact sum of absolute sample differences (samples
        ``min(word, maxval)``) of every pair of two uint16 ``[N,H0,W0,3]`` stacks."""
        return self.engine().pair_stats_u16(f0, f1, depth=depth)

    def forward_yuv16(self, f0, f1, t=0.5, layout="nv12", depth=10, msb=False, coef=None, scene_threshold=None,
                      gate=None, flow_scale=1, plane=None):
        """``forward_yuv`` on 10- or 12-bit 4:2:0 frames in 16-bit words: uint16 ``[N, 3*H0//2, W0]`` in
        and out on the device, ``msb=False`` for samples in the low bits (yuv420p10le, Y4M C420p10),
        ``True`` for the high bits (P010 / P012).  By definition, and bit for bit,
        ``yuv.rgb16_to_yuv420(forward_u16(yuv.yuv420_to_rgb16(f0), yuv.yuv420_to_rgb16(f1), t,
        depth))`` (``RRINEngine.forward_yuv16``); ``coef`` None is BT.709 limited range at this
        depth.  Other depths raise.  Inference-only; not for ``precision='fp32_planar'``."""
        return self._frames("yuv16", f0, f1, t, False, layout=layout, depth=depth, msb=msb, coef=coef,
                            scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_yuv16(self, f0, f1, ts, layout="nv12", depth=10, msb=False, coef=None, scene_threshold=None,
                          gate=None, flow_scale=1, plane=None):
        """``[forward_yuv16(f0, f1, t, ...) for t in ts]`` with the Flow U-Net (and the pairs' sums of
        absolute differences) computed once, as :meth:`interpolate_yuv`."""
        return self._frames("yuv16", f0, f1, ts, True, layout=layout, depth=depth, msb=msb, coef=coef,
                            scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def pair_stats_yuv16(self, f0, f1, depth=10, msb=False, layout="nv12"):
        """int64 device tensor ``[N]``: the exact sum of absolute differences of the samples
        ``min(word >> shift, maxval)``, luma and chroma, of every pair of two uint16 4:2:0 stacks."""
        return self.engine().pair_stats_yuv16(f0, f1, depth=depth, msb=msb, layout=layout)

    # ---- frame metrics: how good an output is, measured where the frames live ---------------
    def frame_metrics_u8(self, a, b, ssim=True):
        """Squared error, PSNR and SSIM per frame and channel of two uint8 ``[N,H0,W0,3]`` device
        stacks -- ``a`` typically a forward's output, ``b`` the truth frames (a device
        ``index_select`` of them is fine) -- as :mod:`rrin_amd.metrics` defines them: a
        ``metrics.FrameMetrics`` of device tensors (``sse`` exact, ``ssim``, ``psnr()``), computed
        by one kernel pass on the forward's stream without a host sync (``RRINEngine.frame_metrics_u8``)."""
        return self.engine().frame_metrics_u8(a, b, ssim=ssim)

    def frame_metrics_yuv(self, a, b, layout="nv12", ssim=True):
        """:meth:`frame_metrics_u8` per Y, U and V plane of two uint8 YUV stacks of ``layout``."""
        return self.engine().frame_metrics_yuv(a, b, layout=layout, ssim=ssim)

    def frame_metrics_u16(self, a, b, depth=10, ssim=True):
        """:meth:`frame_metrics_u8` for uint16 RGB stacks of ``depth`` 9..16 (samples ``min(word, maxval)``)."""
        return self.engine().frame_metrics_u16(a, b, depth=depth, ssim=ssim)

    def frame_metrics_yuv16(self, a, b, layout="nv12", depth=10, msb=False, ssim=True):
        """:meth:`frame_metrics_yuv` for uint16 stacks of ``depth`` 9..16; ``msb`` as in :meth:`forward_yuv16`."""
        return self.engine().frame_metrics_yuv16(a, b, layout=layout, depth=depth, msb=msb, ssim=ssim)

    # ---- item forwards: a batch of (pair index, t) over one frame stack ----------------------
    def _items(self, name, frames, pair, t, **kw):
        """The item forward ``name`` of the engine, after the host checks of ``pair`` and ``t``
        (ValueError before any device work)."""
        from .engine import check_items
        from .flowscale import check_flow_scale
        if not isinstance(frames, torch.Tensor) or frames.dim() < 1:
            raise TypeError(f"{name} takes one stack of frames")
        check_items(pair, t, frames.shape[0] - 1)
        check_flow_scale(kw.get("flow_scale", 1))
        if torch.is_grad_enabled():
            raise RuntimeError(f"rrin_amd.Net.{name} is inference-only: use torch.no_grad()")
        return getattr(self.engine(), name)(frames, pair, t, streams=self.streams, **kw)

    def interpolate_items_u8(self, frames, pair, t, scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """A batch of M items over one stack of 8-bit frames, for frame-rate conversion
        (:mod:`rrin_amd.retime`): ``frames`` uint8 ``[P+1,H0,W0,3]`` on the device (pair p is
        ``frames[p]``, ``frames[p+1]``), ``pair`` M non-decreasing ints in [0, P) (list or int32
        tensor), ``t`` M floats in [0, 1) (list or fp32 tensor) -> uint8 ``[M,H0,W0,3]``.  By
        definition, and bit for bit, ``out[k] == forward_u8(frames[pair[k]:pair[k]+1],
        frames[pair[k]+1:pair[k]+2], t=t[k])[0]``; the Flow U-Net runs once per distinct pair, the
        other three U-Nets once per item (``RRINEngine.interpolate_items_u8``).

        With ``scene_threshold`` or ``gate`` (int32 ``[P]`` pair codes: 1 duplicate, 2 cut) an item
        inherits its pair's decision: a duplicate returns the first frame, a cut the nearer frame
        by the item's own t; :attr:`last_gate` is then ``[M]``.  Output quality at uneven t has not
        been validated on footage."""
        return self._items("interpolate_items_u8", frames, pair, t, scene_threshold=scene_threshold, gate=gate,
                           flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_items_yuv(self, frames, pair, t, layout="nv12", coef=None, scene_threshold=None, gate=None,
                              flow_scale=1, plane=None):
        """:meth:`interpolate_items_u8` on one stack of 8-bit YUV frames, defined by
        :meth:`forward_yuv` with the same ``layout`` and ``coef``."""
        return self._items("interpolate_items_yuv", frames, pair, t, layout=layout, coef=coef,
                           scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_items_u16(self, frames, pair, t, depth=10, scene_threshold=None, gate=None, flow_scale=1,
                              plane=None):
        """:meth:`interpolate_items_u8` on uint16 RGB frames of ``depth``, defined by :meth:`forward_u16`."""
        return self._items("interpolate_items_u16", frames, pair, t, depth=depth, scene_threshold=scene_threshold,
                           gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    def interpolate_items_yuv16(self, frames, pair, t, layout="nv12", depth=10, msb=False, coef=None,
                                scene_threshold=None, gate=None, flow_scale=1, plane=None):
        """:meth:`interpolate_items_yuv` on 10- or 12-bit frames in 16-bit words, defined by
        :meth:`forward_yuv16` with the same ``layout``, ``depth``, ``msb`` and ``coef``."""
        return self._items("interpolate_items_yuv16", frames, pair, t, layout=layout, depth=depth, msb=msb, coef=coef,
                           scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, **_plane_kw(plane))

    # ---- exposures: the mean of S samples over a shutter window (rrin_amd.exposure) -----------
    def _expose(self, name, frames, groups, chunk, **kw):
        """The exposure ``name`` of the engine, after the host checks of ``groups`` and ``chunk``
        (TypeError / ValueError before any device work)."""
        from . import exposure
        from .flowscale import check_flow_scale
        if not isinstance(frames, torch.Tensor) or frames.dim() < 1:
            raise TypeError(f"{name} takes one stack of frames")
        checked = exposure.check_groups(groups, frames.shape[0] - 1)
        exposure.chunks(checked, chunk)
        check_flow_scale(kw.get("flow_scale", 1))
        if kw.get("light") is not None or kw.get("weights") is not None:
            from . import transfer
            exposure.group_weights(kw.get("weights"), [len(group) for group in checked])
            depth = kw.get("depth", 8) if name.endswith("16") else 8
            if kw.get("light") is not None:
                if isinstance(depth, int) and not isinstance(depth, bool) and 12 < depth <= 16:
                    raise ValueError(f"{name}: light needs a depth of at most 12 bits, got {depth}: a table of "
                                     f"2**{depth} entries and its thresholds would not fit in LDS")
                transfer.table_key(kw["light"], depth)
        if torch.is_grad_enabled():
            raise RuntimeError(f"rrin_amd.Net.{name} is inference-only: use torch.no_grad()")
        return getattr(self.engine(), name)(frames, groups, chunk, streams=self.streams, **kw)

    def expose_items_u8(self, frames, groups, chunk=4, scene_threshold=None, gate=None, flow_scale=1, plane=None,
                        light=None, weights=None):
        """``G`` exposed frames over one stack of 8-bit frames: a synthetic shutter
        (:mod:`rrin_amd.exposure` is the definition, :func:`rrin_amd.retime.exposure_schedule` makes the
        groups of a frame-rate conversion).  ``frames`` uint8 ``[P+1,H0,W0,3]`` on the device, ``groups`` a
        list of ``G`` lists of 1..256 samples ``(pair, t)`` with non-decreasing times, ``pair`` in [0, P]
        (``P`` only with ``t == 0``), ``t`` in [0, 1) -> uint8 ``[G,H0,W0,3]``.  A ``t == 0`` sample is
        ``frames[pair]``, never sent to the network; any other is item ``(pair, t)`` of
        :meth:`interpolate_items_u8` with the same keywords, run ``chunk`` items at a time (``chunk``
        changes no bit).  Output g is ``((sum of its samples) + S // 2) // S`` per byte: a mean over code
        values, no transfer function.  With ``scene_threshold`` or ``gate`` the items inherit their pair's
        decision and :attr:`last_gate` is the ``[M]`` codes of the call's network items in order; an
        exposure across a cut mixes both shots.  ``plane``: one ``[P+1,H0,W0]`` stack; the call returns
        ``(frames, plane)``.

        ``light`` names the material's transfer curve (``"srgb"``, ``"bt1886"``, ``"gamma22"``, ``"pq"``,
        ``"hlg"``, or a table: :mod:`rrin_amd.transfer`): the mean is then taken in linear light, ``enc((sum_k
        w_k lin[s_k] + W // 2) // W)`` per element (on YUV per pixel and channel of the RGB between the
        path's two conversions).  ``weights`` (``"box"``, ``"triangle"`` or a list of ints, sum at most 65535)
        weighs the samples; the plane is then the weighted mean of its code values, never through the
        table.  Both are checked before any device work; with both None the call is what it was."""
        return self._expose("expose_items_u8", frames, groups, chunk, scene_threshold=scene_threshold, gate=gate,
                            flow_scale=flow_scale, light=light, weights=weights,
                            **_plane_kw(plane))

    def expose_items_yuv(self, frames, groups, chunk=4, layout="nv12", coef=None, scene_threshold=None, gate=None,
                         flow_scale=1, plane=None, light=None,
                         weights=None):
        """:meth:`expose_items_u8` on one stack of 8-bit YUV frames over :meth:`interpolate_items_yuv`;
        every stored byte, chroma included, is averaged."""
        return self._expose("expose_items_yuv", frames, groups, chunk, layout=layout, coef=coef,
                            scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale, light=light,
                            weights=weights, **_plane_kw(plane))

    def expose_items_u16(self, frames, groups, chunk=4, depth=10, scene_threshold=None, gate=None, flow_scale=1,
                         plane=None, light=None,
                         weights=None):
        """:meth:`expose_items_u8` on uint16 RGB frames of ``depth`` over :meth:`interpolate_items_u16`."""
        return self._expose("expose_items_u16", frames, groups, chunk, depth=depth, scene_threshold=scene_threshold,
                            gate=gate, flow_scale=flow_scale, light=light, weights=weights,
                            **_plane_kw(plane))

    def expose_items_yuv16(self, frames, groups, chunk=4, layout="nv12", depth=10, msb=False, coef=None,
                           scene_threshold=None, gate=None, flow_scale=1, plane=None, light=None,
                           weights=None):
        """:meth:`expose_items_yuv` on 10- or 12-bit frames in 16-bit words over
        :meth:`interpolate_items_yuv16`: a sample is ``min(word >> shift, maxval)``, stored ``<< shift``."""
        return self._expose("expose_items_yuv16", frames, groups, chunk, layout=layout, depth=depth, msb=msb,
                            coef=coef, scene_threshold=scene_threshold, gate=gate, flow_scale=flow_scale,
                            light=light, weights=weights,
                            **_plane_kw(plane))

    @property
    def last_gate(self):
        """The int32 device codes ``[N]`` of the last gated ``forward_u8`` (0: interpolated, 1:
        ``f0``'s frame, 2: ``f1``'s), or None; with ``scene_threshold`` a cached buffer that the
        next gated call overwrites (stream-ordered): clone it to keep it."""
        return self._engine.last_gate if self._engine is not None else None

    def forward(self, input0, input1, t=0.5):
        if torch.is_grad_enabled() and (input0.requires_grad or input1.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            if input0.is_cuda:
                from .autograd import net_forward
                return net_forward(self, input0, input1, t)
            return self._forward_autograd(input0, input1, t)
        return self.engine().forward(input0, input1, t, streams=self.streams)

    @staticmethod
    def _backwarp(img, flow):
        """model.py:8-21 with the grid built on the image's device (the reference
        hard-codes .cuda())."""
        n, _, h, w = img.shape
        gy, gx = torch.meshgrid(torch.arange(h, device=img.device), torch.arange(w, device=img.device),
                                indexing="ij")
        x = gx.unsqueeze(0).expand(n, h, w).float() + flow[:, 0]
        y = gy.unsqueeze(0).expand(n, h, w).float() + flow[:, 1]
        grid = torch.stack((2 * (x / w - 0.5), 2 * (y / h - 0.5)), dim=3)
        return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)

    def _forward_autograd(self, input0, input1, t=0.5):
        """Training path on a CPU device (autograd on): model.py:32-65 with PyTorch operators."""
        x = torch.cat((input0, input1), 1)
        flow = self.Flow(x)
        f01, f10 = flow[:, :2], flow[:, 2:4]
        ft0 = -(1 - t) * t * f01 + t * t * f10
        ft1 = (1 - t) * (1 - t) * f01 - t * (1 - t) * f10
        r = self.refine_flow(torch.cat((ft0, ft1, x), 1))
        ft0 = ft0 + r[:, :2]
        ft1 = ft1 + r[:, 2:4]
        xt1 = self._backwarp(input0, ft0)
        xt2 = self._backwarp(input1, ft1)
        m = torch.sigmoid(self.Mask(torch.cat((ft0, ft1, x, xt1, xt2), 1)))
        w1, w2 = (1 - t) * m[:, 0:1], t * m[:, 1:2]
        out = (w1 * xt1 + w2 * xt2) / (w1 + w2 + 1e-8)
        return (self.final(torch.cat((input0, input1, out), 1)) + out).clamp(0, 1)
