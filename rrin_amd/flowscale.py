"""Low-resolution flow estimation: the ``flow_scale`` knob of every forward (the definition).

Let ``s`` be 1, 2 or 4.  ``Net_s(I0, I1, t)`` is ``model.py``'s ``forward`` with one line replaced:

    Flow = self.Flow(x)

becomes

    Flow = s * F.interpolate(self.Flow(F.avg_pool2d(x, s)), scale_factor=s, mode="bilinear",
                             align_corners=False)

Everything after that line is unchanged and runs at full size: the t-blend, ``refine_flow``, both
warps, ``Mask`` and ``final``.  ``s = 1`` is the plain forward, bit for bit (nothing new is
launched).  The Flow U-Net (depth 5, the largest of the four) then sees the motion of a large
frame at 1/s of its size in pixels, and costs about 1/s^2.

Padding: the padded size (H, W) of a frame path is the frame size rounded up to a multiple of
``16 * s`` (:func:`padded_size`), edge-replicated on top and on the right exactly as for 16, so
that (H/s, W/s) is again a multiple of 16 (the Flow U-Net pools four times).  The float path takes
tensors whose H and W are already such multiples.

On the device (include/rrin_hip.h, csrc/flow_scale.hip) the two new steps are
``rrin_g16_downscale_h8`` (the ``F.avg_pool2d(x, s)``: fp32 sums in raster order of the s x s block,
times 1/s^2) and ``rrin_flow_upscale_h8`` (the ``s * F.interpolate(...)``: source coordinate
``(dst + 0.5)/s - 0.5`` clamped to the image, exact dyadic weights, ``v = (1-wy)*((1-wx)*p00 +
wx*p01) + wy*((1-wx)*p10 + wx*p11)`` with every operation rounded to fp32, then ``* s``), both
stored with the record format's rounding; the Flow U-Net between them runs on a second plan at
(H/s, W/s) with its own workspace, conv table and scratch.  After the upscale the forward continues
on the path of a kept raw Flow (``reuse_flow``): Ft0 / Ft1 are blended from the stored raw Flow.

Not covered: ``NetGraph`` capture (eager only, like ``reuse_flow``), the autograd / fine-tune path,
multi-GPU sharding, the ``fp32_planar`` precision.  No claim about quality is made: judge the knob
on your own footage with ``python -m rrin_amd evaluate --flow_scale``.
"""
from __future__ import annotations

FLOW_SCALES = (1, 2, 4)


def check_flow_scale(flow_scale) -> int:
    """``flow_scale`` as an int in FLOW_SCALES; anything else (bools and floats included) raises
    ValueError -- before any device work."""
    if isinstance(flow_scale, bool) or not isinstance(flow_scale, int) or flow_scale not in FLOW_SCALES:
        raise ValueError(f"flow_scale must be one of {FLOW_SCALES}, got {flow_scale!r}")
    return flow_scale


def pad_multiple(flow_scale: int = 1) -> int:
    """The multiple a frame's size is padded to: 16 * s."""
    return 16 * check_flow_scale(flow_scale)


def padded_size(h0: int, w0: int, flow_scale: int = 1):
    """(H, W): the frame size rounded up to a multiple of 16 * s (720 -> 720 / 736 / 768 for
    s = 1 / 2 / 4; 2160 -> 2160 / 2176 / 2176)."""
    m = pad_multiple(flow_scale)
    return (h0 + m - 1) // m * m, (w0 + m - 1) // m * m


def flow_tag(tag: str, flow_scale: int = 1) -> str:
    """The tag of the raw Flow a workspace keeps after a forward of path ``tag`` at this scale: the
    path's own tag at s = 1, ``tag|s2`` / ``tag|s4`` otherwise, so ``reuse_flow`` never takes the
    Flow of another scale for its own (at s > 1 the kept Flow is the upscaled one)."""
    s = check_flow_scale(flow_scale)
    return tag if s == 1 else f"{tag}|s{s}"
