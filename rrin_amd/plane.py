"""An extra plane through the byte-frame forwards: the ``plane=`` keyword (the definition).

``Net.forward`` (model.py:32-65) with one more single-channel image per input frame.  ``A0``, ``A1``
are float tensors ``[N,1,H,W]`` in [0, 1], padded exactly as the frames are.  With the reference
model's own names:

    at0 = warp(A0, Flow_t_0)        # the refined flows: after "+ Flow_t[:, :2]" / "+ Flow_t[:, 2:4]"
    at1 = warp(A1, Flow_t_1)        # the picture's warp: bilinear, zeros outside, align_corners=False
    A_t = ((w1 * at0 + w2 * at1) / (w1 + w2 + 1e-8)).clamp(0, 1)    # w1, w2: the picture's mask weights

so the plane moves with the motion that the network estimated from the picture and is blended with
the picture's occlusion mask.  The ``final`` U-Net and its residual do not touch it.

Three things to know:

* RGB is taken as stored: the picture is neither premultiplied nor unpremultiplied by the plane.
* The plane need not be a matte; a depth or an ID plane goes the same way (but is blended, not
  selected: values between two IDs appear where both inputs contribute).
* No claim about quality is made.

The byte form follows the byte paths' own rules (``convert.frames_u8_to_float`` /
``frames_float_to_u8`` and their u16 twins, applied to one channel): edge replication on top and on the
right up to the pad multiple ``16 * flow_scale``, ``/ maxval`` on the way in (:func:`plane_to_float`),
``q * maxval`` truncated toward zero and the crop on the way out (:func:`float_to_plane`).  For 16-bit
words a sample is ``min(word >> shift, maxval)`` and is stored ``<< shift``, as on the u16 and yuv16
paths.

On the device (include/rrin_hip.h, csrc/plane.hip): ``rrin_plane_warp_h8`` behind the REFINE head --
it reads the refined flows as the Net buffer's record format stores them, so at fp16 they are the
fp16-rounded flows -- and ``rrin_plane_blend_h8`` behind the MASK head.  Two launches, because the MASK
head overwrites the Net buffer's channels 6-8 with its blend: the refined flows are gone when the mask
is known.

Not covered: ``NetGraph`` capture, ``precision="fp32_planar"``, the float ``Net.forward``, the autograd
/ fine-tune path, multi-GPU sharding, Y4M alpha tags, sub-sampled planes.

Host only: plain torch, nothing here touches a device or loads the library.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .convert import pad_amounts


def check_format(depth: int = 8, shift: int = 0):
    """(dtype, maxval) of a plane of ``depth`` 8 (uint8) or 9..16 (uint16 words, the sample ``shift`` bits up)."""
    if isinstance(depth, bool) or not isinstance(depth, int) or not 8 <= depth <= 16:
        raise ValueError(f"a plane is 8 to 16 bits deep, got {depth!r}")
    if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift <= (16 - depth if depth > 8 else 0):
        raise ValueError(f"shift must be an int in 0..{16 - depth if depth > 8 else 0} at depth {depth}, got {shift!r}")
    return (torch.uint8 if depth == 8 else torch.uint16), (1 << depth) - 1


def samples(plane: torch.Tensor, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """The int32 samples of a uint8 / uint16 plane stack: ``min(word >> shift, maxval)``."""
    dtype, maxval = check_format(depth, shift)
    if plane.dtype != dtype:
        raise TypeError(f"a plane of depth {depth} is {str(dtype).split('.')[-1]}, got {plane.dtype}")
    if depth == 8:
        return plane.to(torch.int32)
    return ((plane.view(torch.int16).to(torch.int32) & 0xFFFF) >> shift).clamp_(max=maxval)


def plane_to_float(plane: torch.Tensor, depth: int = 8, shift: int = 0, flow_scale: int = 1) -> torch.Tensor:
    """The input mapping: ``[..., H0, W0]`` uint8 / uint16 -> float32 ``[..., 1, H, W]``, H and W the next
    multiples of ``16 * flow_scale``, edge-replicated on top and on the right (padded pixel (y, x) reads
    sample (max(y - top, 0), min(x, W0 - 1))), ``sample.float() / float(maxval)``."""
    _, maxval = check_format(depth, shift)
    h0, w0 = plane.shape[-2], plane.shape[-1]
    top, right = pad_amounts(w0, h0, flow_scale)
    rows = (torch.arange(h0 + top, device=plane.device) - top).clamp_(min=0)
    cols = torch.arange(w0 + right, device=plane.device).clamp_(max=w0 - 1)
    x = samples(plane, depth, shift).index_select(-2, rows).index_select(-1, cols)
    return x.unsqueeze(-3).float().div_(float(maxval))


def float_to_plane(a: torch.Tensor, height: int, width: int, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """The output mapping: float ``[..., 1, H, W]`` in [0, 1] -> ``[..., height, width]`` of the plane's
    dtype: the crop (rows ``[H - height, H)``, columns ``[0, width)``), ``a * float(maxval)`` in fp32
    truncated toward zero, stored ``<< shift``."""
    dtype, maxval = check_format(depth, shift)
    top = a.shape[-2] - height
    q = a[..., 0, top:top + height, :width].float().mul(float(maxval)).to(torch.int32) << shift
    return q.to(torch.uint8) if depth == 8 else q.to(torch.int16).view(torch.uint16)


def warp(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """model.py:8-21 in the dtype of ``img``: grid ``2 ((gx + u) / W - 0.5)``, ``grid_sample(bilinear,
    zeros, align_corners=False)``."""
    flow = flow.to(img.dtype)
    n, _, h, w = img.shape
    gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    x = gx.unsqueeze(0).expand(n, h, w).to(img.dtype) + flow[:, 0]
    y = gy.unsqueeze(0).expand(n, h, w).to(img.dtype) + flow[:, 1]
    grid = torch.stack((2 * (x / w - 0.5), 2 * (y / h - 0.5)), dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def _times(t, n: int) -> torch.Tensor:
    tt = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
    tt = tt.expand(n) if tt.numel() == 1 else tt
    if tt.numel() != n:
        raise ValueError(f"t must be one value or {n}, got {tt.numel()}")
    return tt.view(n, 1, 1, 1)


def refined_flows(taps, t):
    """(Flow_t_0, Flow_t_1) in float64 from a forward's intermediates ``taps``: its ``ft0`` / ``ft1``
    (``oracle.ref_net.net_forward``'s names for the refined flows) where present, else from the raw
    outputs ``Flow`` and ``refine_flow`` (``refine``) of the two U-Nets, as ``Net.forward(taps=)`` gives
    them: model.py:38-39 and 44-45."""
    if "ft0" in taps and "ft1" in taps:
        return taps["ft0"].double(), taps["ft1"].double()
    flow = taps["Flow"].double()
    r = (taps["refine_flow"] if "refine_flow" in taps else taps["refine"]).double()
    tt = _times(t, flow.shape[0])
    f01, f10 = flow[:, 0:2], flow[:, 2:4]
    ft0 = -(1 - tt) * tt * f01 + tt * tt * f10
    ft1 = (1 - tt) * (1 - tt) * f01 - tt * (1 - tt) * f10
    return ft0 + r[:, 0:2], ft1 + r[:, 2:4]


def reference(taps, a0: torch.Tensor, a1: torch.Tensor, t=0.5) -> torch.Tensor:
    """``A_t`` ``[N,1,H,W]`` in float64: the definition of the module docstring on padded float planes
    ``a0`` / ``a1`` ``[N,1,H,W]``, the refined flows of :func:`refined_flows` and the mask logits
    ``taps["mask_logits"]`` (``taps["Mask"]``) of the same forward; ``t`` one value or one per image."""
    ft0, ft1 = refined_flows(taps, t)
    logits = (taps["mask_logits"] if "mask_logits" in taps else taps["Mask"]).double()
    tt = _times(t, a0.shape[0])
    at0 = warp(a0.double(), ft0)
    at1 = warp(a1.double(), ft1)
    m = torch.sigmoid(logits)
    w1, w2 = (1 - tt) * m[:, 0:1], tt * m[:, 1:2]
    return ((w1 * at0 + w2 * at1) / (w1 + w2 + 1e-8)).clamp(0, 1)


def reference_plane(taps, p0: torch.Tensor, p1: torch.Tensor, t=0.5, depth: int = 8, shift: int = 0,
                    flow_scale: int = 1):
    """The byte form: planes ``[N,H0,W0]`` in, ``(stored, value)`` out -- ``stored`` ``[N,H0,W0]`` of the
    planes' dtype as a forward with ``plane=(p0, p1)`` defines it, ``value`` the float64 ``A_t`` of the
    crop before the quantisation (``stored == (value * maxval).trunc() << shift`` up to fp32 rounding)."""
    h0, w0 = p0.shape[-2], p0.shape[-1]
    a = reference(taps, plane_to_float(p0, depth, shift, flow_scale), plane_to_float(p1, depth, shift, flow_scale), t)
    top = a.shape[-2] - h0
    return float_to_plane(a, h0, w0, depth, shift), a[:, 0, top:top + h0, :w0]


def check_planes(plane, n_frames: int, h0: int, w0: int, dtype, device, items: bool):
    """The ``plane=`` argument of a forward of ``n_frames`` pairs (items: a stack of ``n_frames + 1``
    frames) of H0 x W0 frames of ``dtype`` on ``device``: ``(a0, a1)`` stacks ``[n_frames, H0, W0]``,
    TypeError / ValueError otherwise -- before the device is touched."""
    name = str(dtype).split(".")[-1]
    if items:
        if not isinstance(plane, torch.Tensor):
            raise TypeError(f"plane= of an item forward is one {name} stack [P+1,H0,W0]")
        pair = (plane[:-1], plane[1:]) if plane.dim() == 3 and plane.shape[0] == n_frames + 1 else None
        if pair is None:
            raise ValueError(f"plane= must be [{n_frames + 1},{h0},{w0}], got {tuple(plane.shape)}")
    else:
        if (not isinstance(plane, (tuple, list)) or len(plane) != 2
                or not all(isinstance(p, torch.Tensor) for p in plane)):
            raise TypeError(f"plane= is a pair (a0, a1) of {name} stacks [N,H0,W0]")
        pair = tuple(plane)
    for p in pair:
        if p.dtype != dtype:
            raise TypeError(f"plane= takes {name} planes, the frames' dtype, got {p.dtype}")
        if tuple(p.shape) != (n_frames, h0, w0):
            raise ValueError(f"plane= stacks must be [{n_frames},{h0},{w0}] (no sub-sampled planes), got "
                             f"{tuple(p.shape)}")
        if p.device != torch.device(device):
            raise ValueError(f"plane= on {p.device}, frames on {device}")
    return pair
