"""PSNR and SSIM of frames as the frame paths emit them -- 8-bit and 16-bit RGB, YUV of any layout --
and the hold-out schedule of ``convert.evaluate_y4m``.

As with :mod:`rrin_amd.yuv`, the functions here are the *definition*: integer arithmetic wherever
possible, float64 for the rest, so the same numbers on any host.  On CPU tensors the public
``frame_metrics_*`` functions run them; on device tensors ``csrc/metrics.hip`` computes the same
without the frames leaving the device (the squared error bit for bit, SSIM up to the order of
one float64 sum).

Planes.  A plane of a frame is ``(off, step, pitch, h, w)``: sample ``(r, c)`` sits at element
``off + r*pitch + c*step`` of the frame, an element being a byte (8-bit frames) or a 16-bit word.
:func:`planes_of` gives the planes of every frame kind.

Samples.  8-bit frames are read as the byte; 16-bit ones as ``min(word >> shift, maxval)``, the
rule of ``rrin_pair_sad_u16``.  No transfer function is applied: the metrics are on code values,
like the network.

SSE.  The sum of squared sample differences over a plane, exact.  ``psnr = 10*log10(maxval^2 *
count / sse)``, ``inf`` at ``sse == 0``.

SSIM.  The 8x8-window, 4-sample-step form of x264 and ffmpeg's ``ssim`` filter, for planes X, Y
with ``h, w >= 8`` and ``M = maxval``:

* ``bh = h // 4``, ``bw = w // 4``; samples beyond ``4*bh``, ``4*bw`` take no part;
* per 4x4 block the integers ``s1 = sum X``, ``s2 = sum Y``, ``ss = sum X^2 + sum Y^2``, ``s12 = sum XY``;
* window ``(i, j)``, ``0 <= i < bh-1``, ``0 <= j < bw-1``, adds the blocks ``(i..i+1, j..j+1)`` to
  ``S1, S2, SS, S12``;
* ``vars = 64*SS - S1^2 - S2^2``, ``covar = 64*S12 - S1*S2`` (int64);
* ``C1 = floor(1e-4 * M^2 * 64 + 0.5)``, ``C2 = floor(9e-4 * M^2 * 64 * 63 + 0.5)`` (416 and 235963 at
  M = 255);
* ``v = ((2*S1*S2 + C1) * (2*covar + C2)) / ((S1^2 + S2^2 + C1) * (vars + C2))``: the four factors
  are exact integers below 2^53, converted to float64; one product above, one below, one division;
* the plane's SSIM is the mean of ``v`` over its ``(bh-1)*(bw-1)`` windows, in float64.

For ``X == Y`` every ``v`` is exactly 1.0, and the denominator is at least ``C1*C2 > 0``.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import torch

from . import yuv
from .framefmt import FrameFormat, check_depth, frame_stride

RGB_NAMES = ("r", "g", "b")
YUV_NAMES = ("y", "u", "v")


# ---- planes ----------------------------------------------------------------------------------
def planes_of(kind: str, h0: int, w0: int, layout=None) -> list:
    """The planes ``(off, step, pitch, h, w)`` of an H0 x W0 frame: ``kind`` "rgb" (``[H0,W0,3]``
    interleaved: three planes), "y" (one ``[H0,W0]`` plane) or "yuv" with a ``layout`` of
    :data:`rrin_amd.yuv.ALL_LAYOUTS` (the dense stacks of :mod:`rrin_amd.yuv`: Y, U, V)."""
    h0, w0 = int(h0), int(w0)
    if h0 < 1 or w0 < 1:
        raise ValueError(f"empty frame: {h0}x{w0}")
    if kind == "rgb":
        return [(ch, 3, 3 * w0, h0, w0) for ch in range(3)]
    if kind == "y":
        return [(0, 1, w0, h0, w0)]
    if kind != "yuv":
        raise ValueError(f"kind must be 'rgb', 'y' or 'yuv', got {kind!r}")
    yuv.check_size(h0, w0, layout)
    by, bx = yuv.block_of(yuv.chroma_of(layout))
    ch, cw = h0 // by, w0 // bx
    base = h0 * w0
    if layout in ("nv12", "nv16"):
        return [(0, 1, w0, h0, w0), (base, 2, 2 * cw, ch, cw), (base + 1, 2, 2 * cw, ch, cw)]
    return [(0, 1, w0, h0, w0), (base, 1, cw, ch, cw), (base + ch * cw, 1, cw, ch, cw)]


def gather_plane(frames: torch.Tensor, plane) -> torch.Tensor:
    """``[N,h,w]`` elements of a plane of a stack of dense frames (any trailing shape), through the map."""
    if frames.dtype == torch.uint16:  # indexed as the same bits
        return gather_plane(frames.view(torch.int16), plane).view(torch.uint16)
    off, step, pitch, h, w = plane
    flat = frames.reshape(frames.shape[0], -1)
    idx = (off + torch.arange(h, device=frames.device).view(h, 1) * pitch
           + torch.arange(w, device=frames.device).view(1, w) * step)
    return flat[:, idx.reshape(-1)].reshape(frames.shape[0], h, w)


def samples_of(x: torch.Tensor, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """int64 samples of uint8 elements, or of uint16 words read as ``min(word >> shift, maxval)``."""
    if x.dtype == torch.uint8:
        return x.to(torch.int64)
    if x.dtype != torch.uint16:
        raise TypeError("frames are uint8 or uint16")
    return (yuv.words_to_int(x).to(torch.int64) >> shift).clamp_(max=(1 << depth) - 1)


# ---- the definitions ---------------------------------------------------------------------------
def ssim_constants(maxval: int):
    """(C1, C2) of the integer SSIM at ``maxval``."""
    m2 = float(int(maxval) * int(maxval))
    return math.floor(1e-4 * m2 * 64.0 + 0.5), math.floor(9e-4 * m2 * 64.0 * 63.0 + 0.5)


def plane_sse(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """int64 ``[...]``: the sum of squared differences of int64 sample planes ``[..., h, w]``."""
    d = x - y
    return (d * d).sum(dim=(-2, -1))


def window_values(x: torch.Tensor, y: torch.Tensor, maxval: int) -> torch.Tensor:
    """float64 ``[..., bh-1, bw-1]``: the value of every window of int64 sample planes ``[..., h, w]``."""
    h, w = x.shape[-2], x.shape[-1]
    if h < 8 or w < 8:
        raise ValueError(f"SSIM needs planes of at least 8x8 samples, got {h}x{w}")
    bh, bw = h // 4, w // 4
    lead = x.shape[:-2]

    def blocks(a):
        return a[..., :4 * bh, :4 * bw].reshape(*lead, bh, 4, bw, 4).sum(dim=(-3, -1))

    def windows(s):
        return s[..., :-1, :-1] + s[..., 1:, :-1] + s[..., :-1, 1:] + s[..., 1:, 1:]

    s1, s2 = windows(blocks(x)), windows(blocks(y))
    ss, s12 = windows(blocks(x * x + y * y)), windows(blocks(x * y))
    c1, c2 = ssim_constants(maxval)
    var, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    num = (2 * s1 * s2 + c1).double() * (2 * covar + c2).double()
    den = (s1 * s1 + s2 * s2 + c1).double() * (var + c2).double()
    return num / den


def plane_ssim(x: torch.Tensor, y: torch.Tensor, maxval: int) -> torch.Tensor:
    """float64 ``[...]``: the mean window value of int64 sample planes ``[..., h, w]``."""
    v = window_values(x, y, maxval)
    return v.reshape(*v.shape[:-2], -1).mean(dim=-1)


def psnr(sse, count, maxval):
    """``10*log10(maxval^2 * count / sse)`` in float64, ``inf`` at ``sse == 0``: a float for an int
    ``sse``, a float64 tensor on its device for a tensor (``count`` an int)."""
    peak = float(int(maxval) * int(maxval) * int(count))
    if isinstance(sse, torch.Tensor):
        return 10.0 * torch.log10(peak / sse.double())
    return math.inf if int(sse) == 0 else 10.0 * math.log10(peak / float(int(sse)))


class FrameMetrics:
    """What ``frame_metrics_*`` return: ``sse`` int64 ``[N,P]``, ``ssim`` float64 ``[N,P]`` or None,
    ``count`` (samples per plane, P ints), ``maxval`` and ``plane_names``; tensors on the frames' device."""

    def __init__(self, sse, ssim, count, maxval, plane_names):
        self.sse, self.ssim, self.count, self.maxval, self.plane_names = sse, ssim, tuple(count), maxval, plane_names

    def psnr(self) -> torch.Tensor:
        """float64 ``[N,P]`` on the same device; no copy to the host, nothing synchronises."""
        return torch.stack([psnr(self.sse[:, p], c, self.maxval) for p, c in enumerate(self.count)], dim=1)


def _check_pair(a, b, dtype, dims):
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
        raise TypeError("frame metrics take two tensors")
    if a.dtype != dtype or b.dtype != dtype:
        raise TypeError(f"expected two {str(dtype).split('.')[-1]} stacks, got {a.dtype} / {b.dtype}")
    if a.dim() != dims or a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f"expected two equal stacks of {dims} dimensions, got {tuple(a.shape)} / {tuple(b.shape)}")
    if a.device != b.device:
        raise RuntimeError(f"frames on {a.device} / {b.device}")


def _host_metrics(a, b, planes, depth, shift, ssim):
    maxval = (1 << depth) - 1
    sse, val = [], []
    for pl in planes:
        x, y = samples_of(gather_plane(a, pl), depth, shift), samples_of(gather_plane(b, pl), depth, shift)
        sse.append(plane_sse(x, y))
        if ssim:
            val.append(plane_ssim(x, y, maxval))
    return torch.stack(sse, dim=1), (torch.stack(val, dim=1) if ssim else None)


def device_metrics(a, b, planes, depth, shift, ssim, workspace=None):
    """The kernels on two checked device stacks, on the current stream: (sse int64 ``[N,P]``, ssim
    float64 ``[N,P]`` or None).  ``workspace``: a function bytes -> device tensor of at least that
    many bytes (default: a fresh one per call)."""
    from . import _lib
    lib = _lib.lib()
    sa, sb = frame_stride(a), frame_stride(b)
    if sa is None:
        a = a.contiguous()
        sa = frame_stride(a)
    if sb is None:
        b = b.contiguous()
        sb = frame_stride(b)
    n, p = a.shape[0], len(planes)
    arr = (_lib.Plane * p)(*[_lib.Plane(off, pitch, step, h, w, 0) for off, step, pitch, h, w in planes])
    flags = 1 if ssim else 0
    need = lib.rrin_frame_metrics_workspace_bytes(n, arr, p, flags)
    if need < 0:
        if ssim and any(pl[3] < 8 or pl[4] < 8 for pl in planes):
            raise ValueError("SSIM needs planes of at least 8x8 samples")
        _lib.check(int(need), "rrin_frame_metrics_workspace_bytes")
    ws = (workspace(need) if workspace is not None
          else torch.empty(max(need, 8) // 8, dtype=torch.int64, device=a.device))
    sse = torch.empty((n, p), dtype=torch.int64, device=a.device)
    val = torch.empty((n, p), dtype=torch.float64, device=a.device) if ssim else None
    with torch.cuda.device(a.device):
        st = C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        vp = val.data_ptr() if ssim else None
        if a.dtype == torch.uint8:
            _lib.check(lib.rrin_frame_metrics_u8(a.data_ptr(), sa, b.data_ptr(), sb, n, arr, p, flags, sse.data_ptr(),
                                                 vp, ws.data_ptr(), need, st), "rrin_frame_metrics_u8")
        else:
            _lib.check(lib.rrin_frame_metrics_u16(a.data_ptr(), sa, b.data_ptr(), sb, n, arr, p, flags, depth, shift,
                                                  sse.data_ptr(), vp, ws.data_ptr(), need, st),
                       "rrin_frame_metrics_u16")
    return sse, val


def _metrics(a, b, planes, depth, shift, ssim, names, workspace=None):
    if ssim and any(pl[3] < 8 or pl[4] < 8 for pl in planes):
        raise ValueError("SSIM needs planes of at least 8x8 samples: pass ssim=False for the squared error alone")
    if a.device.type == "cuda":
        sse, val = device_metrics(a, b, planes, depth, shift, bool(ssim), workspace)
    else:
        sse, val = _host_metrics(a, b, planes, depth, shift, bool(ssim))
    return FrameMetrics(sse, val, [pl[3] * pl[4] for pl in planes], (1 << depth) - 1, names)


def _frame_metrics(fmt: FrameFormat, a, b, ssim, workspace) -> FrameMetrics:
    """The metrics of two stacks of ``fmt`` (only its layout, depth and shift matter here)."""
    _check_pair(a, b, fmt.dtype, 4 if fmt.layout is None else 3)
    if fmt.layout is None:
        if a.shape[3] != 3:
            raise ValueError(f"expected [N,H0,W0,3] frames, got {tuple(a.shape)}")
        h0, w0 = a.shape[1], a.shape[2]
    else:
        h0, w0 = yuv.stack_size(a, fmt.layout)
    names = RGB_NAMES if fmt.layout is None else YUV_NAMES
    return _metrics(a, b, fmt.planes(h0, w0), fmt.depth, fmt.shift, ssim, names, workspace)


def frame_metrics_u8(a, b, ssim=True, _workspace=None) -> FrameMetrics:
    """Per frame and channel of two uint8 ``[N,H0,W0,3]`` RGB stacks (``a`` typically a forward's
    output, ``b`` the truth): squared error, SSIM, PSNR.  Device stacks stay on the device and
    nothing synchronises; every frame dense, any stride between frames (views need no copy)."""
    return _frame_metrics(FrameFormat.u8(), a, b, ssim, _workspace)


def frame_metrics_yuv(a, b, layout="nv12", ssim=True, _workspace=None) -> FrameMetrics:
    """:func:`frame_metrics_u8` per Y, U and V plane of two uint8 YUV stacks of ``layout``
    (:mod:`rrin_amd.yuv`: ``[N, 3*H0//2, W0]``, ``[N, 2*H0, W0]`` or ``[N, 3*H0, W0]``)."""
    return _frame_metrics(FrameFormat.samples(layout), a, b, ssim, _workspace)


def frame_metrics_u16(a, b, depth=10, ssim=True, _workspace=None) -> FrameMetrics:
    """:func:`frame_metrics_u8` for uint16 ``[N,H0,W0,3]`` RGB stacks of ``depth`` 9..16 (samples
    ``min(word, maxval)``)."""
    return _frame_metrics(FrameFormat.samples(None, check_depth(depth)), a, b, ssim, _workspace)


def frame_metrics_yuv16(a, b, layout="nv12", depth=10, msb=False, ssim=True, _workspace=None) -> FrameMetrics:
    """:func:`frame_metrics_yuv` for uint16 stacks of ``depth`` 9..16; ``msb=True`` reads the sample
    from the word's high bits (``shift = 16 - depth``)."""
    depth = check_depth(depth)
    return _frame_metrics(FrameFormat.samples(layout, depth, 16 - depth if msb else 0), a, b, ssim, _workspace)


# ---- the hold-out schedule -----------------------------------------------------------------------
# Frames k*hold are inputs; the hold-1 frames between two inputs are held out and interpolated back
# at t = j/hold.  What comes after the last input is ignored.
def _hold(hold) -> int:
    if isinstance(hold, bool) or not isinstance(hold, int) or hold < 2:
        raise ValueError(f"hold must be an int >= 2 (every hold-th frame is an input), got {hold!r}")
    return hold


def holdout_pair_items(pair: int, hold: int) -> list:
    """The items of input pair ``pair`` (frames ``pair*hold`` and ``(pair+1)*hold``): ``(frame index,
    pair, Fraction t)`` for the ``hold-1`` frames between them, ``t = j/hold``."""
    hold = _hold(hold)
    return [(pair * hold + j, pair, Fraction(j, hold)) for j in range(1, hold)]


def holdout_schedule(n_frames: int, hold: int = 2):
    """(items, ignored) of a clip of ``n_frames``: the items of every whole pair in frame order, and the
    count of frames after the last input.  Fewer than ``hold + 1`` frames: ValueError."""
    hold = _hold(hold)
    if isinstance(n_frames, bool) or not isinstance(n_frames, int) or n_frames < hold + 1:
        raise ValueError(f"hold-out at hold={hold} needs at least {hold + 1} frames, got {n_frames!r}")
    pairs = (n_frames - 1) // hold
    items = [it for p in range(pairs) for it in holdout_pair_items(p, hold)]
    return items, n_frames - 1 - pairs * hold


def nearer_input(t) -> int:
    """0 (the pair's first frame) for t <= 1/2 -- a tie takes the first --, else 1: the frame a player
    shows without interpolation."""
    return 0 if t <= Fraction(1, 2) else 1
