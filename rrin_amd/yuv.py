"""8-bit YUV 4:2:0 frames (NV12 / I420) and the integer colour conversion of ``Net.forward_yuv``.

The YUV path is *defined* as::

    forward_yuv(f0, f1, t) == rgb_to_yuv420(forward_u8(yuv420_to_rgb(f0), yuv420_to_rgb(f1), t))

with the two conversions of this module: pure int32 arithmetic on Q14 coefficients (``>>`` is the
arithmetic shift, i.e. floor), no float anywhere, so the same bits on any device.  The HIP kernels
(``csrc/yuv.hip``, the FINAL head of ``csrc/glue_h8.hip``) compute exactly this without ever
holding an RGB frame; the functions here are the written definition and the tests' oracle.

A frame stack is uint8 ``[N, 3*H0//2, W0]`` with H0 and W0 even, every frame ``H0*W0*3/2`` dense
bytes: H0 rows of luma, then

* ``"nv12"``: H0/2 rows of interleaved U, V samples (what hardware decoders emit);
* ``"i420"``: the U plane, then the V plane, each H0/2 x W0/2 (what Y4M pipes carry), the same
  byte count laid out in the remaining H0/2 rows.

Chroma is one sample per 2x2 block of pixels, replicated on the way in and the block's mean on
the way out (no interpolated siting).

4:2:2 and 4:4:4 (``yuv_to_rgb`` / ``rgb_to_yuv`` and their 16-bit twins, below the 4:2:0 functions)
are the same path with another chroma block -- 2x1 pixels (two wide, one row tall) and one pixel:

* ``"nv16"`` / ``"i422"``: uint8 ``[N, 2*H0, W0]``, H0 luma rows then ``H0*W0`` chroma bytes: H0 rows
  of interleaved U, V, or the U plane then the V plane, each H0 x W0/2.  W0 even, any H0 >= 1.
* ``"i444"``: ``[N, 3*H0, W0]``, the Y, U and V planes; any H0, W0 >= 1.
"""
from __future__ import annotations

from collections import namedtuple

import torch

LAYOUTS = ("nv12", "i420")
LAYOUTS_422 = ("nv16", "i422")
LAYOUTS_444 = ("i444",)
ALL_LAYOUTS = LAYOUTS + LAYOUTS_422 + LAYOUTS_444
CHROMAS = ("420", "422", "444")

Coef = namedtuple("Coef", "y0 ay rv gu gv bu yr yg yb ur ug ub vr vg vb")
Coef.__doc__ = """The 15 Q14 integers of rrin_yuv_coef (include/rrin_hip.h), in its order: y0, ay, rv,
gu, gv, bu take YUV to RGB; yr .. vb take RGB to YUV."""

_KR_KB = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}


def coefficients(standard: str = "bt709", full_range: bool = False, depth: int = 8) -> Coef:
    """The coefficients of a standard, ``round(x * 2**14)`` of the matrix its Kr / Kb give, for
    limited range (Y 16..235, chroma 16..240: the default) or full range.  ``yg``, ``ug`` and
    ``vg`` are remainders, so that grey maps to U = V = 128 exactly.  ``rrin_yuv_coef_std`` holds
    the same numbers.

    ``depth`` d (8..16; the 16-bit YUV path itself takes 10 and 12) scales the limited range to
    d-bit code values: ``y0 = 16 << (d-8)``, luma by ``219 * 2**(d-8) / maxval`` and chroma by
    ``224 * 2**(d-8) / maxval`` with ``maxval = 2**d - 1``; grey then maps to U = V = ``1 << (d-1)``.
    Full range has no scale at any depth.  ``rrin_yuv_coef_std16`` holds the same numbers."""
    if standard not in _KR_KB:
        raise ValueError(f"standard must be one of {sorted(_KR_KB)}, got {standard!r}")
    if not 8 <= int(depth) <= 16:
        raise ValueError(f"depth must be 8..16, got {depth!r}")
    kr, kb = _KR_KB[standard]
    kg = 1.0 - kr - kb
    up, maxval = float(1 << (depth - 8)), float((1 << depth) - 1)
    ys, cs = (1.0, 1.0) if full_range else (219.0 * up / maxval, 224.0 * up / maxval)

    def q(x):
        return int(round(x * 16384.0))

    yr, yb = q(kr * ys), q(kb * ys)
    ur, ub = q(-kr / (2 * (1 - kb)) * cs), q(0.5 * cs)
    vr, vb = q(0.5 * cs), q(-kb / (2 * (1 - kr)) * cs)
    return Coef(y0=0 if full_range else 16 << (depth - 8), ay=q(1.0 / ys),
                rv=q(2 * (1 - kr) / cs), gu=q(-2 * (1 - kb) * kb / kg / cs), gv=q(-2 * (1 - kr) * kr / kg / cs),
                bu=q(2 * (1 - kb) / cs),
                yr=yr, yg=q(ys) - yr - yb, yb=yb, ur=ur, ug=-(ur + ub), ub=ub, vr=vr, vg=-(vr + vb), vb=vb)


def as_coef(coef, depth: int = 8) -> Coef:
    """``None`` (bt709 limited), a :class:`Coef` or any 15 ints -> a validated :class:`Coef`.

    With ``depth`` above 8 (the 16-bit path) ``None`` is bt709 limited at that depth, ``y0`` may
    reach ``maxval`` and the nine RGB -> YUV coefficients are bounded by 2**15 instead of 2**16:
    the chroma sum of a 2x2 block of 12-bit samples, ``3 * (2**15 - 1) * 4 * 4095 + 2**15``, then
    stays below 2**31 (with 2**16 it would not)."""
    if depth == 8:
        if coef is None:
            return coefficients()
        c = Coef(*(int(v) for v in coef))
        if not 0 <= c.y0 <= 255 or any(abs(v) >= 65536 for v in c[1:]):
            raise ValueError("yuv coefficients: 0 <= y0 <= 255 and |coefficient| < 2**16")
        return c
    if coef is None:
        return coefficients(depth=depth)
    c = Coef(*(int(v) for v in coef))
    if (not 0 <= c.y0 <= (1 << depth) - 1 or any(abs(v) >= IN_BOUND for v in c[1:6])
            or any(abs(v) >= OUT_BOUND16 for v in c[6:])):
        raise ValueError(f"yuv coefficients at depth {depth}: 0 <= y0 <= {(1 << depth) - 1}, |ay .. bu| < 2**16 "
                         "and |yr .. vb| < 2**15")
    return c


# bounds of the coefficients (exclusive): YUV -> RGB at any depth; RGB -> YUV on the 16-bit path
IN_BOUND, OUT_BOUND16 = 1 << 16, 1 << 15
DEPTHS16 = (10, 12)


def check_depth16(depth) -> int:
    """The depth of a 16-bit 4:2:0 call: 10 or 12, ValueError otherwise."""
    if isinstance(depth, bool) or not isinstance(depth, int) or depth not in DEPTHS16:
        raise ValueError(f"16-bit 4:2:0 frames are 10 or 12 bits deep, got {depth!r}")
    return int(depth)


def words_to_int(x: torch.Tensor) -> torch.Tensor:
    """uint16 -> int32 values 0..65535."""
    return x.view(torch.int16).to(torch.int32) & 0xFFFF


def int_to_words(x: torch.Tensor) -> torch.Tensor:
    """Integers 0..65535 -> uint16."""
    return x.to(torch.int16).view(torch.uint16)


def _need_420(layout) -> None:
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")


def frame_size(frames: torch.Tensor):
    """(H0, W0) of a uint8 ``[N, 3*H0//2, W0]`` stack; ValueError unless both are even."""
    if frames.dim() != 3:
        raise ValueError(f"expected a [N, 3*H0//2, W0] 4:2:0 stack, got {tuple(frames.shape)}")
    rows, w0 = frames.shape[1], frames.shape[2]
    if rows < 3 or rows % 3 or w0 < 2 or w0 % 2:
        raise ValueError(f"4:2:0 needs even H0 and W0: a [N, 3*H0//2, W0] stack, got {tuple(frames.shape)}")
    return rows // 3 * 2, w0


def split_planes(frames: torch.Tensor, layout: str = "nv12"):
    """Y ``[N,H0,W0]``, U and V ``[N,H0/2,W0/2]`` of a stack (copies, same dtype); for a 4:2:2 or
    4:4:4 layout U and V are ``[N,H0,W0/2]`` / ``[N,H0,W0]``."""
    if layout in LAYOUTS_422 or layout in LAYOUTS_444:
        return _split_planes_4xx(frames, layout)
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    h0, w0 = frame_size(frames)
    n = frames.shape[0]
    y = frames[:, :h0]
    c = frames[:, h0:].reshape(n, -1)
    if layout == "nv12":
        uv = c.reshape(n, h0 // 2, w0 // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    uv = c.reshape(n, 2, h0 // 2, w0 // 2)
    return y, uv[:, 0], uv[:, 1]


def join_planes(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, layout: str = "nv12") -> torch.Tensor:
    """The inverse of :func:`split_planes`: a dense ``[N, 3*H0//2, W0]`` stack (4:2:2: ``[N, 2*H0, W0]``,
    4:4:4: ``[N, 3*H0, W0]``)."""
    if layout in LAYOUTS_422 or layout in LAYOUTS_444:
        n, _, w0 = y.shape
        c = torch.stack((u, v), dim=3 if layout == "nv16" else 1)
        return torch.cat((y, c.reshape(n, -1, w0)), dim=1)
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    n, h0, w0 = y.shape
    c = torch.stack((u, v), dim=3 if layout == "nv12" else 1)
    return torch.cat((y, c.reshape(n, h0 // 2, w0)), dim=1)


def yuv420_to_rgb(frames: torch.Tensor, layout: str = "nv12", coef=None) -> torch.Tensor:
    """uint8 ``[N, 3*H0//2, W0]`` -> uint8 RGB ``[N,H0,W0,3]``.  Per pixel, with the U, V of its
    2x2 block, c = Y - y0, d = U - 128, e = V - 128::

        R = clip255((ay*c        + rv*e + 8192) >> 14)
        G = clip255((ay*c + gu*d + gv*e + 8192) >> 14)
        B = clip255((ay*c + bu*d        + 8192) >> 14)
    """
    if frames.dtype != torch.uint8:
        raise TypeError("4:2:0 frames are uint8")
    _need_420(layout)
    k = as_coef(coef)
    y, u, v = split_planes(frames, layout)
    c = (y.to(torch.int32) - k.y0) * k.ay + 8192
    d = (u.to(torch.int32) - 128).repeat_interleave(2, 1).repeat_interleave(2, 2)
    e = (v.to(torch.int32) - 128).repeat_interleave(2, 1).repeat_interleave(2, 2)
    rgb = torch.stack((c + k.rv * e, c + k.gu * d + k.gv * e, c + k.bu * d), dim=3)
    return (rgb >> 14).clamp_(0, 255).to(torch.uint8)


def rgb_to_yuv420(rgb: torch.Tensor, layout: str = "nv12", coef=None) -> torch.Tensor:
    """uint8 RGB ``[N,H0,W0,3]`` (H0, W0 even) -> uint8 ``[N, 3*H0//2, W0]``.  Per pixel::

        Y = clip255(y0 + ((yr*R + yg*G + yb*B + 8192) >> 14))

    and per 2x2 block, with Rs, Gs, Bs the sums of its four pixels' bytes::

        U = clip255(128 + ((ur*Rs + ug*Gs + ub*Bs + 32768) >> 16))
        V = clip255(128 + ((vr*Rs + vg*Gs + vb*Bs + 32768) >> 16))
    """
    if rgb.dtype != torch.uint8:
        raise TypeError("RGB frames are uint8")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError(f"expected [N,H0,W0,3] RGB frames, got {tuple(rgb.shape)}")
    n, h0, w0, _ = rgb.shape
    if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2:
        raise ValueError(f"4:2:0 needs even H0 and W0, got {h0}x{w0}")
    _need_420(layout)
    k = as_coef(coef)
    p = rgb.to(torch.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (k.y0 + ((k.yr * r + k.yg * g + k.yb * b + 8192) >> 14)).clamp_(0, 255)
    s = p.reshape(n, h0 // 2, 2, w0 // 2, 2, 3).sum(dim=(2, 4), dtype=torch.int32)
    rs, gs, bs = s[..., 0], s[..., 1], s[..., 2]
    u = (128 + ((k.ur * rs + k.ug * gs + k.ub * bs + 32768) >> 16)).clamp_(0, 255)
    v = (128 + ((k.vr * rs + k.vg * gs + k.vb * bs + 32768) >> 16)).clamp_(0, 255)
    return join_planes(y.to(torch.uint8), u.to(torch.uint8), v.to(torch.uint8), layout)


# ---- 10- and 12-bit frames in 16-bit words ------------------------------------------------
# The 16-bit YUV path is defined as
#
#     forward_yuv16(f0, f1, t) == rgb16_to_yuv420(forward_u16(yuv420_to_rgb16(f0), yuv420_to_rgb16(f1), t, depth))
#
# with the conversions below: the 8-bit formulas with 128 replaced by 1 << (depth-1) and clip255 by
# a clip to maxval = 2**depth - 1.  Depths 10 and 12 only: with |coefficient| < 2**16 the sums of the
# way in reach 3 * 2**16 * 2**depth, inside int32 up to 14 bits and not at 16, and the chroma sum
# of the way out (four samples, see as_coef) is the tighter bound.  Frames are uint16
# [N, 3*H0//2, W0] in the 8-bit layouts; ``msb=False`` takes the sample from the word's low bits
# (yuv420p10le, Y4M C420p10), ``msb=True`` from its high bits (``word >> (16 - depth)`` in,
# ``sample << (16 - depth)`` out: P010 / P012).  A sample above maxval is read as maxval.
def samples16(words: torch.Tensor, depth: int, msb: bool) -> torch.Tensor:
    """The int32 samples of uint16 words: ``min(word >> shift, maxval)``."""
    v = words_to_int(words)
    if msb:
        v = v >> (16 - depth)
    return v.clamp_(max=(1 << depth) - 1)


def yuv420_to_rgb16(frames: torch.Tensor, layout: str = "nv12", coef=None, depth: int = 10,
                    msb: bool = False) -> torch.Tensor:
    """uint16 ``[N, 3*H0//2, W0]`` of ``depth`` 10 or 12 -> uint16 RGB ``[N,H0,W0,3]`` samples of that
    depth (low bits), by :func:`yuv420_to_rgb`'s formulas with d = U - half, e = V - half and a
    clip to maxval.  ``coef`` None: BT.709 limited range at this depth."""
    return _to_rgb_words(frames, layout, coef, check_depth16(depth), msb)


def _to_rgb_words(frames, layout, coef, depth, msb):
    """yuv420_to_rgb16 at any depth 8..14 (depth 8 is yuv420_to_rgb on the same values)."""
    if frames.dtype != torch.uint16:
        raise TypeError("16-bit 4:2:0 frames are uint16")
    _need_420(layout)
    k = as_coef(coef, depth)
    half, maxval = 1 << (depth - 1), (1 << depth) - 1
    y, u, v = split_planes(frames, layout)
    c = (samples16(y, depth, msb) - k.y0) * k.ay + 8192
    d = (samples16(u, depth, msb) - half).repeat_interleave(2, 1).repeat_interleave(2, 2)
    e = (samples16(v, depth, msb) - half).repeat_interleave(2, 1).repeat_interleave(2, 2)
    rgb = torch.stack((c + k.rv * e, c + k.gu * d + k.gv * e, c + k.bu * d), dim=3)
    return int_to_words((rgb >> 14).clamp_(0, maxval))


def rgb16_to_yuv420(rgb: torch.Tensor, layout: str = "nv12", coef=None, depth: int = 10,
                    msb: bool = False) -> torch.Tensor:
    """uint16 RGB ``[N,H0,W0,3]`` samples of ``depth`` 10 or 12 (above maxval: read as maxval) ->
    uint16 ``[N, 3*H0//2, W0]``, by :func:`rgb_to_yuv420`'s formulas with ``half`` for 128 and a clip
    to maxval; ``msb`` shifts the samples into the words' high bits."""
    return _to_yuv_words(rgb, layout, coef, check_depth16(depth), msb)


def _to_yuv_words(rgb, layout, coef, depth, msb):
    """rgb16_to_yuv420 at any depth 8..12 (depth 8 is rgb_to_yuv420 on the same values)."""
    if rgb.dtype != torch.uint16:
        raise TypeError("16-bit RGB frames are uint16")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError(f"expected [N,H0,W0,3] RGB frames, got {tuple(rgb.shape)}")
    n, h0, w0, _ = rgb.shape
    if h0 < 2 or w0 < 2 or h0 % 2 or w0 % 2:
        raise ValueError(f"4:2:0 needs even H0 and W0, got {h0}x{w0}")
    _need_420(layout)
    k = as_coef(coef, depth)
    half, maxval = 1 << (depth - 1), (1 << depth) - 1
    p = samples16(rgb, depth, False)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (k.y0 + ((k.yr * r + k.yg * g + k.yb * b + 8192) >> 14)).clamp_(0, maxval)
    s = p.reshape(n, h0 // 2, 2, w0 // 2, 2, 3).sum(dim=(2, 4), dtype=torch.int32)
    rs, gs, bs = s[..., 0], s[..., 1], s[..., 2]
    u = (half + ((k.ur * rs + k.ug * gs + k.ub * bs + 32768) >> 16)).clamp_(0, maxval)
    v = (half + ((k.vr * rs + k.vg * gs + k.vb * bs + 32768) >> 16)).clamp_(0, maxval)
    sh = 16 - depth if msb else 0
    return join_planes(int_to_words(y << sh), int_to_words(u << sh), int_to_words(v << sh), layout)


# ---- any chroma format: 4:2:0, 4:2:2, 4:4:4 ---------------------------------------------------
# The path of a layout is defined as
#
#     forward_yuv(f0, f1, t, layout) == rgb_to_yuv(forward_u8(yuv_to_rgb(f0, layout), yuv_to_rgb(f1, layout), t), layout)
#
# The way in is the per-pixel formula of yuv420_to_rgb with the U, V of the pixel's block.  The way
# out keeps the luma formula; a chroma block of P pixels (4:2:0: 4, 4:2:2: 2, 4:4:4: 1) with
# component sums Rs, Gs, Bs gives
#
#     U = clip(mid + ((ur*Rs + ug*Gs + ub*Bs + 8192*P) >> (14 + log2 P)))        (V likewise)
#
# which for P = 4 is the "+ 32768 >> 16" above: the mean of the block's Q14 values, rounded half
# up.  Since ur + ug + ub == 0, grey still maps to U = V = mid exactly at every P.
def chroma_of(layout: str) -> str:
    """The chroma format of a layout: "420", "422" or "444"; ValueError for an unknown layout."""
    if layout in LAYOUTS:
        return "420"
    if layout in LAYOUTS_422:
        return "422"
    if layout in LAYOUTS_444:
        return "444"
    raise ValueError(f"layout must be one of {ALL_LAYOUTS}, got {layout!r}")


def block_of(chroma: str):
    """(rows, columns) of pixels per chroma sample."""
    return {"420": (2, 2), "422": (1, 2), "444": (1, 1)}[chroma]


def stack_size(frames: torch.Tensor, layout: str = "nv12"):
    """(H0, W0) of a dense stack of ``layout``: :func:`frame_size` for the 4:2:0 layouts,
    ``[N, 2*H0, W0]`` with W0 even for 4:2:2 and ``[N, 3*H0, W0]`` for 4:4:4."""
    chroma = chroma_of(layout)
    if chroma == "420":
        return frame_size(frames)
    if frames.dim() != 3:
        raise ValueError(f"expected a [N, rows, W0] 4:{chroma[1:2]}:{chroma[2:]} stack, got {tuple(frames.shape)}")
    rows, w0 = frames.shape[1], frames.shape[2]
    if chroma == "422":
        if rows < 2 or rows % 2 or w0 < 2 or w0 % 2:
            raise ValueError(f"4:2:2 needs an even W0: a [N, 2*H0, W0] stack, got {tuple(frames.shape)}")
        return rows // 2, w0
    if rows < 3 or rows % 3 or w0 < 1:
        raise ValueError(f"4:4:4 needs a [N, 3*H0, W0] stack, got {tuple(frames.shape)}")
    return rows // 3, w0


def stack_rows(h0: int, layout: str) -> int:
    """Rows of a dense ``[N, rows, W0]`` stack of H0-row frames."""
    return {"420": 3 * h0 // 2, "422": 2 * h0, "444": 3 * h0}[chroma_of(layout)]


def check_size(h0: int, w0: int, layout: str) -> None:
    """ValueError unless H0 x W0 frames exist in ``layout``'s chroma format."""
    chroma = chroma_of(layout)
    by, bx = block_of(chroma)
    if h0 < by or w0 < bx or h0 % by or w0 % bx:
        need = {"420": "even H0 and W0", "422": "an even W0", "444": "H0, W0 >= 1"}[chroma]
        raise ValueError(f"4:{chroma[1]}:{chroma[2]} needs {need}, got {h0}x{w0}")


def _split_planes_4xx(frames: torch.Tensor, layout: str):
    """split_planes for the 4:2:2 and 4:4:4 layouts."""
    chroma = chroma_of(layout)
    h0, w0 = stack_size(frames, layout)
    n = frames.shape[0]
    y = frames[:, :h0]
    c = frames[:, h0:].reshape(n, -1)
    cw = w0 // 2 if chroma == "422" else w0
    if layout == "nv16":
        uv = c.reshape(n, h0, cw, 2)
        return y, uv[..., 0], uv[..., 1]
    uv = c.reshape(n, 2, h0, cw)
    return y, uv[:, 0], uv[:, 1]


def _spread(c: torch.Tensor, chroma: str) -> torch.Tensor:
    """A chroma plane replicated over its blocks: ``[N,H0,W0]``."""
    by, bx = block_of(chroma)
    if by > 1:
        c = c.repeat_interleave(by, 1)
    return c.repeat_interleave(bx, 2) if bx > 1 else c


def _block_chroma(p, kr, kg, kb, mid, maxval, chroma):
    """The chroma plane of int32 RGB samples ``p`` [N,H0,W0,3]: the block rule written above."""
    n, h0, w0, _ = p.shape
    by, bx = block_of(chroma)
    s = p.reshape(n, h0 // by, by, w0 // bx, bx, 3).sum(dim=(2, 4), dtype=torch.int32)
    log2p = {4: 2, 2: 1, 1: 0}[by * bx]
    q = kr * s[..., 0] + kg * s[..., 1] + kb * s[..., 2] + (8192 << log2p)
    return (mid + (q >> (14 + log2p))).clamp_(0, maxval)


def yuv_to_rgb(frames: torch.Tensor, layout: str = "nv12", coef=None) -> torch.Tensor:
    """A uint8 stack of any layout -> uint8 RGB ``[N,H0,W0,3]``: :func:`yuv420_to_rgb`'s formulas with
    the U, V of the pixel's block (2x2, 2x1 or the pixel itself), replicated."""
    chroma = chroma_of(layout)
    if chroma == "420":
        return yuv420_to_rgb(frames, layout, coef)
    if frames.dtype != torch.uint8:
        raise TypeError(f"4:{chroma[1]}:{chroma[2]} frames are uint8")
    k = as_coef(coef)
    y, u, v = split_planes(frames, layout)
    c = (y.to(torch.int32) - k.y0) * k.ay + 8192
    d = _spread(u.to(torch.int32) - 128, chroma)
    e = _spread(v.to(torch.int32) - 128, chroma)
    rgb = torch.stack((c + k.rv * e, c + k.gu * d + k.gv * e, c + k.bu * d), dim=3)
    return (rgb >> 14).clamp_(0, 255).to(torch.uint8)


def rgb_to_yuv(rgb: torch.Tensor, layout: str = "nv12", coef=None) -> torch.Tensor:
    """uint8 RGB ``[N,H0,W0,3]`` -> a uint8 stack of ``layout``: the luma of :func:`rgb_to_yuv420` per
    pixel, and per chroma block of P pixels ``clip255(128 + ((ur*Rs + ug*Gs + ub*Bs + 8192*P) >>
    (14 + log2 P)))`` (V likewise)."""
    chroma = chroma_of(layout)
    if chroma == "420":
        return rgb_to_yuv420(rgb, layout, coef)
    if rgb.dtype != torch.uint8:
        raise TypeError("RGB frames are uint8")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError(f"expected [N,H0,W0,3] RGB frames, got {tuple(rgb.shape)}")
    check_size(rgb.shape[1], rgb.shape[2], layout)
    k = as_coef(coef)
    p = rgb.to(torch.int32)
    y = (k.y0 + ((k.yr * p[..., 0] + k.yg * p[..., 1] + k.yb * p[..., 2] + 8192) >> 14)).clamp_(0, 255)
    u = _block_chroma(p, k.ur, k.ug, k.ub, 128, 255, chroma)
    v = _block_chroma(p, k.vr, k.vg, k.vb, 128, 255, chroma)
    return join_planes(y.to(torch.uint8), u.to(torch.uint8), v.to(torch.uint8), layout)


def yuv_to_rgb16(frames: torch.Tensor, layout: str = "nv12", coef=None, depth: int = 10,
                 msb: bool = False) -> torch.Tensor:
    """:func:`yuv420_to_rgb16` for any layout: a uint16 stack of ``depth`` 10 or 12 -> uint16 RGB
    ``[N,H0,W0,3]`` samples of that depth.  The int32 bound of the way in does not depend on the
    block; that of the way out (:func:`as_coef`: a 2x2 block of 12-bit samples) is only looser
    for the 2- and 1-pixel blocks, so the coefficient bounds are those of 4:2:0."""
    depth = check_depth16(depth)
    chroma = chroma_of(layout)
    if chroma == "420":
        return _to_rgb_words(frames, layout, coef, depth, msb)
    if frames.dtype != torch.uint16:
        raise TypeError(f"16-bit 4:{chroma[1]}:{chroma[2]} frames are uint16")
    k = as_coef(coef, depth)
    half, maxval = 1 << (depth - 1), (1 << depth) - 1
    y, u, v = split_planes(frames, layout)
    c = (samples16(y, depth, msb) - k.y0) * k.ay + 8192
    d = _spread(samples16(u, depth, msb) - half, chroma)
    e = _spread(samples16(v, depth, msb) - half, chroma)
    rgb = torch.stack((c + k.rv * e, c + k.gu * d + k.gv * e, c + k.bu * d), dim=3)
    return int_to_words((rgb >> 14).clamp_(0, maxval))


def rgb16_to_yuv(rgb: torch.Tensor, layout: str = "nv12", coef=None, depth: int = 10,
                 msb: bool = False) -> torch.Tensor:
    """:func:`rgb16_to_yuv420` for any layout, with :func:`rgb_to_yuv`'s block rule, ``half`` for 128
    and a clip to maxval.  The chroma sum of a block of P <= 4 samples, ``3 * (2**15 - 1) * P * 4095 +
    8192 * P``, is largest at P = 4 (:func:`as_coef`): the smaller blocks only loosen the int32 bound."""
    depth = check_depth16(depth)
    chroma = chroma_of(layout)
    if chroma == "420":
        return _to_yuv_words(rgb, layout, coef, depth, msb)
    if rgb.dtype != torch.uint16:
        raise TypeError("16-bit RGB frames are uint16")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise ValueError(f"expected [N,H0,W0,3] RGB frames, got {tuple(rgb.shape)}")
    check_size(rgb.shape[1], rgb.shape[2], layout)
    k = as_coef(coef, depth)
    half, maxval = 1 << (depth - 1), (1 << depth) - 1
    p = samples16(rgb, depth, False)
    y = (k.y0 + ((k.yr * p[..., 0] + k.yg * p[..., 1] + k.yb * p[..., 2] + 8192) >> 14)).clamp_(0, maxval)
    u = _block_chroma(p, k.ur, k.ug, k.ub, half, maxval, chroma)
    v = _block_chroma(p, k.vr, k.vg, k.vb, half, maxval, chroma)
    sh = 16 - depth if msb else 0
    return join_planes(int_to_words(y << sh), int_to_words(u << sh), int_to_words(v << sh), layout)
