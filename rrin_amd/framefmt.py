"""What a stack of byte frames is: the one description behind ``forward_*``, ``interpolate_items_*``,
``pair_stats_*`` and ``frame_metrics_*`` of every frame path.

A :class:`FrameFormat` says how the frames lie in memory -- RGB interleaved ``[N,H0,W0,3]`` or YUV
planes ``[N, rows, W0]`` of a layout of :data:`rrin_amd.yuv.ALL_LAYOUTS`; uint8, or uint16 words at a
``depth`` with the sample ``shift`` bits up -- and, for YUV, the 15 conversion integers.  Everything a
caller derives from that comes from here: dtype and shapes, a frame's length, ``maxval``, the check of
two stacks, the Flow-reuse tag, the key of the cached gate sums, the library's descriptor and entry
names, the planes of the metrics.  Host only: nothing here touches a device, and the library is not
loaded (the ctypes structures of :mod:`rrin_amd._lib` are plain Python).

The four paths are ``u8``, ``u16`` (RGB) and ``yuv``, ``yuv16``; a fifth format is one more constructor,
one row of :data:`ENTRIES` and, if its frames are laid out differently, one branch of ``desc_for``.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch

from . import _lib, yuv

# path -> the library's plain, item and flow_scale entries (include/rrin_hip.h)
ENTRIES = {p: (f"rrin_net_{p}_fwd", f"rrin_net_{p}_items_fwd", f"rrin_net_{p}_scaled_fwd")
           for p in ("u8", "u16", "yuv", "yuv16")}


def check_depth(depth, lo: int = 9, what: str | None = None) -> int:
    """``depth`` if it is an int in ``lo``..16, else ValueError: ``what`` (default "depth must be an int
    in lo..16") followed by ", got ..."."""
    if isinstance(depth, bool) or not isinstance(depth, int) or not lo <= depth <= 16:
        raise ValueError(f"{what or f'depth must be an int in {lo}..16'}, got {depth!r}")
    return depth


def frame_stride(f: torch.Tensor):
    """Elements between the dense frames of a stack (a uniform stride over dim 0, taken as it is), or
    None if a frame is not dense or frames overlap: the stack then needs a copy."""
    dense = 1
    for d in range(f.dim() - 1, 0, -1):  # the trailing dims: dense (a dim of 1 has no stride to check)
        if f.shape[d] > 1 and f.stride(d) != dense:
            return None
        dense *= f.shape[d]
    return dense if f.shape[0] == 1 else (f.stride(0) if f.stride(0) >= dense else None)


@functools.lru_cache(maxsize=8)
def _default_coef(depth: int):
    return yuv.as_coef(None, depth)  # BT.709 limited range at the depth


@functools.lru_cache(maxsize=16)
def _yuv_tag(fmt) -> str:
    k = ",".join(str(v) for v in fmt.coef)
    return f"yuv:{fmt.layout}:{k}" if fmt.depth == 8 else f"yuv16:{fmt.depth}:{fmt.shift}:{fmt.layout}:{k}"


def _stack_geometry(layout: str, esize: int, h0: int, w0: int):
    """Bytes from a frame's Y plane to its U and V planes, chroma pitch and step in elements, enum
    rrin_chroma: the one layout table, the element size a factor."""
    cw = w0 // 2
    # elements from U to V, chroma pitch, chroma step, chroma format
    vo, c_pitch, c_step, chroma = {
        "nv12": (1, w0, 2, _lib.CHROMA_420), "i420": ((h0 // 2) * cw, cw, 1, _lib.CHROMA_420),
        "nv16": (1, w0, 2, _lib.CHROMA_422), "i422": (h0 * cw, cw, 1, _lib.CHROMA_422),
        "i444": (h0 * w0, w0, 1, _lib.CHROMA_444)}[layout]
    u = esize * h0 * w0
    return u, u + esize * vo, c_pitch, c_step, chroma


class FrameFormat(namedtuple("FrameFormat", "layout depth shift coef")):
    """``layout`` None (RGB interleaved) or a YUV layout; ``depth`` 8 (uint8) or the bits of a sample in a
    uint16 word, ``shift`` bits above the word's bit 0; ``coef`` the ``yuv.Coef`` of a YUV format that
    converts (None for RGB, and for calls that only read samples: sums and metrics).  Immutable and
    hashable.  Build one with :meth:`u8`, :meth:`u16`, :meth:`yuv` or :meth:`yuv16`, which make a
    forward's argument checks in its order, or with :meth:`samples`; never from the fields directly."""
    __slots__ = ()

    # ---- the four paths ------------------------------------------------------------------------
    @classmethod
    def u8(cls):
        return _U8

    @classmethod
    def u16(cls, depth, what: str):
        """RGB samples of ``depth`` 9..16 in the words' low bits; ``what`` names the caller in the refusal."""
        return cls(None, check_depth(depth, 9, f"{what}: depth must be an int in 9..16"), 0, None)

    @classmethod
    def yuv(cls, layout, coef=None):
        if layout not in yuv.ALL_LAYOUTS:
            raise ValueError(f"layout must be one of {yuv.ALL_LAYOUTS}, got {layout!r}")
        return cls(layout, 8, 0, _default_coef(8) if coef is None else yuv.as_coef(coef))

    @classmethod
    def yuv16(cls, layout, depth, msb: bool = False, coef=None):
        if layout not in yuv.ALL_LAYOUTS:
            raise ValueError(f"layout must be one of {yuv.ALL_LAYOUTS}, got {layout!r}")
        depth = yuv.check_depth16(depth)
        return cls(layout, depth, 16 - depth if msb else 0,
                   _default_coef(depth) if coef is None else yuv.as_coef(coef, depth))

    @classmethod
    def samples(cls, layout, depth: int = 8, shift: int = 0):
        """A format for the calls that only read samples (pair sums, frame metrics): no matrix, so no
        :attr:`tag` and no :meth:`desc`; ``depth`` is the caller's checked one, and the layout is
        checked with the stack (:meth:`check`, ``yuv.stack_size``), as those calls always did."""
        return cls(layout, depth, shift, None)

    # ---- what the format answers ---------------------------------------------------------------
    @property
    def path(self) -> str:
        return ("u8" if self.depth == 8 else "u16") if self.layout is None else ("yuv" if self.depth == 8 else "yuv16")

    @property
    def dtype(self):
        return torch.uint8 if self.depth == 8 else torch.uint16

    @property
    def esize(self) -> int:
        """Bytes per element."""
        return 1 if self.depth == 8 else 2

    @property
    def maxval(self) -> int:
        return (1 << self.depth) - 1

    @property
    def wide(self):
        """None for bytes, else (depth, shift): a sample is ``min(word >> shift, maxval)``."""
        return None if self.depth == 8 else (self.depth, self.shift)

    @property
    def entries(self):
        """The library's (plain, item, flow_scale) entry names of the path."""
        return ENTRIES[self.path]

    @property
    def plane_entry(self) -> str:
        """The library's entry of the path that also carries an extra plane (:mod:`rrin_amd.plane`): the
        plain, item and flow_scale forwards in one, each companion nullable."""
        return f"rrin_net_{self.path}_plane_fwd"

    @property
    def tag(self) -> str:
        """Names whose raw Flow a workspace keeps: path, and layout, matrix, depth and shift where the
        path has them (the scale is added by :func:`rrin_amd.flowscale.flow_tag`).  Equal tags: the
        same frames give the same Flow."""
        if self.layout is None:
            return "u8" if self.depth == 8 else f"u16:{self.depth}"
        if self.coef is None:
            raise ValueError("a samples-only format (FrameFormat.samples) keeps no Flow: it has no tag")
        return _yuv_tag(self)

    def sums_key(self, n: int, h0: int, w0: int, bounds) -> tuple:
        """Key of the gate's cached sums of absolute differences: they belong to a batch of ``n`` pairs of
        this sample reading (path, depth, shift) and frame size, split into ``bounds``."""
        return (self.path, self.depth, self.shift, n, h0, w0, self.frame_len(h0, w0), tuple(bounds))

    def frame_len(self, h0: int, w0: int) -> int:
        """Elements of a dense H0 x W0 frame: what the gate sums over and copies."""
        return h0 * w0 * 3 if self.layout is None else yuv.stack_rows(h0, self.layout) * w0

    def out_shape(self, n: int, h0: int, w0: int) -> tuple:
        return (n, h0, w0, 3) if self.layout is None else (n, yuv.stack_rows(h0, self.layout), w0)

    def planes(self, h0: int, w0: int) -> list:
        """The planes ``(off, step, pitch, h, w)`` of a frame, as :mod:`rrin_amd.metrics` reads them."""
        from .metrics import planes_of
        return planes_of("rgb", h0, w0) if self.layout is None else planes_of("yuv", h0, w0, self.layout)

    def check(self, f0, f1, device, what: str):
        """Checks two frame stacks of a call ``what`` against this format and ``device`` and returns
        ``(f0, f1, H0, W0, stride)``, the stride in elements between their frames: every frame dense, a
        uniform stride over dim 0 taken as it is (``frames[:-1]`` / ``frames[1:]`` of one stack need no
        copy), anything else copied."""
        dtype = self.dtype
        if not isinstance(device, torch.device):
            device = torch.device(device)
        name = str(dtype).split(".")[-1]
        if not isinstance(f0, torch.Tensor) or not isinstance(f1, torch.Tensor):
            raise TypeError(f"{what} takes two {name} tensors")
        if f0.device != device or f1.device != device:
            raise RuntimeError(f"inputs on {f0.device}/{f1.device}, model on {device}")
        if f0.dtype != dtype or f1.dtype != dtype:
            raise TypeError(f"{what} takes {name} frames (forward takes float32)")
        if self.layout is None:
            if f0.dim() != 4 or f0.shape != f1.shape or f0.shape[3] != 3:
                raise ValueError(f"expected two [N,H0,W0,3] {name} tensors, got {tuple(f0.shape)} / {tuple(f1.shape)}")
            h0, w0 = f0.shape[1:3]
        else:
            if f0.shape != f1.shape:
                raise ValueError(f"expected two equal [N, 3*H0//2, W0] stacks, got {tuple(f0.shape)} / "
                                 f"{tuple(f1.shape)}")
            h0, w0 = yuv.stack_size(f0, self.layout)
        if f0.shape[0] < 1 or h0 < 1 or w0 < 1:
            raise ValueError(f"empty frames: {tuple(f0.shape)}")
        s0 = frame_stride(f0)
        if s0 is None or s0 != frame_stride(f1):
            f0, f1 = f0.contiguous(), f1.contiguous()
            s0 = math.prod(f0.shape[1:])
        return f0, f1, h0, w0, s0

    # ---- the library's descriptor ----------------------------------------------------------------
    def desc_for(self, stride: int, h0: int, w0: int):
        """``make(p0, p1, po) -> (descriptor, its rrin_net_desc)`` for H0 x W0 frames: input stacks at
        device addresses ``p0`` / ``p1`` with ``stride`` elements between frames, the dense output stack
        at ``po``.  Everything but the addresses is filled once, here, into a template that ``make``
        copies: a forward calls it once per part.  Cached per format, stride and size."""
        return _maker(self, stride, h0, w0)

    def desc(self, p0: int, p1: int, stride: int, po: int, h0: int, w0: int):
        """The path's library descriptor and its rrin_net_desc, one at a time (:meth:`desc_for`)."""
        return self.desc_for(stride, h0, w0)(p0, p1, po)


@functools.lru_cache(maxsize=32)
def _maker(fmt, stride: int, h0: int, w0: int):
    """FrameFormat.desc_for, computed."""
    if fmt.layout is None:
        t = _lib.NetU8Desc() if fmt.depth == 8 else _lib.NetU16Desc()
        t.img_stride, t.h0, t.w0 = stride, h0, w0
        out = "out_u8"
        if fmt.depth > 8:
            t.depth, out = fmt.depth, "out_u16"
        cls, buf = type(t), bytes(t)

        def make(p0, p1, po):
            d = cls.from_buffer_copy(buf)
            d.f0, d.f1 = p0, p1
            setattr(d, out, po)
            return d, d.net
        return make
    if fmt.coef is None:
        raise ValueError("a samples-only format (FrameFormat.samples) has no descriptor")
    e = fmt.esize
    uo, vo, c_pitch, c_step, chroma = _stack_geometry(fmt.layout, e, h0, w0)
    t = _lib.NetYuvDesc() if e == 1 else _lib.NetYuv16Desc()
    for st, img_stride in ((t.f0, stride), (t.f1, stride), (t.out, fmt.frame_len(h0, w0))):
        st.img_stride, st.y_pitch, st.c_pitch, st.c_step, st.chroma = img_stride, w0, c_pitch, c_step, chroma
        if e == 2:
            st.depth, st.shift = fmt.depth, fmt.shift
    t.coef, t.h0, t.w0 = _lib.YuvCoef(*fmt.coef), h0, w0
    cls, buf = type(t), bytes(t)

    def make(p0, p1, po):
        d = cls.from_buffer_copy(buf)
        a, b, o = d.f0, d.f1, d.out
        a.y, a.u, a.v = p0, p0 + uo, p0 + vo
        b.y, b.u, b.v = p1, p1 + uo, p1 + vo
        o.y, o.u, o.v = po, po + uo, po + vo
        return d, d.net
    return make


_U8 = FrameFormat(None, 8, 0, None)  # FrameFormat.u8(): one shared value
