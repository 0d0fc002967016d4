"""YUV4MPEG2 (Y4M) streams of 8-bit 4:2:0 frames: what ``ffmpeg -f yuv4mpegpipe`` writes and reads
(and, for callers that ask with ``depths=``, the 10- and 12-bit ``C420p10`` / ``C420p12`` streams of
``-pix_fmt yuv420p10le`` / ``yuv420p12le``; with ``chroma=``, planar 4:2:2 and 4:4:4 of 8, 10 and 12
bits: ``-pix_fmt yuv422p10le`` and its kin).

A stream is one header line ``YUV4MPEG2 W<w> H<h> F<num>:<den> [I..] [A..] [C..] [X..]`` and, per
frame, a line ``FRAME[ params]`` followed by the planes Y, U, V (``w*h*3/2`` bytes for 4:2:0:
the "i420" layout of :mod:`rrin_amd.yuv`).  Reader and Writer only ever read and write
sequentially -- no seek, no tell -- so a pipe works as well as a file.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"YUV4MPEG2"
# colour-space tags that are all the 8-bit I420 byte layout (they differ in chroma siting only)
C420 = ("420", "420jpeg", "420mpeg2", "420paldv")
# tags of 4:2:0 in 16-bit little-endian words, the sample in the low bits: tag -> bit depth
C420_DEEP = {"420p10": 10, "420p12": 12}
# opt-in (``chroma=``): tags of planar 4:2:2 / 4:4:4 -> (chroma format, bit depth); the deep ones in
# 16-bit little-endian words like C420_DEEP
C4XX = {"422": ("422", 8), "444": ("444", 8), "422p10": ("422", 10), "422p12": ("422", 12),
        "444p10": ("444", 10), "444p12": ("444", 12)}
_MAX_LINE = 4096


def _samples(w: int, h: int, chroma: str) -> int:
    """Samples of a w x h frame: Y, U and V planes of the chroma format."""
    return w * h * 3 // 2 if chroma == "420" else w * h * (2 if chroma == "422" else 3)


def _check_size(w: int, h: int, chroma: str) -> None:
    if chroma == "420" and (w % 2 or h % 2):
        raise ValueError(f"Y4M: 4:2:0 frames need even W and H, got {w}x{h}")
    if chroma == "422" and w % 2:
        raise ValueError(f"Y4M: 4:2:2 frames need an even W, got {w}x{h}")


def _read_exact(f, n: int) -> np.ndarray:
    """n bytes of f as a writable uint8 array, or fewer at the end of the stream (a pipe may
    return short reads, so read until the count is there)."""
    buf = np.empty(n, dtype=np.uint8)
    view, got = memoryview(buf), 0
    while got < n:
        k = f.readinto(view[got:])
        if not k:
            break
        got += k
    return buf[:got]


def _read_line(f) -> bytes:
    """One line without its newline, read a byte at a time (no read-ahead: nothing to give back);
    b"" at the end of the stream."""
    out = bytearray()
    while True:
        b = f.read(1)
        if not b:
            if out:
                raise ValueError("Y4M: the stream ends inside a header line")
            return b""
        if b == b"\n":
            return bytes(out)
        out += b
        if len(out) > _MAX_LINE:
            raise ValueError("Y4M: header line too long (not a Y4M stream?)")


class Reader:
    """Iterates over the frames of a Y4M stream open for binary reading: uint8 arrays of
    ``height*width*3/2`` bytes (Y, then U, then V).  ``width``, ``height``, ``fps_num``,
    ``fps_den`` and ``colorspace`` come from the header.  Anything but progressive 8-bit 4:2:0
    (``C420``, ``C420jpeg``, ``C420mpeg2``, ``C420paldv`` or no ``C`` tag) raises ValueError
    naming the tag; a frame cut short raises ValueError.

    ``depths`` lists the bit depths the caller takes.  With the default ``(8,)`` nothing else is
    read.  With 10 and / or 12 in it ``C420p10`` / ``C420p12`` streams are read too: a frame is then
    a uint16 array of ``height*width*3/2`` little-endian samples (``frame_bytes`` is twice that
    count) and ``bit_depth`` says which; an 8-bit stream still yields uint8.

    ``chroma`` lists the chroma formats the caller takes; the default ``("420",)`` reads what is
    described above and nothing else.  With "422" / "444" in it the tags ``C422`` / ``C444`` are read
    too (planar: the "i422" / "i444" layouts of :mod:`rrin_amd.yuv`; ``height*width*2`` resp. ``*3``
    samples a frame), and ``C422p10``, ``C422p12``, ``C444p10``, ``C444p12`` if ``depths`` has the
    depth; ``chroma`` then says which format the stream has.  4:2:2 needs an even W only, 4:4:4 takes
    any size.  ``Cmono``, ``C411``, ``C444alpha`` and interlaced streams are always refused."""

    def __init__(self, fileobj, depths=(8,), chroma=("420",)):
        self.f = fileobj
        self.bit_depth = 8
        self.chroma = "420"
        line = _read_line(fileobj)
        tags = line.split(b" ")
        if tags[0] != MAGIC:
            raise ValueError("not a Y4M stream: the header does not start with YUV4MPEG2")
        self.width = self.height = None
        self.fps_num, self.fps_den = 0, 1
        self.colorspace = "420"
        for raw in tags[1:]:
            if not raw:
                continue
            tag = raw.decode("ascii", "replace")
            key, val = tag[0], tag[1:]
            if key == "W":
                self.width = int(val)
            elif key == "H":
                self.height = int(val)
            elif key == "F":
                num, _, den = val.partition(":")
                self.fps_num, self.fps_den = int(num), int(den or 1)
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"Y4M: interlaced streams are not supported (tag {tag!r})")
            elif key == "C":
                if val in C4XX and C4XX[val][0] in chroma and C4XX[val][1] in depths:
                    self.chroma, self.bit_depth = C4XX[val]
                elif tuple(chroma) != ("420",) and (val not in C420 and val not in C420_DEEP or "420" not in chroma):
                    raise ValueError(f"Y4M: tag {tag!r} is not among the formats asked for (chroma {tuple(chroma)}, "
                                     f"depths {tuple(depths)})")
                elif val in C420_DEEP and C420_DEEP[val] in depths:
                    self.bit_depth = C420_DEEP[val]
                elif val not in C420 or 8 not in depths:
                    raise ValueError(f"Y4M: only 8-bit 4:2:0 is supported (tag {tag!r})" if tuple(depths) == (8,)
                                     else f"Y4M: only 4:2:0 of {tuple(depths)} bits is supported (tag {tag!r})")
                self.colorspace = val
            # A (pixel aspect) and X (comments) do not change the bytes
        if not self.width or not self.height or self.width < 1 or self.height < 1:
            raise ValueError("Y4M: the header lacks W or H")
        _check_size(self.width, self.height, self.chroma)
        self.frame_bytes = _samples(self.width, self.height, self.chroma) * (2 if self.bit_depth > 8 else 1)

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        line = _read_line(self.f)
        if not line:
            raise StopIteration
        if line != b"FRAME" and not line.startswith(b"FRAME "):
            raise ValueError(f"Y4M: expected a FRAME line, got {line[:32]!r}")
        data = _read_exact(self.f, self.frame_bytes)
        if data.size != self.frame_bytes:
            raise ValueError(f"Y4M: truncated frame ({data.size} of {self.frame_bytes} bytes)")
        return data.view("<u2").astype(np.uint16, copy=False) if self.bit_depth > 8 else data


class Writer:
    """Writes a progressive 8-bit 4:2:0 Y4M stream to a file object open for binary writing: the
    header on construction, then :meth:`write` per frame (``height*width*3/2`` bytes: Y, U, V).
    With 10 and / or 12 in ``depths`` the colour spaces ``420p10`` / ``420p12`` are written too:
    a frame is then ``height*width*3/2`` uint16 samples, stored little-endian.  With "422" / "444" in
    ``chroma`` the colour spaces of ``C4XX`` are written as :class:`Reader` reads them."""

    def __init__(self, fileobj, w: int, h: int, fps_num: int, fps_den: int = 1, colorspace: str = "420",
                 depths=(8,), chroma=("420",)):
        self.bit_depth = 8
        self.chroma = "420"
        if colorspace in C4XX and C4XX[colorspace][0] in chroma and C4XX[colorspace][1] in depths:
            self.chroma, self.bit_depth = C4XX[colorspace]
            if w < 1 or h < 1:
                raise ValueError(f"Y4M: W and H must be >= 1, got {w}x{h}")
            _check_size(w, h, self.chroma)
        elif w < 2 or h < 2 or w % 2 or h % 2:
            raise ValueError(f"Y4M: 4:2:0 frames need even W and H, got {w}x{h}")
        elif tuple(chroma) != ("420",) and (colorspace not in C420 and colorspace not in C420_DEEP
                                            or "420" not in chroma):
            raise ValueError(f"Y4M: colour space C{colorspace} is not among the formats asked for "
                             f"(chroma {tuple(chroma)}, depths {tuple(depths)})")
        elif colorspace in C420_DEEP and C420_DEEP[colorspace] in depths:
            self.bit_depth = C420_DEEP[colorspace]
        elif colorspace not in C420 or 8 not in depths:
            raise ValueError(f"Y4M: only 8-bit 4:2:0 is supported (C{colorspace})" if tuple(depths) == (8,)
                             else f"Y4M: only 4:2:0 of {tuple(depths)} bits is supported (C{colorspace})")
        self.f, self.width, self.height = fileobj, int(w), int(h)
        self.frame_bytes = _samples(w, h, self.chroma) * (2 if self.bit_depth > 8 else 1)
        fileobj.write(b"%s W%d H%d F%d:%d Ip C%s\n" % (MAGIC, w, h, fps_num, fps_den, colorspace.encode()))

    def write(self, frame) -> None:
        if self.bit_depth > 8:
            data = np.ascontiguousarray(frame, dtype="<u2").reshape(-1).view(np.uint8)
        else:
            data = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
        if data.size != self.frame_bytes:
            raise ValueError(f"Y4M: a frame is {self.frame_bytes} bytes, got {data.size}")
        self.f.write(b"FRAME\n")
        self.f.write(memoryview(data))

    def flush(self) -> None:
        self.f.flush()
