"""The schedule of a frame-rate conversion: which input pair and which ``t`` every output frame
comes from.  Plain Python on exact rationals -- no device, and no float until ``float(t)``.

Output ``j`` of a conversion from ``fps_in`` to ``fps_out`` sits at source time
``j * fps_in / fps_out`` (in input frames, an exact ``fractions.Fraction``); the outputs run while
that time is ``<= n_frames - 1``.  An output is the item ``(pair, t)`` with ``pair = floor(time)``
and ``t = time - pair``: the frame between input frames ``pair`` and ``pair + 1`` at ``t``.  An item
with ``t == 0`` is a pass-through: input frame ``pair`` itself, written as its own bytes and never
sent to the network (the last output may be one with ``pair == n_frames - 1``).  Every other item is
one item of ``Net.interpolate_items_*``; ``float(t)`` rounds the rational once.

Only ``fps_out > fps_in`` is a conversion here (decimation is out of scope).  Then the step
``s = fps_in / fps_out`` between outputs is below one input frame, and every pair ``p`` gets at least
one item that needs the network: the largest output time ``T <= p + 1`` (it exists, and is in the
schedule since ``p + 1 <= n_frames - 1``) is ``> p + 1 - s > p``; if ``T < p + 1`` it is such an
item, and if ``T == p + 1`` the output before it, at ``p + 1 - s``, lies strictly inside
``(p, p + 1)``.

``schedule`` is the closed form for a known frame count; ``Stream`` the same items for a pipe whose
length is unknown, fed frame by frame; ``batches`` cuts the network items into fixed-size steps.
"""
from __future__ import annotations

from fractions import Fraction


def as_rate(v) -> Fraction:
    """A frame rate as an exact Fraction: a Fraction, an int, or a string ``"60000/1001"`` / ``"60"``
    (floats are refused: 59.94 is not 60000/1001)."""
    if isinstance(v, bool) or isinstance(v, float):
        raise TypeError(f"a frame rate is a Fraction, an int or a string like '60000/1001', got {v!r}")
    try:
        r = Fraction(v.strip()) if isinstance(v, str) else Fraction(v)
    except (ValueError, ZeroDivisionError) as e:
        raise ValueError(f"not a frame rate: {v!r}") from e
    if r <= 0:
        raise ValueError(f"a frame rate is positive, got {v!r}")
    return r


def _rates(fps_in, fps_out):
    fi, fo = as_rate(fps_in), as_rate(fps_out)
    if fo <= fi:
        raise ValueError(f"fps_out ({fo}) must exceed fps_in ({fi}): decimation is out of scope")
    return fi, fo


def schedule(n_frames: int, fps_in, fps_out) -> list:
    """The items ``(pair, Fraction t)`` of every output of ``n_frames`` input frames, in output
    order: ``floor((n_frames - 1) * fps_out / fps_in) + 1`` of them.  ``n_frames < 2`` and
    ``fps_out <= fps_in`` raise ValueError."""
    fi, fo = _rates(fps_in, fps_out)
    if isinstance(n_frames, bool) or not isinstance(n_frames, int) or n_frames < 2:
        raise ValueError(f"a conversion needs at least two frames, got {n_frames!r}")
    step = fi / fo
    out = []
    for j in range((n_frames - 1) * fo // fi + 1):
        time = j * step
        pair = time.numerator // time.denominator
        out.append((pair, time - pair))
    return out


class Stream:
    """``schedule`` for a stream of unknown length: call :meth:`feed` once per arriving frame; it
    returns the items that frame completes, in output order.  After ``n`` calls the items returned
    so far are ``schedule(n, fps_in, fps_out)`` (for ``n >= 2``; the first frame alone completes the
    pass-through ``(0, 0)``)."""

    def __init__(self, fps_in, fps_out):
        self.fps_in, self.fps_out = _rates(fps_in, fps_out)
        self.step = self.fps_in / self.fps_out
        self.frames = 0   # frames fed
        self.outputs = 0  # items returned

    def feed(self) -> list:
        self.frames += 1
        out = []
        while True:
            time = self.outputs * self.step
            if time > self.frames - 1:
                return out
            pair = time.numerator // time.denominator
            out.append((pair, time - pair))
            self.outputs += 1

    def __iter__(self):
        """Iterating feeds one frame per step: ``next`` is :meth:`feed`; it never ends by itself."""
        return self

    def __next__(self) -> list:
        return self.feed()


def is_passthrough(item) -> bool:
    return item[1] == 0


def batches(items, batch: int = 4):
    """The network items of ``items`` (those with ``t != 0``) cut, in order, into steps of ``batch``
    (the last may be shorter): per step ``(first frame, last frame, [pair - first frame], [float
    t])`` -- the frames ``first .. last`` go up as one stack, and the two lists are the ``pair`` and
    ``t`` of ``Net.interpolate_items_*`` on it."""
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    net = [it for it in items if not is_passthrough(it)]
    for i in range(0, len(net), batch):
        part = net[i:i + batch]
        lo, hi = part[0][0], part[-1][0] + 1
        yield lo, hi, [p - lo for p, _ in part], [float(t) for _, t in part]
