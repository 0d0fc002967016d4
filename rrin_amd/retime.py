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

Any rate, an exposure (:mod:`rrin_amd.exposure` is the definition of the exposed frame).  With
``samples = S`` an output is no longer one item but the mean of ``S`` of them, spread over the shutter
window, and ``fps_out`` may be any positive rate: lower, equal or higher.  With ``step = fps_in /
fps_out`` and a shutter ``sh`` in (0, 1], output ``j`` has the sample times

    tau(j, k) = j * step + k * sh * step / S        k = 0 .. S-1

a left Riemann sum over ``[j * step, j * step + sh * step)``, so ``S == 1`` is the point sample at
``j * step``.  Sample ``(pair, t) = (floor tau, tau - floor tau)``; ``t == 0`` is input frame ``pair``
itself (``(n_frames - 1, 0)`` is legal, as the last pass-through above is), every other sample an item
of ``Net.interpolate_items_*``.  The outputs run while the LAST sample ``tau(j, S-1) <= n_frames - 1``.

The count in closed form.  ``tau(j, S-1)`` grows with ``j``, so the outputs are ``j = 0 .. J`` with ``J``
the largest integer for which ``j * step + (S-1) * sh * step / S <= n_frames - 1``.  Dividing by
``step > 0``: ``j <= (n_frames - 1) * fps_out / fps_in - (S-1) * sh / S =: x``.  There are ``floor(x) + 1``
outputs if ``x >= 0`` and none otherwise (``x >= 0`` always holds for ``S == 1``; for ``S > 1`` the first
window must fit: ``n_frames - 1 >= (S-1) * sh * step / S``).  At ``S == 1`` this is ``schedule``'s count
``floor((n_frames - 1) * fps_out / fps_in) + 1``, and the items are ``schedule``'s: for ``fps_out >
fps_in``, ``exposure_schedule(n, fi, fo, sh, 1) == [[it] for it in schedule(n, fi, fo)]`` for every
``sh``.  Times never decrease over the flattened outputs: ``tau(j, S-1) = j * step + (S-1)/S * sh *
step < (j + 1) * step = tau(j + 1, 0)``.

``exposure_schedule`` is that closed form, ``ExposureStream`` the same outputs for a pipe fed frame by
frame, ``as_shutter`` the shutter as an exact Fraction.
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


# ---- any output rate with an exposure: S samples per output over the shutter window --------------
MAX_SAMPLES = 256  # a sum of 256 16-bit samples stays far inside 32 bits (65535 * 256)


def as_shutter(v) -> Fraction:
    """A shutter as an exact Fraction in (0, 1]: a Fraction, an int or a string ``"1/2"`` (floats are
    refused, as :func:`as_rate` refuses them)."""
    if isinstance(v, bool) or isinstance(v, float):
        raise TypeError(f"a shutter is a Fraction, an int or a string like '1/2', got {v!r}")
    try:
        r = Fraction(v.strip()) if isinstance(v, str) else Fraction(v)
    except (ValueError, ZeroDivisionError, TypeError) as e:
        raise ValueError(f"not a shutter: {v!r}") from e
    if not 0 < r <= 1:
        raise ValueError(f"a shutter is in (0, 1], got {v!r}")
    return r


def check_samples(samples) -> int:
    """``samples`` if it is an int in 1..256, else ValueError."""
    if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
        raise ValueError(f"samples must be an int in 1..{MAX_SAMPLES}, got {samples!r}")
    return samples


def _exposure_args(fps_in, fps_out, shutter, samples):
    fi, fo = as_rate(fps_in), as_rate(fps_out)
    return fi, fo, as_shutter(shutter), check_samples(samples)


def _output(j: int, step: Fraction, sub: Fraction, samples: int) -> list:
    """The ``samples`` items of output ``j``: sample k at ``j * step + k * sub``."""
    out = []
    for k in range(samples):
        time = j * step + k * sub
        pair = time.numerator // time.denominator
        out.append((pair, time - pair))
    return out


def exposure_count(n_frames: int, fps_in, fps_out, shutter, samples) -> int:
    """The number of outputs of ``n_frames`` input frames in closed form (the module docstring derives
    it): ``floor((n_frames - 1) * fps_out / fps_in - (S-1) * shutter / S) + 1``, or 0 where that
    argument is negative."""
    fi, fo, sh, s = _exposure_args(fps_in, fps_out, shutter, samples)
    if isinstance(n_frames, bool) or not isinstance(n_frames, int) or n_frames < 1:
        raise ValueError(f"a stream has at least one frame, got {n_frames!r}")
    x = (n_frames - 1) * fo / fi - Fraction(s - 1, s) * sh
    return x.numerator // x.denominator + 1 if x >= 0 else 0


def exposure_schedule(n_frames: int, fps_in, fps_out, shutter, samples) -> list:
    """The outputs of ``n_frames`` input frames converted from ``fps_in`` to any ``fps_out`` with
    ``samples`` sub-frames over the ``shutter``: a list of :func:`exposure_count` outputs, each a list of
    ``samples`` items ``(pair, Fraction t)`` in time order."""
    fi, fo, sh, s = _exposure_args(fps_in, fps_out, shutter, samples)
    step = fi / fo
    sub = sh * step / s
    return [_output(j, step, sub, s) for j in range(exposure_count(n_frames, fi, fo, sh, s))]


class ExposureStream:
    """``exposure_schedule`` for a stream of unknown length: call :meth:`feed` once per arriving frame; it
    returns the outputs that frame completes (an output is complete when its last sample time is
    ``<= frames - 1``), in order.  After ``n`` calls the outputs returned so far are
    ``exposure_schedule(n, fps_in, fps_out, shutter, samples)``."""

    def __init__(self, fps_in, fps_out, shutter, samples):
        self.fps_in, self.fps_out, self.shutter, self.samples = _exposure_args(fps_in, fps_out, shutter, samples)
        self.step = self.fps_in / self.fps_out
        self.sub = self.shutter * self.step / self.samples
        self.frames = 0   # frames fed
        self.outputs = 0  # outputs returned

    def feed(self) -> list:
        self.frames += 1
        out = []
        while self.outputs * self.step + (self.samples - 1) * self.sub <= self.frames - 1:
            out.append(_output(self.outputs, self.step, self.sub, self.samples))
            self.outputs += 1
        return out
