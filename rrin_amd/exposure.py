"""A synthetic shutter: an output frame as the mean of ``S`` frames across an exposure window (the
definition).

A camera at the target rate records the integral of the scene over its shutter, not a point sample.
The network makes that integral cheap to approximate: average ``S`` frames interpolated at sub-times
across the window.  :mod:`rrin_amd.retime` says which samples an output has (``exposure_schedule``:
``tau(j, k) = j * step + k * shutter * step / S``, a left Riemann sum, ``(pair, t) = (floor tau, frac
tau)``); this module says what the exposed frame is, given the samples.

**A sample.**  ``t == 0`` is input frame ``pair`` itself, taken from the stack and never sent to the
network (``pair == P`` of a ``[P+1]`` stack is legal only so).  ``t > 0`` is item ``(pair, float(t))`` of
``Net.interpolate_items_*`` on the stack, with that call's keywords.

**The exposed frame.**  Per stored element ``e`` of the frame's storage -- every byte or word of it,
chroma planes and an extra ``plane=`` included -- with the ``S`` sample frames ``s_0 .. s_{S-1}``:

    out[e] = ((sum_k s_k[e]) + S // 2) // S << shift

where ``s_k[e] = min(word >> shift, maxval)`` is the sample reading of every byte path
(``FrameFormat.wide``); for uint8, ``shift = 0`` and ``maxval = 255``.  Ties round up, the weights are
equal, and ``S <= 256`` so that a sum stays far inside 32 bits (65535 * 256).  The mean is over CODE
VALUES, as everything on the byte paths is: no transfer function is applied, so on gamma-coded
material a bright streak comes out darker than a camera's linear-light integral would make it.

**S = 1.**  The formula gives the single sample back (``(s + 0) // 1``): an item forward's output bit
for bit (its samples never exceed ``maxval``).  For ``t == 0`` the Y4M pipe (``convert.expose_y4m``)
writes the input frame's own bytes without touching the device, exactly as ``retime_y4m`` passes
frames through; that differs from the formula only for words above ``maxval``, which the formula
clamps.  So for ``fps_out > fps_in``, ``S = 1`` reproduces ``retime.schedule`` and its conversion.

**The gate.**  With ``scene_threshold`` or ``gate`` the network items inherit their pair's decision
exactly as in ``interpolate_items_*`` (a duplicate pair: the first frame; a cut pair: the nearer frame
by the item's own t) and are averaged as they come out.  An exposure window that spans a cut therefore
mixes frames of both shots, as a real shutter open across a splice would.

**Linear light and weights** (``light=``, ``weights=``; :func:`mean_frames_linear`).  A shutter integrates
light, not code values.  With a transfer table ``lin`` of the material's curve (:mod:`rrin_amd.transfer`:
``"srgb"``, ``"bt1886"``, ``"gamma22"``, ``"pq"``, ``"hlg"`` or the caller's own, ``lin[c]`` in ``[0, 2**30]``) and
integer weights ``w_k`` with sum ``W <= 65535`` (:func:`shutter_weights`: ``"box"``, ``"triangle"`` or a list):

    v = ((sum_k w_k * lin[s_k[e]]) + W // 2) // W          out[e] = enc(v) << shift

``enc`` the nearest code in linear light (``transfer.encode``), all in 64-bit integers.  Under sRGB the mean
of codes 0 and 255 is 187 or 188, not 128.  On YUV the rule applies per pixel and channel of the RGB that
the path's two integer conversions define (``yuv.yuv_to_rgb`` in, ``yuv.rgb_to_yuv`` out); a table needs
``depth <= 12``.  Without a table (``weights`` alone) it is the weighted mean of code values per stored
element, at any depth, and with box weights the formula above bit for bit.  An extra ``plane=`` is a
matte, depth or ID plane and has no curve: it always takes the weighted mean of code values.

On the device (include/rrin_hip.h, csrc/exposure.hip): ``rrin_mean_frames``, one launch per call of
``Net.expose_items_*`` (a second one for ``plane=``) behind the item forwards on their stream; the sources
are a table of frame pointers -- views of the stack and of the item forwards' outputs, nothing copied.
With ``light`` or ``weights`` the launch is ``rrin_mean_frames_lut``, on YUV with a table
``rrin_mean_frames_yuv_lut`` (csrc/exposure_linear.hip): the table in LDS, the same pointer table with the
weights beside it.

Not covered: ``NetGraph`` capture, ``precision="fp32_planar"``, the float ``Net.forward``, autograd,
multi-GPU sharding, PNG folders, ``evaluate``, 16-bit RGB above 12 bits with ``light``, chroma-siting-aware
resampling (chroma is replicated in and block-averaged out, as on every YUV path).

Host only: plain torch and Python, nothing here touches a device or loads the library.
"""
from __future__ import annotations

from fractions import Fraction

import torch

from .plane import check_format
from .plane import samples as read_samples
from .retime import MAX_SAMPLES


def mean_frames(frames: torch.Tensor, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """The exposed frame of ``S`` sample frames: ``frames`` ``[S, ...]`` uint8 (``depth`` 8) or uint16
    (``depth`` 9..16, the sample ``shift`` bits up) -> ``[...]`` of the same dtype, the formula of the
    module docstring in int64."""
    check_format(depth, shift)
    if frames.dim() < 1 or not 1 <= frames.shape[0] <= MAX_SAMPLES:
        raise ValueError(f"an exposure has 1..{MAX_SAMPLES} sample frames, got {tuple(frames.shape)}")
    s = frames.shape[0]
    total = read_samples(frames, depth, shift).to(torch.int64).sum(dim=0)
    q = ((total + s // 2) // s) << shift
    return q.to(torch.uint8) if depth == 8 else q.to(torch.int16).view(torch.uint16)


def check_groups(groups, n_pairs: int) -> list:
    """The host check of the ``groups`` of an ``expose_items_*`` call over a stack of ``n_pairs + 1`` frames,
    before anything is uploaded: ``G >= 1`` groups of 1..256 samples ``(pair, t)``; ``pair`` an int in
    ``[0, n_pairs]``, ``t`` (a float, an int or a Fraction) in [0, 1), ``pair == n_pairs`` only with ``t ==
    0``; the times ``pair + t`` non-decreasing over the flattened list.  Returns the groups as lists of
    ``(int pair, float t)``; TypeError / ValueError otherwise."""
    if isinstance(groups, (str, bytes, torch.Tensor)) or not hasattr(groups, "__iter__"):
        raise TypeError("groups is a list of lists of (pair, t)")
    if n_pairs < 1:
        raise ValueError("an exposure needs a stack of at least two frames")
    out, prev = [], (0, 0.0)
    for g, group in enumerate(groups):
        if isinstance(group, (str, bytes, torch.Tensor)) or not hasattr(group, "__iter__"):
            raise TypeError(f"groups[{g}] is a list of (pair, t), got {group!r}")
        items = []
        for it in group:
            if not isinstance(it, (tuple, list)) or len(it) != 2:
                raise TypeError(f"groups[{g}] holds (pair, t), got {it!r}")
            p, t = it
            if isinstance(p, bool) or not isinstance(p, int):
                raise ValueError(f"groups[{g}]: pair must be an int, got {p!r}")
            if isinstance(t, bool) or not isinstance(t, (int, float, Fraction)):
                raise ValueError(f"groups[{g}]: t must be a number, got {t!r}")
            tf = float(t)
            if not 0.0 <= tf < 1.0:
                raise ValueError(f"groups[{g}]: t = {t!r} is outside [0, 1)")
            if not 0 <= p <= n_pairs or (p == n_pairs and tf != 0.0):
                raise ValueError(f"groups[{g}]: sample ({p}, {t!r}) is outside a stack of {n_pairs + 1} frames")
            if (p, tf) < prev:
                raise ValueError(f"groups[{g}]: times must be non-decreasing, got ({p}, {t!r}) after {prev}")
            prev = (p, tf)
            items.append((p, tf))
        if not 1 <= len(items) <= MAX_SAMPLES:
            raise ValueError(f"groups[{g}] has {len(items)} samples, an exposure has 1..{MAX_SAMPLES}")
        out.append(items)
    if not out:
        raise ValueError("groups is empty")
    return out


def chunks(groups, chunk: int) -> list:
    """The network items (``t > 0``) of checked ``groups`` in order, cut into consecutive runs of at most
    ``chunk``: per run ``(first frame, last frame, [pair - first frame], [t])`` -- ``frames[first : last +
    1]`` is the view of the stack the run's ``interpolate_items_*`` call works on."""
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"chunk must be an int >= 1, got {chunk!r}")
    net = [(p, t) for group in groups for p, t in group if t != 0.0]
    runs = []
    for i in range(0, len(net), chunk):
        part = net[i:i + chunk]
        lo, hi = part[0][0], part[-1][0] + 1
        runs.append((lo, hi, [p - lo for p, _ in part], [t for _, t in part]))
    return runs


SHUTTERS = ("box", "triangle")
MAX_WEIGHT = 65535  # of one weight and of a group's sum W: W * lin <= 65535 * 2**30 < 2**46


def shutter_weights(kind, s: int) -> list:
    """The ``s`` integer weights of a shutter: ``"box"`` (or None) all 1, ``"triangle"`` ``w_k = min(k + 1, s -
    k)``; an explicit list of ``s`` ints, each in 1..65535, is returned checked.  The sum ``W`` is at most
    65535 (ValueError otherwise: ``W * lin`` must stay below 2**46)."""
    if isinstance(s, bool) or not isinstance(s, int) or not 1 <= s <= MAX_SAMPLES:
        raise ValueError(f"an exposure has 1..{MAX_SAMPLES} samples, got {s!r}")
    if kind is None or (isinstance(kind, str) and kind == "box"):
        w = [1] * s
    elif isinstance(kind, str) and kind == "triangle":
        w = [min(k + 1, s - k) for k in range(s)]
    elif isinstance(kind, (str, bytes, torch.Tensor)) or not hasattr(kind, "__iter__"):
        raise ValueError(f"weights must be one of {SHUTTERS} or a list of ints, got {kind!r}")
    else:
        w = list(kind)
        if any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_WEIGHT for v in w):
            raise ValueError(f"every shutter weight is an int in 1..{MAX_WEIGHT}, got {w!r}")
        if len(w) != s:
            raise ValueError(f"{len(w)} shutter weights for a group of {s} samples: an explicit list needs every "
                             "group of the call to have that many")
    if sum(w) > MAX_WEIGHT:
        raise ValueError(f"the shutter weights sum to {sum(w)}, above {MAX_WEIGHT}")
    return w


def group_weights(weights, sizes) -> list:
    """:func:`shutter_weights` per group of a call whose groups have ``sizes`` samples: a name applies to
    each group at its own size, an explicit list must fit every group."""
    return [shutter_weights(weights, s) for s in sizes]


def _weighted(s: torch.Tensor, w: list, lin, thr) -> torch.Tensor:
    """int64 samples ``[S, ...]`` -> the int64 mean ``[...]``: ``enc((sum_k w_k lin[s_k] + W // 2) // W)``, or
    without a table ``(sum_k w_k s_k + W // 2) // W``."""
    from . import transfer
    wt = torch.tensor(w, dtype=torch.int64).reshape((-1,) + (1,) * (s.dim() - 1))
    tot = sum(w)
    v = ((wt * (s if lin is None else lin[s])).sum(dim=0) + tot // 2) // tot
    return v if lin is None else transfer.encode(thr, v)


def mean_frames_linear(frames: torch.Tensor, fmt, lin=None, weights=None) -> torch.Tensor:
    """The exposed frame of ``S`` sample frames ``frames`` ``[S, ...]`` of the :class:`FrameFormat` ``fmt`` in
    linear light: ``lin`` a transfer table (:func:`rrin_amd.transfer.as_table`: a name or ``maxval + 1``
    integers) or None, ``weights`` a shutter (:func:`shutter_weights`) with sum ``W``.

    RGB formats (and any format without a table), per stored element with ``s_k = min(word >> shift,
    maxval)``: ``v = (sum_k w_k * lin[s_k] + W // 2) // W``, ``out = enc(v) << shift``; ``lin=None`` means no
    table, ``v = (sum_k w_k * s_k + W // 2) // W`` and ``out = v << shift`` at any depth -- YUV is then
    averaged per stored element with no colour conversion, and with box weights this is
    :func:`mean_frames` bit for bit.  A table needs ``depth <= 12`` (ValueError: it would not fit in LDS).

    YUV formats with a table: every sample frame goes to RGB code values by ``yuv.yuv_to_rgb`` /
    ``yuv_to_rgb16`` with the format's ``coef``, the rule above applies per pixel and channel (shift 0), and
    the result goes back by ``yuv.rgb_to_yuv`` / ``rgb16_to_yuv``: the convention of every YUV forward, the
    RGB result between the two conversions.

    ``S = 1``: the formula as it stands.  On RGB with a strictly increasing table it gives the sample back
    (clamped to ``maxval``); on YUV it is then the sample after one round trip through RGB, which a frame that
    is not itself ``rgb_to_yuv`` of some RGB frame does not survive unchanged."""
    from . import transfer, yuv
    check_format(fmt.depth, fmt.shift)
    if frames.dim() < 1 or not 1 <= frames.shape[0] <= MAX_SAMPLES:
        raise ValueError(f"an exposure has 1..{MAX_SAMPLES} sample frames, got {tuple(frames.shape)}")
    if frames.dtype != fmt.dtype:
        raise TypeError(f"frames of depth {fmt.depth} are {fmt.dtype}, got {frames.dtype}")
    w = shutter_weights(weights, frames.shape[0])
    thr = None
    if lin is not None:
        if fmt.depth > 12:
            raise ValueError(f"light needs a depth of at most 12 bits, got {fmt.depth}: a table of 2**{fmt.depth} "
                             "entries and its thresholds would not fit in LDS")
        lin = transfer.as_table(lin, fmt.depth)
        thr = transfer.thresholds(lin)
    if fmt.layout is None or lin is None:
        q = _weighted(read_samples(frames, fmt.depth, fmt.shift).to(torch.int64), w, lin, thr) << fmt.shift
        return q.to(torch.uint8) if fmt.depth == 8 else q.to(torch.int16).view(torch.uint16)
    if fmt.coef is None:
        raise ValueError("a samples-only format has no matrix: linear light on YUV needs FrameFormat.yuv / yuv16")
    if fmt.depth == 8:
        q = _weighted(yuv.yuv_to_rgb(frames, fmt.layout, fmt.coef).to(torch.int64), w, lin, thr)
        return yuv.rgb_to_yuv(q.to(torch.uint8)[None], fmt.layout, fmt.coef)[0]
    msb = fmt.shift != 0
    rgb = yuv.yuv_to_rgb16(frames, fmt.layout, fmt.coef, fmt.depth, msb)
    q = _weighted(yuv.words_to_int(rgb).to(torch.int64), w, lin, thr)
    return yuv.rgb16_to_yuv(yuv.int_to_words(q)[None], fmt.layout, fmt.coef, fmt.depth, msb)[0]


def expose(frames: torch.Tensor, groups, items, depth: int = 8, shift: int = 0, light=None, weights=None,
           fmt=None) -> torch.Tensor:
    """The definition of ``expose_items_*`` on one stack ``frames`` ``[P+1, ...]``: ``items(pair, t)`` gives
    the frame ``[...]`` of the network item ``(pair, t)``, ``t > 0`` (by definition
    ``interpolate_items_*(frames, [pair], [t], ...)[0]``); output g is :func:`mean_frames` of its samples.
    With ``light`` (a transfer table or its name) and / or ``weights`` (a shutter) output g is
    :func:`mean_frames_linear` of them in ``fmt`` -- default: the element reading of ``depth`` and ``shift``,
    which is every RGB format; a YUV call passes its :class:`FrameFormat`.  Returns ``[G, ...]``."""
    groups = check_groups(groups, frames.shape[0] - 1)
    linear = light is not None or weights is not None
    if linear:
        from .framefmt import FrameFormat
        fmt = FrameFormat.samples(None, depth, shift) if fmt is None else fmt
        per_group = group_weights(weights, [len(group) for group in groups])
    out = []
    for g, group in enumerate(groups):
        srcs = torch.stack([frames[p] if t == 0.0 else items(p, t) for p, t in group])
        out.append(mean_frames_linear(srcs, fmt, light, per_group[g]) if linear else mean_frames(srcs, depth, shift))
    return torch.stack(out)
