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

On the device (include/rrin_hip.h, csrc/exposure.hip): ``rrin_mean_frames``, one launch per call of
``Net.expose_items_*`` (a second one for ``plane=``) behind the item forwards on their stream; the sources
are a table of frame pointers -- views of the stack and of the item forwards' outputs, nothing copied.

Not covered: ``NetGraph`` capture, ``precision="fp32_planar"``, the float ``Net.forward``, autograd,
multi-GPU sharding, PNG folders, ``evaluate``, non-uniform shutter weights, linear-light averaging.

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


def expose(frames: torch.Tensor, groups, items, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """The definition of ``expose_items_*`` on one stack ``frames`` ``[P+1, ...]``: ``items(pair, t)`` gives
    the frame ``[...]`` of the network item ``(pair, t)``, ``t > 0`` (by definition
    ``interpolate_items_*(frames, [pair], [t], ...)[0]``); output g is :func:`mean_frames` of its samples.
    Returns ``[G, ...]``."""
    groups = check_groups(groups, frames.shape[0] - 1)
    out = []
    for group in groups:
        srcs = [frames[p] if t == 0.0 else items(p, t) for p, t in group]
        out.append(mean_frames(torch.stack(srcs), depth, shift))
    return torch.stack(out)
