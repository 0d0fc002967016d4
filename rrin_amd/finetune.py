"""Fine-tuning on a Y4M clip: hold frames out as ``convert.evaluate_y4m`` does and train on (first
input, held-out truth, second input) crops of the clip itself.

What is carried over from the reference: its random crop and flip (dataloader.py:36-51,132-138),
its two loss terms that need no downloaded weights with their weights (``charbonnierLoss / 1e3 +
L1Loss / 10``: losses.py:39-42, train.py:105), AdamW at 1e-4 (train.py:49) and its checkpoint
(train.py:158-161).  The VGG19 perceptual term of ``CombinedLoss`` (losses.py:6-36) is optional: it
needs a weights file that is already on disk (:mod:`rrin_amd.perceptual`; ``finetune_y4m(vgg=)``).
What is not: the learning-rate schedule, PNG folders and the resize branch of the data loader.  The
whole clip stays on the device.

As with :mod:`rrin_amd.yuv` and :mod:`rrin_amd.metrics` the functions here are the *definition*;
on a device ``csrc/finetune.hip`` computes the same (the sampler bit for bit, the loss within a few
fp32 roundings per term).

Triplets.  An item is ``(frame0, frame_t, frame1, y0, x0, flip)`` over one frame stack: the crop of
``crop = (ch, cw)`` pixels at rows ``y0 ..``, columns ``x0 ..`` *of the frame* (``convert``'s padding
rows are never sampled) of the three frames, each converted like the frame paths' input --
``convert.frames_u8_to_float(yuv.yuv_to_rgb(frame, layout, coef))`` for bytes,
``convert.frames_u16_to_float(yuv.yuv_to_rgb16(frame, layout, coef, depth, msb), depth)`` for 16-bit
words, the colour conversion left out for ``layout="rgb"`` -- then flipped: 0 none, 1 left-right, 2
top-bottom (the reference's ``flip_map``).  Chroma is replicated over its block, so the conversion
commutes with a crop whose origin is a multiple of the block; that alignment is a precondition.

Loss.  With ``d = out - target`` over ``[N,C,H,W]`` (count elements)::

    sums = (sum sqrt(d^2 + eps), sum |d|, sum d^2)
    loss = w_charb * sums[0] / N + w_l1 * sums[1] / count
    grad = w_charb / N * d / sqrt(d^2 + eps) + w_l1 / count * sign(d)        (sign(0) = 0)
"""
from __future__ import annotations

import ctypes as C
import math
import os
import random
import time
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import metrics, yuv
from .framefmt import check_depth, frame_stride

MAX_ITEMS = 64   # RRIN_TRIPLET_MAX_ITEMS: items of one sampler call
W_CHARB, W_L1, EPS = 1e-3, 1e-1, 1e-6   # train.py:105, losses.py:40

Item = namedtuple("Item", "frame0 frame_t frame1 y0 x0 flip")
Step = namedtuple("Step", "span j t reversed items")
Step.__doc__ = """One step of :func:`triplet_schedule`: the span s, the held-out position j, the step's time
``t`` (a Fraction: j/s, or 1 - j/s when ``reversed``) and its ``batch`` :class:`Item`."""


# ---- the loss ----------------------------------------------------------------------------------
def frame_loss_parts_ref(out, target, w_charb=W_CHARB, w_l1=W_L1, eps=EPS):
    """(sums float64 ``[3]``, grad float64 like ``out``) of the module docstring's definition, in
    float64 on the tensors' device."""
    d = out.detach().double() - target.detach().double()
    s = torch.sqrt(d * d + eps)
    sums = torch.stack((s.sum(), d.abs().sum(), (d * d).sum()))
    grad = (w_charb / out.shape[0]) * d / s + (w_l1 / d.numel()) * torch.sign(d)
    return sums, grad


def frame_loss_ref(out, target, w_charb=W_CHARB, w_l1=W_L1, eps=EPS):
    """The loss of the module docstring in PyTorch float64, differentiable through ``out``: the
    definition ``autograd.frame_loss`` is tested against, and the loss of the CPU loop.  The defaults
    are the reference's ``charbonnierLoss / 1e3 + L1Loss / 10`` (no VGG19 term)."""
    d = out.double() - target.double()
    return w_charb * torch.sqrt(d * d + eps).sum() / out.shape[0] + w_l1 * d.abs().sum() / d.numel()


# ---- the schedule --------------------------------------------------------------------------------
def _crop2(crop):
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    ch, cw = int(ch), int(cw)
    if ch < 16 or cw < 16 or ch % 16 or cw % 16:
        raise ValueError(f"the crop must be a positive multiple of 16 in both directions, got {ch}x{cw}")
    return ch, cw


def triplet_schedule(n_frames, size, block=(2, 2), spans=(2,), steps=1, batch=2, crop=256, seed=0, augment=True,
                     cut_pairs=()):
    """The training triplets of ``steps`` steps over frames ``[0, n_frames)`` of ``size = (H0, W0)``
    pixels with chroma ``block = (rows, columns)``: a list of :class:`Step`.  Pure host code; the same
    arguments give the same schedule on every machine.

    A step has one span ``s`` of ``spans`` and one ``j`` in ``1..s-1``, so one ``t = j/s`` (the training
    forward takes one t per call), and ``batch`` items ``frame0 = a, frame_t = a + j, frame1 = a + s``
    whose pairs ``(a, a+1) .. (a+s-1, a+s)`` avoid ``cut_pairs`` (pair p is frames p and p + 1).  With
    ``augment`` the crop's origin is uniform over the block-aligned positions that fit, the flip
    uniform over 0..2, and the step's direction reversed with probability 1/2: frame0 and frame1
    swap and ``t`` becomes ``1 - j/s``.  Without it: origin (0, 0), flip 0, forward.

    The generator is ``random.Random(seed)``; its draws, in order, per step:
    ``randrange(len(spans))`` (the span), ``randrange(1, s)`` (j), with ``augment`` ``randrange(2)`` (1:
    reversed); then per item ``randrange(len(starts))`` (a, over the ascending list of starts valid
    for s) and, with ``augment``, ``randrange(rows)`` (y0 / block rows), ``randrange(columns)`` (x0 /
    block columns), ``randrange(3)`` (flip).

    ValueError: fewer than ``max(spans) + 1`` frames, a crop larger than the frame or no multiple of
    16, a span below 2, a span that ``cut_pairs`` leaves no triplet for, ``steps < 0``, ``batch < 1``."""
    h0, w0 = int(size[0]), int(size[1])
    by, bx = int(block[0]), int(block[1])
    ch, cw = _crop2(crop)
    spans = tuple(int(s) for s in spans)
    if not spans or any(s < 2 for s in spans):
        raise ValueError(f"spans must be ints >= 2, got {spans!r}")
    if n_frames < max(spans) + 1:
        raise ValueError(f"a span of {max(spans)} needs at least {max(spans) + 1} training frames, got {n_frames}")
    if ch > h0 or cw > w0:
        raise ValueError(f"a {ch}x{cw} crop does not fit a {h0}x{w0} frame")
    if steps < 0 or batch < 1:
        raise ValueError(f"steps must be >= 0 and batch >= 1, got {steps} / {batch}")
    cuts = {int(p) for p in cut_pairs}
    starts = {}
    for s in spans:
        starts[s] = [a for a in range(n_frames - s) if not any(p in cuts for p in range(a, a + s))]
        if not starts[s]:
            raise ValueError(f"the cut pairs leave no triplet of span {s} in {n_frames} frames")
    rows, cols = (h0 - ch) // by + 1, (w0 - cw) // bx + 1
    rng = random.Random(seed)
    out = []
    for _ in range(steps):
        s = spans[rng.randrange(len(spans))]
        j = rng.randrange(1, s)
        rev = bool(rng.randrange(2)) if augment else False
        items = []
        for _ in range(batch):
            a = starts[s][rng.randrange(len(starts[s]))]
            y0 = x0 = flip = 0
            if augment:
                y0, x0, flip = by * rng.randrange(rows), bx * rng.randrange(cols), rng.randrange(3)
            first, last = (a + s, a) if rev else (a, a + s)
            items.append(Item(first, a + j, last, y0, x0, flip))
        t = Fraction(j, s)
        out.append(Step(s, j, 1 - t if rev else t, rev, items))
    return out


# ---- the sampler -----------------------------------------------------------------------------------
def _frame_kind(frames, layout, depth):
    """(h0, w0, planes, (block rows, block columns)) of a stack of ``layout`` ("rgb" or a YUV one)."""
    want = torch.uint8 if depth == 8 else torch.uint16
    if not isinstance(frames, torch.Tensor) or frames.dtype != want:
        raise TypeError(f"frames of depth {depth} are a {str(want).split('.')[-1]} stack")
    if layout == "rgb":
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"expected [N,H0,W0,3] RGB frames, got {tuple(frames.shape)}")
        h0, w0 = frames.shape[1], frames.shape[2]
        return h0, w0, metrics.planes_of("rgb", h0, w0), (1, 1)
    if frames.dim() != 3:
        raise ValueError(f"expected a [N, rows, W0] stack of {layout}, got {tuple(frames.shape)}")
    h0, w0 = yuv.stack_size(frames, layout)
    return h0, w0, metrics.planes_of("yuv", h0, w0, layout), yuv.block_of(yuv.chroma_of(layout))


def _check_items(items, n_frames, h0, w0, ch, cw, block):
    items = [Item(*(int(v) for v in it)) for it in items]
    if not 1 <= len(items) <= MAX_ITEMS:
        raise ValueError(f"a sampler call takes 1..{MAX_ITEMS} items, got {len(items)}")
    for it in items:
        if any(not 0 <= f < n_frames for f in it[:3]):
            raise ValueError(f"frame index outside [0, {n_frames}): {it}")
        if it.flip not in (0, 1, 2):
            raise ValueError(f"flip is 0, 1 or 2: {it}")
        if not (0 <= it.y0 <= h0 - ch and 0 <= it.x0 <= w0 - cw):
            raise ValueError(f"the {ch}x{cw} crop of {it} leaves the {h0}x{w0} frame")
        if it.y0 % block[0] or it.x0 % block[1]:
            raise ValueError(f"the origin of {it} is off the {block[0]}x{block[1]} chroma block")
    return items


def _depth_of(depth, layout, coef):
    check_depth(depth, 8, "depth is 8 or 9..16")
    if layout == "rgb":
        if coef is not None:
            raise ValueError("RGB frames take no colour coefficients")
    elif depth != 8:
        yuv.check_depth16(depth)
    return depth


def _sample_ref(frames, items, ch, cw, layout, coef, depth, msb):
    """The definition, on any device: whole frames through the frame paths' input mapping, then the
    crop (below the mapping's padding rows) and the flip."""
    from . import convert
    cache = {}

    def whole(f):
        if f not in cache:
            fr = frames[f:f + 1]
            if depth == 8:
                rgb = fr if layout == "rgb" else yuv.yuv_to_rgb(fr, layout, coef)
                cache[f] = convert.frames_u8_to_float(rgb)
            else:
                rgb = fr if layout == "rgb" else yuv.yuv_to_rgb16(fr, layout, coef, depth, msb)
                cache[f] = convert.frames_u16_to_float(rgb, depth)
        return cache[f]

    outs = ([], [], [])
    for it in items:
        for k in range(3):
            x = whole(it[k])
            top = x.shape[2] - (frames.shape[1] if layout == "rgb" else yuv.stack_size(frames, layout)[0])
            x = x[:, :, top + it.y0:top + it.y0 + ch, it.x0:it.x0 + cw]
            if it.flip:
                x = x.flip(3 if it.flip == 1 else 2)
            outs[k].append(x)
    return tuple(torch.cat(o).contiguous() for o in outs)


def sample_triplets(frames, items, crop, layout="i420", coef=None, depth=8, msb=False):
    """(I0, It, I1), each fp32 ``[K,3,ch,cw]`` on the frames' device: the K ``items`` (see the module
    docstring) over ``frames`` -- uint8 (``depth`` 8) or uint16 stacks ``[N, rows, W0]`` of a YUV
    ``layout`` of :data:`rrin_amd.yuv.ALL_LAYOUTS`, or ``[N,H0,W0,3]`` with ``layout="rgb"`` (then ``coef``
    stays None and 16-bit depths are 9..16, samples in the low bits).  ``coef`` None is BT.709 limited
    range at the depth; ``msb`` reads 16-bit YUV samples from the words' high bits.  On a ROCm
    device one kernel (rrin_triplet_crop_u8 / _u16), on the CPU the definition; the same bits.
    ValueError for an item that is out of bounds, off the chroma block or has a bad flip, for more
    than :data:`MAX_ITEMS` items and for a crop that is no positive multiple of 16."""
    ch, cw = _crop2(crop)
    depth = _depth_of(depth, layout, coef)
    h0, w0, planes, block = _frame_kind(frames, layout, depth)
    items = _check_items(items, frames.shape[0], h0, w0, ch, cw, block)
    if frames.device.type != "cuda":
        return _sample_ref(frames, items, ch, cw, layout, coef, depth, msb)
    from . import _lib
    lib = _lib.lib()
    stride = frame_stride(frames)
    if stride is None:
        frames = frames.contiguous()
        stride = frame_stride(frames)
    k = len(items)
    arr = (_lib.Plane * 3)(*[_lib.Plane(off, pitch, step, h, w, 0) for off, step, pitch, h, w in planes])
    flat = (C.c_int32 * (6 * k))(*[v for it in items for v in it])
    kc = None if layout == "rgb" else C.byref(_lib.YuvCoef(*yuv.as_coef(coef, depth)))
    outs = [torch.empty((k, 3, ch, cw), dtype=torch.float32, device=frames.device) for _ in range(3)]
    st = C.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream)
    ptrs = [o.data_ptr() for o in outs]
    if depth == 8:
        _lib.check(lib.rrin_triplet_crop_u8(frames.data_ptr(), stride, frames.shape[0], arr, flat, k, ch, cw, kc,
                                            *ptrs, st), "rrin_triplet_crop_u8")
    else:
        shift = 16 - depth if (msb and layout != "rgb") else 0
        _lib.check(lib.rrin_triplet_crop_u16(frames.data_ptr(), stride, frames.shape[0], arr, flat, k, ch, cw, kc,
                                             depth, shift, *ptrs, st), "rrin_triplet_crop_u16")
    return tuple(outs)


# ---- the clip, validation and the loop -------------------------------------------------------------
class Clip:
    """A Y4M clip as one frame stack on a device: ``frames`` ``[N, rows, W0]`` of ``layout`` ("i420",
    "i422" or "i444"), uint8 or, at ``depth`` 10 / 12, uint16 (samples in the low bits); ``tag`` the
    stream's colour-space tag; ``truncated`` whether the read stopped at ``max_bytes``."""

    def __init__(self, frames, layout, depth, width, height, tag, truncated):
        self.frames, self.layout, self.depth = frames, layout, depth
        self.width, self.height, self.tag, self.truncated = width, height, tag, truncated

    @property
    def bit_depth(self):
        """``depth``, under the name a ``y4m.Reader`` gives it."""
        return self.depth

    @property
    def kw(self):
        """The depth arguments of the 16-bit frame paths ({} at 8 bits)."""
        from .convert import frame_path_of
        return frame_path_of(self)[1]


def read_clip(src, device, max_bytes=8 << 30):
    """The frames of a Y4M stream (a path or a binary file object; every format ``convert --y4m_in``
    takes) as a :class:`Clip` on ``device``; stops before the frame that would pass ``max_bytes``."""
    from . import y4m
    opened = None
    if isinstance(src, (str, os.PathLike)):
        src = opened = open(src, "rb")
    try:
        rd = y4m.Reader(src, depths=(8, 10, 12), chroma=yuv.CHROMAS)
        layout = "i" + rd.chroma
        got, truncated = [], False
        for fr in rd:
            if (len(got) + 1) * rd.frame_bytes > max_bytes:
                truncated = True
                break
            got.append(fr)
        if not got:
            raise ValueError("the Y4M stream has no frame (or max_bytes is below one frame)")
        rows = yuv.stack_rows(rd.height, layout)
        host = np.stack(got).reshape(len(got), rows, rd.width)
        if rd.bit_depth > 8:
            stack = torch.from_numpy(host.view(np.int16)).view(torch.uint16)
        else:
            stack = torch.from_numpy(host)
        return Clip(stack.to(device), layout, rd.bit_depth, rd.width, rd.height, "C" + rd.colorspace, truncated)
    finally:
        if opened is not None:
            opened.close()


def _host_forward(model, clip, f0, f1, t, coef):
    """``Net.forward_yuv`` / ``forward_yuv16`` by their definition, with PyTorch operators: for a model on a
    CPU device."""
    from . import convert
    deep = clip.depth > 8
    if deep:
        a, b = (convert.frames_u16_to_float(yuv.yuv_to_rgb16(f, clip.layout, coef, clip.depth, False), clip.depth)
                for f in (f0, f1))
    else:
        a, b = (convert.frames_u8_to_float(yuv.yuv_to_rgb(f, clip.layout, coef)) for f in (f0, f1))
    with torch.enable_grad():   # the PyTorch-operator graph of a CPU model is its autograd path
        out = model._forward_autograd(a, b, t).detach()
    if deep:
        return yuv.rgb16_to_yuv(convert.frames_float_to_u16(out, clip.height, clip.width, clip.depth), clip.layout,
                                coef, clip.depth, False)
    return yuv.rgb_to_yuv(convert.frames_float_to_u8(out, clip.height, clip.width), clip.layout, coef)


def validate(model, clip, first=0, hold=2, batch=4, coef=None):
    """Hold-out squared error of ``model`` on the frames ``first ..`` of ``clip``: the items of
    ``metrics.holdout_schedule`` (frames ``first + k*hold`` are inputs, the ones between are interpolated
    back at ``t = j/hold`` and compared with the originals), under ``no_grad``, ``batch`` items per call.
    On a ROCm device ``Net.interpolate_items_yuv`` / ``_yuv16`` and the on-device metrics; on the CPU
    their definitions.  Returns ``{"frames": [...], "sse": [[y, u, v], ...] (exact ints), "psnr":
    [[...]], "psnr_global_all": float or None, "ignored": frames after the last input}``; None if
    fewer than ``hold + 1`` frames are left."""
    frames = clip.frames[first:]
    n = frames.shape[0]
    if n < hold + 1:
        return None
    items, ignored = metrics.holdout_schedule(n, hold)
    on_gpu = frames.device.type == "cuda"
    deep = clip.depth > 8
    planes = metrics.planes_of("yuv", clip.height, clip.width, clip.layout)
    counts = [p[3] * p[4] for p in planes]
    maxval = (1 << clip.depth) - 1
    from .convert import frame_path_of
    suffix = frame_path_of(clip)[0]
    name = "frame_metrics_" + suffix
    measure = getattr(model, name) if on_gpu else getattr(metrics, name)

    def take(idx):
        i = torch.tensor(idx, dtype=torch.int64, device=frames.device)
        return frames.view(torch.int16).index_select(0, i).view(torch.uint16) if deep else frames.index_select(0, i)

    inputs = take(list(range(0, n, hold))[:(n - 1) // hold + 1])
    sse = []
    with torch.no_grad():
        for lo in range(0, len(items), batch):
            part = items[lo:lo + batch]
            truth = take([f for f, _, _ in part])
            if on_gpu:
                fwd = getattr(model, "interpolate_items_" + suffix)
                p0 = part[0][1]
                out = fwd(inputs[p0:part[-1][1] + 2], [p - p0 for _, p, _ in part], [float(t) for _, _, t in part],
                          layout=clip.layout, coef=coef, **clip.kw)
            else:
                out = torch.cat([_host_forward(model, clip, inputs[p:p + 1], inputs[p + 1:p + 2], float(t), coef)
                                 for _, p, t in part])
            sse.extend(measure(out, truth, layout=clip.layout, ssim=False, **clip.kw).sse.tolist())
    total = sum(sum(r) for r in sse)
    psnr_all = metrics.psnr(total, sum(counts) * len(sse), maxval)
    return {"frames": [first + f for f, _, _ in items], "sse": [[int(v) for v in r] for r in sse],
            "psnr": [[(lambda v: v if math.isfinite(v) else None)(metrics.psnr(v, c, maxval))
                      for v, c in zip(r, counts)] for r in sse],
            "psnr_global_all": psnr_all if math.isfinite(psnr_all) else None, "ignored": ignored}


def excluded_pairs(model, clip, n, scene_threshold):
    """(cut pairs, duplicate pairs) among the first ``n`` frames, as the scene gate of the frame
    paths sees them: pair p (frames p, p + 1) is a duplicate if no sample differs and a cut if its sum
    of absolute sample differences exceeds ``convert.scene_limit_len(scene_threshold, samples)``
    (``Net.pair_stats_yuv`` / ``_yuv16`` on a ROCm device, the same sum in PyTorch on the CPU)."""
    from . import convert
    if n < 2:
        return [], []
    f0, f1 = clip.frames[:n - 1], clip.frames[1:n]
    if clip.frames.device.type == "cuda":
        sad = getattr(model, "pair_stats_" + convert.frame_path_of(clip)[0])(f0, f1, layout=clip.layout, **clip.kw)
    else:
        a, b = metrics.samples_of(f0, clip.depth, 0), metrics.samples_of(f1, clip.depth, 0)
        sad = (a - b).abs().reshape(n - 1, -1).sum(1)
    sad = sad.tolist()
    limit = convert.scene_limit_len(scene_threshold, clip.frames[0].numel(), (1 << clip.depth) - 1)
    return [p for p, v in enumerate(sad) if v > limit], [p for p, v in enumerate(sad) if v == 0]


def finetune_y4m(model, src, steps, batch=2, crop=256, spans=(2,), lr=1e-4, seed=0, scene_threshold=None,
                 val_fraction=0.1, max_bytes=8 << 30, save=None, augment=True, log=print, log_every=50, coef=None,
                 epoch=0, vgg=None, w_vgg=0.1):
    """Fine-tune ``model`` on the Y4M clip ``src`` (a path or a binary file object; every format
    ``convert --y4m_in`` takes), in place, on the model's device.

    The clip is read into one frame stack on the device (:func:`read_clip`; it stops at ``max_bytes``
    and the log says so).  The last ``max(ceil(val_fraction * N), spans[0] + 1)`` frames (none at
    ``val_fraction`` 0) are never sampled: they are measured before and after the loop by
    :func:`validate` with ``hold = spans[0]``.  With ``scene_threshold`` the cut and duplicate pairs of
    the training frames (:func:`excluded_pairs`) are kept out of the schedule.  Every step of
    :func:`triplet_schedule` (``seed``, ``augment``) runs :func:`sample_triplets`, ``model(I0, I1, t)``
    under autograd, the loss (``autograd.frame_loss``; on the CPU :func:`frame_loss_ref` over
    ``Net._forward_autograd``), ``backward`` and ``torch.optim.AdamW(lr)`` (train.py:49).  There is no
    learning-rate schedule.  The CPU path is slow: it is there for tests and for checking.

    ``vgg``: a :class:`rrin_amd.perceptual.VggFeatures` or the path of a VGG19 state dict on disk (read
    before the clip; the file is never fetched).  The loss is then ``frame_loss + w_vgg *
    perceptual_loss(out, truth, vgg)``, the reference's ``CombinedLoss / 10 + charbonnierLoss / 1e3``
    (train.py:105) at the default ``w_vgg`` (``autograd.perceptual_loss``; on the CPU
    ``perceptual.perceptual_loss``).  None (default): no such term, and nothing else changes.

    Returns ``{"losses": [float per step], "logged": [{"step", "loss", "sums", "psnr"} for every
    ``log_every``-th step and the last], "val_before", "val_after" (:func:`validate`'s dicts or None),
    "schedule" (the steps), "cut_pairs", "duplicate_pairs" (counts of excluded pairs), "frames",
    "train_frames", "val_frames", "truncated", "tag", "vgg" (the weights' file name, "synthetic", or None),
    "w_vgg", "perceptual" ([the unweighted term per step], empty without ``vgg``; the logged steps carry
    it too)}``.  ``save``: a path that gets ``{'model':
    state_dict, 'optim': ..., 'epoch': epoch + 1}`` on the CPU, the reference's checkpoint
    (train.py:158-161), which ``convert.load_net`` and a reference ``--resume`` read."""
    from .autograd import frame_loss
    device = next(model.parameters()).device
    if vgg is not None:   # before the clip is read: a missing or mismatching file ends the call here
        from . import perceptual
        if not isinstance(vgg, perceptual.VggFeatures):
            vgg = perceptual.VggFeatures.load(vgg)
        if not math.isfinite(w_vgg):
            raise ValueError(f"w_vgg must be finite, got {w_vgg!r}")
    on_gpu = device.type == "cuda"
    spans = tuple(int(s) for s in spans)
    ch, cw = _crop2(crop)
    if not 0.0 <= val_fraction < 1.0:
        raise ValueError(f"val_fraction is in [0, 1), got {val_fraction!r}")
    t_start = time.time()
    clip = read_clip(src, device, max_bytes)
    n = clip.frames.shape[0]
    if clip.truncated:
        log(f"finetune: stopped reading at max_bytes = {max_bytes}: {n} frames kept")
    hold = spans[0]
    n_val = max(math.ceil(n * val_fraction - 1e-9), hold + 1) if val_fraction > 0 else 0
    n_train = n - n_val
    cuts, dups = (excluded_pairs(model, clip, n_train, scene_threshold) if scene_threshold is not None
                  else ([], []))
    block = yuv.block_of(yuv.chroma_of(clip.layout))
    schedule = triplet_schedule(n_train, (clip.height, clip.width), block, spans, steps, batch, (ch, cw), seed,
                                augment, sorted(set(cuts) | set(dups)))
    val_before = validate(model, clip, n_train, hold, coef=coef) if n_val else None
    optim = torch.optim.AdamW(model.parameters(), lr=lr)
    count = batch * 3 * ch * cw
    losses, logged, percs = [], [], []
    pending = []   # (step, loss tensor, sums tensor, perceptual term): read on the host at the logged steps only
    if vgg is not None and not on_gpu:
        vgg = vgg.to(device)
    for k, step in enumerate(schedule):
        i0, it, i1 = sample_triplets(clip.frames, step.items, (ch, cw), clip.layout, coef, clip.depth)
        t = float(step.t)
        optim.zero_grad(set_to_none=True)
        if on_gpu:
            out = model(i0, i1, t)
            loss, sums = frame_loss(out, it, W_CHARB, W_L1, EPS, return_sums=True)
        else:
            out = model._forward_autograd(i0, i1, t)
            loss = frame_loss_ref(out, it)
            sums = frame_loss_parts_ref(out, it)[0]
        perc = None
        if vgg is not None:
            if on_gpu:
                from .autograd import perceptual_loss
                perc = perceptual_loss(out, it, vgg)
            else:
                perc = perceptual.perceptual_loss(out, it, vgg).double()
            loss = loss + w_vgg * perc
            perc = perc.detach()
        loss.backward()
        optim.step()
        pending.append((k + 1, loss.detach(), sums, perc))
        if (k + 1) % log_every == 0 or k + 1 == len(schedule):
            for s_, l_, m_, p_ in pending:   # one trip to the host per logged step
                losses.append(float(l_))
                if p_ is not None:
                    percs.append(float(p_))
            m = [float(v) for v in sums.tolist()]
            psnr = 10.0 * math.log10(count / m[2]) if m[2] > 0 else None   # train.py:112-113
            logged.append({"step": k + 1, "loss": losses[-1], "sums": m, "psnr": psnr})
            line = (f"step: {k + 1:5d}, psnr {psnr if psnr is None else round(psnr, 4)}, loss {losses[-1]:8.6f} "
                    f"charb {W_CHARB * m[0] / batch:8.6f}, l1 {W_L1 * m[1] / count:8.6f}")
            if vgg is not None:
                logged[-1]["perceptual"] = percs[-1]
                line += f", vgg {w_vgg * percs[-1]:8.6f}"
            log(line)
            pending = []
    val_after = validate(model, clip, n_train, hold, coef=coef) if n_val else None
    if save is not None:
        state = {"model": {k_: v.detach().cpu() for k_, v in model.state_dict().items()},
                 "optim": optim.state_dict(), "epoch": int(epoch) + 1}
        torch.save(state, save)
    if on_gpu:
        torch.cuda.synchronize(device)
    log(f"finetune: {len(schedule)} steps of {batch} x {ch}x{cw} on {n_train} of {n} frames ({clip.width}x{clip.height} "
        f"{clip.tag}) in {time.time() - t_start:.2f} s; {len(cuts)} cut and {len(dups)} duplicate pairs excluded")
    return {"losses": losses, "logged": logged, "val_before": val_before, "val_after": val_after,
            "schedule": schedule, "cut_pairs": len(cuts), "duplicate_pairs": len(dups), "frames": n,
            "train_frames": n_train, "val_frames": n_val, "truncated": clip.truncated, "tag": clip.tag,
            "vgg": None if vgg is None else vgg.name, "w_vgg": None if vgg is None else float(w_vgg),
            "perceptual": percs}


def finetune(args):
    """``finetune --y4m_in PATH|- --steps N [...]``: :func:`finetune_y4m` on the checkpoint of ``--model_name``
    (loaded as ``convert`` loads it); writes ``models/<name><epoch+1:04d>.pth`` and prints the summary."""
    import json
    import sys

    from . import convert
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("finetune runs in a single process (WORLD_SIZE > 1)")
    if args.no_cuda or not torch.cuda.is_available():
        raise RuntimeError("rrin_amd runs on ROCm GPUs only")
    dev = torch.device("cuda", torch.cuda.current_device())
    vgg = None
    if getattr(args, "vgg_weights", None):   # first: a missing or mismatching file is an error before the clip is read
        from .perceptual import VGG19_RELU4_4, VggFeatures
        vgg = VggFeatures.load(args.vgg_weights, getattr(args, "vgg_cfg", None) or VGG19_RELU4_4)
    path = convert.find_checkpoint(args.model_name)
    state = torch.load(path, map_location="cpu", weights_only=True)
    epoch = int(state.get("epoch", 0)) if isinstance(state, dict) and "model" in state else 0
    net = convert.load_net(args.model_name, dev)
    dest = os.path.join("models", f"{args.model_name}{epoch + 1:04d}.pth")
    res = finetune_y4m(net, sys.stdin.buffer if args.y4m_in == "-" else args.y4m_in, args.steps, batch=args.batch,
                       crop=args.crop, spans=args.spans, lr=args.lr, seed=args.seed,
                       scene_threshold=args.scene_threshold, val_fraction=args.val_fraction, save=dest,
                       augment=not args.no_augment, epoch=epoch, vgg=vgg, w_vgg=getattr(args, "w_vgg", 0.1))
    print(f"Saved {dest}.")
    res["schedule"] = [{"span": s.span, "j": s.j, "t": float(s.t), "reversed": s.reversed,
                        "items": [list(i) for i in s.items]} for s in res["schedule"]]
    summary = {k: v for k, v in res.items() if k not in ("schedule", "losses", "perceptual")}
    summary["checkpoint"] = dest
    print(json.dumps(summary, indent=1))
    if args.report:
        res["checkpoint"] = dest
        with open(args.report, "w") as f:
            json.dump(res, f, indent=1)
    return res
