"""The Y4M stream drivers: ``interpolate_y4m`` (a fixed number of frames per pair), ``retime_y4m`` (any
higher rate), ``expose_y4m`` (any rate, with a synthetic shutter) and ``evaluate_y4m`` (hold-out PSNR / SSIM).
:mod:`rrin_amd.convert` re-exports them.

A driver is its argument checks, its schedule loop and a ``send`` that picks a step's frames and makes the
model call.  Everything else is shared: :func:`_streams` opens and closes paths, :class:`_StreamDesc` describes
the opened stream (frame path, keywords of every model call, upload, download, writer), :class:`_Steps` keeps
one step in flight while the previous one is written, and :class:`_Outputs` writes pass-through frames and
step outputs in stream order.  Streams are read and written sequentially, never sought.

Nothing of the package is imported at module level (``engine`` imports ``convert``, which imports this)."""
from __future__ import annotations

import contextlib
import math
import os
import time
from collections import deque

import numpy as np
import torch


def frame_path_of(src):
    """The frame path of an opened ``y4m.Reader`` or a ``finetune.Clip``: the suffix of the model's methods
    (``interpolate_<suffix>``, ``interpolate_items_<suffix>``, ``frame_metrics_<suffix>``, ``pair_stats_<suffix>``)
    and their depth keywords -- ``("yuv", {})`` at 8 bits, else ``("yuv16", {"depth": d, "msb": False})``
    (Y4M keeps its samples in the words' low bits)."""
    depth = src.bit_depth
    return ("yuv16", {"depth": depth, "msb": False}) if depth > 8 else ("yuv", {})


@contextlib.contextmanager
def _streams(src, dst=None):
    """``src`` and ``dst`` as binary file objects: a path is opened here and closed on exit, a file object
    (or None) is handed through and left open."""
    with contextlib.ExitStack() as opened:
        if isinstance(src, (str, os.PathLike)):
            src = opened.enter_context(open(src, "rb"))
        if isinstance(dst, (str, os.PathLike)):
            dst = opened.enter_context(open(dst, "wb"))
        yield src, dst


def _single_process():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("interpolate_y4m runs in a single process (a stream has one reader and one writer)")


def _check_batch(batch, strict=False):
    # The drivers' rules differ and are kept as they were: expose_y4m takes an int only (``strict``), while
    # retime_y4m and evaluate_y4m -- and interpolate_y4m, which checks sf and batch together -- only compare.
    if strict:
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"batch must be an int >= 1, got {batch!r}")
    elif batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")


class _StreamDesc:
    """An opened Y4M stream and the model it goes through: the reader ``rd``, the frame geometry, the
    model's methods for the stream's depth and the keywords ``kw`` every model call gets."""

    def __init__(self, src, model, coef, scene_threshold, flow_scale):
        from . import y4m, yuv
        self.rd = rd = y4m.Reader(src, depths=(8, 10, 12), chroma=yuv.CHROMAS)
        self.model = model
        self.width, self.height = rd.width, rd.height
        self.layout = "i" + rd.chroma
        self.suffix, depth_kw = frame_path_of(rd)
        self.dtype = torch.uint16 if depth_kw else torch.uint8
        self.maxval = (1 << rd.bit_depth) - 1
        self.rows = yuv.stack_rows(rd.height, self.layout)  # of a frame in a stack [N, rows, width]
        self.device = next(model.parameters()).device
        self.on_gpu = self.device.type == "cuda"   # a host model (tests) has nothing to pin for and no events
        self.scene_threshold = scene_threshold
        self.gated = scene_threshold is not None
        gate_kw = {"scene_threshold": scene_threshold} if self.gated else {}
        # kept apart from gate_kw, whose truth means "the scene gate is on"; scale 1 passes no keyword
        scale_kw = {} if flow_scale == 1 else {"flow_scale": flow_scale}
        self.depth_kw = depth_kw
        self.kw = dict(layout=self.layout, coef=coef, **depth_kw, **gate_kw, **scale_kw)

    def method(self, prefix):
        """The model's ``<prefix>_yuv`` or ``<prefix>_yuv16``."""
        return getattr(self.model, f"{prefix}_{self.suffix}")

    def rate(self):
        """The stream's frame rate as a Fraction; a header without one raises."""
        from . import retime
        if self.rd.fps_num < 1 or self.rd.fps_den < 1:
            raise ValueError(f"Y4M: the stream has no frame rate to convert (F{self.rd.fps_num}:{self.rd.fps_den})")
        return retime.as_rate(f"{self.rd.fps_num}/{self.rd.fps_den}")

    def writer(self, dst, fps_num, fps_den):
        """A ``y4m.Writer`` of the stream's size and colour-space tag at another rate (writes the header)."""
        from . import y4m, yuv
        return y4m.Writer(dst, self.width, self.height, fps_num, fps_den, self.rd.colorspace, depths=(8, 10, 12),
                          chroma=yuv.CHROMAS)

    def upload(self, frames):
        """The frames (the reader's arrays) as one ``[N, rows, width]`` stack on the model's device, through
        pinned memory."""
        stack = torch.empty((len(frames), self.rows, self.width), dtype=self.dtype, pin_memory=self.on_gpu)
        for j, fr in enumerate(frames):
            stack[j].view(-1).copy_(torch.from_numpy(fr))
        return stack.to(self.device, non_blocking=True)

    def download(self, t, dtype=None):
        """A pinned host tensor with the copy of ``t`` enqueued: valid once the step's event has passed."""
        host = torch.empty(t.shape, dtype=dtype or t.dtype, pin_memory=self.on_gpu)
        host.copy_(t, non_blocking=True)
        return host

    def gate_message(self, what):
        return f"; scene gate (threshold {self.scene_threshold:g}): {what}" if self.gated else ""


class _Steps:
    """The steps on the device, oldest first, one in flight: a step (a dict of the driver's) is retired --
    waited for, range-checked, marked ``done``, handed to ``retired`` and its gate codes counted -- when the
    next one has been submitted, so the host writes one step while the device computes the next."""

    def __init__(self, st, retired):
        self.st, self.retired, self.queue = st, retired, deque()
        self.cuts = self.dups = self.gated = 0   # gate codes 2, 1 and either of the retired steps

    def submit(self, step):
        """Right after the step's model call and downloads: takes the call's gate codes, marks the stream."""
        st = self.st
        step["codes"] = st.download(st.model.last_gate, torch.int32) if st.gated else None
        step["done"], step["ev"] = False, None
        if st.on_gpu:
            step["ev"] = torch.cuda.Event()
            step["ev"].record()
        self.queue.append(step)
        while len(self.queue) > 1:  # retire the previous step while this one computes
            self._retire(self.queue.popleft())

    def _retire(self, step):
        if step["ev"] is not None:
            step["ev"].synchronize()
        if hasattr(self.st.model, "check_range"):
            self.st.model.check_range(wait=False)  # fp16-stored precisions: raise instead of writing poisoned frames
        step["done"] = True
        self.retired(step)
        if step["codes"] is not None:
            self.cuts += int((step["codes"] == 2).sum())
            self.dups += int((step["codes"] == 1).sum())
            self.gated += int((step["codes"] != 0).sum())

    def finish(self):
        while self.queue:
            self._retire(self.queue.popleft())
        if hasattr(self.st.model, "check_range"):
            self.st.model.check_range()


class _Outputs:
    """The outputs not written yet, in stream order: an input frame's own array (a pass-through), None (a
    network output no step holds yet) or ``(step, index in the step's "host")``."""

    def __init__(self, wr):
        self.wr, self.queue = wr, deque()
        self.written = self.passed = 0

    def passthrough(self, frame):
        self.queue.append(frame)
        self.passed += 1

    def reserve(self):
        self.queue.append(None)

    def assign(self, step, n):
        """The step's ``n`` outputs are the oldest unassigned ones, in order."""
        k = 0
        for i, e in enumerate(self.queue):
            if e is None:
                self.queue[i] = (step, k)
                k += 1
                if k == n:
                    break

    def drain(self, _step=None):
        """Writes what is ready at the head: frames, and outputs of retired steps."""
        q = self.queue
        while q and q[0] is not None and (not isinstance(q[0], tuple) or q[0][0].get("done")):
            e = q.popleft()
            self.wr.write(e[0]["host"][e[1]].numpy() if isinstance(e, tuple) else e)
            self.written += 1


def interpolate_y4m(model, src, dst, sf=None, batch=4, scene_threshold=None, coef=None, log=print, fps_out=None,
                    flow_scale=1, samples=None, shutter=None, light=None, weights=None):
    """Interpolate a Y4M stream (8-bit 4:2:0; also 10 / 12 bits and 4:2:2 / 4:4:4, below) into another: no image folder, no RGB frame anywhere.

    ``flow_scale`` 2 or 4 (:mod:`rrin_amd.flowscale`) goes to the model's ``interpolate_*`` call:
    the Flow U-Net runs at 1/s of the frame size.

    ``src`` / ``dst`` are binary file objects (files or pipes: they are read and written
    sequentially, never sought) or paths.  Every step takes the next ``batch`` pairs: their
    ``batch + 1`` frames go to the model's device as one pinned uint8 stack, and
    ``model.interpolate_yuv(stack[:-1], stack[1:], ts, layout="i420")`` runs on two views of it
    with the t schedule of :func:`interpolate_folder`.  The output holds frame k, its ``sf``
    intermediates, ..., the last frame, at ``sf + 1`` times the input's frame rate; the input
    frames pass through as their own bytes.  ``coef`` (``rrin_amd.yuv.coefficients``; None: BT.709
    limited range) and ``scene_threshold`` go to ``interpolate_yuv`` -- the threshold is a mean over
    luma and chroma bytes there, not the RGB path's number, and no value has been validated on
    footage.  Single process: ``WORLD_SIZE`` > 1 raises.  Returns the frames written.

    A 10- or 12-bit stream (``C420p10`` / ``C420p12``: little-endian 16-bit words, the sample in the
    low bits) runs the same way on uint16 stacks through ``model.interpolate_yuv16`` at the
    stream's depth; ``coef`` None is then BT.709 limited range at that depth, ``scene_threshold``
    a mean absolute sample difference in [0, maxval], and the output keeps the input's tag.

    A 4:2:2 or 4:4:4 stream (``C422``, ``C444`` and their ``p10`` / ``p12`` forms) runs through the same
    two calls with ``layout="i422"`` / ``"i444"`` on ``[N, 2*H0, W0]`` / ``[N, 3*H0, W0]`` stacks; the
    output keeps the tag, and ``scene_threshold`` is a mean over the frame's ``2*H0*W0`` / ``3*H0*W0``
    samples.

    Exactly one of ``sf`` and ``fps_out`` is given.  ``fps_out`` (a ``fractions.Fraction``, an int or
    a string ``"60000/1001"`` / ``"60"``, above the stream's rate) converts the frame rate instead:
    :func:`retime_y4m`.

    ``samples`` (an int in 1..256, with ``fps_out``) turns every output into an exposure: the mean of
    ``samples`` frames across a ``shutter`` (a Fraction, an int or a string ``"1/2"`` in (0, 1]; default
    1/2) of the output's frame time, and ``fps_out`` may then be ANY positive rate, lower, equal or
    higher: :func:`expose_y4m`.  Without ``samples`` nothing changes (``shutter`` alone raises).

    ``light`` (the material's transfer curve: ``"srgb"``, ``"bt1886"``, ``"gamma22"``, ``"pq"``, ``"hlg"`` or a
    table, :mod:`rrin_amd.transfer`) takes that mean in linear light and ``weights`` (``"box"``,
    ``"triangle"`` or ``samples`` ints) weighs the samples; Y4M carries no transfer tag, so nothing is
    guessed.  Either without ``samples``, or with ``samples == 1`` (nothing to average), raises."""
    from .flowscale import check_flow_scale
    check_flow_scale(flow_scale)
    if (sf is None) == (fps_out is None):
        raise ValueError("interpolate_y4m takes exactly one of sf and fps_out")
    if samples is None and shutter is not None:
        raise ValueError("shutter needs samples: an exposure is the mean of `samples` frames over the shutter")
    if samples is None and (light is not None or weights is not None):
        raise ValueError("light and weights need samples: they say how the `samples` frames of an exposure are averaged")
    if samples is not None:
        if fps_out is None:
            raise ValueError("samples needs fps_out: an exposure belongs to a frame-rate conversion")
        return expose_y4m(model, src, dst, fps_out, samples, shutter="1/2" if shutter is None else shutter,
                          batch=batch, scene_threshold=scene_threshold, coef=coef, log=log, flow_scale=flow_scale,
                          light=light, weights=weights)
    if fps_out is not None:
        return retime_y4m(model, src, dst, fps_out, batch=batch, scene_threshold=scene_threshold, coef=coef, log=log,
                          flow_scale=flow_scale)
    _single_process()
    if sf < 1 or batch < 1:
        raise ValueError(f"sf and batch must be >= 1, got {sf} / {batch}")
    with _streams(src, dst) as (src, dst):
        st = _StreamDesc(src, model, coef, scene_threshold, flow_scale)
        wr = st.writer(dst, st.rd.fps_num * (sf + 1), st.rd.fps_den)
        ts = [i / (sf + 1) for i in range(1, sf + 1)]
        forward = st.method("interpolate")
        frames = iter(st.rd)
        prev = next(frames, None)
        if prev is None:
            raise ValueError("need at least two frames in the Y4M stream")
        wr.write(prev)
        written, pairs = 1, 0
        t0 = time.time()

        def write(step):
            nonlocal written
            for p, nxt in enumerate(step["inputs"]):
                for i in range(sf):
                    wr.write(step["host"][i][p].numpy())
                wr.write(nxt)
                written += sf + 1

        steps = _Steps(st, write)
        while True:
            group = [prev]
            for fr in frames:
                group.append(fr)
                if len(group) == batch + 1:
                    break
            if len(group) == 1:
                break
            prev = group[-1]
            stack = st.upload(group)
            with torch.no_grad():
                outs = forward(stack[:-1], stack[1:], ts, **st.kw)
            steps.submit({"host": [st.download(o) for o in outs], "inputs": group[1:]})
            pairs += len(group) - 1
        if pairs == 0:
            raise ValueError("need at least two frames in the Y4M stream")
        steps.finish()
        wr.flush()
        log(f"y4m: {pairs} pairs x {sf} frames of {st.width}x{st.height} in {time.time() - t0:.2f} s, {written} frames "
            f"out at {st.rd.fps_num * (sf + 1)}:{st.rd.fps_den} fps"
            + st.gate_message(f"{steps.cuts} cut pairs, {steps.dups} duplicate pairs"))
        return written


def retime_y4m(model, src, dst, fps_out, batch=4, scene_threshold=None, coef=None, log=print, flow_scale=1):
    """Convert the frame rate of a Y4M stream to any higher rate ``fps_out`` (24 -> 60, 24000/1001 ->
    60000/1001, 25 -> 30, ...): ``interpolate_y4m(fps_out=)``.  Output j is the frame at source time
    ``j * fps_in / fps_out`` (:mod:`rrin_amd.retime`): an input frame's own bytes where that time is
    a whole number (a pass-through, never sent to the network), else one item of
    ``model.interpolate_items_yuv`` / ``interpolate_items_yuv16``.  A step takes the next ``batch``
    ITEMS of the schedule, however unevenly they fall on the pairs (at 24 -> 60 a pair gets 3, 2,
    3, 2, ... of them), and uploads the frames they span as one stack, so the device sees full
    batches until the stream ends; the Flow U-Net runs once per pair of a step.  The header
    carries ``fps_out`` reduced; tag, depth, chroma, ``coef`` and ``scene_threshold`` follow the
    stream as in :func:`interpolate_y4m` (a cut pair's items take the nearer frame by their own t).
    Output quality at uneven t has not been validated on footage.  Returns the frames written."""
    from . import retime
    from .flowscale import check_flow_scale
    check_flow_scale(flow_scale)
    _single_process()
    _check_batch(batch)
    rate_out = retime.as_rate(fps_out)
    with _streams(src, dst) as (src, dst):
        st = _StreamDesc(src, model, coef, scene_threshold, flow_scale)
        rate_in = st.rate()
        sched = retime.Stream(rate_in, rate_out)  # raises unless fps_out > fps_in
        order = _Outputs(st.writer(dst, rate_out.numerator, rate_out.denominator))
        steps = _Steps(st, order.drain)
        forward = st.method("interpolate_items")
        t0 = time.time()
        held = {}   # input frames still needed by an item, by index
        items = []  # network items (pair, float t) not sent yet
        n_in = 0

        def send(part):
            lo, hi = part[0][0], part[-1][0] + 1
            stack = st.upload([held[j] for j in range(lo, hi + 1)])
            with torch.no_grad():
                out = forward(stack, [p - lo for p, _ in part], [t for _, t in part], **st.kw)
            step = {"host": st.download(out)}
            order.assign(step, len(part))
            for j in [j for j in held if j < part[-1][0]]:  # later items start at the last pair
                del held[j]
            steps.submit(step)

        for fr in st.rd:
            held[n_in] = fr
            n_in += 1
            for pair, t in sched.feed():
                if t == 0:  # time == pair: the frame that has just arrived
                    order.passthrough(fr)
                else:
                    order.reserve()  # assigned when its step is sent
                    items.append((pair, float(t)))
            while len(items) >= batch:
                send(items[:batch])
                del items[:batch]
            order.drain()
        if n_in < 2:
            raise ValueError("need at least two frames in the Y4M stream")
        if items:
            send(items)
        steps.finish()
        order.wr.flush()
        log(f"y4m: {n_in} frames of {st.width}x{st.height} at {rate_in.numerator}:{rate_in.denominator} fps -> "
            f"{order.written} frames at {rate_out.numerator}:{rate_out.denominator} fps in {time.time() - t0:.2f} s, "
            f"{order.passed} of them input frames passed through"
            + st.gate_message(f"{steps.gated} items replaced by an input frame"))
        return order.written


def expose_y4m(model, src, dst, fps_out, samples, shutter="1/2", batch=4, scene_threshold=None, coef=None, log=print,
               flow_scale=1, light=None, weights=None):
    """Convert a Y4M stream to ANY frame rate ``fps_out`` -- lower (60 -> 24, 120 -> 24), equal or higher
    -- with a synthetic shutter: ``interpolate_y4m(fps_out=, samples=)``.  Output j is the mean of
    ``samples`` frames at the source times ``j * step + k * shutter * step / samples``, ``step = fps_in /
    fps_out`` (:func:`rrin_amd.retime.exposure_schedule`; :mod:`rrin_amd.exposure` is the definition of the
    mean: per stored byte or word, ties up, over code values -- no transfer function is applied).
    Frames are fed to ``retime.ExposureStream``.  A step takes the next whole outputs until they hold at
    least ``batch`` network items (or ``4 * batch`` outputs, which bounds a step whose samples all fall on
    input frames), uploads the input frames they use as one pinned stack and calls
    ``model.expose_items_yuv`` / ``expose_items_yuv16(stack, groups, chunk=batch, ...)``; one step is in
    flight while the previous one is written.  An input frame that no later output needs is dropped as it
    arrives (at 120 -> 24 with a 1/2 shutter two frames in five never go up).  An output with ``samples ==
    1`` that falls on an input frame is written as that frame's own bytes, as :func:`retime_y4m` does, so
    ``samples=1`` above the input's rate is that conversion.  The header carries ``fps_out`` reduced; tag,
    depth, chroma, ``coef``, ``scene_threshold`` and ``flow_scale`` follow the stream as there (an exposure
    across a cut mixes both shots).  Returns the frames written.

    ``light`` and ``weights`` go to ``expose_items_*``: the mean in linear light under the named transfer
    curve (or a table of the stream's depth), with a box or triangle shutter or ``samples`` explicit integer
    weights (:func:`rrin_amd.exposure.mean_frames_linear`).  With ``samples == 1`` there is nothing to
    average and either raises; the header is the same with and without them."""
    from . import exposure, retime, transfer
    from .flowscale import check_flow_scale
    check_flow_scale(flow_scale)
    _single_process()
    _check_batch(batch, strict=True)
    rate_out = retime.as_rate(fps_out)
    n_samples = retime.check_samples(samples)
    sh = retime.as_shutter(shutter)
    light_kw = {}
    if light is not None or weights is not None:
        if n_samples == 1:
            raise ValueError("light and weights need samples > 1: one sample leaves nothing to average")
        exposure.shutter_weights(weights, n_samples)
        if isinstance(light, str) and light not in transfer.CURVES:
            raise ValueError(f"light must be one of {transfer.NAMES} or a table, got {light!r}")
        light_kw = {"light": light, "weights": weights}
    with _streams(src, dst) as (src, dst):
        st = _StreamDesc(src, model, coef, scene_threshold, flow_scale)
        rate_in = st.rate()
        if light is not None:
            transfer.as_table(light, st.rd.bit_depth)  # a table must fit the stream's depth: refuse before any output
        sched = retime.ExposureStream(rate_in, rate_out, sh, n_samples)
        order = _Outputs(st.writer(dst, rate_out.numerator, rate_out.denominator))
        steps = _Steps(st, order.drain)
        forward = st.method("expose_items")
        t0 = time.time()
        held = {}        # input frames an unsent or a future output needs, by index
        ready = deque()  # complete outputs not sent yet: (output index, its samples (pair, Fraction t))
        n_in = 0

        def uses(output):
            """The input frames an output reads: its samples' frames, and the next one where t > 0."""
            need = set()
            for pair, t in output:
                need.add(pair)
                if t != 0:
                    need.add(pair + 1)
            return need

        def send(outputs):
            """One step: ``outputs`` on the stack of the frames they use.  The frames two used pairs
            share are adjacent in it; a frame no sample reads is not in it (the outputs of a decimation
            leave gaps), which moves no pair: both frames of a network item are always there."""
            need = sorted(set().union(*[uses(o) for o in outputs]))  # two frames at least: samples > 1 or t > 0
            pos = {j: i for i, j in enumerate(need)}
            stack = st.upload([held[j] for j in need])
            groups = [[(pos[p], float(t)) for p, t in o] for o in outputs]
            with torch.no_grad():
                out = forward(stack, groups, chunk=batch, **st.kw, **light_kw)
            step = {"host": st.download(out)}
            order.assign(step, len(outputs))
            steps.submit(step)

        def forget():
            """Drops the frames before the first one that the oldest unsent output, or if there is none
            the next output to come, reads."""
            first = (ready[0][0] if ready else sched.outputs) * sched.step
            first = first.numerator // first.denominator
            for j in [j for j in held if j < first]:
                del held[j]

        def take(final: bool):
            """Sends steps while the ready outputs hold ``batch`` network items or ``4 * batch`` outputs
            (``final``: whatever is left)."""
            while ready:
                n_items, n_out = 0, 0
                for _, o in ready:
                    n_out += 1
                    n_items += sum(1 for _, t in o if t != 0)
                    if n_items >= batch or n_out >= 4 * batch:
                        break
                else:
                    if not final:
                        return
                send([ready.popleft()[1] for _ in range(n_out)])
                forget()

        for fr in st.rd:
            held[n_in] = fr
            first = sched.outputs
            for j, output in enumerate(sched.feed(), first):
                if n_samples == 1 and output[0][1] == 0:  # the frame that has just arrived, as its own bytes
                    order.passthrough(fr)
                else:
                    ready.append((j, output))
                    order.reserve()
            n_in += 1
            take(False)
            forget()
            order.drain()
        if n_in < 2:
            raise ValueError("need at least two frames in the Y4M stream")
        take(True)
        steps.finish()
        order.wr.flush()
        msg = (f"y4m: {n_in} frames of {st.width}x{st.height} at {rate_in.numerator}:{rate_in.denominator} fps -> "
               f"{order.written} frames at {rate_out.numerator}:{rate_out.denominator} fps, each the mean of "
               f"{n_samples} samples over a {sh.numerator}/{sh.denominator} shutter, in {time.time() - t0:.2f} s, "
               f"{order.passed} of them input frames passed through")
        if light_kw:
            curve = light if isinstance(light, str) else "a custom table"
            shape = weights if isinstance(weights, str) else ("box" if weights is None else "explicit")
            msg += (f"; the mean in {'code values' if light is None else 'linear light under ' + curve}, "
                    f"{shape} weights")
        log(msg + st.gate_message(f"{steps.gated} items replaced by an input frame"))
        return order.written


def _finite(values):
    """Floats for a report: an infinite PSNR (no sample differs) is None, JSON's null."""
    return [float(v) if math.isfinite(v) else None for v in values]


def _summarise(sse, ssim, counts, maxval):
    """The summary of one side (interpolated or baseline): ``sse`` / ``ssim`` lists of per-row lists."""
    from .metrics import psnr
    names = range(len(counts))
    per_row = [[psnr(r[p], counts[p], maxval) for p in names] for r in sse]
    finite = [[r[p] for r in per_row if math.isfinite(r[p])] for p in names]
    total = [sum(r[p] for r in sse) for p in names]
    return {
        # mean over the rows whose PSNR is finite (a frame equal to the truth has none)
        "psnr_mean": [sum(f) / len(f) if f else None for f in finite],
        # from the summed squared error: per plane, and over all samples of all planes
        "psnr_global": _finite([psnr(total[p], counts[p] * len(sse), maxval) for p in names]),
        "psnr_global_all": _finite([psnr(sum(total), sum(counts) * len(sse), maxval)])[0],
        "ssim_mean": [sum(r[p] for r in ssim) / len(ssim) for p in names],
    }


def evaluate_y4m(model, src, hold=2, batch=4, scene_threshold=None, coef=None, log=print, report=None, flow_scale=1):
    """Hold-out evaluation on a Y4M clip (any tag :func:`interpolate_y4m` takes): what PSNR and SSIM
    does this model reach on this footage, at the model's precision, with this gate -- and what does
    it gain over repeating a frame?

    Frames ``k*hold`` are the inputs.  The ``hold - 1`` frames between two inputs are held out and
    interpolated back at ``t = j/hold`` (``rrin_amd.metrics.holdout_schedule``), ``batch`` items per
    ``model.interpolate_items_yuv`` / ``_yuv16`` call, so the Flow U-Net runs once per pair of a step;
    frames after the last input are ignored (the log line counts them); fewer than ``hold + 1``
    frames raise ValueError.  Each interpolated frame is compared with the frame that was dropped,
    per Y, U and V plane, by ``model.frame_metrics_yuv`` / ``_yuv16`` (:mod:`rrin_amd.metrics`; on the
    device, on the forward's stream), and so is the *baseline*: the nearer input frame by t (a tie
    takes the first), which is what a player shows without interpolation.  A step's numbers come to
    the host once, behind the next step's launch.

    Hold-out measures at ``hold`` times the clip's frame spacing, so it understates the quality at
    the clip's own spacing; it compares models, precisions and gates on the same footage.

    Returns ``{"summary": ..., "rows": [...]}`` and writes it as JSON to ``report`` (a path or a text
    file object) when given.  A row: ``frame``, ``pair``, ``t``, ``gate`` (the item's code: 0
    interpolated, 1 / 2 replaced by the first / second input), ``sse`` / ``psnr`` / ``ssim`` per plane,
    and the same under ``baseline``.  The summary: per plane the mean PSNR (over rows where it is
    finite), the PSNR of the summed squared error (also over all planes together) and the mean
    SSIM, the same for the baseline, ``cut_pairs`` / ``duplicate_pairs`` (with ``scene_threshold``),
    ``precision``, ``hold``, ``flow_scale``, the stream's ``tag`` and the frame counts.  An infinite
    PSNR is None.

    ``flow_scale`` 2 or 4 (:mod:`rrin_amd.flowscale`) goes to the ``interpolate_items_*`` call: this is
    how to judge the knob on one's own footage."""
    import json

    from . import metrics
    from .flowscale import check_flow_scale
    check_flow_scale(flow_scale)
    hold = metrics._hold(hold)
    _check_batch(batch)
    with _streams(src) as (src, _):
        st = _StreamDesc(src, model, coef, scene_threshold, flow_scale)
        w0, h0, maxval = st.width, st.height, st.maxval
        deep = st.dtype == torch.uint16
        name = "frame_metrics_" + st.suffix
        measure = getattr(model, name, None) or getattr(metrics, name)  # a host model: the definitions
        forward = st.method("interpolate_items")
        counts = [p[3] * p[4] for p in metrics.planes_of("yuv", h0, w0, st.layout)]
        t0 = time.time()
        held = {}   # frames still needed, by index
        items = []  # (frame, pair, Fraction t) not sent yet
        rows = []
        pair_dup, pair_gated = {}, set()

        def report_rows(step):
            sse, val = step["sse"].tolist(), step["ssim"].tolist()
            codes = step["codes"].tolist() if step["codes"] is not None else [0] * len(step["part"])
            for k, (frame, pair, t) in enumerate(step["part"]):
                if codes[k]:
                    pair_gated.add(pair)
                row = {"frame": frame, "pair": pair, "t": float(t), "gate": int(codes[k])}
                for key, side in ((None, 0), ("baseline", 1)):
                    d = {"sse": [int(v) for v in sse[side][k]],
                         "psnr": _finite([metrics.psnr(v, c, maxval) for v, c in zip(sse[side][k], counts)]),
                         "ssim": [float(v) for v in val[side][k]]}
                    if key is None:
                        row.update(d)
                    else:
                        row[key] = d
                rows.append(row)

        steps = _Steps(st, report_rows)

        def send(part):
            lo, hi = part[0][1], part[-1][1] + 1  # the inputs lo .. hi, then the truth frames, as one stack
            n_in_ = hi - lo + 1
            near = torch.tensor([p - lo + metrics.nearer_input(t) for _, p, t in part], dtype=torch.int64)
            if st.on_gpu:
                near = near.pin_memory()
            stack = st.upload([held[j * hold] for j in range(lo, hi + 1)] + [held[frame] for frame, _, _ in part])
            near = near.to(st.device, non_blocking=True)
            inputs, truth = stack[:n_in_], stack[n_in_:]
            with torch.no_grad():
                out = forward(inputs, [p - lo for _, p, _ in part], [float(t) for _, _, t in part], **st.kw)
                got = measure(out, truth, layout=st.layout, **st.depth_kw)
                # 16-bit frames are gathered as the same bits: index_select has no uint16 kernel everywhere
                nearer = (inputs.view(torch.int16).index_select(0, near).view(torch.uint16) if deep
                          else inputs.index_select(0, near))
                base = measure(nearer, truth, layout=st.layout, **st.depth_kw)
                sse = torch.stack((got.sse, base.sse))
                val = torch.stack((got.ssim, base.ssim))
            step = {"part": part, "sse": st.download(sse), "ssim": st.download(val)}
            sent = {frame for frame, _, _ in part}
            for j in [j for j in held if j in sent or j < part[-1][1] * hold]:  # later items start at the last pair
                del held[j]
            steps.submit(step)

        n_in = 0
        for fr in st.rd:
            held[n_in] = fr
            n_in += 1
            if n_in - 1 >= hold and (n_in - 1) % hold == 0:  # the second input of a pair has arrived
                pair = (n_in - 1) // hold - 1
                if st.gated:  # a duplicate pair, as the gate sees it: no sample differs
                    first = held[pair * hold]
                    pair_dup[pair] = bool(np.array_equal(np.minimum(first, maxval), np.minimum(fr, maxval)))
                items.extend(metrics.holdout_pair_items(pair, hold))
                while len(items) >= batch:
                    send(items[:batch])
                    del items[:batch]
        _, ignored = metrics.holdout_schedule(n_in, hold)  # fewer than hold + 1 frames: ValueError
        if items:
            send(items)
        steps.finish()
        dups = sum(1 for v in pair_dup.values() if v)
        summary = {"tag": "C" + st.rd.colorspace, "width": w0, "height": h0, "bit_depth": st.rd.bit_depth,
                   "planes": list(metrics.YUV_NAMES), "precision": getattr(model, "precision", None), "hold": hold,
                   "batch": batch, "scene_threshold": scene_threshold, "flow_scale": flow_scale, "frames": n_in, "held_out": len(rows),
                   "ignored": ignored, "cut_pairs": sum(1 for p in pair_gated if not pair_dup.get(p)),
                   "duplicate_pairs": dups}
        summary.update(_summarise([r["sse"] for r in rows], [r["ssim"] for r in rows], counts, maxval))
        summary["baseline"] = _summarise([r["baseline"]["sse"] for r in rows], [r["baseline"]["ssim"] for r in rows],
                                         counts, maxval)
        log(f"evaluate: {len(rows)} held-out frames of {n_in} ({w0}x{h0}, hold {hold}) in {time.time() - t0:.2f} s; "
            f"{ignored} frames after the last input ignored")
        result = {"summary": summary, "rows": rows}
        if report is not None:
            if isinstance(report, (str, os.PathLike)):
                with open(report, "w") as f:
                    json.dump(result, f, indent=1, allow_nan=False)
            else:
                json.dump(result, report, indent=1, allow_nan=False)
        return result
