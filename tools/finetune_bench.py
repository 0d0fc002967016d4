#!/usr/bin/env python3
"""The fine-tuning step on an MI355X, and its two own kernels against PyTorch operators.

1. Steps per second of the whole step of ``finetune.finetune_y4m`` -- ``sample_triplets``, ``Net.forward``
   under autograd, ``frame_loss``, ``backward``, AdamW -- at ``--crop`` / ``--batch`` over a synthetic
   in-memory 4:2:0 clip: host clock around ``--steps`` steps that end in a device synchronise,
   ``--rounds`` windows after a warm-up.
2. ``sample_triplets`` + ``frame_loss`` (value and gradient) against the same two definitions
   written with PyTorch operators on the device -- the comparison, since there is no other such
   path -- timed with HIP events over ``--calls`` calls a window, alternately, ``--rounds`` windows each.
3. The share of the whole step that the two fused calls take.
4. With ``--vgg``: the step with the perceptual term (``autograd.perceptual_loss`` at ``w_vgg`` 0.1 over keyed
   synthetic weights at VGG19's real widths -- no kernel's time depends on the values), windows with and
   without the term alternating, and the term's own share of the step from ``autograd.PROF`` (HIP events
   around each of its launches over ``--prof-steps`` further steps).

Prints one JSON line.  Not a test; needs a GPU.  One process; ``--time-limit`` seconds end it.

    python tools/finetune_bench.py --crop 256 --batch 2
"""
from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rrin_amd import Net, autograd, yuv  # noqa: E402
from rrin_amd import finetune as ft  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict  # noqa: E402


def torch_sample(frames, items, ch, cw, h0, w0):
    """sample_triplets for 8-bit i420 with PyTorch operators on the device: crop, then convert."""
    k = yuv.coefficients()
    outs = ([], [], [])
    for it in items:
        for j in range(3):
            fr = frames[it[j]]
            y = fr[:h0][it.y0:it.y0 + ch, it.x0:it.x0 + cw].to(torch.int32)
            c = fr[h0:].reshape(2, h0 // 2, w0 // 2)[:, it.y0 // 2:(it.y0 + ch) // 2, it.x0 // 2:(it.x0 + cw) // 2]
            c = c.to(torch.int32).repeat_interleave(2, 1).repeat_interleave(2, 2) - 128
            a = (y - k.y0) * k.ay + 8192
            rgb = torch.stack((a + k.rv * c[1], a + k.gu * c[0] + k.gv * c[1], a + k.bu * c[0]))
            x = (rgb >> 14).clamp_(0, 255).float().div_(255.0)
            if it.flip:
                x = x.flip(2 if it.flip == 1 else 1)
            outs[j].append(x)
    return tuple(torch.stack(o) for o in outs)


def torch_loss(out, tgt):
    """frame_loss and its gradient with PyTorch fp32 operators and autograd."""
    out = out.detach().requires_grad_()
    d = out - tgt
    loss = ft.W_CHARB * torch.sum(torch.sqrt(d * d + ft.EPS)) / out.shape[0] + ft.W_L1 * d.abs().mean()
    loss.backward()
    return loss, out.grad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="steps of a timed window of the whole step")
    ap.add_argument("--calls", type=int, default=200, help="calls of a timed window of the two kernels")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=540)
    ap.add_argument("--vgg", action="store_true", help="also time the step with the VGG19 perceptual term")
    ap.add_argument("--prof-steps", type=int, default=3, help="--vgg: steps under autograd.PROF")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs a ROCm device")
    signal.alarm(a.time_limit)
    dev = torch.device("cuda:0")
    h0, w0, ch = a.height, a.width, a.crop
    g = torch.Generator().manual_seed(1)
    # unrelated random bytes: no kernel's time depends on the values
    frames = torch.randint(0, 256, (a.frames, 3 * h0 // 2, w0), generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
    net = net.to(dev).train()
    optim = torch.optim.AdamW(net.parameters(), lr=1e-4)
    sched = ft.triplet_schedule(a.frames, (h0, w0), (2, 2), (2,), a.warmup + a.steps * a.rounds, a.batch, ch, 0)
    vgg = None
    if a.vgg:
        from rrin_amd.perceptual import VggFeatures
        vgg = VggFeatures.synthetic()

    def step(s, term=False):
        i0, it, i1 = ft.sample_triplets(frames, s.items, ch, "i420")
        optim.zero_grad(set_to_none=True)
        out = net(i0, i1, float(s.t))
        loss = autograd.frame_loss(out, it)
        if term:
            loss = loss + 0.1 * autograd.perceptual_loss(out, it, vgg)
        loss.backward()
        optim.step()

    for s in sched[:a.warmup]:
        step(s)
    torch.cuda.synchronize(dev)
    if a.vgg:
        for s in sched[:a.warmup]:
            step(s, True)
        torch.cuda.synchronize(dev)
    step_ms, vgg_ms = [], []
    for r in range(a.rounds):
        part = sched[a.warmup + r * a.steps:a.warmup + (r + 1) * a.steps]
        for term, dest in ((False, step_ms), (True, vgg_ms))[:2 if a.vgg else 1]:   # alternating windows
            t0 = time.perf_counter()
            for s in part:
                step(s, term)
            torch.cuda.synchronize(dev)
            dest.append((time.perf_counter() - t0) * 1e3 / len(part))
    vgg_report = {}
    if a.vgg:
        autograd.PROF = []
        for s in sched[a.warmup:a.warmup + a.prof_steps]:
            step(s, True)
        torch.cuda.synchronize(dev)
        events, autograd.PROF = autograd.PROF, None
        by_kind = {}
        for e0, e1, _, kind in events:
            if kind.startswith("vgg_"):   # the term's launches (a conv as a whole; its kernel is also under fwd / dgrad)
                by_kind[kind] = by_kind.get(kind, 0.0) + e0.elapsed_time(e1) / a.prof_steps
        med_vgg = statistics.median(vgg_ms)
        vgg_report = {"step_ms_vgg": [round(x, 2) for x in vgg_ms], "median_step_ms_vgg": round(med_vgg, 2),
                      "vgg_event_ms_per_step": {k: round(v, 3) for k, v in sorted(by_kind.items())},
                      "vgg_event_ms_total": round(sum(by_kind.values()), 3),
                      "vgg_share_of_step": round(sum(by_kind.values()) / med_vgg, 4),
                      "record_buffers_cached": len(autograd._R32_BUFS or ()), "record_buffers_max": autograd.R32_BUFS_MAX}

    items = sched[0].items
    out = torch.rand((a.batch, 3, ch, ch), generator=g).to(dev)

    def fused():
        i0, it, i1 = ft.sample_triplets(frames, items, ch, "i420")
        loss = autograd.frame_loss(out.requires_grad_(), it)
        loss.backward()
        out.grad = None

    def plain():
        i0, it, i1 = torch_sample(frames, items, ch, ch, h0, w0)
        torch_loss(out, it)

    # the two spellings agree before they are timed: the triplets to the last bit of x / 255 (a device division by
    # a scalar in PyTorch is a multiply by its reciprocal; the kernel divides), the loss to fp32 rounding
    fa, fb = ft.sample_triplets(frames, items, ch, "i420"), torch_sample(frames, items, ch, ch, h0, w0)
    diff = max((x - y).abs().max().item() for x, y in zip(fa, fb))
    la = autograd.frame_loss(out.detach(), fa[1]).item()
    lb = torch_loss(out, fb[1])[0].item()

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.calls   # microseconds per call

    calls = {"fused": fused, "torch_ops": plain}
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            us[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in us.items()}
    ms = statistics.median(step_ms)
    print(json.dumps({
        "what": "fine-tuning step (host clock, ms per step) and sample_triplets + frame_loss against PyTorch "
                "operators (HIP events, us per call, one value per window)",
        "device": torch.cuda.get_device_name(0), "frame": [h0, w0], "crop": ch, "batch": a.batch,
        "step_ms": [round(x, 2) for x in step_ms], "median_step_ms": round(ms, 2), "steps_per_s": round(1e3 / ms, 2),
        "us_per_call": {k: [round(x, 1) for x in v] for k, v in us.items()},
        "median_us": {k: round(v, 1) for k, v in med.items()},
        "torch_ops_over_fused": round(med["torch_ops"] / med["fused"], 2),
        "fused_share_of_step": round(med["fused"] / (ms * 1e3), 4),
        "triplets_max_abs_diff": diff, "loss_fused": la, "loss_torch_ops": lb, **vgg_report}))


if __name__ == "__main__":
    main()
