#!/usr/bin/env python3
"""How much of a convert step is frame I/O: one step of interpolate_folder's two pipelines on
synthetic in-memory frames, timed with HIP events (no image decode / encode, no files).

  byte chain   pinned uint8 [n+1,H,W,3] stack -> one H2D -> Net.interpolate_u8 -> uint8 D2H
  float chain  pinned fp32 [n,3,H',W'] i0, i1 -> two H2D  -> Net.interpolate    -> fp32 D2H

and, on one CPU core, the host work per frame that the byte chain removes: load_frame's pad /
permute / float / divide and to_uint8_image's multiply / truncate / crop / permute.

The two chains are timed alternately (``--rounds`` windows of ``--steps`` steps each, after
``--warmup`` steps of both); every window is one pair of events around its steps.  Prints one
JSON line.  Not a test; needs a GPU.

``--scene-threshold X`` adds a third chain to every round: the byte chain with the scene gate on
(``interpolate_u8(..., scene_threshold=X)``).  The synthetic frames are unrelated random bytes
(mean absolute difference about 85), so any X below that gates -- and copies -- every frame, the
gate's dearest case; X = 255 gates none and times the sums alone.

    python tools/u8_io_bench.py --height 720 --width 1280 --pairs 4 --sf 1 --precision fp32
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rrin_amd import Net  # noqa: E402
from rrin_amd import convert as cv  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict  # noqa: E402


def host_cost(h0, w0, reps):
    """Seconds per frame, one thread: (load_frame without the decode, to_uint8_image)."""
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    arr = rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)
    top, right = cv.pad_amounts(w0, h0)
    meta = {"top": top, "height": h0, "width": w0}

    def load():
        a = np.pad(arr, ((top, 0), (0, right), (0, 0)), mode="edge") if top or right else arr
        return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0)

    t = load()
    cv.to_uint8_image(t, meta)
    t0 = time.perf_counter()
    for _ in range(reps):
        load()
    t1 = time.perf_counter()
    for _ in range(reps):
        cv.to_uint8_image(t, meta)
    t2 = time.perf_counter()
    return (t1 - t0) / reps, (t2 - t1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--sf", type=int, default=1)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--scene-threshold", type=float, default=None,
                    help="also time the byte chain with the scene gate at this threshold")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("u8_io_bench needs a ROCm device")
    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=True))
    net.precision = a.precision
    net = net.to(dev).eval()
    n, h0, w0 = a.pairs, a.height, a.width
    ts = [i / (a.sf + 1) for i in range(1, a.sf + 1)]
    rng = np.random.default_rng(1)
    stack8 = torch.from_numpy(rng.integers(0, 256, (n + 1, h0, w0, 3), dtype=np.uint8)).pin_memory()
    fl = cv.frames_u8_to_float(stack8).contiguous()
    i0h, i1h = fl[:-1].contiguous().pin_memory(), fl[1:].contiguous().pin_memory()
    out8 = [torch.empty((n, h0, w0, 3), dtype=torch.uint8).pin_memory() for _ in ts]
    out32 = [torch.empty(tuple(i0h.shape), dtype=torch.float32).pin_memory() for _ in ts]

    def step_u8():
        s = stack8.to(dev, non_blocking=True)
        for o, h in zip(net.interpolate_u8(s[:-1], s[1:], ts), out8):
            h.copy_(o, non_blocking=True)

    def step_u8_gated():
        s = stack8.to(dev, non_blocking=True)
        for o, h in zip(net.interpolate_u8(s[:-1], s[1:], ts, scene_threshold=a.scene_threshold), out8):
            h.copy_(o, non_blocking=True)

    def step_f32():
        i0, i1 = i0h.to(dev, non_blocking=True), i1h.to(dev, non_blocking=True)
        for o, h in zip(net.interpolate(i0, i1, ts), out32):
            h.copy_(o, non_blocking=True)

    def window(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    with torch.no_grad():
        for _ in range(a.warmup):
            step_u8()
            step_f32()
        torch.cuda.synchronize(dev)
        net.check_range()
        same = all(np.array_equal(o8.numpy(), cv.frames_float_to_u8(o32, h0, w0).numpy())
                   for o8, o32 in zip(out8, out32))
        ms8, ms32, ms8g = [], [], []
        gated = None
        if a.scene_threshold is not None:
            step_u8_gated()
            torch.cuda.synchronize(dev)
            gated = [int((net.last_gate != 0).sum())]
        for _ in range(a.rounds):
            ms8.append(window(step_u8))
            if a.scene_threshold is not None:
                ms8g.append(window(step_u8_gated))
            ms32.append(window(step_f32))
    load_s, store_s = host_cost(h0, w0, a.host_reps)
    frame8, frame32 = h0 * w0 * 3, int(i0h[0].numel()) * 4
    res = {
        "what": "one convert step on in-memory frames, HIP events; ms per step, one value per window",
        "device": torch.cuda.get_device_name(0), "precision": a.precision,
        "frame": [h0, w0], "padded": list(i0h.shape[2:]), "pairs": n, "sf": a.sf, "steps": a.steps,
        "byte_chain_ms": [round(x, 3) for x in ms8], "float_chain_ms": [round(x, 3) for x in ms32],
        "h2d_bytes_per_step": {"byte": (n + 1) * frame8, "float": 2 * n * frame32},
        "d2h_bytes_per_step": {"byte": n * a.sf * frame8, "float": n * a.sf * frame32},
        "outputs_identical": bool(same),
        **({"scene_threshold": a.scene_threshold, "byte_chain_gated_ms": [round(x, 3) for x in ms8g],
            "gated_pairs_per_step": gated[0]} if gated else {}),
        "host_ms_per_frame_one_core": {"load_frame_pad_float_div": round(load_s * 1e3, 3),
                                       "to_uint8_image": round(store_s * 1e3, 3)},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
