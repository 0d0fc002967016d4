#!/usr/bin/env python3
"""forward_yuv against forward_u8 on the same build: one convert step of each byte chain on
synthetic in-memory frames, timed with HIP events as tools/u8_io_bench.py does.

  yuv chain  pinned uint8 [n+1, 3H/2, W] 4:2:0 stack -> one H2D -> Net.interpolate_yuv -> uint8 D2H
  rgb chain  pinned uint8 [n+1, H, W, 3] RGB stack   -> one H2D -> Net.interpolate_u8  -> uint8 D2H

The RGB frames are yuv420_to_rgb of the YUV ones, so both chains run the network on the same
values, and the outputs are checked against the definition of forward_yuv.  The chains are timed
alternately (``--rounds`` windows of ``--steps`` steps each, after ``--warmup`` steps of both);
``--no-copies`` times the forwards alone (frames resident on the device, no H2D / D2H).  Prints one
JSON line.  Not a test; needs a GPU.

    python tools/yuv_io_bench.py --height 720 --width 1280 --pairs 4 --sf 1 --precision fp32
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rrin_amd import Net, yuv  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--sf", type=int, default=1)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"])
    ap.add_argument("--layout", default="nv12", choices=list(yuv.LAYOUTS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-copies", action="store_true", help="frames stay on the device: the forwards alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_io_bench needs a ROCm device")
    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=True))
    net.precision = a.precision
    net = net.to(dev).eval()
    n, h0, w0 = a.pairs, a.height, a.width
    ts = [i / (a.sf + 1) for i in range(1, a.sf + 1)]
    rng = np.random.default_rng(1)
    # unrelated random bytes: the kernels' time does not depend on the values
    stack_yuv = torch.from_numpy(rng.integers(0, 256, (n + 1, 3 * h0 // 2, w0), dtype=np.uint8)).pin_memory()
    stack_rgb = yuv.yuv420_to_rgb(stack_yuv, a.layout).contiguous().pin_memory()
    out_yuv = [torch.empty((n, 3 * h0 // 2, w0), dtype=torch.uint8).pin_memory() for _ in ts]
    out_rgb = [torch.empty((n, h0, w0, 3), dtype=torch.uint8).pin_memory() for _ in ts]
    dev_yuv, dev_rgb = stack_yuv.to(dev), stack_rgb.to(dev)

    def step_yuv():
        s = dev_yuv if a.no_copies else stack_yuv.to(dev, non_blocking=True)
        outs = net.interpolate_yuv(s[:-1], s[1:], ts, layout=a.layout)
        if not a.no_copies:
            for o, h in zip(outs, out_yuv):
                h.copy_(o, non_blocking=True)
        return outs

    def step_rgb():
        s = dev_rgb if a.no_copies else stack_rgb.to(dev, non_blocking=True)
        outs = net.interpolate_u8(s[:-1], s[1:], ts)
        if not a.no_copies:
            for o, h in zip(outs, out_rgb):
                h.copy_(o, non_blocking=True)
        return outs

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
            oy = step_yuv()
            orgb = step_rgb()
        torch.cuda.synchronize(dev)
        net.check_range()
        same = all(torch.equal(y, yuv.rgb_to_yuv420(r, a.layout)) for y, r in zip(oy, orgb))
        ms_yuv, ms_rgb = [], []
        for _ in range(a.rounds):
            ms_yuv.append(window(step_yuv))
            ms_rgb.append(window(step_rgb))
    fy, fr = h0 * w0 * 3 // 2, h0 * w0 * 3
    print(json.dumps({
        "what": "one convert step on in-memory frames, HIP events; ms per step, one value per window",
        "device": torch.cuda.get_device_name(0), "precision": a.precision, "layout": a.layout,
        "frame": [h0, w0], "pairs": n, "sf": a.sf, "steps": a.steps, "copies": not a.no_copies,
        "yuv_chain_ms": [round(x, 3) for x in ms_yuv], "rgb_chain_ms": [round(x, 3) for x in ms_rgb],
        "h2d_bytes_per_step": {"yuv": (n + 1) * fy, "rgb": (n + 1) * fr},
        "d2h_bytes_per_step": {"yuv": n * a.sf * fy, "rgb": n * a.sf * fr},
        "yuv_equals_definition": bool(same),
    }))


if __name__ == "__main__":
    main()
