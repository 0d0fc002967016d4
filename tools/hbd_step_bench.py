"""Step times of the 16-bit frame paths next to forward_yuv of the same build: frames
resident on the device, HIP events, alternating windows after a warm-up, random weights and frames.

    python tools/hbd_step_bench.py --precision fp32 [--size 720x1280] [--pairs 4] [--windows 3] [--steps 10]

Prints one JSON line: ms per step and window for forward_yuv (NV12), forward_yuv16 (10-bit, low bits, NV12)
and forward_u16 (10-bit RGB).  For the record only: no threshold is attached to these numbers."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rrin_amd import Net  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--size", default="720x1280")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    h0, w0 = (int(v) for v in a.size.split("x"))
    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False), strict=True)
    net.precision = a.precision
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    n = a.pairs
    y8 = torch.randint(0, 256, (n + 1, 3 * h0 // 2, w0), generator=g).to(torch.uint8).to(dev)
    y16 = torch.randint(0, 1024, (n + 1, 3 * h0 // 2, w0), generator=g).to(torch.int16).view(torch.uint16).to(dev)
    r16 = torch.randint(0, 1024, (n + 1, h0, w0, 3), generator=g).to(torch.int16).view(torch.uint16).to(dev)
    paths = {
        "forward_yuv": lambda: net.forward_yuv(y8[:-1], y8[1:], 0.5),
        "forward_yuv16_10": lambda: net.forward_yuv16(y16[:-1], y16[1:], 0.5, depth=10),
        "forward_u16_10": lambda: net.forward_u16(r16[:-1], r16[1:], 0.5, depth=10),
    }
    ms = {k: [] for k in paths}
    with torch.no_grad():
        for f in paths.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for name, f in paths.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                e1.synchronize()
                ms[name].append(round(e0.elapsed_time(e1) / a.steps, 3))
    net.check_range()
    print(json.dumps({"tool": "hbd_step_bench", "precision": a.precision, "size": a.size, "pairs": n,
                      "steps": a.steps, "device": torch.cuda.get_device_name(0), "ms_per_step": ms}))


if __name__ == "__main__":
    main()
