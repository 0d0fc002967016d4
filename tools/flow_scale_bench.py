#!/usr/bin/env python3
"""ms per step of ``forward_u8`` at flow_scale 1, 2 and 4 (rrin_amd/flowscale.py).

One build, one fresh process per configuration (frame size x pairs x precision x scale): the parent
never opens the GPU, it starts ``--child`` processes one after the other and collects their JSON
lines.  A child times like bench.py: frames resident in HBM, ``--warmup`` steps, then
``--steps`` steps between two HIP events, ``--rounds`` such windows; one step is one
``engine.forward_u8`` over the pairs on the precision's default streams.  Weights are the keyed
synthetic ones; the frames are random bytes (no kernel's time depends on the values).

Prints one JSON line.  Not a test; needs a GPU.

    python tools/flow_scale_bench.py > profiles/flow_scale/forward_u8.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((2160, 3840, 1), (720, 1280, 4))   # H0, W0, pairs
PRECISIONS = ("fp16", "fp32")
SCALES = (1, 2, 4)


def child(a):
    import numpy as np
    import torch

    from rrin_amd import Net
    from rrin_amd.flowscale import padded_size
    from rrin_amd.synthetic import keyed_state_dict

    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
    net.precision = a.precision
    net = net.to(dev).eval()
    rng = np.random.default_rng(1)
    f0 = torch.from_numpy(rng.integers(0, 256, (a.pairs, a.height, a.width, 3), dtype=np.uint8)).to(dev)
    f1 = torch.from_numpy(rng.integers(0, 256, (a.pairs, a.height, a.width, 3), dtype=np.uint8)).to(dev)
    eng = net.engine()
    ms = []
    with torch.no_grad():
        for _ in range(a.warmup):
            eng.forward_u8(f0, f1, 0.5, flow_scale=a.flow_scale)
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            for _ in range(a.steps):
                eng.forward_u8(f0, f1, 0.5, flow_scale=a.flow_scale)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
    eng.check_range()
    print(json.dumps({"frame": [a.height, a.width], "padded": list(padded_size(a.height, a.width, a.flow_scale)),
                      "pairs": a.pairs, "precision": a.precision, "flow_scale": a.flow_scale,
                      "ms_per_step": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
                      "pairs_per_s": round(a.pairs * 1e3 / statistics.median(ms), 1)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="time one configuration in this process")
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--flow_scale", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per configuration")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for h, w, n in SIZES:
        for precision in PRECISIONS:
            for s in SCALES:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--height", str(h), "--width", str(w),
                       "--pairs", str(n), "--precision", precision, "--flow_scale", str(s), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
                if r.returncode != 0:   # nothing more on the GPU after a failed configuration
                    raise SystemExit(f"configuration {h}x{w}x{n} {precision} s={s} ended with {r.returncode}")
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"what": "forward_u8 ms per step by flow_scale (HIP events, one process per configuration)",
                      "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "rows": rows}))


if __name__ == "__main__":
    main()
