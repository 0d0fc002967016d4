#!/usr/bin/env python3
"""ms per step of ``forward_u8`` with and without ``plane=`` (rrin_amd/plane.py), beside a build of the
parent commit.

One fresh process per measurement: the parent process never opens the GPU, it starts ``--child``
processes one after the other and collects their JSON lines.  For every configuration (frame size x
pairs x precision) the variants alternate, ``--repeats`` times over: ``parent`` (the library given by
``--parent_lib``, a build of the commit before the plane kernels, loaded through RRIN_LIB_AB; left out
when the option is absent), ``base`` (this build, no keyword) and ``plane`` (this build, ``plane=``).
A child times like bench.py: frames resident in HBM, ``--warmup`` steps, then ``--steps``
steps between two HIP events, ``--rounds`` such windows; one step is one ``engine.forward_u8`` over the
pairs on the precision's default streams.  It also times a device-to-device copy of 256 MiB, the box's
copy bandwidth, to set beside the plane's traffic estimate of 50 B per padded pixel.  Weights are the
keyed synthetic ones; frames and planes are random bytes (no kernel's time depends on the values).

Prints one JSON line per measurement and a last one with the medians.  Asserted, with ``--parent_lib``:
without the keyword the step time is the parent's -- the two medians differ by no more than the
run-to-run spread of that configuration, the larger of the two variants' max - min over all their windows
of this session -- and the tool ends with status 1 otherwise.  The added time of ``plane=`` is only
reported.  Not a test; needs a GPU.

    python tools/plane_bench.py --parent_lib ab/librrin_hip_parent.so > profiles/plane/forward_u8.jsonl
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

SIZES = ((720, 1280, 4), (2160, 3840, 1))   # H0, W0, pairs
PRECISIONS = ("fp16", "fp32")
PLANE_BYTES_PER_PIXEL = 50  # warp: 2 records (32) + 8 taps (8, cached) + 8 out; blend: 16 in + 1 out; see DESIGN.md


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
    kw = {}
    if a.variant == "plane":
        kw["plane"] = tuple(torch.from_numpy(rng.integers(0, 256, (a.pairs, a.height, a.width), dtype=np.uint8)).to(dev)
                            for _ in range(2))
    eng = net.engine()

    def window(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    ms = []
    with torch.no_grad():
        for _ in range(a.warmup):
            eng.forward_u8(f0, f1, 0.5, **kw)
        for _ in range(a.rounds):
            ms.append(window(lambda: eng.forward_u8(f0, f1, 0.5, **kw), a.steps))
    eng.check_range()
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = min(window(lambda: dst.copy_(src), 10) for _ in range(3))
    h, w = padded_size(a.height, a.width)
    print(json.dumps({"variant": a.variant, "frame": [a.height, a.width], "pairs": a.pairs, "precision": a.precision,
                      "ms_per_step": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
                      "copy_GBps": round(2 * (256 << 20) / copy_ms / 1e6, 1),
                      "plane_bytes": PLANE_BYTES_PER_PIXEL * a.pairs * h * w}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2, help="times the variants of a configuration alternate")
    ap.add_argument("--parent_lib", default=None, help="librrin_hip.so built from the parent commit")
    ap.add_argument("--child", action="store_true", help="time one measurement in this process")
    ap.add_argument("--variant", default="base", choices=["parent", "base", "plane"])
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--timeout", type=int, default=180, help="seconds per measurement")
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = (["parent"] if a.parent_lib else []) + ["base", "plane"]
    rows = []
    for h, w, n in SIZES:
        for precision in PRECISIONS:
            for _ in range(a.repeats):
                for v in variants:
                    env = dict(os.environ)
                    if v == "parent":
                        env["RRIN_LIB_AB"] = os.path.abspath(a.parent_lib)
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", v, "--height", str(h),
                           "--width", str(w), "--pairs", str(n), "--precision", precision, "--steps", str(a.steps),
                           "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
                    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=env)
                    if r.returncode != 0:   # nothing more on the GPU after a failed measurement
                        raise SystemExit(f"{v} {h}x{w}x{n} {precision} ended with {r.returncode}")
                    rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
                    print(json.dumps(rows[-1]), flush=True)
    table = []
    for h, w, n in SIZES:
        for precision in PRECISIONS:
            sel = [r for r in rows if r["frame"] == [h, w] and r["precision"] == precision]
            row = {"frame": [h, w], "pairs": n, "precision": precision}
            for v in variants:
                all_ms = [x for r in sel if r["variant"] == v for x in r["ms_per_step"]]
                row[v] = {"median_ms": round(statistics.median(all_ms), 3), "min_ms": min(all_ms), "max_ms": max(all_ms)}
            row["plane_added_ms"] = round(row["plane"]["median_ms"] - row["base"]["median_ms"], 3)
            if a.parent_lib:
                row["spread_ms"] = round(max(row[v]["max_ms"] - row[v]["min_ms"] for v in ("parent", "base")), 3)
                row["base_minus_parent_ms"] = round(row["base"]["median_ms"] - row["parent"]["median_ms"], 3)
                row["base_equals_parent"] = abs(row["base_minus_parent_ms"]) <= row["spread_ms"]
            gbps = statistics.median(r["copy_GBps"] for r in sel)
            row["copy_GBps"] = gbps
            row["plane_traffic_ms_at_copy_bw"] = round(sel[0]["plane_bytes"] / gbps / 1e6, 3)
            table.append(row)
    print(json.dumps({"what": "forward_u8 ms per step: parent build, this build, this build with plane= (HIP events, one "
                              "process per measurement, variants alternating)",
                      "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "repeats": a.repeats, "table": table}))
    slower = [r for r in table if not r.get("base_equals_parent", True)]
    if slower:
        raise SystemExit(f"without plane= the step time left the parent's spread: {slower}")


if __name__ == "__main__":
    main()
