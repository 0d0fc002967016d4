#!/usr/bin/env python3
"""The frame-metrics kernel against its floor, and evaluate_y4m against interpolate_y4m.

1. ``rrin_frame_metrics_u8`` (squared error and SSIM of every plane) on two 4:2:0 stacks, timed beside
   ``rrin_pair_sad_u8_len`` over the same two stacks in the same process: the SAD kernel reads the
   same bytes once and computes next to nothing, so it is the floor.  Both are timed with HIP
   events over ``--steps`` calls a window, alternately, ``--rounds`` windows each, after a warm-up.
2. With ``--pipes``: ``convert.evaluate_y4m(hold=2)`` per held-out frame against
   ``convert.interpolate_y4m(sf=1)`` per output frame on the same synthetic in-memory Y4M stream, fp32
   and fp16, host clock around the whole call (which ends in a device synchronise), medians of
   ``--pipe-runs`` runs after one warm-up run of each.

Prints one JSON line.  Not a test; needs a GPU.

    python tools/metrics_bench.py --height 720 --width 1280 --frames 4 --pipes
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rrin_amd import Net, _lib, metrics, y4m  # noqa: E402
from rrin_amd import convert as cv  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict  # noqa: E402


def kernel_times(a, dev):
    n, h0, w0 = a.frames, a.height, a.width
    rng = np.random.default_rng(1)
    # unrelated random bytes: neither kernel's time depends on the values
    fa = torch.from_numpy(rng.integers(0, 256, (n, 3 * h0 // 2, w0), dtype=np.uint8)).to(dev)
    fb = torch.from_numpy(rng.integers(0, 256, (n, 3 * h0 // 2, w0), dtype=np.uint8)).to(dev)
    lib = _lib.lib()
    frame = fa.stride(0)
    planes = metrics.planes_of("yuv", h0, w0, "i420")
    arr = (_lib.Plane * 3)(*[_lib.Plane(off, pitch, step, h, w, 0) for off, step, pitch, h, w in planes])
    need = lib.rrin_frame_metrics_workspace_bytes(n, arr, 3, 1)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    sse = torch.empty((n, 3), dtype=torch.int64, device=dev)
    val = torch.empty((n, 3), dtype=torch.float64, device=dev)
    sad = torch.empty(n, dtype=torch.int64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run_metrics(flags):
        _lib.check(lib.rrin_frame_metrics_u8(fa.data_ptr(), frame, fb.data_ptr(), frame, n, arr, 3, flags,
                                             sse.data_ptr(), val.data_ptr(), ws.data_ptr(), need, st))

    def run_sad():
        _lib.check(lib.rrin_pair_sad_u8_len(fa.data_ptr(), fb.data_ptr(), frame, n, frame, sad.data_ptr(), st))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.steps   # microseconds per call

    calls = {"metrics_ssim": lambda: run_metrics(1), "metrics_sse_only": lambda: run_metrics(0), "pair_sad": run_sad}
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    us = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            us[k].append(window(fn))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"frame": [h0, w0], "frames": n, "layout": "i420", "bytes_read_per_call": 2 * n * frame,
            "us_per_call": {k: [round(x, 2) for x in v] for k, v in us.items()},
            "median_us": {k: round(v, 2) for k, v in med.items()},
            "ratio_metrics_ssim_to_sad": round(med["metrics_ssim"] / med["pair_sad"], 2),
            "ratio_sse_only_to_sad": round(med["metrics_sse_only"] / med["pair_sad"], 2),
            "gbytes_per_s": {k: round(2 * n * frame / v / 1e3, 1) for k, v in med.items()}}


def pipe_times(a, dev):
    h0, w0, n = a.height, a.width, a.pipe_frames
    yy, xx = np.mgrid[0:3 * h0 // 2, 0:w0]
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 24, 1)
    for k in range(n):   # a smooth pattern that moves a pixel a frame
        wr.write(np.clip((0.5 + 0.2 * np.sin((xx + k) / 6.0) + 0.15 * np.cos((yy - k) / 9.0)) * 255, 0, 255)
                 .astype(np.uint8))
    raw = src.getvalue()
    out = {}
    for precision in ("fp32", "fp16"):
        net = Net()
        net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
        net.precision = precision
        net = net.to(dev).eval()

        def evaluate():
            t0 = time.perf_counter()
            res = cv.evaluate_y4m(net, io.BytesIO(raw), hold=2, batch=a.batch, log=lambda *x: None)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / len(res["rows"])

        def interpolate():
            t0 = time.perf_counter()
            written = cv.interpolate_y4m(net, io.BytesIO(raw), io.BytesIO(), sf=1, batch=a.batch, log=lambda *x: None)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3 / written

        evaluate(), interpolate()   # warm-up: packing, workspaces, code objects
        ev, ip = [], []
        for _ in range(a.pipe_runs):
            ev.append(evaluate())
            ip.append(interpolate())
        out[precision] = {"evaluate_ms_per_held_out_frame": round(statistics.median(ev), 3),
                          "interpolate_ms_per_output_frame": round(statistics.median(ip), 3),
                          "evaluate_runs": [round(x, 3) for x in ev], "interpolate_runs": [round(x, 3) for x in ip]}
    return {"frame": [h0, w0], "stream_frames": n, "batch": a.batch, "runs": a.pipe_runs, **out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pipes", action="store_true", help="also time evaluate_y4m against interpolate_y4m")
    ap.add_argument("--pipe-frames", type=int, default=17)
    ap.add_argument("--pipe-runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a ROCm device")
    dev = torch.device("cuda:0")
    res = {"what": "frame metrics against the SAD floor (HIP events, us per call, one value per window)",
           "device": torch.cuda.get_device_name(0), "kernel": kernel_times(a, dev)}
    if a.pipes:
        with torch.no_grad():
            res["pipes"] = pipe_times(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
