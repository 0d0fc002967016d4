#!/usr/bin/env python3
"""What the synthetic shutter costs (rrin_amd/exposure.py): rrin_mean_frames alone, and a 60 -> 24
conversion with 8 samples over a 1/2 shutter beside the same network items without the exposure.

``kernel``: rrin_mean_frames on 4:2:0 frames (``H0 * W0 * 3 / 2`` elements) of 1280x720 and 3840x2160, uint8
and uint16 (depth 10), for S = 2, 8 and 32 sources per output.  Every output has sources of its own and
there are enough outputs per launch to move ``--min_mib`` MiB, far more than the caches hold, so the
figure is an HBM one.  The pointer table is built once; a window is ``--reps`` launches through the C
entry between two HIP events, after a warm-up; the best of ``--rounds`` windows is reported with the
others beside it.  Bytes are what the algorithm needs, ``(S + 1) * len * element size`` per output, and
the rate is set beside a device-to-device copy of 256 MiB timed the same way (read + write bytes).

``pipe``: ``--frames`` frames of 1280x720 C420 at 60 fps, made from ``rrin_amd.synthetic.synthetic_pair``,
as an in-memory Y4M stream through ``convert.expose_y4m`` to 24 fps (S = 8, shutter 1/2, ``--batch`` items
a chunk), host clock, the stream already in memory and the output kept there; then, with the frames
resident on the device, ``Net.expose_items_yuv`` on the whole schedule and ``Net.interpolate_items_yuv``
on the same network items in the same chunks, both between HIP events.  The difference of the last two
is the exposure's own share: the mean launches and their tables.

One JSON line per measurement.  Not a test; needs a GPU.

    python tools/exposure_bench.py kernel > profiles/exposure/kernel.jsonl
    python tools/exposure_bench.py pipe --precision fp32 > profiles/exposure/pipe_fp32.jsonl
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(torch, dev, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def copy_rate(torch, dev):
    """GB/s (read + write) of a device-to-device copy of 256 MiB."""
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    ms = min(window(torch, dev, lambda: dst.copy_(src), 20) for _ in range(3))
    return 2 * (256 << 20) / ms / 1e6


def kernel(a):
    import torch

    from rrin_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    copy = copy_rate(torch, dev)
    for h0, w0 in ((720, 1280), (2160, 3840)):
        flen = h0 * w0 * 3 // 2
        for depth in (8, 10):
            esize = 1 if depth == 8 else 2
            for s in (2, 8, 32):
                g = max(1, -(-(a.min_mib << 20) // ((s + 1) * flen * esize)))
                srcs = torch.randint(0, 256, (g * s, flen * esize), dtype=torch.uint8, device=dev)
                out = torch.empty((g, flen * esize), dtype=torch.uint8, device=dev)
                table = torch.zeros(g * s + (g + 2) // 2, dtype=torch.int64)
                table[:g * s] = torch.tensor([srcs[k].data_ptr() for k in range(g * s)], dtype=torch.int64)
                table[g * s:].view(torch.int32)[:g + 1] = torch.arange(0, g * s + 1, s, dtype=torch.int32)
                table = table.to(dev)

                def launch():
                    _lib.check(lib.rrin_mean_frames(table.data_ptr(), g * s, table[g * s:].data_ptr(), g, out.data_ptr(),
                                                    flen, flen, depth, 0, 16, stream), "rrin_mean_frames")

                for _ in range(3):
                    launch()
                ms = sorted(window(torch, dev, launch, a.reps) for _ in range(a.rounds))
                nbytes = (s + 1) * g * flen * esize
                print(json.dumps({"what": "rrin_mean_frames", "frame": [h0, w0], "layout": "nv12", "depth": depth,
                                  "samples": s, "outputs": g, "bytes": nbytes, "ms": [round(x, 4) for x in ms],
                                  "GBps": round(nbytes / ms[0] / 1e6, 1), "copy_GBps": round(copy, 1),
                                  "share_of_copy": round(nbytes / ms[0] / 1e6 / copy, 3)}), flush=True)
                del srcs, out, table


def pipe(a):
    import numpy as np
    import torch

    from rrin_amd import Net, exposure, retime, y4m
    from rrin_amd import convert as cv
    from rrin_amd.synthetic import keyed_state_dict, synthetic_pair
    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
    net.precision = a.precision
    net = net.to(dev).eval()
    h0, w0, n, s, sh = 720, 1280, a.frames, 8, "1/2"
    frames = []
    for k in range(n):
        rgb = (synthetic_pair(h0, w0, k)[0][0] * 255.0).to(torch.uint8)
        frames.append(torch.cat([rgb[0].reshape(-1), rgb[1, ::2, ::2].reshape(-1), rgb[2, ::2, ::2].reshape(-1)]).numpy())
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 60, 1)
    for f in frames:
        wr.write(f)
    raw = src.getvalue()
    sched = retime.exposure_schedule(n, 60, 24, sh, s)
    groups = [[(p, float(t)) for p, t in o] for o in sched]
    runs = exposure.chunks(exposure.check_groups(groups, n - 1), a.batch)
    stack = torch.from_numpy(np.stack(frames)).view(n, 3 * h0 // 2, w0).to(dev)

    def whole():
        t0 = time.perf_counter()
        cv.expose_y4m(net, io.BytesIO(raw), io.BytesIO(), 24, s, shutter=sh, batch=a.batch, log=lambda m: None)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def exposed():
        net.expose_items_yuv(stack, groups, chunk=a.batch, layout="i420")

    def items_only():
        for lo, hi, pairs, ts in runs:
            net.interpolate_items_yuv(stack[lo:hi + 1], pairs, ts, layout="i420")

    with torch.no_grad():
        whole()
        pipe_ms = sorted(whole() for _ in range(a.rounds))
        exposed()
        items_only()
        ex, it = [], []
        for _ in range(a.rounds):   # alternating
            ex.append(window(torch, dev, exposed, 1))
            it.append(window(torch, dev, items_only, 1))
    net.check_range()
    ex.sort()
    it.sort()
    print(json.dumps({"what": "60 -> 24, 8 samples over a 1/2 shutter, 1280x720 C420", "precision": a.precision,
                      "frames_in": n, "frames_out": len(sched), "network_items": sum(len(r[2]) for r in runs),
                      "batch": a.batch, "expose_y4m_ms": [round(x, 1) for x in pipe_ms],
                      "expose_items_yuv_ms": [round(x, 2) for x in ex],
                      "interpolate_items_yuv_ms": [round(x, 2) for x in it],
                      "exposure_share_ms": round(ex[len(ex) // 2] - it[len(it) // 2], 2),
                      "exposure_share": round((ex[len(ex) // 2] - it[len(it) // 2]) / ex[len(ex) // 2], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernel", "pipe"])
    ap.add_argument("--reps", type=int, default=20, help="kernel: launches per window")
    ap.add_argument("--rounds", type=int, default=3, help="windows per measurement")
    ap.add_argument("--min_mib", type=int, default=1024, help="kernel: MiB moved per launch, at least")
    ap.add_argument("--frames", type=int, default=26, help="pipe: input frames")
    ap.add_argument("--batch", type=int, default=4, help="pipe: network items per chunk")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"])
    a = ap.parse_args()
    (kernel if a.mode == "kernel" else pipe)(a)


if __name__ == "__main__":
    main()
