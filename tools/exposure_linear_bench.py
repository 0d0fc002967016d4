#!/usr/bin/env python3
"""What the linear-light shutter costs (rrin_amd/exposure.py, rrin_amd/transfer.py): the two table kernels
beside rrin_mean_frames, and a 60 -> 24 conversion with ``light="srgb"`` beside the same run without it.

``kernel``: 4:2:0 frames (I420, ``H0 * W0 * 3 / 2`` elements) of 1280x720 and 3840x2160, uint8 and uint16 at
depth 10, S = 2, 8 and 32 sources per output, every output with sources of its own and enough outputs per
launch to move ``--min_mib`` MiB.  Per shape, in this order and timed the same way (a window is ``--reps``
launches through the C entry between two HIP events after a warm-up, the best of ``--rounds`` windows is
the figure, all of them are printed):

* ``rrin_mean_frames``: the yardstick, every ratio is against it;
* ``lut_none``: rrin_mean_frames_lut without a table, box weights -- the 64-bit weighted sums alone;
* ``lut_srgb``: rrin_mean_frames_lut with the sRGB table on random samples: S gathers from LDS per element
  and ``depth`` more for the encode, at random banks;
* ``lut_srgb_const``: the same launch on frames that hold one value, so that every lane of a gather reads
  one address (a broadcast: no bank conflict).  ``lut_srgb - lut_srgb_const`` is what the conflicts cost;
  ``lut_srgb_const - lut_none`` what the gathers and the table load cost without them;
* ``yuv_lut_srgb`` / ``yuv_lut_srgb_const``: rrin_mean_frames_yuv_lut, one chroma block per lane.

The table load itself (2 KiB at 8 bits, 8 KiB at 10, 32 KiB at 12, once per workgroup) is measured by
``lut_srgb_const`` at depth 12 beside depth 10 on the same words: ``--depth12`` adds those rows.

``pipe``: ``--frames`` frames of 1280x720 C420 at 60 fps through ``convert.expose_y4m`` to 24 fps (S = 8,
shutter 1/2), host clock, the stream in memory: ``--rounds`` runs without ``light`` and as many with
``light="srgb"``, alternating.

One JSON line per measurement.  Not a test; needs a GPU.

    python tools/exposure_linear_bench.py kernel > profiles/exposure_linear/kernel.jsonl
    python tools/exposure_linear_bench.py pipe --precision fp16 > profiles/exposure_linear/pipe_fp16.jsonl
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


def kernel(a):
    import torch

    from rrin_amd import _lib, yuv
    from rrin_amd.engine import device_table
    from rrin_amd.framefmt import _stack_geometry
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for h0, w0 in ((720, 1280), (2160, 3840)):
        flen = h0 * w0 * 3 // 2
        uo, vo, c_pitch, c_step, chroma = _stack_geometry("i420", 1, h0, w0)
        for depth in (8, 10) + ((12,) if a.depth12 else ()):
            esize = 1 if depth == 8 else 2
            lut = device_table("srgb", depth, dev)
            geom = _lib.YuvPlanes(uo, vo, w0, c_pitch, c_step, chroma, depth, 0)
            coef = _lib.YuvCoef(*yuv.coefficients(depth=depth))
            for s in (2, 8, 32):
                g = max(1, -(-(a.min_mib << 20) // ((s + 1) * flen * esize)))
                k = g * s
                rand = torch.randint(0, 256, (k, flen * esize), dtype=torch.uint8, device=dev)
                if esize == 2:   # samples of the depth, not words above maxval that all clamp to one entry
                    rand.view(torch.int16).bitwise_and_((1 << depth) - 1)
                const = torch.full((k, flen * esize), 0x01, dtype=torch.uint8, device=dev)   # sample 1 / 257
                out = torch.empty((g, flen * esize), dtype=torch.uint8, device=dev)

                def upload(srcs):
                    t = torch.zeros(k + (g + 1 + k + 1) // 2, dtype=torch.int64)
                    t[:k] = torch.tensor([srcs[j].data_ptr() for j in range(k)], dtype=torch.int64)
                    w = t[k:].view(torch.int32)
                    w[:g + 1] = torch.arange(0, k + 1, s, dtype=torch.int32)
                    w[g + 1:g + 1 + k] = 1
                    return t.to(dev)

                tabs = {"rand": upload(rand), "const": upload(const)}

                def ptrs(t):
                    return t.data_ptr(), t[k:].data_ptr(), t[k:].data_ptr() + 4 * (g + 1)

                def mean(t):
                    p, st, _ = ptrs(t)
                    return lambda: _lib.check(lib.rrin_mean_frames(p, k, st, g, out.data_ptr(), flen, flen, depth, 0, 16,
                                                                   stream), "rrin_mean_frames")

                def element(t, table):
                    p, st, wt = ptrs(t)
                    return lambda: _lib.check(lib.rrin_mean_frames_lut(p, k, st, g, out.data_ptr(), flen, flen, depth, 0,
                                                                       16, wt, table, stream), "rrin_mean_frames_lut")

                def planes(t):
                    p, st, wt = ptrs(t)
                    return lambda: _lib.check(lib.rrin_mean_frames_yuv_lut(p, k, st, g, out.data_ptr(), flen,
                                                                           C.byref(geom), C.byref(coef), h0, w0, wt,
                                                                           lut.data_ptr(), stream),
                                              "rrin_mean_frames_yuv_lut")

                cases = [("rrin_mean_frames", mean(tabs["rand"])),
                         ("lut_none", element(tabs["rand"], None)),
                         ("lut_srgb", element(tabs["rand"], lut.data_ptr())),
                         ("lut_srgb_const", element(tabs["const"], lut.data_ptr())),
                         ("yuv_lut_srgb", planes(tabs["rand"])),
                         ("yuv_lut_srgb_const", planes(tabs["const"]))]
                if depth == 12:
                    cases = [c for c in cases if c[0] in ("rrin_mean_frames", "lut_srgb", "lut_srgb_const")]
                base = None
                nbytes = (s + 1) * g * flen * esize
                for name, launch in cases:
                    for _ in range(3):
                        launch()
                    ms = sorted(window(torch, dev, launch, a.reps) for _ in range(a.rounds))
                    base = ms[0] if base is None else base
                    print(json.dumps({"what": name, "frame": [h0, w0], "layout": "i420", "depth": depth, "samples": s,
                                      "outputs": g, "bytes": nbytes, "ms": [round(x, 4) for x in ms],
                                      "GBps": round(nbytes / ms[0] / 1e6, 1),
                                      "ratio_to_mean_frames": round(ms[0] / base, 3)}), flush=True)
                del rand, const, out, tabs


def pipe(a):
    import torch

    from rrin_amd import Net, y4m
    from rrin_amd import convert as cv
    from rrin_amd.synthetic import keyed_state_dict, synthetic_pair
    dev = torch.device("cuda:0")
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=False))
    net.precision = a.precision
    net = net.to(dev).eval()
    h0, w0, n, s, sh = 720, 1280, a.frames, 8, "1/2"
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 60, 1)
    for k in range(n):
        rgb = (synthetic_pair(h0, w0, k)[0][0] * 255.0).to(torch.uint8)
        wr.write(torch.cat([rgb[0].reshape(-1), rgb[1, ::2, ::2].reshape(-1), rgb[2, ::2, ::2].reshape(-1)]).numpy())
    raw = src.getvalue()

    def whole(light):
        t0 = time.perf_counter()
        kw = {} if light is None else {"light": light}
        written = cv.expose_y4m(net, io.BytesIO(raw), io.BytesIO(), 24, s, shutter=sh, batch=a.batch,
                                log=lambda m: None, **kw)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, written

    with torch.no_grad():
        whole(None)
        whole("srgb")
        plain, linear = [], []
        for _ in range(a.rounds):   # alternating
            ms, written = whole(None)
            plain.append(ms)
            linear.append(whole("srgb")[0])
    net.check_range()
    print(json.dumps({"what": "60 -> 24, 8 samples over a 1/2 shutter, 1280x720 C420", "precision": a.precision,
                      "frames_in": n, "frames_out": written, "batch": a.batch,
                      "expose_y4m_ms": [round(x, 1) for x in plain],
                      "expose_y4m_srgb_ms": [round(x, 1) for x in linear],
                      "median_difference_ms": round(sorted(linear)[len(linear) // 2] - sorted(plain)[len(plain) // 2], 1),
                      "spread_ms": round(max(max(plain) - min(plain), max(linear) - min(linear)), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["kernel", "pipe"])
    ap.add_argument("--reps", type=int, default=10, help="kernel: launches per window")
    ap.add_argument("--rounds", type=int, default=3, help="windows per measurement; pipe: runs per variant")
    ap.add_argument("--min_mib", type=int, default=512, help="kernel: MiB moved per launch, at least")
    ap.add_argument("--depth12", action="store_true", help="kernel: also the element kernel at depth 12 (32 KiB table)")
    ap.add_argument("--frames", type=int, default=26, help="pipe: input frames")
    ap.add_argument("--batch", type=int, default=4, help="pipe: network items per chunk")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32_split16", "fp16"])
    a = ap.parse_args()
    (kernel if a.mode == "kernel" else pipe)(a)


if __name__ == "__main__":
    main()
