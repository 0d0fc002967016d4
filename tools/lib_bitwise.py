#!/usr/bin/env python3
"""Are two builds of librrin_hip.so bitwise the same on the Net?  Run once per build (the library
is loaded once per process; RRIN_LIB_AB selects an A/B build) with the same arguments:

  RRIN_LIB_AB=ab/librrin_hip_old.so python tools/lib_bitwise.py --save gpurun_out/a.pt
  python tools/lib_bitwise.py --compare gpurun_out/a.pt

Every precision's forward of --batch pairs at --height x --width (stress weights, t = 0.5 and a
per-pair t) is saved / compared with torch.equal; exit 1 on any difference.

So are, at every record precision and at the small --frame-height x --frame-width x --frame-batch,
the entries behind the byte-frame paths: forward_u8, forward_yuv (nv12), forward_u16 and
forward_yuv16 (nv12) at depth 10, interpolate_items_u8, forward_u8 with flow_scale=2 and with a
plane, forward(reuse_flow=True) after a forward, and a U-Net alone (rrin_unet_fwd); and the launch
lists -- (kind, FLOPs) per launch, from the launch profiler -- of a streams=1 float forward and of
an items call, compared with ==."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rrin_amd import Net, _lib  # noqa: E402
from rrin_amd.engine import UNET_ORDER  # noqa: E402
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--save")
ap.add_argument("--compare")
ap.add_argument("--height", type=int, default=736)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--precisions", default="fp16,fp32_split16,fp32")
ap.add_argument("--frame-height", type=int, default=90)
ap.add_argument("--frame-width", type=int, default=122)
ap.add_argument("--frame-batch", type=int, default=2)
a = ap.parse_args()
dev = torch.device("cuda:0")
net = Net()
net.load_state_dict(keyed_state_dict(net.state_dict(), stress=True), strict=True)
net = net.to(dev).eval()
i0, i1 = synthetic_batch(a.batch, a.height, a.width, first_index=17)
i0, i1 = i0.to(dev), i1.to(dev)
PAIR, T = [0, 0, 1, 2, 2], [0.4, 0.8, 0.2, 0.5, 0.9375]  # 5 items over 3 pairs (4 frames)


def stack(shape, seed, maxval=255):
    """Random samples in [0, maxval], smoothed a little along the last axis."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, maxval + 1, shape, generator=g)
    v = (v + v.roll(1, -1) + v.roll(2, -1)) // 3
    return v.to(torch.uint16 if maxval > 255 else torch.uint8).to(dev)


def launches(call):
    """[(kind, FLOPs)] of the launches call(prof) makes, from the library's launch profiler."""
    lib, prof, cap = _lib.lib(), C.c_void_p(), 4096
    _lib.check(lib.rrin_prof_create(cap, C.byref(prof)), "rrin_prof_create")
    try:
        call(prof)
        torch.cuda.synchronize(dev)
        kinds, fl, cnt = (C.c_int32 * cap)(), (C.c_double * cap)(), C.c_int32()
        _lib.check(lib.rrin_prof_read(prof, kinds, None, fl, cap, C.byref(cnt)), "rrin_prof_read")
        return [(kinds[i], fl[i]) for i in range(cnt.value)]
    finally:
        lib.rrin_prof_destroy(prof)


def frame_cases(p, res):
    n, h, w = a.frame_batch, a.frame_height, a.frame_width
    rgb0, rgb1 = stack((n, h, w, 3), 1), stack((n, h, w, 3), 2)
    res[f"{p}/forward_u8"] = net.forward_u8(rgb0, rgb1, 0.4)
    res[f"{p}/forward_yuv"] = net.forward_yuv(stack((n, 3 * h // 2, w), 3), stack((n, 3 * h // 2, w), 4), 0.4)
    res[f"{p}/forward_u16"] = net.forward_u16(stack((n, h, w, 3), 5, 1023), stack((n, h, w, 3), 6, 1023), 0.4, depth=10)
    res[f"{p}/forward_yuv16"] = net.forward_yuv16(stack((n, 3 * h // 2, w), 7, 1023), stack((n, 3 * h // 2, w), 8, 1023),
                                                  0.4, depth=10)
    frames = stack((4, h, w, 3), 9)
    res[f"{p}/interpolate_items_u8"] = net.interpolate_items_u8(frames, PAIR, T)
    res[f"{p}/forward_u8(flow_scale=2)"] = net.forward_u8(rgb0, rgb1, 0.4, flow_scale=2)
    out, plane = net.forward_u8(rgb0, rgb1, 0.4, plane=(stack((n, h, w), 10), stack((n, h, w), 11)))
    res[f"{p}/forward_u8(plane)"], res[f"{p}/forward_u8(plane).plane"] = out, plane
    eng = net.engine()
    j0, j1 = i0[:n, :, :96, :128].contiguous(), i1[:n, :, :96, :128].contiguous()
    eng.forward(j0, j1, 0.3, streams=net.streams)
    res[f"{p}/forward(reuse_flow)"] = eng.forward(j0, j1, 0.7, reuse_flow=True, streams=net.streams)
    unet = getattr(net, UNET_ORDER[1])
    unet.precision = p
    res[f"{p}/unet_forward"] = unet(torch.cat((j0, j1, j0[:, :1], j1), 1)[:, :unet.in_channels].contiguous())
    res[f"{p}/launches/forward"] = launches(lambda prof: eng.forward(j0, j1, 0.5, prof=prof, streams=1))
    res[f"{p}/launches/items"] = launches(lambda prof: eng.interpolate_items_u8(frames, PAIR, T, streams=1, prof=prof))


res = {}
with torch.no_grad():
    for p in a.precisions.split(","):
        net.precision = p
        for t in (0.5, torch.linspace(0.1, 0.9, a.batch)):
            key = f"{p}@{'vec' if isinstance(t, torch.Tensor) else t}"
            res[key] = net(i0, i1, t).cpu()
        frame_cases(p, res)
        net.check_range()
def on_host(v):  # uint16 frames as int32: torch.equal has no uint16 kernel
    if not isinstance(v, torch.Tensor):
        return v
    return v.cpu().to(torch.int32) if v.dtype == torch.uint16 else v.cpu()


res = {k: on_host(v) for k, v in res.items()}
print(f"library {_lib.LIB_PATH} build {_lib.build_id()}")
if a.save:
    torch.save(res, a.save)
    print(f"saved {len(res)} results")
if a.compare:
    ref = torch.load(a.compare, weights_only=True)

    def same(x, y):
        return torch.equal(x, y) if isinstance(x, torch.Tensor) else [tuple(v) for v in x] == [tuple(v) for v in y]

    bad = [k for k in res if k not in ref or not same(res[k], ref[k])]
    for k in res:
        if k not in bad:
            what = "bitwise equal" if isinstance(res[k], torch.Tensor) else f"equal ({len(res[k])} launches)"
        elif k in ref and isinstance(res[k], torch.Tensor):
            what = "DIFFERS max %.3e" % (res[k].double() - ref[k].double()).abs().max()
        else:
            what = "DIFFERS"
        print(f"{k:40s} {what}")
    sys.exit(1 if bad or set(ref) - set(res) else 0)
