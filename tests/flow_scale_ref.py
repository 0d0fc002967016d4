"""References of the flow_scale forward (rrin_amd/flowscale.py is the definition), CPU only:

* ``net_forward_scaled``: ``oracle.ref_net.net_forward`` with its Flow line replaced, composed of
  the oracle's own ``unet_forward`` and ``warp``; at s = 1 it runs the oracle's operations in the
  oracle's order, so the two agree exactly;
* ``downscale_np`` / ``upscale_np``: NumPy fp32 restatements of rrin_g16_downscale_h8 and
  rrin_flow_upscale_h8 in the pinned operation order (include/rrin_hip.h).  NumPy rounds every
  fp32 operation to fp32 and fuses nothing, which is what the kernels are built to do.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.ref_net import unet_forward, warp

F32 = np.float32


def net_forward_scaled(sd, i0, i1, t=0.5, s=1):
    x = torch.cat((i0, i1), 1)
    if s == 1:
        flow = unet_forward(sd, "Flow", x)
    else:
        flow = s * F.interpolate(unet_forward(sd, "Flow", F.avg_pool2d(x, s)), scale_factor=s, mode="bilinear",
                                 align_corners=False)
    f01, f10 = flow[:, :2], flow[:, 2:4]
    ft0 = -(1 - t) * t * f01 + t * t * f10
    ft1 = (1 - t) * (1 - t) * f01 - t * (1 - t) * f10
    r = unet_forward(sd, "refine_flow", torch.cat((ft0, ft1, x), 1))
    ft0 = ft0 + r[:, :2]
    ft1 = ft1 + r[:, 2:4]
    xt1 = warp(i0, ft0)
    xt2 = warp(i1, ft1)
    m = torch.sigmoid(unet_forward(sd, "Mask", torch.cat((ft0, ft1, x, xt1, xt2), 1)))
    w1, w2 = (1 - t) * m[:, 0:1], t * m[:, 1:2]
    out = (w1 * xt1 + w2 * xt2) / (w1 + w2 + 1e-8)
    final = unet_forward(sd, "final", torch.cat((i0, i1, out), 1)) + out
    return final.clamp(0, 1)


def downscale_np(x, s):
    """x fp32 [n, c, H, W] -> [n, c, H/s, W/s]: the s x s block summed in raster order, one fp32
    add at a time, then one multiply by 1 / s^2 (0.25f, 0.0625f)."""
    x = np.ascontiguousarray(x, dtype=F32)
    assert s in (2, 4) and x.shape[2] % s == 0 and x.shape[3] % s == 0
    acc = None
    for r in range(s):
        for c in range(s):
            p = x[:, :, r::s, c::s]
            acc = p.copy() if acc is None else (acc + p).astype(F32)
    return (acc * F32(1.0 / (s * s))).astype(F32)


def upscale_taps(size, s):
    """Per full-size index: (i0, i1, w) of source coordinate (dst + 0.5) / s - 0.5 clamped at 0,
    the second tap clamped to the last sample; w = (num mod 2s) / 2s exactly, fp32."""
    d = np.arange(size * s)
    num = np.maximum(2 * d + 1 - s, 0)
    i0 = num // (2 * s)
    i1 = np.minimum(i0 + 1, size - 1)
    w = ((num % (2 * s)).astype(F32) * F32(0.5 / s)).astype(F32)
    return i0, i1, w


def upscale_np(f, s):
    """f fp32 [n, c, h, w] -> [n, c, s h, s w]: v = (1-wy)*((1-wx)*p00 + wx*p01) + wy*((1-wx)*p10 +
    wx*p11), every operation rounded to fp32, then v * s."""
    f = np.ascontiguousarray(f, dtype=F32)
    assert s in (2, 4)
    y0, y1, wy = upscale_taps(f.shape[2], s)
    x0, x1, wx = upscale_taps(f.shape[3], s)
    wy = wy[:, None]
    uy, ux = (F32(1) - wy).astype(F32), (F32(1) - wx).astype(F32)
    p00, p01 = f[:, :, y0][:, :, :, x0], f[:, :, y0][:, :, :, x1]
    p10, p11 = f[:, :, y1][:, :, :, x0], f[:, :, y1][:, :, :, x1]
    top = ((ux * p00).astype(F32) + (wx * p01).astype(F32)).astype(F32)
    bot = ((ux * p10).astype(F32) + (wx * p11).astype(F32)).astype(F32)
    v = ((uy * top).astype(F32) + (wy * bot).astype(F32)).astype(F32)
    return (v * F32(s)).astype(F32)
