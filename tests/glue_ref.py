"""Reference of the Net glue (model.py:37-63) for the per-kernel tests: the four head
epilogues FLOW / REFINE / MASK / FINAL and the t-blend, on NCHW tensors, no GPU.

* float64 stages (``flow_blend``, ``refine``, ``mask_blend``, ``final``): what the
  kernels approximate.  They restate oracle/ref_net.py's glue lines and its ``warp``
  in double; tests/test_glue_ref.py pins them to that oracle.
* fp32 twins (``flow_blend32``, ``refine_add32``, ``final32``): the parts the kernels
  reproduce bit for bit.  Every arithmetic step is its own float32 torch op in the
  operand order of rrin_amd/csrc/net_glue.hpp, so nothing is fused or contracted.
* ``store_round``: a value as the record layout holds it (include/rrin_hip.h).

``coef`` is the kernels' [n, 8] table: -(1-t)t, t t, (1-t)^2, t(1-t), 1-t, t, 0, 0."""
import torch
import torch.nn.functional as F

PRECS = ("R32", "F16X3", "F16")
# relative storage rounding of one value: S of the tolerance A + S |ref|
STORE_REL = {"R32": 0.0, "F16X3": 2.0 ** -21, "F16": 2.0 ** -11}
LO_SCALE = 2048.0  # F16X3: lo = f16((v - hi) * 2^11), v = hi + lo * 2^-11


def coefficients(t, n):
    """[n, 8] float64 coefficient table of t (a float or n values)."""
    tt = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
    tt = tt.expand(n) if tt.numel() == 1 else tt
    assert tt.numel() == n
    om = 1 - tt
    z = torch.zeros_like(tt)
    return torch.stack([-om * tt, tt * tt, om * om, tt * om, om, tt, z, z], dim=1)


def _c(coef, k, dtype):
    return coef[:, k].to(dtype).view(-1, 1, 1, 1)


# ---- float64 stages ---------------------------------------------------------------
def flow_blend(coef, raw):
    """Ft0, Ft1 of model.py:38-39 from the raw flow [n, 4] = F01 (u, v), F10 (u, v)."""
    raw = raw.double()
    f01, f10 = raw[:, 0:2], raw[:, 2:4]
    ft0 = _c(coef, 0, torch.float64) * f01 + _c(coef, 1, torch.float64) * f10
    ft1 = _c(coef, 2, torch.float64) * f01 - _c(coef, 3, torch.float64) * f10
    return ft0, ft1


def warp(img, flow):
    """oracle.ref_net.warp in double: grid 2 ((gx + u) / W - 0.5), grid_sample(bilinear,
    zeros, align_corners=False); taps outside the frame read 0."""
    img, flow = img.double(), flow.double()
    n, _, h, w = img.shape
    gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    x = gx.unsqueeze(0).expand(n, h, w).double() + flow[:, 0]
    y = gy.unsqueeze(0).expand(n, h, w).double() + flow[:, 1]
    grid = torch.stack((2 * (x / w - 0.5), 2 * (y / h - 0.5)), dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def refine(ft0, ft1, r, x0, x1):
    """model.py:44-48: Ft += refine_flow output [n, 4], then the two backwarps with the
    sums themselves (not with what a layout stores of them)."""
    r = r.double()
    ft0 = ft0.double() + r[:, 0:2]
    ft1 = ft1.double() + r[:, 2:4]
    return ft0, ft1, warp(x0, ft0), warp(x1, ft1)


def mask_blend(coef, logits, xt1, xt2):
    """model.py:52-55: (w1 xt1 + w2 xt2) / (w1 + w2 + 1e-8), w1 = (1-t) sigmoid(logit0),
    w2 = t sigmoid(logit1)."""
    m = torch.sigmoid(logits.double())
    w1 = _c(coef, 4, torch.float64) * m[:, 0:1]
    w2 = _c(coef, 5, torch.float64) * m[:, 1:2]
    return (w1 * xt1.double() + w2 * xt2.double()) / (w1 + w2 + 1e-8)


def final(acc, blend):
    """model.py:62-63: clamp(final U-Net output + blend, 0, 1)."""
    return (acc.double() + blend.double()).clamp(0, 1)


# ---- fp32 twins ---------------------------------------------------------------------
def _f32(*ts):
    for t in ts:
        assert t.dtype == torch.float32, t.dtype


def flow_blend32(coef, raw):
    """net_glue.hpp flow_blend: ft0 = cf0 raw[k] + cf1 raw[2+k], ft1 = cf2 raw[k] - cf3 raw[2+k],
    two rounded products and one rounded add / sub per component."""
    _f32(coef, raw)
    f01, f10 = raw[:, 0:2], raw[:, 2:4]
    a = _c(coef, 0, torch.float32) * f01
    b = _c(coef, 1, torch.float32) * f10
    c = _c(coef, 2, torch.float32) * f01
    d = _c(coef, 3, torch.float32) * f10
    return a + b, c - d


def refine_add32(ft, r):
    """The REFINE add: stored Ft (read back as fp32) + head conv output, one fp32 add."""
    _f32(ft, r)
    return ft + r


def final32(acc, blend):
    """net_glue.hpp final_clamp: one fp32 add, then the clamp to [0, 1]."""
    _f32(acc, blend)
    return (acc + blend).clamp(0, 1)


def to_u8(q):
    """FINAL's 8-bit store: (uint8)(q * 255.0f), one fp32 multiply and truncation."""
    _f32(q)
    return (q * 255.0).to(torch.uint8)


# ---- storage ----------------------------------------------------------------------
def split16(v):
    """(hi, lo) halves of F16X3: hi = f16(v), lo = f16((v - hi) * 2^11), from the fp32 v."""
    v = v.float()
    hi = v.half()
    lo = ((v - hi.float()) * LO_SCALE).half()
    return hi, lo


def store_round(v, prec):
    """The fp32 value read back from a record that stored v (rounded to fp32 first, as the
    kernels hold it).  R32: v.  F16: f16(v).  F16X3: fma(lo, 2^-11, hi) of ``split16`` --
    the layout of include/rrin_hip.h, whose lo half carries the factor 2^11 so that it
    stays a normal fp16 for small v."""
    v = v.float()
    if prec == "R32":
        return v.clone()
    if prec == "F16":
        return v.half().float()
    assert prec == "F16X3", prec
    hi, lo = split16(v)
    return (hi.double() + lo.double() / LO_SCALE).float()  # exact in double: one rounding, as fmaf


# ---- the inputs of tests/test_gpu_glue.py (built on the CPU, so that the fp32 oracle's own
# deviation from the float64 stages can be measured on them without a GPU) -------------------
SHAPES = [(1, 16, 32), (2, 24, 40), (3, 16, 80)]  # head tile 16 x 32: exact, ragged 2 x 2 (+ image stride), ragged third column
SCALES = [1.0, 300.0]                              # of the FLOW / REFINE weights: sub-pixel flows, flows leaving tile and frame
T_PER_IMAGE = [0.3, 0.75, 0.5]
G16_CHANNELS = 24                                  # allocated past channel 15: storage the glue must not touch
HEAD_COUT = {"flow": 4, "refine": 4, "mask": 2, "final": 3}
# A of the tolerance A + S |ref| where a kernel is not bit-exact: 4 x the largest deviation of the
# fp32 oracle (oracle.ref_net.warp; the torch.sigmoid blend of oracle.ref_net.net_forward) from the
# float64 stage on these inputs, and never above the planar test's 1e-5.  DEV_*: those deviations as
# tests/test_glue_ref.py measures them on the CPU (it fails if they move).  The warp's is position
# rounding -- ulp(1) / 2 of the normalised coordinate times W / 2 = 40 at w = 80 -- so it is largest
# at the widest shape and at x1 flows (7.2e-6; 3.3e-6 at x300, where most taps leave the frame).
DEV_WARP = 7.3e-6
DEV_MASK = 2.9e-7
A_WARP = min(4 * DEV_WARP, 1e-5)
A_MASK = min(4 * DEV_MASK, 1e-5)
MASK_EDGE_BIAS = [(100.0, -100.0), (-100.0, 100.0)]  # the extra MASK case: logits pushed to +-100, t = 0 and 1


def keyed_head(stage, scale=1.0):
    from rrin_amd.synthetic import keyed_tensor
    cout = HEAD_COUT[stage]
    w = keyed_tensor(f"glue.{stage}.w", (cout, 32, 3, 3), 288) * scale
    return w, keyed_tensor(f"glue.{stage}.b", (cout,), 288)


def case(n, h, w):
    """Frames x0, x1 in [0, 1] and one 32-channel feature tensor in [-1, 1] per stage."""
    g = torch.Generator().manual_seed(7919 * n + 131 * h + w)
    c = {"x0": torch.rand(n, 3, h, w, generator=g), "x1": torch.rand(n, 3, h, w, generator=g)}
    for stage in HEAD_COUT:
        c[stage] = torch.rand(n, 32, h, w, generator=g) * 2 - 1
    return c


def pattern(shape, seed, dtype=torch.float32):
    """Deterministic finite non-zero fill of a record tensor's raw storage: +-[0.25, 2)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.rand(tuple(shape), generator=g) * 1.75 + 0.25
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return (mag * sign).to(dtype)


def record_geom(h, w):
    """hp, wp of the record layout (include/rrin_hip.h): pixel (y, x) at record (y + 1, x + 8)."""
    return (h + 15) // 16 * 16 + 2, (w + 31) // 32 * 32 + 16


def records_to_nchw(hi, lo, ch_off, c, h, w):
    """Channels [ch_off, ch_off + c) of raw record storage [n, groups, hp, wp, cpr] as fp32 NCHW
    (CPU restatement of rrin_h8_to_nchw: F16X3 joins fma(lo, 2^-11, hi))."""
    cpr = hi.shape[-1]
    out = []
    for ch in range(ch_off, ch_off + c):
        v = hi[:, ch // cpr, 1:h + 1, 8:8 + w, ch % cpr]
        if lo is not None:
            v = (v.double() + lo[:, ch // cpr, 1:h + 1, 8:8 + w, ch % cpr].double() / LO_SCALE)
        out.append(v.float())
    return torch.stack(out, dim=1)


def conv64(x, w, b):
    return F.conv2d(x.double(), w.double(), b.double(), padding=1)
