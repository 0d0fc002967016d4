"""GPU: the YUV 4:2:2 / 4:4:4 frame paths (rrin_yuv420.chroma: the input pack kernels, the FINAL head's
store, rrin_net_yuv_fwd / rrin_net_yuv16_fwd, Net.forward_yuv / forward_yuv16 with the layouts "nv16",
"i422" and "i444", the scene gate on blobs of any length) are, bit for bit, their definition

    forward_yuv(f0, f1, t, layout) == rgb_to_yuv(forward_u8(yuv_to_rgb(f0, layout), yuv_to_rgb(f1, layout), t), layout)

with the integer conversions of rrin_amd.yuv as the oracle.  Every comparison is exact equality.

Pack shapes -- 4:2:2: 1x2 (a single row and block), 3x258 (a second 256-pixel run that holds one block; an odd
top padding of 13 rows), 17x34 (odd height, pads on both sides).  4:4:4: 1x1, 3x257 (a second run of one
pixel: an odd tail), 17x33 (odd sizes), 16x256 (no padding, exactly one run)."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import _lib, yuv
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from tests import glue_ref as G
from tests import record_ref as R

from . import hip_helpers as H
from .test_gpu_u8 import net_of

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
REC = {"fp32": "R32", "fp32_split16": "F16X3", "fp16": "F16"}
PACK_CASES = [("nv16", (1, 2)), ("i422", (3, 258)), ("nv16", (17, 34)), ("i422", (17, 34)),
              ("i444", (1, 1)), ("i444", (3, 257)), ("i444", (17, 33)), ("i444", (16, 256))]
CHROMA = {"420": _lib.CHROMA_420, "422": _lib.CHROMA_422, "444": _lib.CHROMA_444}
ids = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}" if isinstance(c, tuple) and isinstance(c[0], str) else str(c)  # noqa: E731


def stack_of(n, h0, w0, layout, seed, dev, wide=False, top=None):
    """n frames of ``layout`` as views of one flat buffer that starts one element into its allocation, so
    that with a byte stack every frame -- also those of the even-sized 4:2:2 frames -- starts at an odd
    address.  uint8, or uint16 words below ``top`` (default: all 16 bits)."""
    rows = yuv.stack_rows(h0, layout)
    rng = np.random.default_rng(seed)
    if wide:
        a = rng.integers(0, top or 65536, (n, rows, w0)).astype(np.uint16)
    else:
        a = rng.integers(0, 256, (n, rows, w0), dtype=np.uint8)
        k = min(256, a[0].size)
        a.reshape(n, -1)[:, :k] = np.arange(k, dtype=np.uint8)
    flat = torch.from_numpy(np.concatenate((np.zeros(1, a.dtype), a.reshape(-1)))).to(dev)
    return flat[1:].view(n, rows, w0)


def desc_of(t, h0, w0, layout, cls=_lib.Yuv420, depth=10, shift=0):
    """The rrin_yuv420 / rrin_yuv420_16 of a dense stack tensor, written out here by hand."""
    chroma = yuv.chroma_of(layout)
    es = t.element_size()
    ch = h0 // 2 if chroma == "420" else h0
    cw = w0 if chroma == "444" else w0 // 2
    semi = layout in ("nv12", "nv16")
    s = cls()
    s.y, s.u = t.data_ptr(), t.data_ptr() + es * h0 * w0
    s.v = s.u + es * (1 if semi else ch * cw)
    s.img_stride, s.y_pitch = t.stride(0), w0
    s.c_pitch, s.c_step = (2 * cw, 2) if semi else (cw, 1)
    s.chroma = CHROMA[chroma]
    if cls is _lib.Yuv420x16:
        s.depth, s.shift = depth, shift
    return s


def padded_nchw(rgb, h, w, maxval):
    """float64 [n,3,h,w]: the frames edge-padded on top and on the right, divided as the packs divide."""
    n, h0, w0, _ = rgb.shape
    ys = (torch.arange(h) - (h - h0)).clamp(min=0)
    xs = torch.arange(w).clamp(max=w0 - 1)
    v = (yuv.words_to_int(rgb.cpu()) if rgb.dtype == torch.uint16 else rgb.cpu().to(torch.int32)).float()
    v = (v.clamp(max=float(maxval)) / float(maxval))[:, ys][:, :, xs]     # the fp32 division of the kernels
    return v.permute(0, 3, 1, 2).double()


def check_pack(dev, precision, h0, w0, run_yuv, run_rgb, r0, r1, maxval=255):
    """run_yuv(view) against run_rgb(view) on two guarded g16 buffers with the same prefill: the raw
    storage -- both planes, padding, the groups past channel 15, the guard bands -- is bitwise equal, and by
    record_ref.check_storage the interior holds the padded RGB frames and zeros and nothing else changed."""
    prec = _lib.PRECISIONS[precision]
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    got = R.GuardedH8(2, G.G16_CHANNELS, h, w, dev, prec, seed=31)
    want = R.GuardedH8(2, G.G16_CHANNELS, h, w, dev, prec, seed=31)
    before = got.snapshot()
    v = got.view(0, 16)
    run_yuv(v, prec)
    v2 = want.view(0, 16)
    run_rgb(v2, prec)
    torch.cuda.synchronize(dev)
    after = got.snapshot()
    for a, b in zip(after, want.snapshot()):
        assert torch.equal(R.bits(a), R.bits(b))
    expect = torch.zeros(2, 16, h, w, dtype=torch.float64)
    expect[:, 0:3], expect[:, 3:6] = padded_nchw(r0, h, w, maxval), padded_nchw(r1, h, w, maxval)
    rel = G.STORE_REL[REC[precision]]
    R.check_storage(before, after, got.storage(0, 16), h, w, expect, {"rtol": rel, "atol": 0.0}, what="yuv pack")


@pytest.mark.parametrize("case", PACK_CASES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_equals_u8_pack_of_the_converted_frames(gpu, precision, case):
    """n = 2 as the views [:-1] / [1:] of one 3-frame stack whose frames start at odd addresses."""
    layout, (h0, w0) = case
    L = _lib.lib()
    fr = stack_of(3, h0, w0, layout, 1, gpu)
    assert fr.data_ptr() % 2 == 1
    f0, f1 = fr[:-1], fr[1:]
    for coef in (None, yuv.coefficients("bt601", True)):
        k = _lib.YuvCoef(*yuv.as_coef(coef))
        r0, r1 = yuv.yuv_to_rgb(f0, layout, coef).contiguous(), yuv.yuv_to_rgb(f1, layout, coef).contiguous()
        s0, s1 = desc_of(f0, h0, w0, layout), desc_of(f1, h0, w0, layout)

        def run_yuv(v, prec):
            _lib.check(L.rrin_pack_g16_yuv_h8(C.byref(s0), C.byref(s1), C.byref(k), 2, h0, w0, C.byref(v), prec,
                                              H.stream(gpu)), "rrin_pack_g16_yuv_h8")

        def run_rgb(v, prec):
            _lib.check(L.rrin_pack_g16_u8_h8(r0.data_ptr(), r1.data_ptr(), h0 * w0 * 3, 2, h0, w0, C.byref(v), prec,
                                             H.stream(gpu)), "rrin_pack_g16_u8_h8")

        check_pack(gpu, precision, h0, w0, run_yuv, run_rgb, r0, r1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_444_semi_planar_with_padded_pitches(gpu, precision):
    """4:4:4 with c_step 2 (U, V interleaved) and pitches beyond the rows, built by hand: per frame h0 luma
    rows of pitch w0 + 3, then h0 rows of pitch 2 * w0 + 5 holding U at the even and V at the odd bytes."""
    h0, w0, n = 17, 33, 2
    L = _lib.lib()
    yp, cp = w0 + 3, 2 * w0 + 5
    frame = h0 * yp + h0 * cp
    rng = np.random.default_rng(3)
    buf = torch.from_numpy(rng.integers(0, 256, (2, n, frame), dtype=np.uint8)).to(gpu)
    rgb, descs = [], []
    for f in range(2):
        ypl = buf[f, :, :h0 * yp].view(n, h0, yp)[:, :, :w0]
        uv = buf[f, :, h0 * yp:].view(n, h0, cp)
        dense = yuv.join_planes(ypl, uv[:, :, 0:2 * w0:2], uv[:, :, 1:2 * w0:2], "i444")
        rgb.append(yuv.yuv_to_rgb(dense, "i444").contiguous())
        s = _lib.Yuv420()
        s.y = buf[f].data_ptr()
        s.u = s.y + h0 * yp
        s.v = s.u + 1
        s.img_stride, s.y_pitch, s.c_pitch, s.c_step, s.chroma = frame, yp, cp, 2, _lib.CHROMA_444
        descs.append(s)
    k = _lib.YuvCoef(*yuv.coefficients())

    def run_yuv(v, prec):
        _lib.check(L.rrin_pack_g16_yuv_h8(C.byref(descs[0]), C.byref(descs[1]), C.byref(k), n, h0, w0, C.byref(v), prec,
                                          H.stream(gpu)), "rrin_pack_g16_yuv_h8")

    def run_rgb(v, prec):
        _lib.check(L.rrin_pack_g16_u8_h8(rgb[0].data_ptr(), rgb[1].data_ptr(), h0 * w0 * 3, n, h0, w0, C.byref(v), prec,
                                         H.stream(gpu)), "rrin_pack_g16_u8_h8")

    check_pack(gpu, precision, h0, w0, run_yuv, run_rgb, rgb[0], rgb[1])


@pytest.mark.parametrize("layout,shape,depth,msb", [("nv16", (17, 34), 10, True), ("i422", (3, 258), 12, False),
                                                    ("i444", (17, 33), 10, False)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack16_equals_u16_pack_of_the_converted_frames(gpu, precision, layout, shape, depth, msb):
    """Words of all 16 bits: with msb=False most are above maxval and read as maxval."""
    h0, w0 = shape
    L = _lib.lib()
    shift = 16 - depth if msb else 0
    fr = stack_of(3, h0, w0, layout, 5, gpu, wide=True)
    assert msb or int((yuv.words_to_int(fr) > (1 << depth) - 1).sum()) > 0
    f0, f1 = fr[:-1], fr[1:]
    k = _lib.YuvCoef(*yuv.as_coef(None, depth))
    r0 = yuv.yuv_to_rgb16(f0, layout, None, depth, msb).contiguous()
    r1 = yuv.yuv_to_rgb16(f1, layout, None, depth, msb).contiguous()
    s0 = desc_of(f0, h0, w0, layout, _lib.Yuv420x16, depth, shift)
    s1 = desc_of(f1, h0, w0, layout, _lib.Yuv420x16, depth, shift)

    def run_yuv(v, prec):
        _lib.check(L.rrin_pack_g16_yuv16_h8(C.byref(s0), C.byref(s1), C.byref(k), 2, h0, w0, C.byref(v), prec,
                                            H.stream(gpu)), "rrin_pack_g16_yuv16_h8")

    def run_rgb(v, prec):
        _lib.check(L.rrin_pack_g16_u16_h8(r0.data_ptr(), r1.data_ptr(), h0 * w0 * 3, 2, h0, w0, depth, C.byref(v), prec,
                                          H.stream(gpu)), "rrin_pack_g16_u16_h8")

    check_pack(gpu, precision, h0, w0, run_yuv, run_rgb, r0, r1, maxval=(1 << depth) - 1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_of_a_replicated_444_stack_equals_the_420_pack(gpu, precision):
    """The records from a 4:2:0 stack (chroma 0, as every caller before ABI 24 passes it) equal those from the
    4:4:4 and 4:2:2 stacks that hold its chroma replicated."""
    prec = _lib.PRECISIONS[precision]
    L = _lib.lib()
    h0, w0, h, w = 18, 34, 32, 48
    fr = stack_of(3, h0, w0, "i420", 7, gpu)
    y, u, v = yuv.split_planes(fr, "i420")
    up = lambda c, d: c.repeat_interleave(2, d)  # noqa: E731
    stacks = {"i420": fr, "i444": yuv.join_planes(y, up(up(u, 1), 2), up(up(v, 1), 2), "i444").contiguous(),
              "nv16": yuv.join_planes(y, up(u, 1), up(v, 1), "nv16").contiguous()}
    k = _lib.YuvCoef(*yuv.coefficients())
    out = {}
    for layout, st in stacks.items():
        t = H8Tensor(2, 16, h, w, gpu, prec)
        view = t.view(0, 16)
        s0, s1 = desc_of(st[:-1], h0, w0, layout), desc_of(st[1:], h0, w0, layout)
        _lib.check(L.rrin_pack_g16_yuv_h8(C.byref(s0), C.byref(s1), C.byref(k), 2, h0, w0, C.byref(view), prec,
                                          H.stream(gpu)), "rrin_pack_g16_yuv_h8")
        out[layout] = t
    torch.cuda.synchronize(gpu)
    assert out["i420"].hi.any()
    for layout in ("i444", "nv16"):
        assert torch.equal(out[layout].hi.view(torch.uint8), out["i420"].hi.view(torch.uint8)), layout
        if out["i420"].lo is not None:
            assert torch.equal(out[layout].lo.view(torch.uint8), out["i420"].lo.view(torch.uint8)), layout


# ---- the FINAL head's store --------------------------------------------------------------------
GUARD = 0xA5


def filled(shape, dev, wide):
    """uint8 of 0xA5, or uint16 of 0xA5A5."""
    if wide:
        return torch.full(shape, 0xA5A5 - 65536, dtype=torch.int16, device=dev).view(torch.uint16)
    return torch.full(shape, GUARD, dtype=torch.uint8, device=dev)


class GuardedPlanes:
    """Y, U and V planes of n frames with pitches beyond their rows, each inside one allocation with 256
    guard elements before and after it, everything prefilled with 0xA5 (16-bit: 0xA5A5)."""

    def __init__(self, n, h0, w0, chroma, semi, dev, wide):
        self.n, self.h0, self.w0, self.semi = n, h0, w0, semi
        self.cw = w0 if chroma == "444" else w0 // 2
        self.step = 2 if semi else 1
        self.yp, self.cp = w0 + 5, self.cw * self.step + 3
        self.stride = h0 * max(self.yp, self.cp)
        self.fill = 0xA5A5 if wide else GUARD
        self.raw = [filled((n * self.stride + 512,), dev, wide) for _ in range(2 if semi else 3)]
        self.es = 2 if wide else 1

    def desc(self, cls, chroma, depth=10, shift=0):
        s = cls()
        p = [r.data_ptr() + 256 * self.es for r in self.raw]
        s.y, s.u = p[0], p[1]
        s.v = p[1] + self.es if self.semi else p[2]
        s.img_stride, s.y_pitch, s.c_pitch, s.c_step, s.chroma = self.stride, self.yp, self.cp, self.step, CHROMA[chroma]
        if cls is _lib.Yuv420x16:
            s.depth, s.shift = depth, shift
        return s

    def check(self, y, u, v):
        """The planes hold y, u, v; every other element of the three allocations is still the prefill."""
        n, h0 = self.n, self.h0
        raw = [yuv.words_to_int(r) if r.dtype == torch.uint16 else r.to(torch.int32) for r in self.raw]
        want = [torch.full_like(r, self.fill) for r in raw]
        rows = lambda t, pitch: t[256:256 + n * self.stride].view(n, self.stride)[:, :h0 * pitch].view(n, h0, pitch)  # noqa: E731
        as_int = lambda t: yuv.words_to_int(t) if t.dtype == torch.uint16 else t.to(torch.int32)  # noqa: E731
        rows(want[0], self.yp)[:, :, :self.w0] = as_int(y)
        if self.semi:
            rows(want[1], self.cp)[:, :, 0:2 * self.cw:2] = as_int(u)
            rows(want[1], self.cp)[:, :, 1:2 * self.cw:2] = as_int(v)
        else:
            rows(want[1], self.cp)[:, :, :self.cw] = as_int(u)
            rows(want[2], self.cp)[:, :, :self.cw] = as_int(v)
        for name, a, b in zip(("Y", "U", "V"), raw, want):
            bad = a != b
            assert not bool(bad.any()), f"{name} allocation differs at element {int(bad.nonzero()[0]) - 256} of the plane"


def run_final_head(dev, prec, n, h, w, fill_desc, status=0):
    """rrin_head_h8_fwd, FINAL, on the inputs of tests/test_gpu_glue_bits.py; fill_desc(d) sets the output."""
    from .test_gpu_glue_bits import coef, net_buffer
    g, c = net_buffer(dev, prec, n, h, w)
    wt, b = G.keyed_head("final", 1.0)
    src = H8Tensor.from_nchw(c["final"].to(dev), prec)
    st = torch.full((1,), status, dtype=torch.int32, device=dev)
    d = _lib.HeadH8Desc()
    d.n, d.cin, d.cout, d.mode, d.prec = n, 32, 3, _lib.HEAD_FINAL, prec
    d.src, d.g16 = src.view(0, 32), g.view(0, g.c)
    wd, bd, cf = wt.contiguous().to(dev), b.contiguous().to(dev), coef(n, dev)
    d.w, d.bias, d.coef, d.status = wd.data_ptr(), bd.data_ptr(), cf.data_ptr(), st.data_ptr()
    fill_desc(d)
    _lib.check(_lib.lib().rrin_head_h8_fwd(C.byref(d), H.stream(dev)), "rrin_head_h8_fwd")
    torch.cuda.synchronize(dev)


# odd h0 (hence an odd top) at 4:2:2; odd w0 at 4:4:4; the net buffer is 24x40: two tiles each way
HEAD_CASES = [("422", True, 19, 34, 5), ("422", False, 19, 34, 5), ("422", False, 24, 40, 0),
              ("444", False, 19, 33, 5), ("444", True, 19, 33, 5), ("444", False, 1, 1, 23)]


@pytest.mark.parametrize("chroma,semi,h0,w0,top", HEAD_CASES)
@pytest.mark.parametrize("precision,status", [("fp32", 0), ("fp32_split16", 0), ("fp16", 0), ("fp16", 1)])
def test_final_head_store_8bit(gpu, precision, status, chroma, semi, h0, w0, top):
    """The planes equal rgb_to_yuv of the bytes the same head writes through out_u8; pitch padding, everything
    outside the planes and the guards keep their prefill.  status 1: the range flag is set, every pixel is
    poisoned and the bytes are RGB (0,0,0) before the conversion."""
    prec = _lib.PRECISIONS[precision]
    n, h, w = 2, 24, 40
    layout = {"422": "nv16" if semi else "i422", "444": "i444"}[chroma]
    rgb = filled((n, h0, w0, 3), gpu, False)

    def as_u8(d):
        d.h0, d.w0, d.top, d.out_u8 = h0, w0, top, rgb.data_ptr()

    run_final_head(gpu, prec, n, h, w, as_u8, status)
    assert bool((rgb == 0).all()) == bool(status)
    planes = GuardedPlanes(n, h0, w0, chroma, semi, gpu, wide=False)

    def as_yuv(d):
        d.h0, d.w0, d.top = h0, w0, top
        d.out_yuv = planes.desc(_lib.Yuv420, chroma)
        d.yuv_coef = _lib.YuvCoef(*yuv.coefficients("bt601", True))

    run_final_head(gpu, prec, n, h, w, as_yuv, status)
    # the semi-planar 4:4:4 has no Python layout: compare plane by plane
    y, u, v = yuv.split_planes(yuv.rgb_to_yuv(rgb, layout, yuv.coefficients("bt601", True)), layout)
    planes.check(y, u, v)


@pytest.mark.parametrize("chroma,semi,h0,w0,top,depth,msb", [("422", True, 19, 34, 5, 10, True),
                                                             ("422", False, 19, 34, 5, 12, False),
                                                             ("444", False, 19, 33, 5, 10, False)])
@pytest.mark.parametrize("precision,status", [("fp32", 0), ("fp16", 0), ("fp16", 1)])
def test_final_head_store_16bit(gpu, precision, status, chroma, semi, h0, w0, top, depth, msb):
    prec = _lib.PRECISIONS[precision]
    n, h, w = 2, 24, 40
    layout = {"422": "nv16" if semi else "i422", "444": "i444"}[chroma]
    rgb = filled((n, h0, w0, 3), gpu, True)

    def as_u16(d):
        d.h0, d.w0, d.top, d.out_u16, d.u16_depth = h0, w0, top, rgb.data_ptr(), depth

    run_final_head(gpu, prec, n, h, w, as_u16, status)
    planes = GuardedPlanes(n, h0, w0, chroma, semi, gpu, wide=True)

    def as_yuv(d):
        d.h0, d.w0, d.top = h0, w0, top
        d.out_yuv16 = planes.desc(_lib.Yuv420x16, chroma, depth, 16 - depth if msb else 0)
        d.yuv_coef = _lib.YuvCoef(*yuv.as_coef(None, depth))

    run_final_head(gpu, prec, n, h, w, as_yuv, status)
    y, u, v = yuv.split_planes(yuv.rgb16_to_yuv(rgb, layout, None, depth, msb), layout)
    planes.check(y, u, v)


# ---- the whole path ----------------------------------------------------------------------------
PATH_CASES = [("nv16", (17, 34)), ("i422", (17, 34)), ("i422", (2, 2)), ("i444", (17, 33)), ("i444", (1, 1))]


@pytest.mark.parametrize("case", PATH_CASES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv_equals_its_definition(gpu, precision, case):
    layout, (h0, w0) = case
    net = net_of(gpu, precision)
    fr = stack_of(3, h0, w0, layout, 10, gpu)
    r = yuv.yuv_to_rgb(fr, layout)
    with torch.no_grad():
        for t in (0.5, 0.25):
            want = yuv.rgb_to_yuv(net.forward_u8(r[:-1], r[1:], t), layout)
            got = net.forward_yuv(fr[:-1], fr[1:], t, layout=layout)
            assert got.dtype == torch.uint8 and got.shape == fr[1:].shape and got.device == fr.device
            assert torch.equal(got, want), t
    net.check_range()


@pytest.mark.parametrize("case", PATH_CASES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv16_equals_its_definition(gpu, precision, case):
    layout, (h0, w0) = case
    net = net_of(gpu, precision)
    fr = stack_of(3, h0, w0, layout, 12, gpu, wide=True, top=1100)      # depth 10, some words above maxval
    r = yuv.yuv_to_rgb16(fr, layout, None, 10)
    with torch.no_grad():
        want = yuv.rgb16_to_yuv(net.forward_u16(r[:-1], r[1:], 0.5, depth=10), layout, None, 10)
        got = net.forward_yuv16(fr[:-1], fr[1:], 0.5, layout=layout, depth=10)
        assert got.dtype == torch.uint16 and got.shape == fr[1:].shape
        assert torch.equal(yuv.words_to_int(got), yuv.words_to_int(want))
    net.check_range()


@pytest.mark.parametrize("layout,shape", [("i422", (17, 34)), ("i444", (17, 33))])
def test_interpolate_yuv_reuses_flow_under_the_layouts_tag(gpu, layout, shape):
    net = net_of(gpu, "fp32")
    eng = net.engine()
    h0, w0 = shape
    fr = stack_of(3, h0, w0, layout, 14, gpu)
    f0, f1 = fr[:-1], fr[1:]
    ts = [0.25, 0.5, 0.75]
    with torch.no_grad():
        each = [net.forward_yuv(f0, f1, t, layout=layout) for t in ts]
        for a, b in zip(net.interpolate_yuv(f0, f1, ts, layout=layout), each):
            assert torch.equal(a, b)
        if layout == "i422":
            # the same bytes read as nv16 are other frames: its kept Flow must not serve this layout, nor this one's it
            other = eng.forward_yuv(f0, f1, 0.5, layout="nv16", streams=net.streams)
            assert torch.equal(eng.forward_yuv(f0, f1, 0.5, layout=layout, reuse_flow=True, streams=net.streams), each[1])
            assert torch.equal(eng.forward_yuv(f0, f1, 0.5, layout="nv16", reuse_flow=True, streams=net.streams), other)
    net.check_range()


# ---- the scene gate on blobs -------------------------------------------------------------------
def torch_sad(f0, f1):
    a = yuv.words_to_int(f0) if f0.dtype == torch.uint16 else f0.to(torch.int32)
    b = yuv.words_to_int(f1) if f1.dtype == torch.uint16 else f1.to(torch.int32)
    return (a.long() - b.long()).abs().reshape(f0.shape[0], -1).sum(1)


@pytest.mark.parametrize("layout,shape", [("i422", (17, 34)), ("i444", (17, 33))])
def test_scene_gate_returns_the_input_bytes(gpu, layout, shape):
    """Pairs: ordinary, duplicate, cut.  A 17x34 4:2:2 frame is 1156 bytes, no multiple of 3."""
    net = net_of(gpu, "fp32")
    h0, w0 = shape
    rows = yuv.stack_rows(h0, layout)
    assert layout != "i422" or (rows * w0) % 3
    yy, xx = np.mgrid[0:rows, 0:w0]
    ramp = (60 + yy + 2 * xx).astype(np.uint8)
    noise = np.random.default_rng(8).integers(0, 256, (rows, w0), dtype=np.uint8)
    f0 = torch.from_numpy(np.stack([ramp, np.roll(ramp, 2, axis=1), ramp])).to(gpu)
    f1 = torch.from_numpy(np.stack([np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), noise])).to(gpu)
    sad = torch_sad(f0, f1).cpu()
    mean = sad.float() / (rows * w0)
    assert mean[0] < 10 and mean[1] == 0 and mean[2] > 40, mean
    with torch.no_grad():
        stats = net.pair_stats_yuv(f0, f1, layout=layout)
        assert stats.dtype == torch.int64 and stats.cpu().tolist() == sad.tolist()
        fr = stack_of(4, h0, w0, layout, 9, gpu)                               # frames at odd addresses
        assert net.pair_stats_yuv(fr[:-1], fr[1:], layout=layout).cpu().tolist() == torch_sad(fr[:-1], fr[1:]).cpu().tolist()
        for t in (0.25, 0.5):
            cut = 1 if t < 0.5 else 2
            plain = net.forward_yuv(f0, f1, t, layout=layout)
            got = net.forward_yuv(f0, f1, t, layout=layout, scene_threshold=20)
            assert net.last_gate.cpu().tolist() == [0, 1, cut]
            assert torch.equal(got[0], plain[0])
            assert torch.equal(got[1], f0[1]) and torch.equal(got[2], f0[2] if cut == 1 else f1[2])
            assert not torch.equal(plain[1], f0[1])
        # the limit is floor(threshold * samples of a frame): pair 0 is a cut just below its mean, not just above
        assert torch.equal(net.forward_yuv(f0, f1, 0.5, layout=layout, scene_threshold=float(mean[0]) - 0.01)[0], f1[0])
        assert torch.equal(net.forward_yuv(f0, f1, 0.5, layout=layout, scene_threshold=float(mean[0]) + 0.01)[0], plain[0])
        outs = net.interpolate_yuv(f0, f1, [0.25, 0.75], layout=layout, scene_threshold=20)
        assert torch.equal(outs[0][2], f0[2]) and torch.equal(outs[1][2], f1[2]) and torch.equal(outs[1][1], f0[1])
        # 16 bits: the same frames as words (x 4: depth 10), the gate on samples
        w0_, w1_ = yuv.int_to_words(f0.to(torch.int32) * 4), yuv.int_to_words(f1.to(torch.int32) * 4)
        assert net.pair_stats_yuv16(w0_, w1_, depth=10, layout=layout).cpu().tolist() == (sad * 4).tolist()
        got = net.forward_yuv16(w0_, w1_, 0.5, layout=layout, depth=10, scene_threshold=80)
        assert net.last_gate.cpu().tolist() == [0, 1, 2]
        assert torch.equal(yuv.words_to_int(got[1]), yuv.words_to_int(w0_[1]))
        assert torch.equal(yuv.words_to_int(got[2]), yuv.words_to_int(w1_[2]))


def test_len_entry_points_equal_the_old_ones(gpu):
    L = _lib.lib()
    h0, w0, n = 17, 33, 3                                                     # 1683 bytes a frame: odd addresses
    rng = np.random.default_rng(4)
    fr = torch.from_numpy(rng.integers(0, 256, (n + 1, h0, w0, 3), dtype=np.uint8)).to(gpu)
    fr[2] = fr[1]
    f0, f1, stride, length = fr[:-1], fr[1:], h0 * w0 * 3, h0 * w0 * 3
    sads = torch.full((4, n), -1, dtype=torch.int64, device=gpu)
    st = H.stream(gpu)
    _lib.check(L.rrin_pair_sad_u8(f0.data_ptr(), f1.data_ptr(), stride, n, h0, w0, sads[0].data_ptr(), st))
    _lib.check(L.rrin_pair_sad_u8_len(f0.data_ptr(), f1.data_ptr(), stride, n, length, sads[1].data_ptr(), st))
    wd = torch.from_numpy(rng.integers(0, 65536, (n + 1, h0, w0, 3)).astype(np.uint16)).to(gpu)
    _lib.check(L.rrin_pair_sad_u16(wd[:-1].data_ptr(), wd[1:].data_ptr(), stride, n, h0, w0, 10, 0, sads[2].data_ptr(), st))
    _lib.check(L.rrin_pair_sad_u16_len(wd[:-1].data_ptr(), wd[1:].data_ptr(), stride, n, length, 10, 0,
                                       sads[3].data_ptr(), st))
    gate = torch.tensor([1, 0, 2], dtype=torch.int32, device=gpu)
    outs = torch.full((2, n, h0, w0, 3), GUARD, dtype=torch.uint8, device=gpu)
    _lib.check(L.rrin_gate_frames_u8(f0.data_ptr(), f1.data_ptr(), stride, n, h0, w0, gate.data_ptr(), outs[0].data_ptr(), st))
    _lib.check(L.rrin_gate_frames_u8_len(f0.data_ptr(), f1.data_ptr(), stride, n, length, gate.data_ptr(),
                                         outs[1].data_ptr(), st))
    torch.cuda.synchronize(gpu)
    assert sads[0].cpu().tolist() == torch_sad(f0, f1).cpu().tolist() and sads[0, 1] == 0
    assert torch.equal(sads[1], sads[0]) and torch.equal(sads[3], sads[2])
    assert sads[2].cpu().tolist() == torch_sad(yuv.int_to_words(yuv.words_to_int(wd[:-1]).clamp(max=1023)),
                                               yuv.int_to_words(yuv.words_to_int(wd[1:]).clamp(max=1023))).cpu().tolist()
    assert torch.equal(outs[1], outs[0])
    assert torch.equal(outs[0][0], f0[0]) and bool((outs[0][1] == GUARD).all()) and torch.equal(outs[0][2], f1[2])
    # a length of one element, at an odd address
    one = torch.tensor([7, 200, 9], dtype=torch.uint8, device=gpu)
    s1 = torch.zeros(1, dtype=torch.int64, device=gpu)
    _lib.check(L.rrin_pair_sad_u8_len(one[1:].data_ptr(), one[2:].data_ptr(), 1, 1, 1, s1.data_ptr(), st))
    torch.cuda.synchronize(gpu)
    assert int(s1) == 191
