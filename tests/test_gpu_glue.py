"""GPU: the record-path Net glue kernel by kernel -- the FLOW / REFINE / MASK / FINAL epilogues of
rrin_head_h8_fwd (head_kernel over RecH8<2> at fp32_split16, RecH8<1> at fp16, RecR32 at fp32) and the t-blend
kernels rrin_flow_tblend_h8 / rrin_flow_tblend_fwd -- against tests/glue_ref.py.

Every call runs on a Net buffer whose whole raw storage (both planes, padding ring, groups past
channel 15) holds a non-zero pattern, with per-image t, and is followed by a bit-for-bit comparison
of everything the mode must not write.  What the kernels reproduce exactly (the stored raw flow,
Ft, the FINAL frame and its 8-bit crop) is compared exactly with the fp32 twins; the backwarp and
the mask blend are held to A + S |ref| against the float64 stage, A from the fp32 oracle's own
deviation on these inputs (glue_ref.A_WARP / A_MASK, measured by tests/test_glue_ref.py) and S
the storage rounding of the precision.  The stored value is compared with the unrounded
float64 reference: S is that one rounding."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import _lib
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor, PPTensor
from tests import glue_ref as G
from tests import hip_helpers as H

pytestmark = pytest.mark.gpu
PREC = {"R32": _lib.PREC_F32R, "F16X3": _lib.PREC_F16X3, "F16": _lib.PREC_F16}
MODE = {"flow": _lib.HEAD_FLOW, "refine": _lib.HEAD_REFINE, "mask": _lib.HEAD_MASK, "final": _lib.HEAD_FINAL}
# the head conv's tolerances of test_gpu_h8.test_h8_head_plain
CONV_TOL = {"F16X3": (1e-4, 1e-4), "R32": (1e-5, 1e-5), "F16": (2e-2, 2e-2)}
E_SHAPE, E_ARG = -1, -2


def bits(a):
    return a.view(torch.int32 if a.dtype == torch.float32 else torch.int16)


def storage(t):
    if isinstance(t, PPTensor):
        return [t.t]
    return [a for a in (t.hi, t.lo) if a is not None]


def snapshot(t):
    return [a.clone() for a in storage(t)]


def fill_pattern(t, seed):
    for k, a in enumerate(storage(t)):
        a.copy_(G.pattern(a.shape, seed + k, a.dtype))


def assert_only_moved(t, snap, channels, what):
    """The raw storage of t equals snap bit for bit outside the interior pixels of `channels`."""
    keep = torch.ones(storage(t)[0].shape, dtype=torch.bool, device=storage(t)[0].device)
    for ch in channels:
        if isinstance(t, PPTensor):
            keep[:, ch, 1:t.h + 1, 32:32 + t.w] = False
        else:
            keep[:, ch // t.cpr, 1:t.h + 1, 8:8 + t.w, ch % t.cpr] = False
    for plane, (a, s) in enumerate(zip(storage(t), snap)):
        bad = (bits(a) != bits(s)) & keep
        assert not bool(bad.any()), (f"{what}: plane {plane}: {int(bad.sum())} values outside channels "
                                     f"{list(channels)} changed, first at {bad.nonzero()[:4].tolist()}")


def assert_same_bits(t, u, what):
    for plane, (a, b) in enumerate(zip(storage(t), storage(u))):
        assert torch.equal(bits(a), bits(b)), f"{what}: plane {plane} differs"


def assert_close(got, ref, a_tol, prec, what):
    err = (got.double() - ref).abs()
    lim = a_tol + G.STORE_REL[prec] * ref.abs()
    print(f"{what}: max err {float(err.max()):.3e}, max err / limit {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all()), f"{what}: {int((err > lim).sum())} of {err.numel()} values past A + S |ref|"


class Rig:
    """One (precision, shape) case of glue_ref.case on the device."""

    def __init__(self, dev, prec, n, h, w, t=None):
        self.dev, self.pname, self.prec, self.n, self.h, self.w = dev, prec, PREC[prec], n, h, w
        self.c = G.case(n, h, w)
        self.coef = t_coefficients(torch.tensor(G.T_PER_IMAGE[:n] if t is None else t), n)
        self.coef_d = self.coef.to(dev)

    def g16(self, seed=1):
        """The Net buffer: pattern everywhere, then the frames in channels 0-5."""
        g = H8Tensor(self.n, G.G16_CHANNELS, self.h, self.w, self.dev, self.prec)
        fill_pattern(g, seed)
        g.load(self.c["x0"].to(self.dev), 0)
        g.load(self.c["x1"].to(self.dev), 3)
        return g

    def status(self, v=0):
        return torch.full((1,), v, dtype=torch.int32, device=self.dev)

    def head(self, stage, g16, scale=1.0, bias=None, coef=None, **kw):
        """One head call with raw_out requested; checks the head conv against float64 and that
        the 32-channel source is unchanged.  Returns raw_out on the CPU."""
        w, b = G.keyed_head(stage, scale)
        if bias is not None:
            b = torch.tensor(bias)
        src = H8Tensor.from_nchw(self.c[stage].to(self.dev), self.prec)
        src_snap = snapshot(src)
        raw = torch.full((self.n, w.shape[0], self.h, self.w), float("nan"), device=self.dev)
        H.head_h8(src, g16, w, b, MODE[stage], self.coef_d if coef is None else coef, prec=self.prec, raw_out=raw, **kw)
        assert_only_moved(src, src_snap, [], f"{stage}: source")
        rtol, atol = CONV_TOL[self.pname]
        np.testing.assert_allclose(raw.cpu().double().numpy(), G.conv64(self.c[stage], w, b).numpy(), rtol=rtol,
                                   atol=atol * max(scale, 1.0), err_msg=f"{stage}: head conv")
        return raw.cpu()


@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n,h,w", G.SHAPES)
@pytest.mark.parametrize("prec", G.PRECS)
def test_flow(gpu, prec, n, h, w, scale):
    """FLOW: the kept raw flow is the stored form of the head conv's output, Ft0 / Ft1 are the fp32
    blend of that stored raw flow, stored -- both exactly; channels 6-9 only; same bits without
    flow_raw; the range flag stays 0."""
    rig = Rig(gpu, prec, n, h, w)
    g16 = rig.g16()
    snap = snapshot(g16)
    fr = H8Tensor(n, 4, h, w, gpu, rig.prec)
    fill_pattern(fr, 7)
    fr_snap = snapshot(fr)
    status = rig.status()
    raw = rig.head("flow", g16, scale, flow_raw=fr, status=status)
    stored = G.store_round(raw, prec)
    assert torch.equal(fr.to_nchw(0, 4).cpu(), stored), "flow_raw != store_round(raw_out)"
    ft = torch.cat(G.flow_blend32(rig.coef, stored), 1)
    assert torch.equal(g16.to_nchw(6, 4).cpu(), G.store_round(ft, prec)), "Ft != store_round(flow_blend32(stored raw))"
    assert_only_moved(g16, snap, range(6, 10), "FLOW g16")
    assert_only_moved(fr, fr_snap, range(0, 4), "FLOW flow_raw")
    assert int(status) == 0
    g2 = rig.g16()
    rig.head("flow", g2, scale)
    assert_same_bits(g16, g2, "FLOW without flow_raw")


@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n,h,w", G.SHAPES)
@pytest.mark.parametrize("prec", G.PRECS)
def test_refine(gpu, prec, n, h, w, scale):
    """REFINE: the stored Ft is store_round(fp32(Ft_before + raw_out)) exactly; xt1 / xt2 are the
    backwarps of x0 / x1 with those fp32 sums (not with the stored Ft) within A_WARP + S |ref| of the
    float64 warp, every pixel; channels 6-15 only.  x300: flows across the 16 x 32 tile, the frame
    border and (n > 1) towards the next image.
    A_WARP = 1e-5: the fp32 oracle's warp deviates 7.2e-6 (x1) / 3.3e-6 (x300) from float64 here."""
    rig = Rig(gpu, prec, n, h, w)
    g16 = rig.g16()
    before = g16.to_nchw(0, 16).cpu()
    snap = snapshot(g16)
    status = rig.status()
    raw = rig.head("refine", g16, scale, status=status)
    s32 = G.refine_add32(before[:, 6:10], raw)
    assert torch.equal(g16.to_nchw(6, 4).cpu(), G.store_round(s32, prec)), "Ft != store_round(fp32(Ft + raw_out))"
    ref = torch.cat([G.warp(before[:, 0:3], s32[:, 0:2]), G.warp(before[:, 3:6], s32[:, 2:4])], 1)
    assert float(ref.abs().max()) > 0.5  # taps inside the frame remain
    assert_close(g16.to_nchw(10, 6).cpu(), ref, G.A_WARP, prec, f"REFINE warp x{scale:g}")
    assert_only_moved(g16, snap, range(6, 16), "REFINE g16")
    assert int(status) == 0


def check_mask(rig, bias=None):
    g16 = rig.g16()
    before = g16.to_nchw(0, 16).cpu()
    snap = snapshot(g16)
    raw = rig.head("mask", g16, bias=bias)
    ref = G.mask_blend(rig.coef, raw, before[:, 10:13], before[:, 13:16])
    assert_close(g16.to_nchw(6, 3).cpu(), ref, G.A_MASK, rig.pname, f"MASK blend {bias}")
    assert_only_moved(g16, snap, range(6, 9), "MASK g16")
    return raw


@pytest.mark.parametrize("n,h,w", G.SHAPES)
@pytest.mark.parametrize("prec", G.PRECS)
def test_mask(gpu, prec, n, h, w):
    """MASK: the blend within A_MASK + S |ref| of float64; channels 6-8 only.
    A_MASK = 1.16e-6: the fp32 torch.sigmoid blend deviates 2.9e-7 from float64 on these inputs."""
    check_mask(Rig(gpu, prec, n, h, w))


@pytest.mark.parametrize("prec", G.PRECS)
def test_mask_saturated(gpu, prec):
    """MASK with logits at +-100 (through the bias), t = 0 and t = 1, xt1 != xt2: a zero weight,
    expf overflow, and both weights zero (den -> 1e-8)."""
    rig = Rig(gpu, prec, 2, 16, 32, t=[0.0, 1.0])
    for bias in G.MASK_EDGE_BIAS:
        raw = check_mask(rig, bias)
        assert float(raw.abs().min()) > 95


@pytest.mark.parametrize("n,h,w", G.SHAPES)
@pytest.mark.parametrize("prec", G.PRECS)
def test_final(gpu, prec, n, h, w):
    """FINAL: out is clamp(fp32(raw_out + blend), 0, 1) exactly; out_u8 is (uint8)(out * 255) of the
    crop exactly, with and without the fp32 output; g16 is not written."""
    rig = Rig(gpu, prec, n, h, w)
    g16 = rig.g16()
    blend = g16.to_nchw(6, 3).cpu()
    snap = snapshot(g16)
    for h0, w0, top in [(h - 5, w - 7, 5), (h, w, 0)]:
        out = torch.full((n, 3, h, w), float("nan"), device=gpu)
        u8 = torch.full((n, h0, w0, 3), 0xA5, dtype=torch.uint8, device=gpu)
        raw = rig.head("final", g16, out=out, out_u8=u8, crop=(h0, w0, top))
        q = G.final32(raw, blend)
        assert float(q.min()) == 0.0 and float(q.max()) == 1.0
        assert torch.equal(out.cpu(), q), "out != final32(raw_out, blend)"
        want8 = G.to_u8(q)[:, :, top:top + h0, :w0].permute(0, 2, 3, 1)
        assert torch.equal(u8.cpu(), want8), f"out_u8 crop {(h0, w0, top)}"
        only8 = torch.full_like(u8, 0xA5)
        rig.head("final", g16, out_u8=only8, crop=(h0, w0, top))
        assert torch.equal(only8, u8), "out_u8 with out = NULL"
    assert_only_moved(g16, snap, [], "FINAL g16")


@pytest.mark.parametrize("prec", G.PRECS)
def test_final_rejects(gpu, prec):
    """No output at all is RRIN_E_ARG, a crop past the frame RRIN_E_SHAPE; nothing is launched."""
    n, h, w = 1, 16, 32
    rig = Rig(gpu, prec, n, h, w)
    g16 = rig.g16()
    snap = snapshot(g16)
    wt, b = G.keyed_head("final")
    src = H8Tensor.from_nchw(rig.c["final"].to(gpu), rig.prec)
    out = torch.full((n, 3, h, w), float("nan"), device=gpu)
    u8 = torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device=gpu)
    call = lambda **kw: H.head_h8(src, g16, wt, b, _lib.HEAD_FINAL, rig.coef_d, prec=rig.prec, rc=True, **kw)  # noqa: E731
    assert call() == E_ARG
    for crop in [(h, w, 1), (h - 4, w, 5), (h, w + 1, 0), (0, w, 0), (h, 0, 0), (h - 1, w, -1)]:
        assert call(out=out, out_u8=u8, crop=crop) == E_SHAPE, crop
    assert bool(torch.isnan(out).all()) and bool((u8 == 0xA5).all())
    assert_only_moved(g16, snap, [], "rejected FINAL")
    assert call(out=out, out_u8=u8, crop=(h - 4, w, 4)) == 0


@pytest.mark.parametrize("prec", G.PRECS)
def test_range_guard(gpu, prec):
    """fp32_split16 / fp16: a FLOW whose raw flow passes 65504 sets status; FINAL with status set
    writes NaN to every out pixel and 0 to every out_u8 byte of the crop, with status clear the
    normal frame.  fp32 records: status is neither set nor obeyed."""
    n, h, w = 2, 24, 40
    rig = Rig(gpu, prec, n, h, w)
    half = prec != "R32"
    status = rig.status()
    raw = rig.head("flow", rig.g16(), 1e6, status=status)
    assert float(raw.abs().max()) > 65504
    assert int(status) == (1 if half else 0)
    h0, w0, top = h - 5, w - 7, 5
    for flag in (1, 0):
        g16 = rig.g16()
        blend = g16.to_nchw(6, 3).cpu()
        status = rig.status(flag)
        out = torch.zeros((n, 3, h, w), device=gpu)
        u8 = torch.full((n, h0, w0, 3), 0xA5, dtype=torch.uint8, device=gpu)
        raw = rig.head("final", g16, out=out, out_u8=u8, crop=(h0, w0, top), status=status)
        if flag and half:
            assert bool(torch.isnan(out).all()) and not bool(u8.any())
        else:
            q = G.final32(raw, blend)
            assert torch.equal(out.cpu(), q)
            assert torch.equal(u8.cpu(), G.to_u8(q)[:, :, top:top + h0, :w0].permute(0, 2, 3, 1))
        assert int(status) == flag


T2 = [0.6, 0.1]


@pytest.mark.parametrize("n,h,w", [(2, 24, 40), (1, 16, 32)])
@pytest.mark.parametrize("prec", G.PRECS)
def test_tblend_h8(gpu, prec, n, h, w):
    """rrin_flow_tblend_h8 of a raw flow kept by a FLOW at t1, with per-image t2, into a
    pattern-filled g16: channels 6-9 bit for bit those of a FLOW run directly at t2, nothing else
    moved; fp32 records: also exactly the fp32 twin.  Mismatched geometry and g_off != 0 are
    RRIN_E_SHAPE."""
    lib = _lib.lib()
    rig = Rig(gpu, prec, n, h, w)
    coef2 = t_coefficients(torch.tensor(T2[:n]), n)
    coef2_d = coef2.to(gpu)
    fr = H8Tensor(n, 4, h, w, gpu, rig.prec)
    rig.head("flow", rig.g16(), 300.0, flow_raw=fr)
    gb = rig.g16(seed=5)
    snap = snapshot(gb)
    frv, gv = fr.view(0, 4), gb.view(0, gb.c)
    blend = lambda f, g: lib.rrin_flow_tblend_h8(C.byref(f), C.byref(g), coef2_d.data_ptr(), n, rig.prec, H.stream(gpu))  # noqa: E731
    assert blend(frv, gv) == 0
    torch.cuda.synchronize()
    gc = rig.g16(seed=5)
    rig.head("flow", gc, 300.0, coef=coef2_d)
    assert_only_moved(gb, snap, range(6, 10), "t-blend g16")
    assert_same_bits(gb, gc, "t-blend vs FLOW at t2")
    assert not torch.equal(bits(gb.hi), bits(snap[0]))
    if prec == "R32":
        ft = torch.cat(G.flow_blend32(coef2, fr.to_nchw(0, 4).cpu()), 1)
        assert torch.equal(gb.to_nchw(6, 4).cpu(), ft)
    after = snapshot(gb)
    assert blend(H8Tensor(n, 4, h + 16, w, gpu, rig.prec).view(0, 4), gv) == E_SHAPE
    assert blend(H8Tensor(n, 4, h, w + 32, gpu, rig.prec).view(0, 4), gv) == E_SHAPE
    assert blend(frv, gb.view(2 * gb.cpr, 16)) == E_SHAPE  # 16 channels, but not from group 0
    torch.cuda.synchronize()
    assert_only_moved(gb, after, [], "rejected t-blend")


@pytest.mark.parametrize("n,h,w", [(2, 24, 40), (1, 16, 32)])
def test_tblend_planar(gpu, n, h, w):
    """rrin_flow_tblend_fwd (planar fp32): the same contract on PPTensor with the planar FLOW head."""
    lib = _lib.lib()
    c = G.case(n, h, w)
    wt, b = G.keyed_head("flow", 300.0)
    coef1 = t_coefficients(torch.tensor(G.T_PER_IMAGE[:n]), n).to(gpu)
    coef2 = t_coefficients(torch.tensor(T2[:n]), n)
    coef2_d = coef2.to(gpu)
    src = PPTensor.from_nchw(c["flow"].to(gpu))

    def g16(seed):
        g = PPTensor(n, G.G16_CHANNELS, h, w, gpu)
        fill_pattern(g, seed)
        g.load(c["x0"].to(gpu), 0)
        g.load(c["x1"].to(gpu), 3)
        return g

    fr = PPTensor(n, 4, h, w, gpu)
    raw = torch.full((n, 4, h, w), float("nan"), device=gpu)
    H.head(src, g16(1), wt, b, _lib.HEAD_FLOW, coef1, flow_raw=fr, raw_out=raw)
    np.testing.assert_allclose(raw.cpu().double().numpy(), G.conv64(c["flow"], wt, b).numpy(), rtol=1e-4, atol=1e-4 * 300)
    assert torch.equal(fr.to_nchw(0, 4), raw)
    gb = g16(5)
    snap = snapshot(gb)
    frv, gv = fr.view(0, 4), gb.view(0, gb.c)
    blend = lambda f, g: lib.rrin_flow_tblend_fwd(C.byref(f), C.byref(g), coef2_d.data_ptr(), n, H.stream(gpu))  # noqa: E731
    assert blend(frv, gv) == 0
    torch.cuda.synchronize()
    gc = g16(5)
    H.head(src, gc, wt, b, _lib.HEAD_FLOW, coef2_d)
    assert_only_moved(gb, snap, range(6, 10), "planar t-blend g16")
    assert_same_bits(gb, gc, "planar t-blend vs FLOW at t2")
    assert torch.equal(gb.to_nchw(6, 4).cpu(), torch.cat(G.flow_blend32(coef2, raw.cpu()), 1))
    after = snapshot(gb)
    assert blend(PPTensor(n, 4, h + 16, w, gpu).view(0, 4), gv) == E_SHAPE
    assert blend(frv, gb.view(8, 16)) == E_ARG  # the planar entry's code for a g16 view off channel 0
    torch.cuda.synchronize()
    assert_only_moved(gb, after, [], "rejected planar t-blend")
