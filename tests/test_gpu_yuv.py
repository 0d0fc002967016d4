"""GPU: the YUV 4:2:0 frame path (rrin_pack_g16_yuv_h8, the FINAL head's 4:2:0 store,
rrin_net_yuv_fwd, RRINEngine.forward_yuv, Net.forward_yuv / interpolate_yuv / pair_stats_yuv,
convert.interpolate_y4m) is, bit for bit, its definition

    forward_yuv(f0, f1, t) == rgb_to_yuv420(forward_u8(yuv420_to_rgb(f0), yuv420_to_rgb(f1), t))

with the integer conversions of rrin_amd.yuv as the oracle.  Every comparison is exact equality.
Shapes (even sizes only): 18x34 (the largest pads of an even size: 14 rows on top, 14 columns on the
right), 38x50 (medium pads), 64x96 (no padding), 2x2 (the minimum: one block, padded to 16x16),
16x258 (a second 256-pixel run of the pack kernel that holds a single block)."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, y4m, yuv
from rrin_amd import convert as cv
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from rrin_amd.synthetic import synthetic_batch

from . import hip_helpers as H
from .test_gpu_u8 import _SD, net_of, padded
from .test_gpu_u8 import frames as rgb_frames

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
SHAPES = [(18, 34), (38, 50), (64, 96), (2, 2), (16, 258)]
COEFS = [None, yuv.coefficients("bt601", True)]
ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def frames(n, h0, w0, seed, dev=None):
    """uint8 [n, 3*h0//2, w0] of random bytes; the first 256 bytes of every frame hold every byte value."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 3 * h0 // 2, w0), dtype=np.uint8)
    k = min(256, a[0].size)
    a.reshape(n, -1)[:, :k] = np.arange(k, dtype=np.uint8)
    t = torch.from_numpy(a)
    return t.to(dev) if dev is not None else t


def relayout(fr, src, dst):
    """The same planes in another layout."""
    return yuv.join_planes(*yuv.split_planes(fr, src), dst).contiguous()


def stack_desc(t, h0, w0, layout, stride=None):
    """rrin_yuv420 of a dense-frame stack tensor."""
    s = _lib.Yuv420()
    s.y, s.u = t.data_ptr(), t.data_ptr() + h0 * w0
    s.img_stride, s.y_pitch = (t.stride(0) if stride is None else stride), w0
    if layout == "nv12":
        s.v, s.c_pitch, s.c_step = s.u + 1, w0, 2
    else:
        s.v, s.c_pitch, s.c_step = s.u + h0 * w0 // 4, w0 // 2, 1
    return s


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_yuv_equals_u8_pack_of_the_converted_frames(gpu, precision, shape):
    """The whole record buffers (hi and lo, padding included) are those rrin_pack_g16_u8_h8 writes from
    yuv420_to_rgb of the frames: both layouts, two coefficient sets, frames at an odd offset of a stack."""
    prec = _lib.PRECISIONS[precision]
    L = _lib.lib()
    h0, w0 = shape
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    nv12 = frames(3, h0, w0, 1, gpu)
    for layout in yuv.LAYOUTS:
        fr = nv12 if layout == "nv12" else relayout(nv12, "nv12", "i420")
        f0, f1 = fr[:-1], fr[1:]                           # pair p = frames p, p + 1 of one stack
        for coef in COEFS:
            k = _lib.YuvCoef(*yuv.as_coef(coef))
            got = H8Tensor(2, 16, h, w, gpu, prec)
            want = H8Tensor(2, 16, h, w, gpu, prec)
            v = got.view(0, 16)
            s0, s1 = stack_desc(f0, h0, w0, layout), stack_desc(f1, h0, w0, layout)
            _lib.check(L.rrin_pack_g16_yuv_h8(C.byref(s0), C.byref(s1), C.byref(k), 2, h0, w0, C.byref(v), prec,
                                              H.stream(gpu)), "rrin_pack_g16_yuv_h8")
            r0 = yuv.yuv420_to_rgb(f0, layout, coef).contiguous()
            r1 = yuv.yuv420_to_rgb(f1, layout, coef).contiguous()
            v = want.view(0, 16)
            _lib.check(L.rrin_pack_g16_u8_h8(r0.data_ptr(), r1.data_ptr(), h0 * w0 * 3, 2, h0, w0, C.byref(v), prec,
                                             H.stream(gpu)), "rrin_pack_g16_u8_h8")
            torch.cuda.synchronize(gpu)
            assert want.hi.any()
            assert torch.equal(got.hi.view(torch.uint8), want.hi.view(torch.uint8)), (layout, coef)
            if want.lo is not None:
                assert torch.equal(got.lo.view(torch.uint8), want.lo.view(torch.uint8)), (layout, coef)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv_equals_its_definition(gpu, precision, shape):
    """n = 2 on the views [:-1] / [1:] of one 3-frame stack, t = 0.5 and 0.25, both layouts: the RGB
    reference is computed once per t (the layouts hold the same planes)."""
    net = net_of(gpu, precision)
    h0, w0 = shape
    nv12 = frames(3, h0, w0, 10, gpu)
    i420 = relayout(nv12, "nv12", "i420")
    r = yuv.yuv420_to_rgb(nv12, "nv12")
    assert torch.equal(r, yuv.yuv420_to_rgb(i420, "i420"))
    for t in (0.5, 0.25):
        with torch.no_grad():
            rgb = net.forward_u8(r[:-1], r[1:], t)
            for layout, fr in (("nv12", nv12), ("i420", i420)):
                got = net.forward_yuv(fr[:-1], fr[1:], t, layout=layout)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3 * h0 // 2, w0) and got.device == fr.device
                assert torch.equal(got, yuv.rgb_to_yuv420(rgb, layout)), (layout, t)
    net.check_range()


def test_forward_yuv_with_other_coefficients_and_copied_inputs(gpu):
    net = net_of(gpu, "fp32")
    k = yuv.coefficients("bt601", True)
    fr = frames(3, 38, 50, 11, gpu)
    r = yuv.yuv420_to_rgb(fr, "nv12", k)
    with torch.no_grad():
        want = yuv.rgb_to_yuv420(net.forward_u8(r[:-1], r[1:], 0.5), "nv12", k)
        assert torch.equal(net.forward_yuv(fr[:-1], fr[1:], 0.5, coef=k), want)
        assert torch.equal(net.forward_yuv(fr[:-1], fr[1:], 0.5, coef=tuple(k)), want)   # any 15 ints
        # frames that are not dense are copied, not misread
        wide = torch.zeros((2, 57, 60), dtype=torch.uint8, device=gpu)
        wide[:, :, :50] = fr[:-1]
        assert torch.equal(net.forward_yuv(wide[:, :, :50], fr[1:], 0.5, coef=k), want)


@pytest.mark.parametrize("layout", yuv.LAYOUTS)
def test_pitched_output_through_the_c_abi(gpu, layout):
    """rrin_net_yuv_fwd into planes of their own with y_pitch = w0 + 6 and the chroma pitch to match,
    prefilled with 0xA5: the planes equal the dense result, every other byte is still 0xA5."""
    net = net_of(gpu, "fp32")
    eng = net.engine()
    h0, w0, n = 38, 50, 2
    h, w = 48, 64
    fr = frames(3, h0, w0, 12, gpu)
    if layout == "i420":
        fr = relayout(fr, "nv12", "i420")
    with torch.no_grad():
        dense = eng.forward_yuv(fr[:-1], fr[1:], 0.5, layout=layout, streams=1)   # one part of n pairs, as below
    torch.cuda.synchronize(gpu)
    yp = w0 + 6
    cp = yp if layout == "nv12" else w0 // 2 + 3
    cw = w0 if layout == "nv12" else w0 // 2                 # bytes of a chroma row that hold samples
    ybuf = torch.full((n, h0, yp), 0xA5, dtype=torch.uint8, device=gpu)
    ubuf = torch.full((n, h0, yp), 0xA5, dtype=torch.uint8, device=gpu)   # the size of ybuf: one img_stride
    vbuf = torch.full((n, h0, yp), 0xA5, dtype=torch.uint8, device=gpu)
    d = _lib.NetYuvDesc()
    nd = d.net
    nd.n, nd.h, nd.w, nd.prec = n, h, w, eng.prec
    coef = t_coefficients(0.5, n).to(gpu)
    nd.coef = coef.data_ptr()
    nd.convs, nd.heads = eng.conv_table_for(n, h, w), eng.head_table
    ws = eng.workspace(n, h, w, 7)
    nd.workspace, nd.workspace_bytes = ws.data_ptr(), ws.numel()
    sc = eng._net_scratch(n, h, w, 7)
    if sc is not None:
        nd.scratch, nd.scratch_bytes = sc.data_ptr(), sc.numel()
    d.f0, d.f1 = stack_desc(fr[:-1], h0, w0, layout), stack_desc(fr[1:], h0, w0, layout)
    o = d.out
    o.y, o.img_stride, o.y_pitch, o.c_pitch = ybuf.data_ptr(), h0 * yp, yp, cp
    if layout == "nv12":
        o.u, o.v, o.c_step = ubuf.data_ptr(), ubuf.data_ptr() + 1, 2
    else:
        o.u, o.v, o.c_step = ubuf.data_ptr(), vbuf.data_ptr(), 1
    d.coef = _lib.YuvCoef(*yuv.coefficients())
    d.h0, d.w0 = h0, w0
    _lib.check(_lib.lib().rrin_net_yuv_fwd(C.byref(d), H.stream(gpu)), "rrin_net_yuv_fwd")
    torch.cuda.synchronize(gpu)
    y, u, v = yuv.split_planes(dense, layout)
    assert torch.equal(ybuf[:, :, :w0], y) and (ybuf[:, :, w0:] == 0xA5).all()
    crows = ubuf.view(n, -1)[:, :(h0 // 2) * cp].view(n, h0 // 2, cp)
    assert (ubuf.view(n, -1)[:, (h0 // 2) * cp:] == 0xA5).all() and (crows[:, :, cw:] == 0xA5).all()
    if layout == "nv12":
        assert torch.equal(crows[:, :, 0:cw:2], u) and torch.equal(crows[:, :, 1:cw:2], v)
        assert (vbuf == 0xA5).all()
    else:
        vrows = vbuf.view(n, -1)[:, :(h0 // 2) * cp].view(n, h0 // 2, cp)
        assert torch.equal(crows[:, :, :cw], u) and torch.equal(vrows[:, :, :cw], v)
        assert (vbuf.view(n, -1)[:, (h0 // 2) * cp:] == 0xA5).all() and (vrows[:, :, cw:] == 0xA5).all()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_interpolate_yuv_reuses_flow_and_keeps_the_other_paths_apart(gpu, precision):
    net = net_of(gpu, precision)
    eng = net.engine()
    f0, f1 = frames(2, 38, 50, 41, gpu), frames(2, 38, 50, 42, gpu)
    ts = [0.25, 0.5, 0.75]
    with torch.no_grad():
        each = [net.forward_yuv(f0, f1, t) for t in ts]
        outs = net.interpolate_yuv(f0, f1, ts)
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        # the workspaces now hold the raw Flow of (f0, f1) as YUV: a float forward at the same padded
        # shape with other frames and reuse_flow=True must not take it for its own previous pair
        g0, g1 = rgb_frames(2, 38, 50, 43, gpu), rgb_frames(2, 38, 50, 44, gpu)
        j0, j1 = padded(g0, gpu), padded(g1, gpu)
        got = eng.forward(j0, j1, 0.5, reuse_flow=True, streams=net.streams)
        assert torch.equal(got, eng.forward(j0, j1, 0.5, streams=net.streams))
        # nor the RGB byte path
        eng.forward_yuv(f0, f1, 0.5, streams=net.streams)
        got8 = eng.forward_u8(g0, g1, 0.5, reuse_flow=True, streams=net.streams)
        assert torch.equal(got8, eng.forward_u8(g0, g1, 0.5, streams=net.streams))
        # nor forward_yuv theirs
        eng.forward_u8(g0, g1, 0.5, streams=net.streams)
        assert torch.equal(eng.forward_yuv(f0, f1, 0.5, reuse_flow=True, streams=net.streams), each[1])
        eng.forward(j0, j1, 0.5, streams=net.streams)
        assert torch.equal(eng.forward_yuv(f0, f1, 0.5, reuse_flow=True, streams=net.streams), each[1])
        # nor forward_yuv with another matrix: other RGB values, another Flow
        k = yuv.coefficients("bt601", True)
        fresh = eng.forward_yuv(f0, f1, 0.5, coef=k, streams=net.streams)
        eng.forward_yuv(f0, f1, 0.5, streams=net.streams)
        assert torch.equal(eng.forward_yuv(f0, f1, 0.5, coef=k, reuse_flow=True, streams=net.streams), fresh)
        assert not torch.equal(fresh, each[1])
    net.check_range()


def gate_inputs(dev):
    """f0 / f1 uint8 [4,57,50] (38x50 frames): two ordinary pairs (a smooth ramp against itself rolled
    by one byte column), a duplicate pair, a cut pair (the ramp against random bytes)."""
    yy, xx = np.mgrid[0:57, 0:50]
    ramp = (60 + yy + 2 * xx).astype(np.uint8)
    noise = np.random.default_rng(8).integers(0, 256, (57, 50), dtype=np.uint8)
    f0 = np.stack([ramp, np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), ramp])
    f1 = np.stack([np.roll(ramp, 1, axis=1), np.roll(ramp, 1, axis=0), np.roll(ramp, 2, axis=1), noise])
    return torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)


def torch_sad(f0, f1):
    return (f0.long() - f1.long()).abs().reshape(f0.shape[0], -1).sum(1)


def test_forward_yuv_scene_gate(gpu):
    net = net_of(gpu, "fp32")
    f0, f1 = gate_inputs(gpu)
    sad = torch_sad(f0, f1).cpu()
    mean = sad.float() / (57 * 50)
    assert max(mean[0], mean[1]) < 10 and mean[2] == 0 and mean[3] > 40, mean   # far from 20 either way
    with torch.no_grad():
        stats = net.pair_stats_yuv(f0, f1)
        assert stats.dtype == torch.int64 and stats.cpu().tolist() == sad.tolist()
        fr = frames(4, 38, 50, 9, gpu)
        assert net.pair_stats_yuv(fr[:-1], fr[1:]).cpu().tolist() == torch_sad(fr[:-1], fr[1:]).cpu().tolist()
        for t in (0.25, 0.5):
            cut = 1 if t < 0.5 else 2
            plain = net.forward_yuv(f0, f1, t)
            assert torch.equal(net.forward_yuv(f0, f1, t, scene_threshold=None), plain)
            got = net.forward_yuv(f0, f1, t, scene_threshold=20)
            codes = net.last_gate.clone()
            assert torch.equal(got[:2], plain[:2])                           # ungated pairs: untouched
            assert torch.equal(got[2], f0[2])                                # the duplicate: f0's bytes
            assert torch.equal(got[3], f0[3] if cut == 1 else f1[3])         # the cut: the nearer input
            assert not torch.equal(plain[2], f0[2]) and not torch.equal(plain[3], got[3])   # the gate did it
            assert codes.dtype == torch.int32 and codes.cpu().tolist() == [0, 0, 1, cut]
        # the limit is floor(threshold * bytes of a frame): the ordinary pair 0 is a cut just below its mean
        low = float(mean[0]) - 0.01
        assert torch.equal(net.forward_yuv(f0, f1, 0.5, scene_threshold=low)[0], f1[0])
        # interpolate_yuv: the sums are computed once; last_gate is that of ts[-1]
        ts = [0.25, 0.5, 0.75]
        each = [net.forward_yuv(f0, f1, t, scene_threshold=20) for t in ts]
        outs = net.interpolate_yuv(f0, f1, ts, scene_threshold=20)
        assert net.last_gate.cpu().tolist() == [0, 0, 1, 2]
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        # explicit codes
        g = torch.tensor([2, 0, 9, 1], dtype=torch.int32, device=gpu)
        gated = net.forward_yuv(f0, f1, 0.5, gate=g)
        assert net.last_gate is g
        plain = net.forward_yuv(f0, f1, 0.5)
        assert torch.equal(gated[0], f1[0]) and torch.equal(gated[1:3], plain[1:3]) and torch.equal(gated[3], f0[3])


def byte_gate_codes(f0, f1, threshold, t):
    """convert.scene_gate_codes on the bytes of 4:2:0 frames: H0/2 x W0 x 3 of them per frame."""
    sad = torch_sad(f0, f1)
    limit = cv.scene_limit(threshold, f0.shape[1] // 3, f0.shape[2])
    codes = torch.where(sad > limit, cv.scene_cut_code(t), 0)
    return torch.where(sad == 0, 1, codes).to(torch.int32)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_uneven_split_equals_one_stream(gpu, precision):
    """test_gpu_scene.py::test_uneven_split_equals_one_stream on 30x44 NV12 frames ([3,45,44]; the net
    runs at 32x48): split=[1, 2] against streams=1 byte for byte in the frames and in last_gate, then
    reuse_flow=True at another t against a fresh call.  As there, the gate takes one t for the batch: one
    leg has scene_threshold and a scalar t, the other the per-pair t = (0.25, 0.5, 0.75) and the codes
    of the same rule as ``gate``."""
    eng = net_of(gpu, precision).engine()
    yy, xx = np.mgrid[0:45, 0:44]
    ramp = (60 + yy + 2 * xx).astype(np.uint8)
    moved = np.roll(ramp, 2, axis=0)
    noise = np.random.default_rng(8).integers(0, 256, (45, 44), dtype=np.uint8)
    f0 = torch.from_numpy(np.stack([ramp, moved, ramp])).to(gpu)
    f1 = torch.from_numpy(np.stack([np.roll(ramp, 1, axis=1), moved, noise])).to(gpu)
    assert byte_gate_codes(f0, f1, 20, 0.75).tolist() == [0, 1, 2]
    assert byte_gate_codes(f0, f1, 20, 0.25).tolist() == [0, 1, 1]
    with torch.no_grad():
        one = eng.forward_yuv(f0, f1, 0.75, streams=1, scene_threshold=20)
        codes1 = eng.last_gate.clone()
        two = eng.forward_yuv(f0, f1, 0.75, split=[1, 2], scene_threshold=20)
        assert torch.equal(two, one) and torch.equal(eng.last_gate, codes1)
        assert codes1.cpu().tolist() == [0, 1, 2]
        assert torch.equal(two[1], f0[1]) and torch.equal(two[2], f1[2]) and not torch.equal(two[0], f0[0])
        again = eng.forward_yuv(f0, f1, 0.25, split=[1, 2], reuse_flow=True, scene_threshold=20)   # kept Flow and sums
        codes2 = eng.last_gate.clone()
        fresh = eng.forward_yuv(f0, f1, 0.25, streams=1, scene_threshold=20)
        assert torch.equal(again, fresh) and torch.equal(codes2, eng.last_gate)
        assert codes2.cpu().tolist() == [0, 1, 1] and torch.equal(again[2], f0[2])
        t = torch.tensor([0.25, 0.5, 0.75])
        g = torch.cat([byte_gate_codes(f0[p:p + 1], f1[p:p + 1], 20, float(t[p])) for p in range(3)])
        assert g.cpu().tolist() == [0, 1, 2]
        one = eng.forward_yuv(f0, f1, t, streams=1, gate=g)
        two = eng.forward_yuv(f0, f1, t, split=[1, 2], gate=g)
        assert torch.equal(two, one) and eng.last_gate is g
        again = eng.forward_yuv(f0, f1, t.flip(0), split=[1, 2], reuse_flow=True, gate=g)
        assert torch.equal(again, eng.forward_yuv(f0, f1, t.flip(0), streams=1, gate=g))
        assert not torch.equal(again[0], two[0])                         # another t: another frame
    eng.check_range()


def test_range_guard_writes_black_and_check_range_raises(gpu):
    """An fp16 overflow (the recipe of test_range_guard_writes_zeros_and_check_range_raises): the output
    is rgb_to_yuv420 of zeros, and check_range raises."""
    from .test_gpu_configs import wide_range_sd
    net = Net()
    net.load_state_dict(wide_range_sd(1e5), strict=True)
    net.precision = "fp32_split16"
    net = net.to(gpu).eval()
    i0, i1 = synthetic_batch(1, 64, 96, first_index=2)
    r0 = i0.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu)
    r1 = i1.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu)
    f0, f1 = yuv.rgb_to_yuv420(r0), yuv.rgb_to_yuv420(r1)
    with torch.no_grad():
        out = net.forward_yuv(f0, f1, 0.5)
    black = yuv.rgb_to_yuv420(torch.zeros_like(r0))
    assert int(black[0, 0, 0]) == 16 and int(black[0, -1, -1]) == 128
    assert torch.equal(out, black)
    with pytest.raises(RuntimeError, match="fp16 range"):
        net.check_range()
    net.precision = "fp32"                               # exact fp32 has no guard: real frames
    with torch.no_grad():
        assert not torch.equal(net.forward_yuv(f0, f1, 0.5), black)


def test_forward_yuv_rejects_bad_inputs(gpu):
    net = net_of(gpu, "fp32")
    f = frames(1, 32, 48, 61, gpu)
    g = torch.zeros(1, dtype=torch.int32, device=gpu)
    with torch.no_grad():
        with pytest.raises(TypeError):
            net.forward_yuv(f.float(), f.float())
        with pytest.raises(ValueError):
            net.forward_yuv(f[:, :47], f[:, :47])                                # 47 rows are not 3*H0/2
        with pytest.raises(ValueError):
            net.forward_yuv(f[:, :, :47], f[:, :, :47])                          # odd W0
        with pytest.raises(ValueError):
            net.forward_yuv(f, f[:, :24])
        with pytest.raises(ValueError):
            net.forward_yuv(f, f, layout="yv12")
        with pytest.raises(ValueError):
            net.forward_yuv(f, f, coef=(1, 2, 3) * 4 + (1, 2, 1 << 16))
        with pytest.raises(ValueError):
            net.forward_yuv(f, f, scene_threshold=20, gate=g)
        with pytest.raises(ValueError):
            net.forward_yuv(f, f, gate=g.long())
        with pytest.raises(RuntimeError):
            net.forward_yuv(f.cpu(), f.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        net.forward_yuv(f, f)                                                    # autograd on
    planar = Net()
    planar.load_state_dict(_SD["sd"], strict=True)
    planar.precision = "fp32_planar"
    planar = planar.to(gpu).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="'fp32', 'fp32_split16' or 'fp16'"):
        planar.forward_yuv(f, f)


def test_other_paths_untouched_by_forward_yuv(gpu):
    net = net_of(gpu, "fp32")
    i0, i1 = synthetic_batch(2, 64, 96)
    i0, i1 = i0.to(gpu), i1.to(gpu)
    r0, r1 = rgb_frames(2, 64, 96, 51, gpu), rgb_frames(2, 64, 96, 52, gpu)
    with torch.no_grad():
        before = net(i0, i1, 0.5).clone()
        before8 = net.forward_u8(r0, r1, 0.5).clone()
        net.forward_yuv(frames(2, 64, 96, 53, gpu), frames(2, 64, 96, 54, gpu), 0.5)
        after = net(i0, i1, 0.5)
        after8 = net.forward_u8(r0, r1, 0.5)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert torch.equal(before8, after8)


def test_y4m_end_to_end(tmp_path, gpu):
    """Five 38x50 frames, sf = 2, batch = 2: 13 frames at 3 F; every third is an input's bytes, the
    others are interpolate_yuv of the pairs."""
    net = net_of(gpu, "fp32")
    h0, w0, sf = 38, 50, 2
    src_frames = frames(5, h0, w0, 71)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with open(src, "wb") as f:
        wr = y4m.Writer(f, w0, h0, 30000, 1001, "420jpeg")
        for fr in src_frames:
            wr.write(fr.numpy())
    logs = []
    n = cv.interpolate_y4m(net, src, dst, sf, batch=2, log=logs.append)
    assert n == 13 and len(logs) == 1
    with open(dst, "rb") as f:
        rd = y4m.Reader(f)
        got = [torch.from_numpy(g).view(3 * h0 // 2, w0) for g in rd]
    assert (rd.width, rd.height, rd.fps_num, rd.fps_den, rd.colorspace) == (w0, h0, 90000, 1001, "420jpeg")
    assert len(got) == 13
    stack = src_frames.to(gpu)
    for k in range(5):
        assert torch.equal(got[3 * k], src_frames[k]), k
    for a in (0, 2):                                         # the steps of batch = 2
        with torch.no_grad():
            want = net.interpolate_yuv(stack[a:a + 2], stack[a + 1:a + 3], [1 / 3, 2 / 3], layout="i420")
        for p in range(2):
            for i in range(sf):
                assert torch.equal(got[3 * (a + p) + 1 + i], want[i][p].cpu()), (a + p, i)
    # file objects work as paths do, and a one-frame stream is refused
    with open(src, "rb") as fi, open(str(tmp_path / "again.y4m"), "wb") as fo:
        assert cv.interpolate_y4m(net, fi, fo, sf, batch=2, log=lambda *x: None) == 13
    assert open(str(tmp_path / "again.y4m"), "rb").read() == open(dst, "rb").read()
    one = str(tmp_path / "one.y4m")
    with open(one, "wb") as f:
        y4m.Writer(f, w0, h0, 25, 1).write(src_frames[0].numpy())
    with pytest.raises(ValueError, match="two frames"):
        cv.interpolate_y4m(net, one, str(tmp_path / "none.y4m"), sf, log=lambda *x: None)
