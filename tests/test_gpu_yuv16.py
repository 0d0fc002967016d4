"""GPU: the 16-bit YUV 4:2:0 frame path (rrin_pack_g16_yuv16_h8, the FINAL head's 16-bit 4:2:0 store,
rrin_net_yuv16_fwd, RRINEngine / Net.forward_yuv16, interpolate_yuv16, pair_stats_yuv16, the 10-bit route
of convert.interpolate_y4m) is, bit for bit, its definition

    forward_yuv16(f0, f1, t) == rgb16_to_yuv420(forward_u16(yuv420_to_rgb16(f0), yuv420_to_rgb16(f1), t, depth))

with the integer conversions of rrin_amd.yuv as the oracle: depths 10 and 12, both layouts, samples in the
low bits (msb=False) and in the high bits (msb=True).  Every comparison is exact equality.  Shapes: those
of tests/test_gpu_yuv.py, and 64x64 luma planes that hold every code of a depth."""
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
from .test_gpu_u8 import net_of, padded
from .test_gpu_u8 import frames as rgb_frames
from .test_gpu_u16 import assert_same_records, float_pack, floats16, odd_stack, sad16
from .test_gpu_yuv import frames as yuv_frames

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
SHAPES = [(18, 34), (38, 50), (64, 96), (2, 2), (16, 258)]
ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def coefs(depth):
    return [None, yuv.coefficients("bt601", True, depth)]


def frames(n, h0, w0, depth, seed, dev, msb=False, over=True):
    """uint16 [n, 3*h0//2, w0] at an address that is 2 mod 4.  msb=False: random samples of the depth, with
    (``over``) a few words above maxval; msb=True: the samples in the high bits over random low bits."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << depth, (n, 3 * h0 // 2, w0), dtype=np.uint16)
    if msb:
        a = (a << (16 - depth)) | rng.integers(0, 1 << (16 - depth), a.shape, dtype=np.uint16)
    elif over:
        a.reshape(n, -1)[:, ::5] |= rng.integers(0, 2, (n, (a[0].size + 4) // 5), dtype=np.uint16) << 15
    return odd_stack(a, dev)


def relayout(fr, src, dst):
    return yuv.join_planes(*yuv.split_planes(fr, src), dst).contiguous()


def stack_desc(t, h0, w0, layout, depth, msb, stride=None):
    """rrin_yuv420_16 of a dense-frame uint16 stack tensor."""
    s = _lib.Yuv420x16()
    s.y, s.u = t.data_ptr(), t.data_ptr() + 2 * h0 * w0
    s.img_stride, s.y_pitch = (t.stride(0) if stride is None else stride), w0
    s.depth, s.shift = depth, (16 - depth if msb else 0)
    if layout == "nv12":
        s.v, s.c_pitch, s.c_step = s.u + 2, w0, 2
    else:
        s.v, s.c_pitch, s.c_step = s.u + 2 * (h0 * w0 // 4), w0 // 2, 1
    return s


def check_pack_yuv16(fr, layout, coef, depth, msb, precision, dev):
    """rrin_pack_g16_yuv16_h8 of the pairs (fr[:-1], fr[1:]) against rrin_pack_g16_h8 of
    frames_u16_to_float(yuv420_to_rgb16(...)): the whole record buffers."""
    prec = _lib.PRECISIONS[precision]
    n, (h0, w0) = fr.shape[0] - 1, yuv.frame_size(fr)
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    f0, f1 = fr[:-1], fr[1:]
    k = _lib.YuvCoef(*yuv.as_coef(coef, depth))
    got = H8Tensor(n, 16, h, w, dev, prec)
    v = got.view(0, 16)
    s0, s1 = stack_desc(f0, h0, w0, layout, depth, msb), stack_desc(f1, h0, w0, layout, depth, msb)
    _lib.check(_lib.lib().rrin_pack_g16_yuv16_h8(C.byref(s0), C.byref(s1), C.byref(k), n, h0, w0, C.byref(v), prec,
                                                 H.stream(dev)), "rrin_pack_g16_yuv16_h8")
    r0 = yuv.yuv420_to_rgb16(f0, layout, coef, depth, msb)
    r1 = yuv.yuv420_to_rgb16(f1, layout, coef, depth, msb)
    want = float_pack(floats16(r0, depth, dev), floats16(r1, depth, dev), n, h, w, prec, dev)
    torch.cuda.synchronize(dev)
    assert_same_records(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_yuv16_equals_float_pack_of_the_converted_frames(gpu, precision, shape):
    h0, w0 = shape
    for depth in (10, 12):
        for msb in (False, True):
            nv12 = frames(3, h0, w0, depth, depth + msb, gpu, msb)
            for layout in yuv.LAYOUTS:
                fr = nv12 if layout == "nv12" else odd_stack(relayout(nv12, "nv12", "i420").cpu().numpy(), gpu)
                for coef in coefs(depth):
                    check_pack_yuv16(fr, layout, coef, depth, msb, precision, gpu)


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_yuv16_every_code(gpu, precision, depth):
    """64 x 64 luma samples (4096) hold every code of the depth (depth 10: four times) over grey chroma
    (U = V = mid), full range: R = G = B = Y, so float(v) / float(maxval) is checked for every code v.  A
    second frame holds random chroma; both alignments."""
    rng = np.random.default_rng(depth)
    mid = 1 << (depth - 1)
    y = (np.arange(4096) % (1 << depth)).astype(np.uint16).reshape(64, 64)
    grey = np.concatenate([y, np.full((32, 64), mid, dtype=np.uint16)])
    other = np.concatenate([rng.permutation(y.reshape(-1)).reshape(64, 64), rng.integers(0, 1 << depth, (32, 64), dtype=np.uint16)])
    a = np.stack([grey, other])
    full = yuv.coefficients("bt709", True, depth)
    rgb = yuv.yuv420_to_rgb16(torch.from_numpy(a[:1].copy()), "i420", full, depth)
    assert torch.equal(torch.sort(yuv.words_to_int(rgb[..., 0]).reshape(-1))[0], torch.from_numpy(np.sort(y.reshape(-1)).astype(np.int32)))
    for msb in (False, True):
        fr = odd_stack(a << (16 - depth) if msb else a, gpu)
        check_pack_yuv16(fr, "i420", full, depth, msb, precision, gpu)
        check_pack_yuv16(fr, "nv12", None, depth, msb, precision, gpu)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv16_equals_its_definition(gpu, precision, shape):
    """n = 2 on the views [:-1] / [1:] of one 3-frame stack; depths 10 and 12, both layouts, both alignments,
    the default and the BT.601 full-range coefficients.  The RGB reference is computed once per depth,
    alignment and matrix (the layouts hold the same planes)."""
    net = net_of(gpu, precision)
    h0, w0 = shape
    for depth, t in ((10, 0.5), (12, 0.25)):
        for msb in (False, True):
            nv12 = frames(3, h0, w0, depth, 10 + depth + msb, gpu, msb)
            i420 = odd_stack(relayout(nv12, "nv12", "i420").cpu().numpy(), gpu)
            for coef in coefs(depth):
                r = yuv.yuv420_to_rgb16(nv12, "nv12", coef, depth, msb)
                with torch.no_grad():
                    rgb = net.forward_u16(r[:-1], r[1:], t, depth=depth)
                    for layout, fr in (("nv12", nv12), ("i420", i420)):
                        got = net.forward_yuv16(fr[:-1], fr[1:], t, layout=layout, depth=depth, msb=msb, coef=coef)
                        assert got.dtype == torch.uint16 and tuple(got.shape) == (2, 3 * h0 // 2, w0)
                        assert torch.equal(got, yuv.rgb16_to_yuv420(rgb, layout, coef, depth, msb)), (depth, msb, layout, coef)
    net.check_range()


@pytest.mark.parametrize("layout", yuv.LAYOUTS)
def test_pitched_output_through_the_c_abi(gpu, layout):
    """rrin_net_yuv16_fwd into planes of their own with y_pitch = w0 + 6 words and the chroma pitch to
    match, prefilled with 0xA5A5: the planes equal the dense result, every other word is still 0xA5A5."""
    net = net_of(gpu, "fp32")
    eng = net.engine()
    h0, w0, n, depth, msb = 38, 50, 2, 10, True
    h, w = 48, 64
    fr = frames(3, h0, w0, depth, 12, gpu, msb)
    if layout == "i420":
        fr = relayout(fr, "nv12", "i420")
    with torch.no_grad():
        dense = eng.forward_yuv16(fr[:-1], fr[1:], 0.5, layout=layout, depth=depth, msb=msb, streams=1)
    torch.cuda.synchronize(gpu)
    yp = w0 + 6
    cp = yp if layout == "nv12" else w0 // 2 + 3
    cw = w0 if layout == "nv12" else w0 // 2
    fill = lambda: torch.full((n, h0, yp), 0xA5A5 - 65536, dtype=torch.int16, device=gpu).view(torch.uint16)  # noqa: E731
    ybuf, ubuf, vbuf = fill(), fill(), fill()
    sentinel = lambda x: (yuv.words_to_int(x) == 0xA5A5).all()  # noqa: E731
    d = _lib.NetYuv16Desc()
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
    d.f0 = stack_desc(fr[:-1], h0, w0, layout, depth, msb)
    d.f1 = stack_desc(fr[1:], h0, w0, layout, depth, msb)
    o = d.out
    o.y, o.img_stride, o.y_pitch, o.c_pitch, o.depth, o.shift = ybuf.data_ptr(), h0 * yp, yp, cp, depth, 16 - depth
    if layout == "nv12":
        o.u, o.v, o.c_step = ubuf.data_ptr(), ubuf.data_ptr() + 2, 2
    else:
        o.u, o.v, o.c_step = ubuf.data_ptr(), vbuf.data_ptr(), 1
    d.coef = _lib.YuvCoef(*yuv.coefficients(depth=depth))
    d.h0, d.w0 = h0, w0
    L = _lib.lib()
    # depth, shift and sizes are checked before anything is launched
    for field, bad, rc in (("depth", 11, -2), ("shift", 3, -2), ("c_step", 3, -2), ("y_pitch", w0 - 1, -1)):
        keep = getattr(o, field)
        setattr(o, field, bad)
        assert L.rrin_net_yuv16_fwd(C.byref(d), H.stream(gpu)) == rc, field
        setattr(o, field, keep)
    d.f1.shift = 0
    assert L.rrin_net_yuv16_fwd(C.byref(d), H.stream(gpu)) == -2                 # the stacks' alignments differ
    d.f1.shift = 16 - depth
    d.h0 = h0 - 1
    assert L.rrin_net_yuv16_fwd(C.byref(d), H.stream(gpu)) == -1                 # odd size
    d.h0 = h0
    torch.cuda.synchronize(gpu)
    assert sentinel(ybuf) and sentinel(ubuf) and sentinel(vbuf)
    _lib.check(L.rrin_net_yuv16_fwd(C.byref(d), H.stream(gpu)), "rrin_net_yuv16_fwd")
    torch.cuda.synchronize(gpu)
    y, u, v = yuv.split_planes(dense, layout)
    assert torch.equal(ybuf[:, :, :w0], y) and sentinel(ybuf[:, :, w0:])
    crows = ubuf.view(n, -1)[:, :(h0 // 2) * cp].view(n, h0 // 2, cp)
    assert sentinel(ubuf.view(n, -1)[:, (h0 // 2) * cp:]) and sentinel(crows[:, :, cw:])
    if layout == "nv12":
        assert torch.equal(crows[:, :, 0:cw:2], u) and torch.equal(crows[:, :, 1:cw:2], v)
        assert sentinel(vbuf)
    else:
        vrows = vbuf.view(n, -1)[:, :(h0 // 2) * cp].view(n, h0 // 2, cp)
        assert torch.equal(crows[:, :, :cw], u) and torch.equal(vrows[:, :, :cw], v)
        assert sentinel(vbuf.view(n, -1)[:, (h0 // 2) * cp:]) and sentinel(vrows[:, :, cw:])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_interpolate_yuv16_reuses_flow_and_keeps_the_other_paths_apart(gpu, precision):
    net = net_of(gpu, precision)
    eng = net.engine()
    f0, f1 = frames(2, 38, 50, 10, 41, gpu), frames(2, 38, 50, 10, 42, gpu)
    ts = [0.25, 0.5, 0.75]
    kw = dict(streams=net.streams)
    with torch.no_grad():
        each = [net.forward_yuv16(f0, f1, t) for t in ts]
        outs = net.interpolate_yuv16(f0, f1, ts)
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        g0, g1 = rgb_frames(2, 38, 50, 43, gpu), rgb_frames(2, 38, 50, 44, gpu)
        j0, j1 = padded(g0, gpu), padded(g1, gpu)
        y0, y1 = yuv_frames(2, 38, 50, 45, gpu), yuv_frames(2, 38, 50, 46, gpu)
        others = {
            "forward": lambda **k: eng.forward(j0, j1, 0.5, **k, **kw),
            "u8": lambda **k: eng.forward_u8(g0, g1, 0.5, **k, **kw),
            "yuv": lambda **k: eng.forward_yuv(y0, y1, 0.5, **k, **kw),
            "msb": lambda **k: eng.forward_yuv16(f1, f0, 0.5, msb=True, **k, **kw),
            "depth 12": lambda **k: eng.forward_yuv16(f1, f0, 0.5, depth=12, **k, **kw),
            "i420": lambda **k: eng.forward_yuv16(f1, f0, 0.5, layout="i420", **k, **kw),
            "bt601": lambda **k: eng.forward_yuv16(f1, f0, 0.5, coef=yuv.coefficients("bt601", True, 10), **k, **kw),
        }
        for name, call in others.items():
            fresh = call()
            eng.forward_yuv16(f0, f1, 0.5, **kw)
            assert torch.equal(call(reuse_flow=True), fresh), name           # does not take the yuv16 Flow
            assert torch.equal(eng.forward_yuv16(f0, f1, 0.5, reuse_flow=True, **kw), each[1]), name   # nor the reverse
    net.check_range()


def test_forward_yuv16_scene_gate_and_sums(gpu):
    net = net_of(gpu, "fp32")
    depth, up = 10, 4
    yy, xx = np.mgrid[0:57, 0:50]
    ramp = ((60 + yy + 2 * xx) * up).astype(np.uint16)
    noise = np.random.default_rng(8).integers(0, 1 << depth, (57, 50), dtype=np.uint16)
    a0 = np.stack([ramp, np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), ramp])
    a1 = np.stack([np.roll(ramp, 1, axis=1), np.roll(ramp, 1, axis=0), np.roll(ramp, 2, axis=1), noise])
    for msb in (False, True):
        sh = 16 - depth if msb else 0
        dirt = np.random.default_rng(9).integers(0, 1 << sh, a0.shape, dtype=np.uint16) if msb else 0
        f0, f1 = odd_stack(a0 << sh, gpu), odd_stack((a1 << sh) | dirt, gpu)      # msb: f1 has dirty low bits
        sad = sad16(f0, f1, depth, sh).cpu()
        assert sad[2] == 0 and (not msb or not torch.equal(f0[2], f1[2]))           # a duplicate in its samples
        with torch.no_grad():
            stats = net.pair_stats_yuv16(f0, f1, depth=depth, msb=msb)
            assert stats.dtype == torch.int64 and stats.cpu().tolist() == sad.tolist()
            for t in (0.25, 0.5):
                cut = 1 if t < 0.5 else 2
                plain = net.forward_yuv16(f0, f1, t, depth=depth, msb=msb)
                got = net.forward_yuv16(f0, f1, t, depth=depth, msb=msb, scene_threshold=20 * up)
                assert net.last_gate.cpu().tolist() == [0, 0, 1, cut]
                assert torch.equal(got[:2], plain[:2]) and torch.equal(got[2], f0[2])
                assert torch.equal(got[3], f0[3] if cut == 1 else f1[3]) and not torch.equal(plain[3], got[3])
            g = torch.tensor([2, 0, 9, 1], dtype=torch.int32, device=gpu)
            gated = net.forward_yuv16(f0, f1, 0.5, depth=depth, msb=msb, gate=g)
            plain = net.forward_yuv16(f0, f1, 0.5, depth=depth, msb=msb)
            assert torch.equal(gated[0], f1[0]) and torch.equal(gated[1:3], plain[1:3]) and torch.equal(gated[3], f0[3])
            # the uneven split equals one stream, frames and codes
            eng = net.engine()
            one = eng.forward_yuv16(f0, f1, 0.75, depth=depth, msb=msb, streams=1, scene_threshold=20 * up)
            codes = eng.last_gate.clone()
            two = eng.forward_yuv16(f0, f1, 0.75, depth=depth, msb=msb, split=[1, 3], scene_threshold=20 * up)
            assert torch.equal(two, one) and torch.equal(eng.last_gate, codes)
    # all maxval against zero at depth 12, samples in the high bits
    hi = torch.full((2, 96, 64), 0xFFF0 - 65536, dtype=torch.int16, device=gpu).view(torch.uint16)
    assert net.pair_stats_yuv16(hi, torch.zeros_like(hi), depth=12, msb=True).cpu().tolist() == [96 * 64 * 4095] * 2


def test_range_guard_writes_black_and_check_range_raises(gpu):
    from .test_gpu_configs import wide_range_sd
    net = Net()
    net.load_state_dict(wide_range_sd(1e5), strict=True)
    net.precision = "fp32_split16"
    net = net.to(gpu).eval()
    i0, i1 = synthetic_batch(1, 64, 96, first_index=2)
    r0 = cv.frames_float_to_u16(i0, 64, 96, 10).to(gpu)
    r1 = cv.frames_float_to_u16(i1, 64, 96, 10).to(gpu)
    f0, f1 = yuv.rgb16_to_yuv420(r0), yuv.rgb16_to_yuv420(r1)
    with torch.no_grad():
        out = net.forward_yuv16(f0, f1, 0.5)
    black = yuv.rgb16_to_yuv420(torch.zeros_like(r0))
    assert int(black[0, 0, 0]) == 64 and int(black[0, -1, -1]) == 512
    assert torch.equal(out, black)
    with pytest.raises(RuntimeError, match="fp16 range"):
        net.check_range()


def test_forward_yuv16_rejects_bad_inputs(gpu):
    net = net_of(gpu, "fp32")
    f = frames(1, 32, 48, 10, 61, gpu)
    with torch.no_grad():
        with pytest.raises(TypeError):
            net.forward_yuv16(f.to(torch.uint8), f.to(torch.uint8))
        with pytest.raises(ValueError):
            net.forward_yuv16(f[:, :47], f[:, :47])
        with pytest.raises(ValueError):
            net.forward_yuv16(f[:, :, :47], f[:, :, :47])
        with pytest.raises(ValueError):
            net.forward_yuv16(f, f, layout="yv12")
        for depth in (8, 9, 14, 16):
            with pytest.raises(ValueError):
                net.forward_yuv16(f, f, depth=depth)
            with pytest.raises(ValueError):
                net.pair_stats_yuv16(f, f, depth=depth)
        with pytest.raises(ValueError):
            net.forward_yuv16(f, f, coef=(1, 2, 3) * 4 + (1, 2, 1 << 15))
        with pytest.raises(ValueError):
            net.forward_yuv16(f, f, scene_threshold=1024)
    with pytest.raises(RuntimeError, match="inference-only"):
        net.forward_yuv16(f, f)


def test_y4m_10_bit_end_to_end(tmp_path, gpu):
    """Three 38x50 frames of C420p10, sf = 2, batch = 2: 7 frames at 3 F under the input's tag; every third
    is an input's words, the others are interpolate_yuv16 of the pairs with the depth's default matrix."""
    net = net_of(gpu, "fp32")
    h0, w0, sf = 38, 50, 2
    src_frames = frames(3, h0, w0, 10, 71, "cpu", over=False)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    with open(src, "wb") as f:
        wr = y4m.Writer(f, w0, h0, 30000, 1001, "420p10", depths=(8, 10, 12))
        for fr in src_frames:
            wr.write(fr.numpy())
    assert cv.interpolate_y4m(net, src, dst, sf, batch=2, log=lambda *x: None) == 7
    with open(dst, "rb") as f:
        rd = y4m.Reader(f, depths=(8, 10, 12))
        got = [torch.from_numpy(g).view(3 * h0 // 2, w0) for g in rd]
    assert (rd.width, rd.height, rd.fps_num, rd.fps_den, rd.colorspace, rd.bit_depth) == (w0, h0, 90000, 1001, "420p10", 10)
    assert len(got) == 7
    stack = src_frames.to(gpu)
    for k in range(3):
        assert torch.equal(got[3 * k], src_frames[k]), k
    with torch.no_grad():
        want = net.interpolate_yuv16(stack[:-1], stack[1:], [1 / 3, 2 / 3], layout="i420", depth=10, msb=False)
    for p in range(2):
        for i in range(sf):
            assert torch.equal(got[3 * p + 1 + i], want[i][p].cpu()), (p, i)
