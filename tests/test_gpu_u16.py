"""GPU: the 16-bit RGB frame path (rrin_pack_g16_u16_h8, the FINAL head's uint16 store, rrin_net_u16_fwd,
rrin_pair_sad_u16, RRINEngine / Net.forward_u16, interpolate_u16, pair_stats_u16) is, bit for bit, its
definition

    forward_u16(f0, f1, t, depth) == frames_float_to_u16(forward(frames_u16_to_float(f0, depth),
                                                                 frames_u16_to_float(f1, depth), t), H0, W0, depth)

evaluated with the same build's Net.forward.  Every comparison is exact equality.  Shapes: those of
tests/test_gpu_yuv.py -- 18x34 and 38x50 (top and right padding), 64x96 (none), 2x2 (the smallest),
16x258 (a second 256-pixel run of the pack kernel) -- and 148x148, whose 65 712 samples hold every
16-bit word.  Frame stacks start one word into their buffer, so a frame's address is only 2-byte aligned."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, yuv
from rrin_amd import convert as cv
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from rrin_amd.synthetic import synthetic_batch

from . import hip_helpers as H
from .test_gpu_u8 import _SD, net_of, padded
from .test_gpu_u8 import frames as rgb_frames
from .test_gpu_yuv import frames as yuv_frames

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
SHAPES = [(18, 34), (38, 50), (64, 96), (2, 2), (16, 258)]
DEPTHS = [10, 12, 16]
ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def odd_stack(a, dev):
    """The uint16 array ``a`` on the device, starting one word into its buffer (address 2 mod 4)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16))
    buf = torch.zeros(t.numel() + 1, dtype=torch.uint16, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t.to(dev))
    assert out.data_ptr() % 4 == 2
    return out


def frames16(n, h0, w0, depth, seed, dev, over=True):
    """uint16 [n,h0,w0,3] of random words (``over``: any word, so some exceed maxval; else samples of the
    depth); the first words of every frame are 0, maxval, maxval + 1 and 65535."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 65536 if over else 1 << depth, (n, h0, w0, 3), dtype=np.uint16)
    maxval = (1 << depth) - 1
    edge = np.array([0, maxval, min(maxval + 1, 65535) if over else 1, 65535 if over else maxval - 1], dtype=np.uint16)
    k = min(4, a[0].size)
    a.reshape(n, -1)[:, :k] = edge[:k]
    return odd_stack(a, dev)


def floats16(f, depth, dev):
    return cv.frames_u16_to_float(f.cpu(), depth).contiguous().to(dev)


def definition_u16(net, f0, f1, t, depth):
    h0, w0 = f0.shape[1:3]
    dev = f0.device
    out = net(floats16(f0, depth, dev), floats16(f1, depth, dev), t)
    return cv.frames_float_to_u16(out, h0, w0, depth)


def float_pack(i0, i1, n, h, w, prec, dev):
    want = H8Tensor(n, 16, h, w, dev, prec)
    v = want.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_h8(i0.data_ptr(), i1.data_ptr(), n, C.byref(v), prec, H.stream(dev)),
               "rrin_pack_g16_h8")
    return want


def assert_same_records(got, want):
    assert want.hi.any()
    assert torch.equal(got.hi.view(torch.uint8), want.hi.view(torch.uint8))
    if want.lo is not None:
        assert torch.equal(got.lo.view(torch.uint8), want.lo.view(torch.uint8))


def check_pack_u16(stack, depth, precision, dev):
    """rrin_pack_g16_u16_h8 of the pairs (stack[:-1], stack[1:]) against rrin_pack_g16_h8 of the float frames."""
    prec = _lib.PRECISIONS[precision]
    n, h0, w0 = stack.shape[0] - 1, stack.shape[1], stack.shape[2]
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    f0, f1 = stack[:-1], stack[1:]
    got = H8Tensor(n, 16, h, w, dev, prec)
    v = got.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_u16_h8(f0.data_ptr(), f1.data_ptr(), h0 * w0 * 3, n, h0, w0, depth, C.byref(v),
                                               prec, H.stream(dev)), "rrin_pack_g16_u16_h8")
    want = float_pack(floats16(f0, depth, dev), floats16(f1, depth, dev), n, h, w, prec, dev)
    torch.cuda.synchronize(dev)
    assert_same_records(got, want)


def test_eight_bit_paths_are_untouched_by_the_16_bit_ones(gpu):
    """forward, forward_u8 and forward_yuv on fixed inputs, before any 16-bit call of this process (this
    module is the first to make one, and this test its first) and after calls of both 16-bit paths at
    the same shape."""
    net = net_of(gpu, "fp32")
    i0, i1 = synthetic_batch(2, 64, 96)
    i0, i1 = i0.to(gpu), i1.to(gpu)
    r0, r1 = rgb_frames(2, 64, 96, 51, gpu), rgb_frames(2, 64, 96, 52, gpu)
    y0, y1 = yuv_frames(2, 64, 96, 53, gpu), yuv_frames(2, 64, 96, 54, gpu)
    with torch.no_grad():
        before = net(i0, i1, 0.5).clone()
        before8 = net.forward_u8(r0, r1, 0.5).clone()
        beforey = net.forward_yuv(y0, y1, 0.5).clone()
        net.forward_u16(frames16(2, 64, 96, 12, 55, gpu), frames16(2, 64, 96, 12, 56, gpu), 0.5, depth=12)
        w = frames16(2, 96, 32, 10, 57, gpu, over=False).view(2, 96, 96)
        net.forward_yuv16(w, w.flip(0), 0.5, depth=10)
        assert torch.equal(net(i0, i1, 0.5).view(torch.int32), before.view(torch.int32))
        assert torch.equal(net.forward_u8(r0, r1, 0.5), before8)
        assert torch.equal(net.forward_yuv(y0, y1, 0.5), beforey)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_u16_equals_float_pack(gpu, precision, shape):
    """The whole record buffers (hi and lo, padding included), depths 10, 12 and 16, two pairs of one
    3-frame stack at an address that is 2 mod 4."""
    h0, w0 = shape
    for depth in DEPTHS:
        check_pack_u16(frames16(3, h0, w0, depth, depth, gpu), depth, precision, gpu)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_u16_every_word(gpu, precision):
    """148 x 148 x 3 = 65 712 samples: frame 0 holds every 16-bit word once (ascending), frame 1 the same
    words in another order, so float(v) / 65535.0f is checked for every v; at depth 10 the same frames
    check the clamp of every word above 1023."""
    rng = np.random.default_rng(16)
    a = np.concatenate([np.arange(65536), rng.integers(0, 65536, 148 * 148 * 3 - 65536)]).astype(np.uint16)
    stack = odd_stack(np.stack([a, rng.permutation(a)]).reshape(2, 148, 148, 3), gpu)
    assert torch.equal(torch.sort(yuv.words_to_int(stack[0]).reshape(-1)[:65536])[0].cpu(), torch.arange(65536, dtype=torch.int32))
    check_pack_u16(stack, 16, precision, gpu)
    check_pack_u16(stack, 10, precision, gpu)


def test_pack_u16_rejects_bad_arguments(gpu):
    L = _lib.lib()
    prec = _lib.PREC_F32R
    f = frames16(2, 18, 34, 10, 1, gpu)
    g = H8Tensor(2, 16, 32, 48, gpu, prec).view(0, 16)
    st = H.stream(gpu)
    call = lambda *a: L.rrin_pack_g16_u16_h8(*a)  # noqa: E731
    assert call(f.data_ptr(), f.data_ptr(), 18 * 34 * 3, 2, 18, 34, 8, C.byref(g), prec, st) == -2      # depth
    assert call(f.data_ptr(), f.data_ptr(), 18 * 34 * 3, 2, 18, 34, 17, C.byref(g), prec, st) == -2
    assert call(None, f.data_ptr(), 18 * 34 * 3, 2, 18, 34, 10, C.byref(g), prec, st) == -2
    assert call(f.data_ptr(), f.data_ptr(), 18 * 34 * 3 - 1, 2, 18, 34, 10, C.byref(g), prec, st) == -2  # overlapping frames
    assert call(f.data_ptr(), f.data_ptr(), 18 * 34 * 3, 2, 18, 50, 10, C.byref(g), prec, st) == -1      # another g16 size
    assert call(f.data_ptr(), f.data_ptr(), 18 * 34 * 3, 2, 18, 34, 10, C.byref(g), _lib.PREC_F32, st) == -2
    # the FINAL head: at most one frame output form, and a depth of 9..16
    d = _lib.HeadH8Desc()
    src = H8Tensor(1, 32, 32, 48, gpu, prec)
    g16 = H8Tensor(1, 16, 32, 48, gpu, prec)
    wt, coef = torch.zeros(3 * 32 * 9 + 3, device=gpu), torch.zeros(8, device=gpu)
    out = torch.zeros(18 * 34 * 3, dtype=torch.uint16, device=gpu)
    d.n, d.cin, d.cout, d.mode, d.prec = 1, 32, 3, _lib.HEAD_FINAL, prec
    d.src, d.g16 = src.view(0, 32), g16.view(0, 16)
    d.w, d.bias, d.coef = wt.data_ptr(), wt.data_ptr() + 4 * 3 * 32 * 9, coef.data_ptr()
    d.h0, d.w0, d.top = 18, 34, 14
    d.out_u16, d.u16_depth = out.data_ptr(), 10
    d.out_u8 = out.data_ptr()
    assert L.rrin_head_h8_fwd(C.byref(d), st) == -2                                   # out_u8 and out_u16
    d.out_u8 = None
    d.out_yuv.y = d.out_yuv.u = d.out_yuv.v = out.data_ptr()
    assert L.rrin_head_h8_fwd(C.byref(d), st) == -2                                   # out_yuv and out_u16
    d.out_yuv.y = None
    d.out_yuv16.y = d.out_yuv16.u = d.out_yuv16.v = out.data_ptr()
    assert L.rrin_head_h8_fwd(C.byref(d), st) == -2                                   # out_yuv16 and out_u16
    d.out_yuv16.y = None
    d.u16_depth = 8
    assert L.rrin_head_h8_fwd(C.byref(d), st) == -2
    d.u16_depth, d.top = 10, 15
    assert L.rrin_head_h8_fwd(C.byref(d), st) == -1                                   # the crop leaves the frame
    torch.cuda.synchronize(gpu)
    assert not out.view(torch.int16).any()                                            # nothing was launched


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_u16_equals_its_definition(gpu, precision, shape):
    """n = 2 on the views [:-1] / [1:] of one 3-frame stack (no copy), depths 10, 12 and 16."""
    net = net_of(gpu, precision)
    h0, w0 = shape
    for depth, t in ((10, 0.5), (12, 0.25), (16, 0.5)):
        fr = frames16(3, h0, w0, depth, 20 + depth, gpu)
        with torch.no_grad():
            want = definition_u16(net, fr[:-1], fr[1:], t, depth)
            got = net.forward_u16(fr[:-1], fr[1:], t, depth=depth)
        assert got.dtype == torch.uint16 and tuple(got.shape) == (2, h0, w0, 3) and got.device == fr.device
        assert torch.equal(got, want), (depth, t)
        assert int(yuv.words_to_int(got).max()) <= (1 << depth) - 1
    net.check_range()


def test_forward_u16_copies_frames_that_are_not_dense(gpu):
    net = net_of(gpu, "fp32")
    fr = frames16(3, 38, 50, 10, 31, gpu)
    with torch.no_grad():
        want = net.forward_u16(fr[:-1], fr[1:], 0.5)
        wide = torch.zeros((2, 38, 60, 3), dtype=torch.uint16, device=gpu)
        wide[:, :, :50] = fr[:-1]
        assert torch.equal(net.forward_u16(wide[:, :, :50], fr[1:], 0.5), want)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_interpolate_u16_reuses_flow_and_keeps_the_other_paths_apart(gpu, precision):
    net = net_of(gpu, precision)
    eng = net.engine()
    f0, f1 = frames16(2, 38, 50, 10, 41, gpu), frames16(2, 38, 50, 10, 42, gpu)
    ts = [0.25, 0.5, 0.75]
    kw = dict(streams=net.streams)
    with torch.no_grad():
        each = [net.forward_u16(f0, f1, t) for t in ts]
        outs = net.interpolate_u16(f0, f1, ts)
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        # the workspaces hold the raw Flow of (f0, f1) at depth 10: no other path, and no other depth,
        # at the same padded shape may take it for its own previous pair
        g0, g1 = rgb_frames(2, 38, 50, 43, gpu), rgb_frames(2, 38, 50, 44, gpu)
        j0, j1 = padded(g0, gpu), padded(g1, gpu)
        y0, y1 = yuv_frames(2, 38, 50, 45, gpu), yuv_frames(2, 38, 50, 46, gpu)
        fresh = {"f": eng.forward(j0, j1, 0.5, **kw), "u8": eng.forward_u8(g0, g1, 0.5, **kw),
                 "yuv": eng.forward_yuv(y0, y1, 0.5, **kw), "u16:12": eng.forward_u16(f1, f0, 0.5, depth=12, **kw)}
        for name in fresh:
            eng.forward_u16(f0, f1, 0.5, **kw)
            got = {"f": lambda: eng.forward(j0, j1, 0.5, reuse_flow=True, **kw),
                   "u8": lambda: eng.forward_u8(g0, g1, 0.5, reuse_flow=True, **kw),
                   "yuv": lambda: eng.forward_yuv(y0, y1, 0.5, reuse_flow=True, **kw),
                   "u16:12": lambda: eng.forward_u16(f1, f0, 0.5, depth=12, reuse_flow=True, **kw)}[name]()
            assert torch.equal(got, fresh[name]), name
        # and the reverse: after each of them forward_u16(reuse_flow=True) recomputes its own Flow
        for other in (lambda: eng.forward(j0, j1, 0.5, **kw), lambda: eng.forward_u8(g0, g1, 0.5, **kw),
                      lambda: eng.forward_yuv(y0, y1, 0.5, **kw), lambda: eng.forward_u16(f1, f0, 0.5, depth=12, **kw)):
            other()
            assert torch.equal(eng.forward_u16(f0, f1, 0.5, reuse_flow=True, **kw), each[1])
    net.check_range()


def sad16(f0, f1, depth, shift=0):
    maxval = (1 << depth) - 1
    a = (yuv.words_to_int(f0) >> shift).clamp(max=maxval).long()
    b = (yuv.words_to_int(f1) >> shift).clamp(max=maxval).long()
    return (a - b).abs().reshape(f0.shape[0], -1).sum(1)


def test_pair_sad_u16_is_exact(gpu):
    net = net_of(gpu, "fp32")
    for depth in (10, 16):
        for h0, w0 in ((17, 33), (2, 2), (1, 1), (64, 96)):            # odd word counts: both alignments of a pair
            fr = frames16(4, h0, w0, depth, 3, gpu)
            got = net.pair_stats_u16(fr[:-1], fr[1:], depth=depth)
            assert got.dtype == torch.int64 and got.cpu().tolist() == sad16(fr[:-1], fr[1:], depth).cpu().tolist()
    # all maxval against zero, large enough for several workgroups per pair: 300*300*3 * 65535 > 2**32
    hi = torch.full((2, 300, 300, 3), 65535, dtype=torch.int32).to(torch.int16).view(torch.uint16).to(gpu)
    lo = torch.zeros_like(hi)
    assert net.pair_stats_u16(hi, lo, depth=16).cpu().tolist() == [300 * 300 * 3 * 65535] * 2
    assert net.pair_stats_u16(hi, lo, depth=10).cpu().tolist() == [300 * 300 * 3 * 1023] * 2     # the clamp
    assert net.pair_stats_u16(hi, hi, depth=16).cpu().tolist() == [0, 0]
    L = _lib.lib()
    s = torch.zeros(2, dtype=torch.int64, device=gpu)
    args = (hi.data_ptr(), lo.data_ptr(), 300 * 300 * 3, 2, 300, 300)
    assert L.rrin_pair_sad_u16(*args, 8, 0, s.data_ptr(), H.stream(gpu)) == -2
    assert L.rrin_pair_sad_u16(*args, 10, 7, s.data_ptr(), H.stream(gpu)) == -2
    assert L.rrin_pair_sad_u16(hi.data_ptr() + 1, lo.data_ptr(), 300 * 300 * 3, 2, 300, 300, 10, 0, s.data_ptr(),
                               H.stream(gpu)) == -2


def gate_inputs16(dev, depth):
    """f0 / f1 uint16 [4,38,50,3]: two ordinary pairs (a smooth ramp against itself moved by a column), a
    duplicate pair, a cut pair (the ramp against random samples)."""
    up = 1 << (depth - 8)
    yy, xx, cc = np.mgrid[0:38, 0:50, 0:3]
    ramp = ((60 + yy + 2 * xx + 5 * cc) * up).astype(np.uint16)
    noise = np.random.default_rng(8).integers(0, 1 << depth, ramp.shape, dtype=np.uint16)
    f0 = np.stack([ramp, np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), ramp])
    f1 = np.stack([np.roll(ramp, 1, axis=1), np.roll(ramp, 1, axis=0), np.roll(ramp, 2, axis=1), noise])
    return odd_stack(f0, dev), odd_stack(f1, dev)


def test_forward_u16_scene_gate(gpu):
    net = net_of(gpu, "fp32")
    depth, up = 10, 4
    f0, f1 = gate_inputs16(gpu, depth)
    sad = sad16(f0, f1, depth).cpu()
    mean = sad.float() / (38 * 50 * 3)
    assert max(mean[0], mean[1]) < 10 * up and mean[2] == 0 and mean[3] > 40 * up, mean
    th = 20 * up
    with torch.no_grad():
        assert net.pair_stats_u16(f0, f1, depth=depth).cpu().tolist() == sad.tolist()
        for t in (0.25, 0.5):
            cut = 1 if t < 0.5 else 2
            plain = net.forward_u16(f0, f1, t, depth=depth)
            got = net.forward_u16(f0, f1, t, depth=depth, scene_threshold=th)
            codes = net.last_gate.clone()
            assert codes.cpu().tolist() == [0, 0, 1, cut]
            assert torch.equal(got[:2], plain[:2]) and torch.equal(got[2], f0[2])
            assert torch.equal(got[3], f0[3] if cut == 1 else f1[3]) and not torch.equal(plain[3], got[3])
        ts = [0.25, 0.5, 0.75]
        each = [net.forward_u16(f0, f1, t, depth=depth, scene_threshold=th) for t in ts]
        outs = net.interpolate_u16(f0, f1, ts, depth=depth, scene_threshold=th)
        assert net.last_gate.cpu().tolist() == [0, 0, 1, 2]
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        g = torch.tensor([2, 0, 9, 1], dtype=torch.int32, device=gpu)
        gated = net.forward_u16(f0, f1, 0.5, depth=depth, gate=g)
        assert net.last_gate is g
        plain = net.forward_u16(f0, f1, 0.5, depth=depth)
        assert torch.equal(gated[0], f1[0]) and torch.equal(gated[1:3], plain[1:3]) and torch.equal(gated[3], f0[3])
        with pytest.raises(ValueError):
            net.forward_u16(f0, f1, 0.5, depth=depth, scene_threshold=1024)            # above maxval


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_uneven_split_equals_one_stream(gpu, precision):
    eng = net_of(gpu, precision).engine()
    f0, f1 = gate_inputs16(gpu, 12)
    f0, f1 = f0[1:], f1[1:]                                      # ordinary, duplicate, cut
    with torch.no_grad():
        one = eng.forward_u16(f0, f1, 0.75, depth=12, streams=1, scene_threshold=320)
        codes1 = eng.last_gate.clone()
        two = eng.forward_u16(f0, f1, 0.75, depth=12, split=[1, 2], scene_threshold=320)
        assert torch.equal(two, one) and torch.equal(eng.last_gate, codes1) and codes1.cpu().tolist() == [0, 1, 2]
        again = eng.forward_u16(f0, f1, 0.25, depth=12, split=[1, 2], reuse_flow=True, scene_threshold=320)
        codes2 = eng.last_gate.clone()
        fresh = eng.forward_u16(f0, f1, 0.25, depth=12, streams=1, scene_threshold=320)
        assert torch.equal(again, fresh) and codes2.cpu().tolist() == [0, 1, 1]
        assert torch.equal(eng.forward_u16(f0, f1, 0.25, depth=12, split=[2, 1]), eng.forward_u16(f0, f1, 0.25, depth=12, streams=1))
    eng.check_range()


def test_range_guard_writes_zeros_and_check_range_raises(gpu):
    """The recipe of the 8-bit test: weights that overflow fp16; the frames are all zero words."""
    from .test_gpu_configs import wide_range_sd
    net = Net()
    net.load_state_dict(wide_range_sd(1e5), strict=True)
    net.precision = "fp32_split16"
    net = net.to(gpu).eval()
    i0, i1 = synthetic_batch(1, 64, 96, first_index=2)
    f0 = cv.frames_float_to_u16(i0, 64, 96, 10).to(gpu)
    f1 = cv.frames_float_to_u16(i1, 64, 96, 10).to(gpu)
    with torch.no_grad():
        out = net.forward_u16(f0, f1, 0.5)
    assert not out.view(torch.int16).any()
    with pytest.raises(RuntimeError, match="fp16 range"):
        net.check_range()
    net.precision = "fp32"
    with torch.no_grad():
        assert net.forward_u16(f0, f1, 0.5).view(torch.int16).any()


def test_forward_u16_rejects_bad_inputs(gpu):
    net = net_of(gpu, "fp32")
    f = frames16(1, 32, 48, 10, 61, gpu)
    g = torch.zeros(1, dtype=torch.int32, device=gpu)
    with torch.no_grad():
        with pytest.raises(TypeError):
            net.forward_u16(f.view(torch.int16), f.view(torch.int16))
        with pytest.raises(TypeError):
            net.forward_u16(f.to(torch.uint8), f.to(torch.uint8))
        with pytest.raises(ValueError):
            net.forward_u16(f, f[:, :16])
        for depth in (8, 17, 10.0, None):
            with pytest.raises(ValueError):
                net.forward_u16(f, f, depth=depth)
            with pytest.raises(ValueError):
                net.pair_stats_u16(f, f, depth=depth)
        with pytest.raises(ValueError):
            net.forward_u16(f, f, scene_threshold=20, gate=g)
        with pytest.raises(RuntimeError):
            net.forward_u16(f.cpu(), f.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        net.forward_u16(f, f)
    planar = Net()
    planar.load_state_dict(_SD["sd"], strict=True)
    planar.precision = "fp32_planar"
    planar = planar.to(gpu).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="'fp32', 'fp32_split16' or 'fp16'"):
        planar.forward_u16(f, f)
    d = _lib.NetU16Desc()
    assert _lib.lib().rrin_net_u16_fwd(C.byref(d), H.stream(gpu)) == -2
    assert t_coefficients(0.5, 1).shape == (1, 8)
