"""GPU: the scene-cut / duplicate-frame gate of the 8-bit frame path -- rrin_pair_sad_u8,
rrin_gate_from_sad_u8, rrin_gate_frames_u8, Net.forward_u8 / interpolate_u8 (scene_threshold=,
gate=), Net.pair_stats_u8 / last_gate and interpolate_folder(scene_threshold=).  Every comparison
is exact equality: the sums are integers, the gated frames are copies, the ungated frames are the
bits of the same call without the gate."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from rrin_amd import _lib
from rrin_amd import convert as cv

from . import hip_helpers as H
from .test_gpu_u8 import net_of
from .test_scene_host import read, scene_frames, write_frames

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A5A5A5A5A5A5A5A


def stack_of(n, h0, w0, seed):
    """uint8 [n,h0,w0,3] random frames (numpy)."""
    return np.random.default_rng(seed).integers(0, 256, (n, h0, w0, 3), dtype=np.uint8)


def np_sad(a, b):
    return [int(np.abs(x.astype(np.int64) - y).sum()) for x, y in zip(a, b)]


def run_sad(f0, f1, stride, n, h0, w0, dev):
    """rrin_pair_sad_u8 twice into a buffer pre-filled with garbage; both results as lists."""
    sad = torch.full((n,), GARBAGE, dtype=torch.int64, device=dev)
    got = []
    for _ in range(2):
        _lib.check(_lib.lib().rrin_pair_sad_u8(f0.data_ptr(), f1.data_ptr(), stride, n, h0, w0, sad.data_ptr(),
                                               H.stream(dev)), "rrin_pair_sad_u8")
        got.append(sad.cpu().tolist())
    return got


@pytest.mark.parametrize("shape", [(1, 1), (17, 33), (37, 50), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_sad_equals_numpy(gpu, shape):
    h0, w0 = shape
    n, frame = 3, h0 * w0 * 3
    a, b = stack_of(n, h0, w0, 1), stack_of(n, h0, w0, 2)
    b[1] = a[1]                                          # an identical pair: 0
    a[2], b[2] = 0, 255                                  # the largest sum of the shape
    want = np_sad(a, b)
    assert want[1] == 0 and want[2] == 255 * frame
    f0, f1 = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    assert run_sad(f0, f1, frame, n, h0, w0, gpu) == [want, want]
    # two views of one 4-frame stack: f1 starts one frame (an odd number of bytes) after f0
    s = stack_of(4, h0, w0, 3)
    s[2] = s[1]
    fr = torch.from_numpy(s).to(gpu)
    want = np_sad(s[:-1], s[1:])
    assert want[1] == 0
    assert run_sad(fr[:-1], fr[1:], frame, n, h0, w0, gpu) == [want, want]
    # frames further apart than their size (stride = frame + 7: every frame at another alignment)
    wide0 = torch.zeros((n, frame + 7), dtype=torch.uint8, device=gpu)
    wide1 = torch.full((n, frame + 7), 255, dtype=torch.uint8, device=gpu)
    wide0[:, :frame] = f0.view(n, frame)
    wide1[:, :frame] = f1.view(n, frame)
    want = np_sad(a, b)
    assert run_sad(wide0, wide1, frame + 7, n, h0, w0, gpu) == [want, want]


def test_pair_sad_sums_in_64_bits(gpu):
    """2400 x 2400 zeros against 255: 4,406,400,000 > 2^32."""
    h0 = w0 = 2400
    f0 = torch.zeros((1, h0, w0, 3), dtype=torch.uint8, device=gpu)
    f1 = torch.full((1, h0, w0, 3), 255, dtype=torch.uint8, device=gpu)
    assert run_sad(f0, f1, h0 * w0 * 3, 1, h0, w0, gpu) == [[4_406_400_000]] * 2


def test_gate_from_sad(gpu):
    L = _lib.lib()
    limit = 123_456_789_012                              # above 2^32: a 64-bit compare
    sad = torch.tensor([0, limit, limit + 1, 1], dtype=torch.int64, device=gpu)
    for cut in (1, 2):
        gate = torch.full((4,), -9, dtype=torch.int32, device=gpu)
        _lib.check(L.rrin_gate_from_sad_u8(sad.data_ptr(), 4, limit, cut, gate.data_ptr(), H.stream(gpu)),
                   "rrin_gate_from_sad_u8")
        assert gate.cpu().tolist() == [1, 0, cut, 0]
    gate = torch.full((4,), -9, dtype=torch.int32, device=gpu)
    for bad in (0, 3, -1):
        assert L.rrin_gate_from_sad_u8(sad.data_ptr(), 4, limit, bad, gate.data_ptr(), H.stream(gpu)) == -2
    assert gate.cpu().tolist() == [-9] * 4


@pytest.mark.parametrize("shape", [(17, 33), (37, 50)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gate_frames(gpu, shape):
    L = _lib.lib()
    h0, w0 = shape
    n, frame = 5, h0 * w0 * 3
    codes = [0, 1, 2, 7, 1]
    gate = torch.tensor(codes, dtype=torch.int32, device=gpu)
    pattern = (torch.arange(n * frame, dtype=torch.int64) * 7 + 3).to(torch.uint8).view(n, h0, w0, 3)

    def check(f0, f1, stride):
        out = pattern.to(gpu)
        _lib.check(L.rrin_gate_frames_u8(f0.data_ptr(), f1.data_ptr(), stride, n, h0, w0, gate.data_ptr(),
                                         out.data_ptr(), H.stream(gpu)), "rrin_gate_frames_u8")
        out = out.cpu()
        for p, c in enumerate(codes):
            want = f0[p].cpu() if c == 1 else f1[p].cpu() if c == 2 else pattern[p]
            assert torch.equal(out[p], want), (p, c)

    f0, f1 = torch.from_numpy(stack_of(n, h0, w0, 4)).to(gpu), torch.from_numpy(stack_of(n, h0, w0, 5)).to(gpu)
    check(f0, f1, frame)
    fr = torch.from_numpy(stack_of(n + 1, h0, w0, 6)).to(gpu)        # views of one stack
    check(fr[:-1], fr[1:], frame)
    # an output that starts at every alignment: frames of out begin at odd addresses anyway (frame
    # is odd for these shapes), here the buffer itself is shifted too
    for shift in (1, 2, 3, 5, 15):
        buf = torch.full((n * frame + 32,), 0xEE, dtype=torch.uint8, device=gpu)
        out = buf[shift:shift + n * frame]
        out.copy_(pattern.view(-1))
        _lib.check(L.rrin_gate_frames_u8(f0.data_ptr(), f1.data_ptr(), frame, n, h0, w0, gate.data_ptr(),
                                         out.data_ptr(), H.stream(gpu)), "rrin_gate_frames_u8")
        host = buf.cpu()
        assert (host[:shift] == 0xEE).all() and (host[shift + n * frame:] == 0xEE).all(), shift
        got = host[shift:shift + n * frame].view(n, h0, w0, 3)
        for p, c in enumerate(codes):
            want = f0[p].cpu() if c == 1 else f1[p].cpu() if c == 2 else pattern[p]
            assert torch.equal(got[p], want), (shift, p, c)
    # argument errors: nothing is launched, the output keeps its bytes
    out = pattern.to(gpu)
    a, b, g, o, st = f0.data_ptr(), f1.data_ptr(), gate.data_ptr(), out.data_ptr(), H.stream(gpu)
    assert L.rrin_gate_frames_u8(None, b, frame, n, h0, w0, g, o, st) == -2
    assert L.rrin_gate_frames_u8(a, None, frame, n, h0, w0, g, o, st) == -2
    assert L.rrin_gate_frames_u8(a, b, frame, n, h0, w0, None, o, st) == -2
    assert L.rrin_gate_frames_u8(a, b, frame, n, h0, w0, g, None, st) == -2
    assert L.rrin_gate_frames_u8(a, b, frame, 0, h0, w0, g, o, st) == -1
    assert L.rrin_gate_frames_u8(a, b, frame, n, 0, w0, g, o, st) == -1
    assert L.rrin_gate_frames_u8(a, b, frame, n, h0, 0, g, o, st) == -1
    assert L.rrin_gate_frames_u8(a, b, frame - 1, n, h0, w0, g, o, st) == -2
    assert torch.equal(out.cpu(), pattern)


def gate_inputs(dev):
    """f0 / f1 uint8 [4,37,50,3]: two ordinary pairs (a smooth ramp against itself rolled by one
    pixel), a duplicate pair, a cut pair (the ramp against uniform random bytes)."""
    ramp = scene_frames()[0]
    noise = stack_of(1, 37, 50, 8)[0]
    f0 = np.stack([ramp, np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), ramp])
    f1 = np.stack([np.roll(ramp, 1, axis=1), np.roll(ramp, 1, axis=0), np.roll(ramp, 2, axis=1), noise])
    return torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_forward_u8_scene_threshold(gpu, precision):
    net = net_of(gpu, precision)
    f0, f1 = gate_inputs(gpu)
    mean = (f0.long() - f1.long()).abs().reshape(4, -1).float().mean(1).cpu()
    assert max(mean[0], mean[1]) < 10 and mean[2] == 0 and mean[3] > 40, mean   # far from 20 either way
    for t in (0.25, 0.5, 0.75):
        cut = 1 if t < 0.5 else 2
        ref = cv.scene_gate_codes(f0.cpu(), f1.cpu(), 20, t)
        assert ref.tolist() == [0, 0, 1, cut]
        with torch.no_grad():
            plain = net.forward_u8(f0, f1, t)
            off = net.forward_u8(f0, f1, t, scene_threshold=None)
            got = net.forward_u8(f0, f1, t, scene_threshold=20)
            codes = net.last_gate.clone()
        assert torch.equal(off, plain)                                   # gate off: today's bits
        assert torch.equal(got[:2], plain[:2])                           # ungated pairs: untouched
        assert torch.equal(got[2], f0[2])                                # the duplicate
        assert torch.equal(got[3], f0[3] if cut == 1 else f1[3])         # the cut: the nearer input
        assert not torch.equal(plain[2], f0[2]) and not torch.equal(plain[3], got[3])   # the gate did it
        assert codes.dtype == torch.int32 and codes.cpu().tolist() == ref.tolist()
        assert torch.equal(got.cpu(), cv.apply_gate_u8(plain.cpu(), f0.cpu(), f1.cpu(), ref))
    net.check_range()


def test_interpolate_u8_gate_and_pair_stats(gpu):
    net = net_of(gpu, "fp32")
    f0, f1 = gate_inputs(gpu)
    ts = [0.25, 0.5, 0.75]
    with torch.no_grad():
        each = [net.forward_u8(f0, f1, t, scene_threshold=20) for t in ts]
        outs = net.interpolate_u8(f0, f1, ts, scene_threshold=20)
        assert net.last_gate.cpu().tolist() == [0, 0, 1, 2]             # the codes of ts[-1]
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        # explicit codes: the same frames as the threshold that gives them
        for t, want in zip(ts, each):
            g = cv.scene_gate_codes(f0, f1, 20, t)
            assert g.device == f0.device
            assert torch.equal(net.forward_u8(f0, f1, t, gate=g), want)
            assert net.last_gate is g
        gated = net.interpolate_u8(f0, f1, ts, gate=torch.tensor([2, 0, 9, 1], dtype=torch.int32, device=gpu))
        plain = net.interpolate_u8(f0, f1, ts)
        for a, b in zip(gated, plain):
            assert torch.equal(a[0], f1[0]) and torch.equal(a[1:3], b[1:3]) and torch.equal(a[3], f0[3])
        # a changed pair after a gated call: the kept sums are not taken for the new pair's
        h0 = f0.clone()
        h0[0] = f1[0]                                                    # pair 0 becomes a duplicate
        assert torch.equal(net.forward_u8(h0, f1, 0.5, scene_threshold=20)[0], h0[0])
        assert net.last_gate.cpu().tolist() == [1, 0, 1, 2]
        with pytest.raises(ValueError):
            net.forward_u8(f0, f1, 0.5, scene_threshold=20, gate=g)
        with pytest.raises(ValueError):
            net.forward_u8(f0, f1, 0.5, gate=g.long())
        with pytest.raises(ValueError):
            net.forward_u8(f0, f1, 0.5, scene_threshold=300)
        stats = net.pair_stats_u8(f0, f1)
    assert stats.dtype == torch.int64 and stats.device == f0.device
    assert stats.cpu().tolist() == np_sad(f0.cpu().numpy(), f1.cpu().numpy())
    fr = torch.from_numpy(stack_of(4, 37, 50, 9)).to(gpu)
    with torch.no_grad():
        assert net.pair_stats_u8(fr[:-1], fr[1:]).cpu().tolist() == np_sad(fr[:-1].cpu().numpy(), fr[1:].cpu().numpy())


def test_folder_run_gates_on_gpu(tmp_path, gpu):
    """Six 37x50 PNGs with one repeated frame and one cut, sf = 3, batch = 2."""
    frames = scene_frames()
    src = str(tmp_path / "in")
    write_frames(src, frames)
    net = net_of(gpu, "fp32")
    sf, logs = 3, []
    a, b = str(tmp_path / "gated"), str(tmp_path / "plain")
    na = cv.interpolate_folder(net, src, a, sf=sf, batch=2, device=gpu, scene_threshold=20, log=logs.append)
    nb = cv.interpolate_folder(net, src, b, sf=sf, batch=2, device=gpu, log=lambda *x: None)
    assert na == nb == 1 + 5 * (sf + 1) and sorted(os.listdir(a)) == sorted(os.listdir(b))
    assert logs[-1].endswith("1 cut pairs, 1 duplicate pairs"), logs
    for k in range(5):
        base = 1 + k * (sf + 1)
        for i in range(sf):
            name = f"{base + i + 1:09d}.png"
            if k == 1:
                np.testing.assert_array_equal(read(os.path.join(a, name)), frames[1])
            elif k == 3:
                want = frames[3] if (i + 1) / (sf + 1) < 0.5 else frames[4]
                np.testing.assert_array_equal(read(os.path.join(a, name)), want)
            else:
                assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
        name = f"{base + sf + 1:09d}.png"
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


def uneven_inputs(dev):
    """f0 / f1 uint8 [3,30,44,3] (the net runs at 32x48: both paddings are non-zero): an ordinary pair (a
    smooth ramp against itself rolled by one pixel), a duplicate pair, a cut pair (the ramp against noise)."""
    yy, xx = np.mgrid[0:30, 0:44]
    ramp = np.stack([60 + yy + 2 * xx, 40 + 2 * yy + xx, 80 + yy + xx], axis=-1).astype(np.uint8)
    moved = np.roll(ramp, 2, axis=0)
    f0 = np.stack([ramp, moved, ramp])
    f1 = np.stack([np.roll(ramp, 1, axis=1), moved, stack_of(1, 30, 44, 8)[0]])
    return torch.from_numpy(f0).to(dev), torch.from_numpy(f1).to(dev)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_uneven_split_equals_one_stream(gpu, precision):
    """split=[1, 2] against streams=1, byte for byte in the frames and in last_gate: every part slices the
    coefficient rows, the sums, the codes and the output by [lo:hi], and the other tests split evenly or
    not at all.  Then reuse_flow=True at another t against a fresh call at that t.

    The scene gate takes one t for the batch (scene_cut_code raises for a per-pair tensor), so the
    per-pair t = (0.25, 0.5, 0.75) cannot go with scene_threshold.  Two legs cover the slices between
    them: scene_threshold with a scalar t (the sums and the codes derived from them), and the per-pair t
    with the same codes given as ``gate`` (the coefficient rows)."""
    eng = net_of(gpu, precision).engine()
    f0, f1 = uneven_inputs(gpu)
    for t, want in ((0.75, [0, 1, 2]), (0.25, [0, 1, 1])):
        assert cv.scene_gate_codes(f0.cpu(), f1.cpu(), 20, t).tolist() == want
    with torch.no_grad():
        one = eng.forward_u8(f0, f1, 0.75, streams=1, scene_threshold=20)
        codes1 = eng.last_gate.clone()
        two = eng.forward_u8(f0, f1, 0.75, split=[1, 2], scene_threshold=20)
        assert torch.equal(two, one) and torch.equal(eng.last_gate, codes1)
        assert codes1.cpu().tolist() == [0, 1, 2]
        assert torch.equal(two[1], f0[1]) and torch.equal(two[2], f1[2]) and not torch.equal(two[0], f0[0])
        again = eng.forward_u8(f0, f1, 0.25, split=[1, 2], reuse_flow=True, scene_threshold=20)   # kept Flow and sums
        codes2 = eng.last_gate.clone()
        fresh = eng.forward_u8(f0, f1, 0.25, streams=1, scene_threshold=20)
        assert torch.equal(again, fresh) and torch.equal(codes2, eng.last_gate)
        assert codes2.cpu().tolist() == [0, 1, 1] and torch.equal(again[2], f0[2])
        # the per-pair t, each pair's code by the rule at its own t
        t = torch.tensor([0.25, 0.5, 0.75])
        g = torch.cat([cv.scene_gate_codes(f0[p:p + 1], f1[p:p + 1], 20, float(t[p])) for p in range(3)])
        assert g.cpu().tolist() == [0, 1, 2]
        one = eng.forward_u8(f0, f1, t, streams=1, gate=g)
        two = eng.forward_u8(f0, f1, t, split=[1, 2], gate=g)
        assert torch.equal(two, one) and eng.last_gate is g
        again = eng.forward_u8(f0, f1, t.flip(0), split=[1, 2], reuse_flow=True, gate=g)
        assert torch.equal(again, eng.forward_u8(f0, f1, t.flip(0), streams=1, gate=g))
        assert not torch.equal(again[0], two[0])                         # another t: another frame
    eng.check_range()
