"""CPU: the host definitions of the 16-bit frame paths -- yuv.coefficients(depth=), yuv420_to_rgb16 /
rgb16_to_yuv420, convert.frames_u16_to_float / frames_float_to_u16 -- and the 10- / 12-bit Y4M streams.
These functions are the oracle of tests/test_gpu_u16.py and tests/test_gpu_yuv16.py."""
import io
import os

import numpy as np
import pytest
import torch

from rrin_amd import _lib, y4m, yuv
from rrin_amd import convert as cv

STANDARDS = [(s, fr) for s in ("bt709", "bt601") for fr in (False, True)]
# rrin_yuv_coef_std's table (csrc/yuv.hip): what coefficients() returned before it took a depth
TODAY = {
    ("bt709", False): (16, 19077, 29372, -3494, -8731, 34610, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660),
    ("bt709", True): (0, 16384, 25802, -3069, -7670, 30402, 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751),
    ("bt601", False): (16, 19077, 26149, -6419, -13320, 33050, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026,
                       -1170),
    ("bt601", True): (0, 16384, 22970, -5638, -11700, 29032, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332),
}


def words(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16))


def ints(t):
    return yuv.words_to_int(t)


def rand_frames(n, h0, w0, depth, seed, msb=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << depth, (n, 3 * h0 // 2, w0), dtype=np.uint16)
    return words(a << (16 - depth) if msb else a)


@pytest.mark.parametrize("standard,full", STANDARDS)
def test_depth_8_coefficients_are_todays(standard, full):
    assert tuple(yuv.coefficients(standard, full, depth=8)) == TODAY[(standard, full)]
    assert tuple(yuv.coefficients(standard, full)) == TODAY[(standard, full)]
    assert yuv.as_coef(None) == yuv.coefficients() and yuv.as_coef(TODAY[("bt601", True)]) == TODAY[("bt601", True)]


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("standard,full", STANDARDS)
def test_deep_coefficients(standard, full, depth):
    k = yuv.coefficients(standard, full, depth)
    maxval, mid = (1 << depth) - 1, 1 << (depth - 1)
    assert k.y0 == (0 if full else 16 << (depth - 8))
    ys = 1.0 if full else 219.0 * (1 << (depth - 8)) / maxval
    assert k.yr + k.yg + k.yb == round(ys * 2 ** 14)
    assert k.ur + k.ug + k.ub == 0 and k.vr + k.vg + k.vb == 0
    assert yuv.as_coef(k, depth) == k
    # grey (R = G = B) maps to U = V = mid exactly, at every level
    g = torch.arange(0, maxval + 1, dtype=torch.int32)[: (maxval + 1) // 4 * 4].reshape(1, -1, 2, 1)
    rgb = yuv.int_to_words(g.expand(1, -1, 2, 3).contiguous())
    _, u, v = yuv.split_planes(yuv.rgb16_to_yuv420(rgb, "i420", k, depth), "i420")
    # a 2x2 block holds levels 4i .. 4i+3 in pairs of rows: U, V stay mid whatever the block's sum
    assert (ints(u) == mid).all() and (ints(v) == mid).all()
    # the library's host table holds the same numbers
    c = _lib.YuvCoef()
    std = _lib.YUV_BT709 if standard == "bt709" else _lib.YUV_BT601
    assert _lib.lib().rrin_yuv_coef_std16(std, int(full), depth, c) == 0
    assert tuple(getattr(c, f) for f in yuv.Coef._fields) == tuple(k)


def test_library_table_at_every_depth():
    L = _lib.lib()
    for depth in range(8, 17):
        for standard, full in STANDARDS:
            c = _lib.YuvCoef()
            assert L.rrin_yuv_coef_std16(_lib.YUV_BT709 if standard == "bt709" else _lib.YUV_BT601, int(full), depth, c) == 0
            assert tuple(getattr(c, f) for f in yuv.Coef._fields) == tuple(yuv.coefficients(standard, full, depth))
    assert L.rrin_yuv_coef_std16(0, 0, 7, _lib.YuvCoef()) == -2 and L.rrin_yuv_coef_std16(2, 0, 10, _lib.YuvCoef()) == -2


@pytest.mark.parametrize("layout", yuv.LAYOUTS)
def test_depth_8_reproduces_the_8_bit_functions(layout):
    """The formulas at depth 8 with the samples in the low bits, on the same values."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (2, 27, 22), dtype=np.uint8)
    a.reshape(2, -1)[:, :256] = np.arange(256, dtype=np.uint8)
    f8, f16 = torch.from_numpy(a), words(a)
    for coef in (None, yuv.coefficients("bt601", True)):
        r8 = yuv.yuv420_to_rgb(f8, layout, coef)
        r16 = yuv._to_rgb_words(f16, layout, coef, 8, False)
        assert r16.dtype == torch.uint16 and torch.equal(ints(r16), r8.to(torch.int32))
        back = yuv._to_yuv_words(r16, layout, coef, 8, False)
        assert torch.equal(ints(back), yuv.rgb_to_yuv420(r8, layout, coef).to(torch.int32))


@pytest.mark.parametrize("depth", [10, 12])
def test_round_trip_deviation(depth):
    """rgb16_to_yuv420(yuv420_to_rgb16(x)) on frames whose 2x2 blocks are flat and inside the legal
    range (so that neither the chroma mean nor a clip loses anything).  Recorded maximum deviation: 0 code
    values at depth 10 and 12, both layouts and alignments, BT.709 limited and BT.601 full.  The bound
    asserted is 1: each direction rounds to the nearest code value once (half a code value each), and the
    Q14 rounding of the coefficients moves a sum by less than 3 * 2**-15 of full scale."""
    up = 1 << (depth - 8)
    rng = np.random.default_rng(5)
    y = rng.integers(64 * up, 192 * up, (2, 8, 12))
    y = np.repeat(np.repeat(y, 2, 1), 2, 2)
    u = rng.integers(120 * up, 136 * up, (2, 8, 12))
    v = rng.integers(120 * up, 136 * up, (2, 8, 12))
    for coef in (None, yuv.coefficients("bt601", True, depth)):
        for layout in yuv.LAYOUTS:
            for msb in (False, True):
                x = yuv.join_planes(words(y), words(u), words(v), layout)
                if msb:
                    x = yuv.int_to_words(ints(x) << (16 - depth))
                back = yuv.rgb16_to_yuv420(yuv.yuv420_to_rgb16(x, layout, coef, depth, msb), layout, coef, depth, msb)
                sh = 16 - depth if msb else 0
                dev = ((ints(back) >> sh) - (ints(x) >> sh)).abs().max().item()
                print(f"depth {depth} {layout} msb={msb} coef={'default' if coef is None else 'bt601 full'}: max dev {dev}")
                assert dev <= 1


def test_clamp_msb_and_refused_depths():
    depth, maxval = 10, 1023
    a = np.array([[[0, 1023, 1024, 65535], [512, 700, 2047, 4096], [512, 512, 1024, 65535]]], dtype=np.uint16)
    over, clamped = words(a), words(np.minimum(a, maxval))
    for layout in yuv.LAYOUTS:
        assert torch.equal(yuv.yuv420_to_rgb16(over, layout, None, depth), yuv.yuv420_to_rgb16(clamped, layout, None, depth))
    # msb: word >> 6 in (dirty low bits dropped), sample << 6 out
    rng = np.random.default_rng(7)
    low = rand_frames(2, 6, 8, depth, 7)
    dirty = yuv.int_to_words((ints(low) << 6) | torch.from_numpy(rng.integers(0, 64, tuple(low.shape))).to(torch.int32))
    rgb = yuv.yuv420_to_rgb16(low, "nv12", None, depth, False)
    assert torch.equal(yuv.yuv420_to_rgb16(dirty, "nv12", None, depth, True), rgb)
    out_low, out_msb = yuv.rgb16_to_yuv420(rgb, "nv12", None, depth, False), yuv.rgb16_to_yuv420(rgb, "nv12", None, depth, True)
    assert torch.equal(ints(out_msb), ints(out_low) << 6)
    # RGB samples above maxval are read as maxval on the way out
    assert torch.equal(yuv.rgb16_to_yuv420(words(np.full((1, 2, 2, 3), 60000)), "i420", None, depth),
                       yuv.rgb16_to_yuv420(words(np.full((1, 2, 2, 3), maxval)), "i420", None, depth))
    for bad in (8, 9, 11, 14, 16, 10.0, None):
        with pytest.raises(ValueError):
            yuv.yuv420_to_rgb16(low, "nv12", None, bad)
        with pytest.raises(ValueError):
            yuv.rgb16_to_yuv420(rgb, "nv12", None, bad)
    with pytest.raises(TypeError):
        yuv.yuv420_to_rgb16(low.view(torch.int16), "nv12", None, 10)
    with pytest.raises(TypeError):
        yuv.rgb16_to_yuv420(rgb.view(torch.int16), "nv12", None, 10)
    # coefficient bounds of the deep variant; the 8-bit call keeps its own
    k = list(yuv.coefficients(depth=10))
    assert yuv.as_coef(k[:0] + [1023] + k[1:], 10).y0 == 1023
    for i, v in ((0, 1024), (0, -1), (1, 1 << 16), (6, 1 << 15), (14, -(1 << 15))):
        with pytest.raises(ValueError):
            yuv.as_coef(k[:i] + [v] + k[i + 1:], 10)
    assert yuv.as_coef(k[:6] + [(1 << 16) - 1] + k[7:]).yr == (1 << 16) - 1          # 8-bit bounds as today
    with pytest.raises(ValueError):
        yuv.as_coef([256] + k[1:])


def test_int32_safety_at_depth_12():
    """The worst-case intermediates from the coefficient bounds (as_coef at depth 12), in Python
    integers: every one inside int32."""
    maxval, mid = 4095, 2048
    cin, cout = yuv.IN_BOUND - 1, yuv.OUT_BOUND16 - 1
    lim = 2 ** 31 - 1
    to_rgb = cin * maxval + 8192 + 2 * cin * mid                  # |ay*(Y-y0)| + 8192 + |gu*d| + |gv*e|
    luma = 3 * cout * maxval + 8192
    chroma = 3 * cout * 4 * maxval + 32768                          # a block's sums are four samples each
    assert to_rgb <= lim and luma <= lim and chroma <= lim
    assert 3 * (yuv.IN_BOUND - 1) * 4 * maxval + 32768 > lim        # why the out bound is 2**15, not 2**16
    assert 3 * cin * (1 << 16) > lim                                # and why 16-bit YUV is refused
    assert max(abs(v) for v in yuv.coefficients("bt601", False, 12)[6:]) < yuv.OUT_BOUND16
    # the extreme frames evaluate without wrapping: compare int32 torch with Python integers
    k = yuv.Coef(maxval, cin, cin, -cin, -cin, cin, cout, cout, cout, cout, cout, cout, -cout, -cout, -cout)
    rgb = words(np.full((1, 2, 2, 3), maxval))
    out = ints(yuv.rgb16_to_yuv420(rgb, "i420", k, 12))
    assert out[0, 0, 0].item() == min(maxval, maxval + ((3 * cout * maxval + 8192) >> 14))
    assert out[0, 2, 0].item() == min(maxval, mid + ((chroma) >> 16)) and out[0, 2, 1].item() == 0


@pytest.mark.parametrize("depth", [9, 10, 12, 16])
def test_frames_u16_float_mappings(depth):
    maxval = (1 << depth) - 1
    rng = np.random.default_rng(depth)
    a = rng.integers(0, 65536, (2, 18, 34, 3), dtype=np.uint16)
    a.reshape(-1)[: 4] = (0, maxval, min(maxval + 1, 65535), 65535)
    t = cv.frames_u16_to_float(words(a), depth)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3, 32, 48)
    # float64 model: the correctly rounded fp32 quotient, edge-padded 14 rows on top and 14 columns right
    s = np.minimum(a, maxval).astype(np.float64)
    s = np.pad(s, ((0, 0), (14, 0), (0, 14), (0, 0)), mode="edge").transpose(0, 3, 1, 2)
    assert np.array_equal(t.numpy(), (s / maxval).astype(np.float32))
    assert t.max().item() == 1.0
    # and back: crop, one fp32 multiply, truncation; q = 1.0 -> maxval
    q = torch.from_numpy(rng.random((2, 3, 32, 48), dtype=np.float32))
    q.view(-1)[:3] = torch.tensor([0.0, 1.0, 0.5])
    q[0, 0, 14, 0], q[0, 1, 31, 33] = 1.0, 1.0
    back = cv.frames_float_to_u16(q, 18, 34, depth)
    assert back.dtype == torch.uint16 and tuple(back.shape) == (2, 18, 34, 3)
    model = np.trunc((q.numpy() * np.float32(maxval)).astype(np.float64))[:, :, 14:, :34].transpose(0, 2, 3, 1)
    assert np.array_equal(back.numpy().astype(np.float64), model)
    assert back[0, 0, 0, 0].item() == maxval and back[0, 17, 33, 1].item() == maxval
    # exact samples survive the round trip
    exact = cv.frames_float_to_u16(cv.frames_u16_to_float(words(np.minimum(a, maxval)), depth), 18, 34, depth)
    assert (ints(exact) - torch.from_numpy(np.minimum(a, maxval).astype(np.int32))).abs().max().item() <= 1
    for bad in (8, 17, 10.0):
        with pytest.raises(ValueError):
            cv.frames_u16_to_float(words(a), bad)
        with pytest.raises(ValueError):
            cv.frames_float_to_u16(q, 18, 34, bad)
    with pytest.raises(TypeError):
        cv.frames_u16_to_float(torch.zeros(1, 2, 2, 3, dtype=torch.uint8), depth)


def test_scene_limit_takes_a_maxval():
    assert cv.scene_limit(20, 4, 5) == 1200 and cv.scene_limit(1023, 2, 2, 1023) == 1023 * 12
    with pytest.raises(ValueError):
        cv.scene_limit(256, 4, 5)
    with pytest.raises(ValueError):
        cv.scene_limit(1024, 4, 5, 1023)


@pytest.mark.parametrize("depth", [10, 12])
def test_y4m_deep_streams_round_trip_through_a_pipe(depth):
    w0, h0 = 6, 4
    fr = rand_frames(3, h0, w0, depth, 11).numpy()
    r, w = os.pipe()
    with os.fdopen(w, "wb") as fo:
        wr = y4m.Writer(fo, w0, h0, 24, 1, f"420p{depth}", depths=(8, 10, 12))
        assert wr.bit_depth == depth and wr.frame_bytes == w0 * h0 * 3
        for f in fr:
            wr.write(f)
        wr.flush()
    with os.fdopen(r, "rb") as fi:
        raw = fi.read()
    assert raw.startswith(b"YUV4MPEG2 W6 H4 F24:1 Ip C420p%d\n" % depth)
    assert raw[-2:] == int(fr[-1].reshape(-1)[-1]).to_bytes(2, "little")          # little-endian words
    rd = y4m.Reader(io.BytesIO(raw), depths=(8, 10, 12))
    assert (rd.bit_depth, rd.frame_bytes, rd.colorspace) == (depth, w0 * h0 * 3, f"420p{depth}")
    got = list(rd)
    assert len(got) == 3 and all(g.dtype == np.uint16 and np.array_equal(g, f.reshape(-1)) for g, f in zip(got, fr))
    # the default Reader and Writer still refuse them; so does a reader that asked for the other depth
    with pytest.raises(ValueError, match="only 8-bit 4:2:0"):
        y4m.Reader(io.BytesIO(raw))
    with pytest.raises(ValueError, match="only 8-bit 4:2:0"):
        y4m.Writer(io.BytesIO(), w0, h0, 24, 1, f"420p{depth}")
    with pytest.raises(ValueError):
        y4m.Reader(io.BytesIO(raw), depths=(8, 22 - depth))
    # a truncated 16-bit frame raises, also when it ends inside a word
    for cut in (1, 2, w0 * h0 * 3 - 1):
        with pytest.raises(ValueError, match="truncated"):
            list(y4m.Reader(io.BytesIO(raw[:-cut]), depths=(8, 10, 12)))
    with pytest.raises(ValueError, match="a frame is"):
        y4m.Writer(io.BytesIO(), w0, h0, 24, 1, f"420p{depth}", depths=(10, 12)).write(fr[0][:-1])
    # an 8-bit stream through a reader that takes all three depths is what it was
    buf = io.BytesIO()
    y4m.Writer(buf, w0, h0, 24, 1, "420jpeg", depths=(8, 10, 12)).write(np.arange(36, dtype=np.uint8))
    rd = y4m.Reader(io.BytesIO(buf.getvalue()), depths=(8, 10, 12))
    assert rd.bit_depth == 8 and rd.frame_bytes == 36 and next(rd).dtype == np.uint8
