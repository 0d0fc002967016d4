"""CPU: the host side of the YUV 4:2:0 frame path -- the coefficient sets (rrin_amd.yuv against the
table of the standards and against rrin_yuv_coef_std), the two integer conversions that define
Net.forward_yuv, the argument validation of rrin_net_yuv_fwd / rrin_pack_g16_yuv_h8 (nothing is
launched) and the Y4M reader / writer."""
import ctypes as C
import io
import os
import threading

import numpy as np
import pytest
import torch

from rrin_amd import _lib, y4m, yuv

FAKE = 1 << 30  # a fabricated non-null device pointer: never dereferenced

# y0 ay rv gu gv bu | yr yg yb ur ug ub vr vg vb: round(x * 2^14) of the Kr / Kb matrices
TABLE = {
    ("bt709", False): (16, 19077, 29372, -3494, -8731, 34610, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660),
    ("bt709", True): (0, 16384, 25802, -3069, -7670, 30402, 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751),
    ("bt601", False): (16, 19077, 26149, -6419, -13320, 33050, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026,
                       -1170),
    ("bt601", True): (0, 16384, 22970, -5638, -11700, 29032, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332),
}
SETS = sorted(TABLE)


@pytest.mark.parametrize("std,full", SETS)
def test_coefficient_sets(std, full):
    k = yuv.coefficients(std, full)
    assert tuple(k) == TABLE[(std, full)]
    c = _lib.YuvCoef()
    assert _lib.lib().rrin_yuv_coef_std(_lib.YUV_BT709 if std == "bt709" else _lib.YUV_BT601, int(full), C.byref(c)) == 0
    assert tuple(getattr(c, f) for f in k._fields) == tuple(k)
    # the remainders: luma weights sum to round(2^14 * luma scale), chroma weights to 0
    assert k.yr + k.yg + k.yb == round(16384 * (1.0 if full else 219 / 255))
    assert k.ur + k.ug + k.ub == 0 and k.vr + k.vg + k.vb == 0


def test_coefficient_defaults_and_errors():
    assert yuv.coefficients() == yuv.coefficients("bt709", False) == yuv.as_coef(None)
    assert yuv.as_coef(list(TABLE[("bt601", True)])) == yuv.coefficients("bt601", True)
    with pytest.raises(ValueError):
        yuv.coefficients("bt2020")
    with pytest.raises(ValueError):
        yuv.as_coef((16,) + (65536,) * 14)
    with pytest.raises(TypeError):
        yuv.as_coef((1, 2, 3))
    c = _lib.YuvCoef()
    assert _lib.lib().rrin_yuv_coef_std(2, 0, C.byref(c)) == -2
    assert _lib.lib().rrin_yuv_coef_std(0, 0, None) == -2


@pytest.mark.parametrize("std,full", SETS)
def test_grey_maps_to_neutral_chroma(std, full):
    k = yuv.coefficients(std, full)
    levels = torch.arange(256, dtype=torch.uint8)
    rgb = levels.view(256, 1, 1, 1).expand(256, 2, 2, 3).contiguous()
    for layout in yuv.LAYOUTS:
        y, u, v = yuv.split_planes(yuv.rgb_to_yuv420(rgb, layout, k), layout)
        assert (u == 128).all() and (v == 128).all()
        assert (y[:, 0, 0].int().diff() >= 0).all()
        if not full:
            assert int(y.min()) == 16 and int(y.max()) == 235
        else:
            assert torch.equal(y[:, 0, 0], levels)


@pytest.mark.parametrize("std", ["bt709", "bt601"])
def test_limited_range_keeps_the_primaries_inside(std):
    k = yuv.coefficients(std, False)
    cols = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]   # black, white, primaries, secondaries
    rgb = torch.tensor(cols, dtype=torch.uint8).view(8, 1, 1, 3).expand(8, 2, 2, 3).contiguous()
    y, u, v = yuv.split_planes(yuv.rgb_to_yuv420(rgb, "i420", k), "i420")
    assert 16 <= int(y.min()) and int(y.max()) <= 235
    for c in (u, v):
        assert 16 <= int(c.min()) and int(c.max()) <= 240
    assert int(u.max()) == 240 and int(v.max()) == 240 and int(u.min()) == 16 and int(v.min()) == 16  # blue, red; yellow, cyan


def test_yuv_to_rgb_exhaustive_against_the_float_matrix():
    """All 2^24 (Y, U, V) triples, BT.709 limited: within 1 LSB of clip(floor(x + 0.5)) of the float64
    matrix of the standard.  A frame per V: block row = U, the 256 pixels of a block row = Y."""
    k = yuv.coefficients("bt709", False)
    kr, kb = 0.2126, 0.0722
    kg = 1 - kr - kb
    yy = torch.empty((512, 128), dtype=torch.uint8)
    c = torch.arange(64).view(1, 64)
    for dy in range(2):
        for dx in range(2):
            yy[dy::2, dx::2] = (4 * c + 2 * dy + dx).to(torch.uint8).expand(256, 64)
    uu = torch.arange(256, dtype=torch.uint8).view(256, 1).expand(256, 64)
    yf = (yy.double() - 16) * (255 / 219)
    d = (uu.double() - 128).repeat_interleave(2, 0).repeat_interleave(2, 1) * (255 / 224)
    worst = 0
    for v0 in range(0, 256, 32):
        n = 32
        vs = torch.arange(v0, v0 + n, dtype=torch.uint8)
        frames = yuv.join_planes(yy.expand(n, 512, 128), uu.expand(n, 256, 64), vs.view(n, 1, 1).expand(n, 256, 64), "nv12")
        got = yuv.yuv420_to_rgb(frames, "nv12", k).int()
        e = (vs.double() - 128).view(n, 1, 1) * (255 / 224)
        want = torch.stack((yf + 2 * (1 - kr) * e,
                            yf - 2 * (1 - kb) * kb / kg * d - 2 * (1 - kr) * kr / kg * e,
                            yf + 2 * (1 - kb) * d + 0 * e), dim=3)
        want = torch.floor(want + 0.5).clamp_(0, 255).int()
        worst = max(worst, int((got - want).abs().max()))
    assert worst <= 1, worst


def random_planes(n, h0, w0, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, h0, w0), dtype=torch.uint8, generator=g),
            torch.randint(0, 256, (n, h0 // 2, w0 // 2), dtype=torch.uint8, generator=g),
            torch.randint(0, 256, (n, h0 // 2, w0 // 2), dtype=torch.uint8, generator=g))


def test_layouts_hold_the_same_planes():
    y, u, v = random_planes(2, 6, 10, 1)
    nv12, i420 = yuv.join_planes(y, u, v, "nv12"), yuv.join_planes(y, u, v, "i420")
    assert tuple(nv12.shape) == tuple(i420.shape) == (2, 9, 10) and not torch.equal(nv12, i420)
    # the byte layouts, spelled out
    assert torch.equal(nv12[:, 6:].reshape(2, -1)[:, 0::2], u.reshape(2, -1))
    assert torch.equal(nv12[:, 6:].reshape(2, -1)[:, 1::2], v.reshape(2, -1))
    assert torch.equal(i420[:, 6:].reshape(2, -1), torch.cat((u.reshape(2, -1), v.reshape(2, -1)), 1))
    for a, b in zip(yuv.split_planes(nv12, "nv12"), (y, u, v)):
        assert torch.equal(a, b)
    for a, b in zip(yuv.split_planes(i420, "i420"), (y, u, v)):
        assert torch.equal(a, b)
    for k in (None, yuv.coefficients("bt601", True)):
        rgb = yuv.yuv420_to_rgb(nv12, "nv12", k)
        assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (2, 6, 10, 3)
        assert torch.equal(rgb, yuv.yuv420_to_rgb(i420, "i420", k))
        # chroma is replicated over its 2x2 block: a pixel's RGB depends on its own luma only within a block
        back_nv12, back_i420 = yuv.rgb_to_yuv420(rgb, "nv12", k), yuv.rgb_to_yuv420(rgb, "i420", k)
        for a, b in zip(yuv.split_planes(back_nv12, "nv12"), yuv.split_planes(back_i420, "i420")):
            assert torch.equal(a, b)


def test_rgb_to_yuv_is_the_written_formula():
    """One block by hand, in Python integers (>> on a negative int is floor there too)."""
    k = yuv.coefficients("bt601", False)
    g = torch.Generator().manual_seed(3)
    rgb = torch.randint(0, 256, (1, 2, 2, 3), dtype=torch.uint8, generator=g)
    y, u, v = yuv.split_planes(yuv.rgb_to_yuv420(rgb, "i420", k), "i420")
    px = [tuple(int(c) for c in rgb[0, a, b]) for a in range(2) for b in range(2)]
    clip = lambda x: min(max(x, 0), 255)  # noqa: E731
    assert y.reshape(-1).tolist() == [clip(k.y0 + ((k.yr * r + k.yg * gg + k.yb * b + 8192) >> 14)) for r, gg, b in px]
    rs, gs, bs = (sum(p[i] for p in px) for i in range(3))
    assert int(u) == clip(128 + ((k.ur * rs + k.ug * gs + k.ub * bs + 32768) >> 16))
    assert int(v) == clip(128 + ((k.vr * rs + k.vg * gs + k.vb * bs + 32768) >> 16))


def test_bad_sizes_and_types_raise():
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(torch.zeros((1, 3, 4, 3), dtype=torch.uint8))        # odd H0
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(torch.zeros((1, 4, 3, 3), dtype=torch.uint8))        # odd W0
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros((1, 4, 4), dtype=torch.uint8))           # 4 rows are not 3*H0/2
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros((1, 3, 3), dtype=torch.uint8))           # odd W0
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros((6, 4), dtype=torch.uint8))              # no frame axis
    with pytest.raises(TypeError):
        yuv.yuv420_to_rgb(torch.zeros((1, 3, 2), dtype=torch.int32))
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(torch.zeros((1, 3, 2), dtype=torch.uint8), "yv12")


# ---- C ABI: validation before any HIP call ------------------------------------------------
def _stack(h0, w0, layout="nv12", y=FAKE, y_pitch=None, c_pitch=None, c_step=None, stride=None):
    s = _lib.Yuv420()
    s.y, s.u = y, FAKE + h0 * w0
    s.v = s.u + (1 if layout == "nv12" else h0 * w0 // 4)
    s.img_stride = h0 * w0 * 3 // 2 if stride is None else stride
    s.y_pitch = w0 if y_pitch is None else y_pitch
    s.c_pitch = (w0 if layout == "nv12" else w0 // 2) if c_pitch is None else c_pitch
    s.c_step = (2 if layout == "nv12" else 1) if c_step is None else c_step
    return s


def _yuv_desc(h0, w0, h, w, n=2, prec=_lib.PREC_F32R, **kw):
    d = _lib.NetYuvDesc()
    d.net.n, d.net.h, d.net.w, d.net.prec = n, h, w, prec
    d.net.coef = d.net.workspace = FAKE
    d.net.workspace_bytes = 1 << 40
    d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))
    d.f0, d.f1, d.out = _stack(h0, w0, **kw), _stack(h0, w0), _stack(h0, w0)
    d.coef = _lib.YuvCoef(*yuv.coefficients())
    d.h0, d.w0 = h0, w0
    return d


def test_net_yuv_fwd_validates_before_any_launch():
    fwd = _lib.lib().rrin_net_yuv_fwd
    E_SHAPE, E_ARG = -1, -2
    assert fwd(C.byref(_yuv_desc(38, 50, 32, 64)), None) == E_SHAPE          # h != round_up(h0, 16)
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 48)), None) == E_SHAPE          # w != round_up(w0, 16)
    assert fwd(C.byref(_yuv_desc(37, 50, 48, 64)), None) == E_SHAPE          # odd h0
    assert fwd(C.byref(_yuv_desc(38, 49, 48, 64)), None) == E_SHAPE          # odd w0
    assert fwd(C.byref(_yuv_desc(0, 50, 16, 64)), None) == E_SHAPE
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, y_pitch=49)), None) == E_SHAPE
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, c_pitch=49)), None) == E_SHAPE   # NV12 rows are w0 bytes
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, layout="i420", c_pitch=24)), None) == E_SHAPE
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, stride=38 * 50 - 1)), None) == E_SHAPE   # frames overlap
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, c_step=3)), None) == E_ARG
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, c_step=0)), None) == E_ARG
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, y=None)), None) == E_ARG
    assert fwd(C.byref(_yuv_desc(38, 50, 48, 64, prec=_lib.PREC_F32)), None) == E_ARG  # planar: no byte path
    bad = _yuv_desc(38, 50, 48, 64)
    bad.out.v = None
    assert fwd(C.byref(bad), None) == E_ARG
    bad = _yuv_desc(38, 50, 48, 64)
    bad.coef.bu = 1 << 16
    assert fwd(C.byref(bad), None) == E_ARG
    assert fwd(None, None) == E_ARG


def test_pack_yuv_validates_before_any_launch():
    pack = _lib.lib().rrin_pack_g16_yuv_h8
    g = _lib.Geom()
    _lib.check(_lib.lib().rrin_make_geom_h8(48, 64, C.byref(g)))
    v = _lib.H8(FAKE, None, 4 * g.plane, 0, 4, g)
    k = _lib.YuvCoef(*yuv.coefficients())
    ok, odd = _stack(38, 50), _stack(37, 50)
    assert pack(C.byref(odd), C.byref(odd), C.byref(k), 1, 37, 50, C.byref(v), _lib.PREC_F32R, None) == -1
    assert pack(C.byref(ok), C.byref(ok), C.byref(k), 1, 22, 50, C.byref(v), _lib.PREC_F32R, None) == -1   # g16 is 48 rows
    assert pack(C.byref(ok), C.byref(ok), None, 1, 38, 50, C.byref(v), _lib.PREC_F32R, None) == -2
    assert pack(None, C.byref(ok), C.byref(k), 1, 38, 50, C.byref(v), _lib.PREC_F32R, None) == -2
    assert pack(C.byref(ok), C.byref(_stack(38, 50, c_step=4)), C.byref(k), 1, 38, 50, C.byref(v), _lib.PREC_F32R,
                None) == -2


# ---- Y4M ----------------------------------------------------------------------------------
def y4m_frames(n, w, h, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for _ in range(n)]


def test_y4m_round_trip_through_bytesio():
    frames = y4m_frames(3, 6, 4)
    buf = io.BytesIO()
    wr = y4m.Writer(buf, 6, 4, 30000, 1001)
    for f in frames:
        wr.write(f)
    raw = buf.getvalue()
    assert raw.startswith(b"YUV4MPEG2 W6 H4 F30000:1001 Ip C420\nFRAME\n")
    assert len(raw) == len(b"YUV4MPEG2 W6 H4 F30000:1001 Ip C420\n") + 3 * (6 + 36)
    rd = y4m.Reader(io.BytesIO(raw))
    assert (rd.width, rd.height, rd.fps_num, rd.fps_den, rd.colorspace) == (6, 4, 30000, 1001, "420")
    got = list(rd)
    assert len(got) == 3 and all(g.dtype == np.uint8 and np.array_equal(g, f) for g, f in zip(got, frames))
    # written again: the same bytes
    again = io.BytesIO()
    wr = y4m.Writer(again, rd.width, rd.height, rd.fps_num, rd.fps_den)
    for g in got:
        wr.write(g)
    assert again.getvalue() == raw


def test_y4m_round_trip_through_a_pipe():
    """A pipe cannot seek or tell, and hands out short reads: 64x48 frames exceed one pipe read."""
    frames = y4m_frames(4, 64, 48, seed=6)
    r, w = os.pipe()

    def produce():
        with os.fdopen(w, "wb") as f:
            wr = y4m.Writer(f, 64, 48, 25, 1, "420mpeg2")
            for fr in frames:
                wr.write(fr)

    th = threading.Thread(target=produce)
    th.start()
    with os.fdopen(r, "rb", buffering=0) as f:       # unbuffered: the raw pipe's short reads
        assert not f.seekable()
        rd = y4m.Reader(f)
        got = list(rd)
    th.join()
    assert (rd.width, rd.height, rd.fps_num, rd.fps_den, rd.colorspace) == (64, 48, 25, 1, "420mpeg2")
    assert len(got) == 4 and all(np.array_equal(g, f) for g, f in zip(got, frames))


def test_y4m_headers():
    body = b"FRAME\n" + bytes(6)
    rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1\n" + body))                     # no C tag: 4:2:0
    assert rd.colorspace == "420" and len(list(rd)) == 1
    for tag in (b"C420jpeg", b"C420paldv", b"C420mpeg2", b"C420"):
        rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 Ip A1:1 " + tag + b" XYSCSS=420JPEG\n" + body))
        assert len(list(rd)) == 1
    rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1\nFRAME Ip\n" + bytes(6)))       # frame parameters
    assert len(list(rd)) == 1
    for tag in ("C444", "C420p10", "Ib", "It", "C422", "Cmono"):
        with pytest.raises(ValueError, match=tag):
            y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 " + tag.encode() + b"\n" + body))
    with pytest.raises(ValueError):
        y4m.Reader(io.BytesIO(b"RIFF W2 H2\n"))
    with pytest.raises(ValueError):
        y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 F24:1\n"))                                  # no H
    with pytest.raises(ValueError):
        y4m.Reader(io.BytesIO(b"YUV4MPEG2 W3 H2 F24:1\n"))                               # odd W
    with pytest.raises(ValueError):
        y4m.Writer(io.BytesIO(), 3, 2, 24, 1)
    with pytest.raises(ValueError):
        y4m.Writer(io.BytesIO(), 2, 2, 24, 1).write(np.zeros(5, np.uint8))


def test_y4m_truncated_last_frame_raises():
    frames = y4m_frames(2, 6, 4)
    buf = io.BytesIO()
    wr = y4m.Writer(buf, 6, 4, 24, 1)
    for f in frames:
        wr.write(f)
    rd = y4m.Reader(io.BytesIO(buf.getvalue()[:-1]))
    assert np.array_equal(next(rd), frames[0])
    with pytest.raises(ValueError, match="truncated"):
        next(rd)
    with pytest.raises(ValueError):
        list(y4m.Reader(io.BytesIO(buf.getvalue()[:-36 - 3])))                           # ends inside "FRAME\n"


def test_cli_has_the_y4m_options():
    from rrin_amd.__main__ import build_parser
    a = build_parser().parse_args(["--model_name", "M", "convert", "--sf", "1", "--fps", "0", "--y4m_in", "-",
                                   "--y4m_out", "out.y4m"])
    assert a.y4m_in == "-" and a.y4m_out == "out.y4m"
    b = build_parser().parse_args(["--model_name", "M", "convert", "--sf", "1", "--fps", "30", "--image_folder", "d"])
    assert b.y4m_in is None and b.y4m_out is None
