"""CPU: the host side of the YUV 4:2:2 / 4:4:4 frame paths -- the integer conversions that define
Net.forward_yuv / forward_yuv16 for the layouts "nv16", "i422" and "i444" (rrin_amd.yuv), the argument
validation of the entry points that honour rrin_yuv420.chroma (nothing is launched), the opt-in Y4M
tags, and convert.interpolate_y4m on an in-memory 4:2:2 stream with a host model."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from rrin_amd import _lib, y4m, yuv
from rrin_amd import convert as cv

FAKE = 1 << 30  # a fabricated non-null device pointer: never dereferenced
E_SHAPE, E_ARG = -1, -2
NEW_LAYOUTS = yuv.LAYOUTS_422 + yuv.LAYOUTS_444
CHROMA = {"420": _lib.CHROMA_420, "422": _lib.CHROMA_422, "444": _lib.CHROMA_444}


def words(x):
    return yuv.int_to_words(x.to(torch.int32))


# ---- the definition ---------------------------------------------------------------------------
def test_layout_tables():
    assert yuv.LAYOUTS == ("nv12", "i420")                       # what existing callers iterate over
    assert yuv.LAYOUTS_422 == ("nv16", "i422") and yuv.LAYOUTS_444 == ("i444",)
    assert [yuv.chroma_of(x) for x in ("nv12", "i420", "nv16", "i422", "i444")] == ["420", "420", "422", "422", "444"]
    with pytest.raises(ValueError):
        yuv.chroma_of("nv24")
    assert yuv.stack_rows(6, "i420") == 9 and yuv.stack_rows(5, "nv16") == 10 and yuv.stack_rows(5, "i444") == 15


@pytest.mark.parametrize("layout", NEW_LAYOUTS)
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_grey_maps_to_neutral_chroma(layout, depth):
    maxval, mid = (1 << depth) - 1, 1 << (depth - 1)
    for std in ("bt709", "bt601"):
        for full in (False, True):
            k = yuv.coefficients(std, full, depth)
            levels = torch.arange(0, maxval + 1, max(1, maxval // 255))
            rgb = levels.view(-1, 1, 1, 1).expand(-1, 3, 4, 3).contiguous()
            if depth == 8:
                out = yuv.rgb_to_yuv(rgb.to(torch.uint8), layout, k)
            else:
                out = yuv.words_to_int(yuv.rgb16_to_yuv(words(rgb), layout, k, depth))
            _, u, v = yuv.split_planes(out, layout)
            assert (u == mid).all() and (v == mid).all(), (std, full)


def test_row_pair_and_block_identities():
    """Rows in identical pairs: the 4:2:0 chroma row equals both 4:2:2 chroma rows of its pair.  Identical
    2x2 blocks: the same chroma in all three formats."""
    g = torch.Generator().manual_seed(4)
    for k in (None, yuv.coefficients("bt601", True)):
        rows = torch.randint(0, 256, (2, 5, 12, 3), dtype=torch.uint8, generator=g)
        rgb = rows.repeat_interleave(2, 1)                                   # [2,10,12,3], rows paired
        _, u0, v0 = yuv.split_planes(yuv.rgb_to_yuv420(rgb, "i420", k), "i420")
        y2, u2, v2 = yuv.split_planes(yuv.rgb_to_yuv(rgb, "i422", k), "i422")
        assert torch.equal(u2[:, 0::2], u0) and torch.equal(u2[:, 1::2], u0)
        assert torch.equal(v2[:, 0::2], v0) and torch.equal(v2[:, 1::2], v0)
        assert torch.equal(y2, yuv.split_planes(yuv.rgb_to_yuv420(rgb, "i420", k), "i420")[0])   # luma unchanged
        blocks = torch.randint(0, 256, (2, 5, 6, 3), dtype=torch.uint8, generator=g)
        rgb = blocks.repeat_interleave(2, 1).repeat_interleave(2, 2)
        _, u0, v0 = yuv.split_planes(yuv.rgb_to_yuv420(rgb, "nv12", k), "nv12")
        _, u2, v2 = yuv.split_planes(yuv.rgb_to_yuv(rgb, "nv16", k), "nv16")
        _, u4, v4 = yuv.split_planes(yuv.rgb_to_yuv(rgb, "i444", k), "i444")
        assert torch.equal(u2[:, 0::2], u0) and torch.equal(u4[:, 0::2, 0::2], u0) and torch.equal(u4[:, 1::2, 1::2], u0)
        assert torch.equal(v2[:, 1::2], v0) and torch.equal(v4[:, 0::2, 1::2], v0) and torch.equal(v4[:, 1::2, 0::2], v0)
    # and at depth 12 through the 16-bit functions
    blocks = torch.randint(0, 4096, (1, 3, 4, 3), generator=g)
    rgb = words(blocks.repeat_interleave(2, 1).repeat_interleave(2, 2))
    _, u0, _ = yuv.split_planes(yuv.rgb16_to_yuv420(rgb, "i420", None, 12), "i420")
    _, u2, _ = yuv.split_planes(yuv.rgb16_to_yuv(rgb, "i422", None, 12), "i422")
    _, u4, _ = yuv.split_planes(yuv.rgb16_to_yuv(rgb, "i444", None, 12), "i444")
    assert torch.equal(yuv.words_to_int(u2[:, 0::2]), yuv.words_to_int(u0))
    assert torch.equal(yuv.words_to_int(u4[:, 0::2, 0::2]), yuv.words_to_int(u0))


def test_block_rule_is_the_written_formula():
    """One 2x1 block and one pixel by hand, in Python integers."""
    k = yuv.coefficients("bt601", False)
    clip = lambda x: min(max(x, 0), 255)  # noqa: E731
    rgb = torch.tensor([[[[200, 10, 30], [90, 250, 3]]]], dtype=torch.uint8)
    _, u, v = yuv.split_planes(yuv.rgb_to_yuv(rgb, "i422", k), "i422")
    rs, gs, bs = 290, 260, 33
    assert int(u) == clip(128 + ((k.ur * rs + k.ug * gs + k.ub * bs + 16384) >> 15))
    assert int(v) == clip(128 + ((k.vr * rs + k.vg * gs + k.vb * bs + 16384) >> 15))
    _, u, v = yuv.split_planes(yuv.rgb_to_yuv(rgb, "i444", k), "i444")
    for i, (r, gg, b) in enumerate([(200, 10, 30), (90, 250, 3)]):
        assert int(u[0, 0, i]) == clip(128 + ((k.ur * r + k.ug * gg + k.ub * b + 8192) >> 14))
        assert int(v[0, 0, i]) == clip(128 + ((k.vr * r + k.vg * gg + k.vb * b + 8192) >> 14))


@pytest.mark.parametrize("layout,shape", [("nv16", (3, 6)), ("i422", (1, 2)), ("i444", (3, 5)), ("i444", (1, 1))])
def test_split_join_round_trip_and_byte_layout(layout, shape):
    h0, w0 = shape
    g = torch.Generator().manual_seed(2)
    fr = torch.randint(0, 256, (2, yuv.stack_rows(h0, layout), w0), dtype=torch.uint8, generator=g)
    assert yuv.stack_size(fr, layout) == (h0, w0)
    y, u, v = yuv.split_planes(fr, layout)
    cw = w0 if layout == "i444" else w0 // 2
    assert tuple(y.shape) == (2, h0, w0) and tuple(u.shape) == tuple(v.shape) == (2, h0, cw)
    assert torch.equal(yuv.join_planes(y, u, v, layout), fr)
    c = fr[:, h0:].reshape(2, -1)
    if layout == "nv16":
        assert torch.equal(c[:, 0::2], u.reshape(2, -1)) and torch.equal(c[:, 1::2], v.reshape(2, -1))
    else:
        assert torch.equal(c, torch.cat((u.reshape(2, -1), v.reshape(2, -1)), 1))
    rgb = yuv.yuv_to_rgb(fr, layout)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (2, h0, w0, 3)
    back = yuv.rgb_to_yuv(rgb, layout)
    assert back.dtype == torch.uint8 and back.shape == fr.shape


def test_444_of_a_replicated_420_stack_is_the_420_conversion():
    g = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 256, (2, 9, 10), dtype=torch.uint8, generator=g)
    for layout in yuv.LAYOUTS:
        for k in (None, yuv.coefficients("bt601", True)):
            y, u, v = yuv.split_planes(fr, layout)
            up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)  # noqa: E731
            assert torch.equal(yuv.yuv_to_rgb(yuv.join_planes(y, up(u), up(v), "i444"), "i444", k),
                               yuv.yuv420_to_rgb(fr, layout, k))
            assert torch.equal(yuv.yuv_to_rgb(yuv.join_planes(y, u.repeat_interleave(2, 1), v.repeat_interleave(2, 1),
                                                              "nv16"), "nv16", k), yuv.yuv420_to_rgb(fr, layout, k))
            assert torch.equal(yuv.yuv_to_rgb(fr, layout, k), yuv.yuv420_to_rgb(fr, layout, k))   # the 4:2:0 default
    f16 = words(torch.randint(0, 1024, (1, 9, 10), generator=g))
    y, u, v = yuv.split_planes(f16, "i420")
    up = lambda c: c.repeat_interleave(2, 1).repeat_interleave(2, 2)  # noqa: E731
    a = yuv.yuv_to_rgb16(yuv.join_planes(y, up(u), up(v), "i444"), "i444", None, 10)
    assert torch.equal(yuv.words_to_int(a), yuv.words_to_int(yuv.yuv420_to_rgb16(f16, "i420", None, 10)))


def test_words_above_maxval_and_msb():
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 65536, (1, 6, 4), generator=g)
    lo = yuv.yuv_to_rgb16(words(raw), "i422", None, 12, False)
    assert torch.equal(yuv.words_to_int(lo), yuv.words_to_int(yuv.yuv_to_rgb16(words(raw.clamp(max=4095)), "i422", None, 12)))
    hi = yuv.yuv_to_rgb16(words(raw), "i422", None, 10, True)
    assert torch.equal(yuv.words_to_int(hi), yuv.words_to_int(yuv.yuv_to_rgb16(words(raw >> 6), "i422", None, 10)))
    out = yuv.words_to_int(yuv.rgb16_to_yuv(hi, "nv16", None, 10, True))
    assert (out & 63).eq(0).all() and torch.equal(out >> 6, yuv.words_to_int(yuv.rgb16_to_yuv(hi, "nv16", None, 10)))


def test_bad_sizes_and_types_raise():
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv(z8(1, 2, 3, 3), "i422")                 # odd W0
    yuv.rgb_to_yuv(z8(1, 3, 2, 3), "nv16")                     # odd H0 is legal
    yuv.rgb_to_yuv(z8(1, 1, 1, 3), "i444")
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv(z8(1, 3, 3, 3), "i420")                 # the 4:2:0 rule through the new name
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(z8(1, 3, 2), "nv16")                    # 3 rows are not 2*H0
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(z8(1, 4, 3), "i422")                    # odd W0
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(z8(1, 4, 3), "i444")                    # 4 rows are not 3*H0
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(z8(4, 2), "i444")                       # no frame axis
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb(z8(1, 3, 2), "nv24")
    with pytest.raises(TypeError):
        yuv.yuv_to_rgb(torch.zeros((1, 3, 2), dtype=torch.int32), "i444")
    with pytest.raises(TypeError):
        yuv.yuv_to_rgb16(z8(1, 3, 2), "i444")
    with pytest.raises(TypeError):
        yuv.rgb16_to_yuv(z8(1, 1, 2, 3), "i422")
    with pytest.raises(ValueError):
        yuv.yuv_to_rgb16(torch.zeros((1, 3, 2), dtype=torch.uint16), "i444", depth=14)
    with pytest.raises(ValueError):
        yuv.yuv420_to_rgb(z8(1, 4, 2), "i422")                 # the 4:2:0 functions keep to their layouts
    with pytest.raises(ValueError):
        yuv.rgb_to_yuv420(z8(1, 2, 2, 3), "i444")


# ---- C ABI: validation before any HIP call ----------------------------------------------------
def _stack(h0, w0, layout, cls=_lib.Yuv420, **kw):
    """A dense stack of ``layout`` at a fabricated address; kw overrides fields."""
    chroma = yuv.chroma_of(layout)
    ch = h0 // 2 if chroma == "420" else h0
    cw = w0 if chroma == "444" else w0 // 2
    semi = layout in ("nv12", "nv16")
    s = cls()
    s.y, s.u = FAKE, FAKE + h0 * w0
    s.v = s.u + (1 if semi else ch * cw)
    s.img_stride = h0 * w0 + 2 * ch * cw
    s.y_pitch, s.c_pitch, s.c_step = w0, cw * (2 if semi else 1), 2 if semi else 1
    s.chroma = CHROMA[chroma]
    if cls is _lib.Yuv420x16:
        s.depth, s.shift = 10, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _net(d, n, h, w):
    d.net.n, d.net.h, d.net.w, d.net.prec = n, h, w, _lib.PREC_F32R
    d.net.coef = d.net.workspace = FAKE
    d.net.workspace_bytes = 1 << 40
    d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))


def _desc(h0, w0, layout, wide=False, out_layout=None, **kw):
    d = _lib.NetYuv16Desc() if wide else _lib.NetYuvDesc()
    cls = _lib.Yuv420x16 if wide else _lib.Yuv420
    _net(d, 2, (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16)
    d.f0, d.f1 = _stack(h0, w0, layout, cls, **kw), _stack(h0, w0, layout, cls)
    d.out = _stack(h0, w0, out_layout or layout, cls)
    d.coef = _lib.YuvCoef(*yuv.coefficients(depth=10 if wide else 8))
    d.h0, d.w0 = h0, w0
    return d


@pytest.mark.parametrize("wide", [False, True])
def test_net_yuv_fwd_validates_chroma_before_any_launch(wide):
    fwd = _lib.lib().rrin_net_yuv16_fwd if wide else _lib.lib().rrin_net_yuv_fwd
    run = lambda *a, **kw: fwd(C.byref(_desc(*a, wide=wide, **kw)), None)  # noqa: E731
    assert run(38, 50, "i422", chroma=3) == E_ARG                       # no such format
    assert run(38, 50, "i422", chroma=-1) == E_ARG
    assert run(38, 50, "i422", out_layout="i444") == E_ARG              # f0, f1, out share chroma
    assert run(38, 50, "i444", chroma=_lib.CHROMA_422) == E_ARG         # f0 (valid as 4:2:2 too) differs from f1
    assert run(38, 49, "nv16") == E_SHAPE                               # odd w0 at 4:2:2
    assert run(38, 0, "i444") == E_SHAPE
    assert run(0, 50, "i422") == E_SHAPE
    assert run(37, 50, "i420") == E_SHAPE                               # 4:2:0 keeps its rule
    # pitches one too small
    assert run(37, 50, "i422", y_pitch=49) == E_SHAPE
    assert run(37, 50, "i422", c_pitch=24) == E_SHAPE
    assert run(37, 50, "nv16", c_pitch=49) == E_SHAPE
    assert run(37, 49, "i444", c_pitch=48) == E_SHAPE
    assert run(37, 49, "i444", c_pitch=97, c_step=2) == E_SHAPE         # a semi-planar 4:4:4 row is 2 * w0
    assert run(37, 49, "i444", c_step=3) == E_ARG
    # overlapping frames: the stride must cover the luma and the format's chroma span
    assert run(37, 50, "i422", img_stride=37 * 50 - 1) == E_SHAPE
    # the chroma span of rows 0 .. h0-1: 4:2:0 would stop at row h0/2 - 1
    assert run(38, 50, "i444", y_pitch=50, c_pitch=200, img_stride=37 * 200 + 49) == E_SHAPE
    assert run(38, 50, "i422", c_pitch=200, img_stride=37 * 200 + 24) == E_SHAPE


def test_pack_and_head_validate_chroma_before_any_launch():
    L = _lib.lib()
    k = _lib.YuvCoef(*yuv.coefficients())
    g = _lib.Geom()
    _lib.check(L.rrin_make_geom_h8(48, 64, C.byref(g)))
    v = _lib.H8(FAKE, None, 4 * g.plane, 0, 4, g)
    pack = lambda a, b, h0=38, w0=50: L.rrin_pack_g16_yuv_h8(C.byref(a), C.byref(b), C.byref(k), 1, h0, w0, C.byref(v),  # noqa: E731
                                                             _lib.PREC_F32R, None)
    assert pack(_stack(38, 50, "i422"), _stack(38, 50, "i444")) == E_ARG
    assert pack(_stack(38, 50, "i422", chroma=7), _stack(38, 50, "i422", chroma=7)) == E_ARG
    assert pack(_stack(38, 49, "i422"), _stack(38, 49, "i422"), 38, 49) == E_SHAPE
    assert pack(_stack(38, 50, "i444", c_pitch=49), _stack(38, 50, "i444")) == E_SHAPE
    assert pack(_stack(22, 50, "i444"), _stack(22, 50, "i444"), 22, 50) == E_SHAPE      # g16 is 48 rows
    k16 = _lib.YuvCoef(*yuv.coefficients(depth=10))
    a, b = _stack(38, 50, "i422", _lib.Yuv420x16), _stack(38, 50, "i444", _lib.Yuv420x16)
    assert L.rrin_pack_g16_yuv16_h8(C.byref(a), C.byref(b), C.byref(k16), 1, 38, 50, C.byref(v), _lib.PREC_F32R,
                                    None) == E_ARG

    def head(layout, h0, w0, top, **kw):
        d = _lib.HeadH8Desc()
        d.n, d.cin, d.cout, d.mode, d.prec = 1, 32, 3, _lib.HEAD_FINAL, _lib.PREC_F32R
        d.src = _lib.H8(FAKE, None, 8 * g.plane, 0, 8, g)
        d.g16 = v
        d.w = d.bias = d.coef = FAKE
        d.h0, d.w0, d.top = h0, w0, top
        d.out_yuv = _stack(h0, w0, layout, **kw)
        d.yuv_coef = k
        return L.rrin_head_h8_fwd(C.byref(d), None)

    assert head("i420", 38, 50, 9) == E_SHAPE                           # 4:2:0: top even, as before
    assert head("i420", 37, 50, 10) == E_SHAPE
    assert head("i422", 37, 49, 11) == E_SHAPE                          # 4:2:2: w0 even
    assert head("i422", 37, 50, 11, chroma=5) == E_ARG
    assert head("i444", 37, 49, 12) == E_SHAPE                          # top + h0 > 48


def test_smallest_frames_pass_the_validation():
    """h0 = 1 at 4:2:2 / 4:4:4, 1x1 at 4:4:4 and odd tops are accepted.  Nothing may be launched on
    fabricated pointers, so the call is a FINAL head with cout 4: that is refused (RRIN_E_ARG) only after
    every check of the output stack has passed, while a size the format does not take comes back
    RRIN_E_SHAPE before it -- as the same sizes do at chroma 4:2:0."""
    L = _lib.lib()
    g = _lib.Geom()
    _lib.check(L.rrin_make_geom_h8(48, 64, C.byref(g)))

    def head(layout, h0, w0, top, wide, chroma=None):
        d = _lib.HeadH8Desc()
        d.n, d.cin, d.cout, d.mode, d.prec = 2, 32, 4, _lib.HEAD_FINAL, _lib.PREC_F32R
        d.src = _lib.H8(FAKE, None, 8 * g.plane, 0, 8, g)
        d.g16 = _lib.H8(FAKE, None, 4 * g.plane, 0, 4, g)
        d.w = d.bias = d.coef = FAKE
        d.h0, d.w0, d.top = h0, w0, top
        kw = {} if chroma is None else {"chroma": chroma}
        if wide:
            d.out_yuv16 = _stack(h0, w0, layout, _lib.Yuv420x16, **kw)
        else:
            d.out_yuv = _stack(h0, w0, layout, **kw)
        d.yuv_coef = _lib.YuvCoef(*yuv.coefficients(depth=10 if wide else 8))
        return L.rrin_head_h8_fwd(C.byref(d), None)

    for wide in (False, True):
        for layout, h0, w0, top in (("i422", 1, 2, 47), ("nv16", 1, 2, 0), ("i444", 1, 2, 3), ("i444", 1, 1, 47),
                                    ("i444", 3, 1, 45), ("i422", 37, 50, 11), ("i444", 37, 49, 11)):
            assert head(layout, h0, w0, top, wide) == E_ARG, (layout, h0, w0, wide)
            assert head(layout, h0, w0, top, wide, chroma=_lib.CHROMA_420) == E_SHAPE, (layout, h0, w0, wide)
        assert head("i420", 38, 50, 10, wide) == E_ARG                      # the probe itself: a valid 4:2:0 store
        assert head("i422", 1, 1, 47, wide) == E_SHAPE
        assert head("i444", 0, 1, 47, wide) == E_SHAPE


def test_len_entry_points_validate():
    L = _lib.lib()
    sad = FAKE
    assert L.rrin_pair_sad_u8_len(FAKE, FAKE, 10, 1, 0, sad, None) == E_SHAPE
    assert L.rrin_pair_sad_u8_len(FAKE, FAKE, 10, 0, 10, sad, None) == E_SHAPE
    assert L.rrin_pair_sad_u8_len(FAKE, FAKE, 9, 1, 10, sad, None) == E_ARG        # frames overlap
    assert L.rrin_pair_sad_u8_len(None, FAKE, 10, 1, 10, sad, None) == E_ARG
    assert L.rrin_pair_sad_u8_len(FAKE, FAKE, 10, 1, 10, sad + 4, None) == E_ARG   # sad is 8-byte aligned
    assert L.rrin_pair_sad_u16_len(FAKE, FAKE, 10, 1, 0, 10, 0, sad, None) == E_SHAPE
    assert L.rrin_pair_sad_u16_len(FAKE, FAKE, 10, 1, 10, 8, 0, sad, None) == E_ARG
    assert L.rrin_pair_sad_u16_len(FAKE + 1, FAKE, 10, 1, 10, 10, 0, sad, None) == E_ARG
    assert L.rrin_gate_frames_u8_len(FAKE, FAKE, 10, 1, 0, FAKE, FAKE, None) == E_SHAPE
    assert L.rrin_gate_frames_u8_len(FAKE, FAKE, 10, 1, 10, None, FAKE, None) == E_ARG
    assert L.rrin_gate_frames_u8_len(FAKE, FAKE, 9, 1, 10, FAKE, FAKE, None) == E_ARG
    # the old names keep their codes
    assert L.rrin_pair_sad_u8(FAKE, FAKE, 10, 1, 0, 4, sad, None) == E_SHAPE
    assert L.rrin_pair_sad_u8(FAKE, FAKE, 11, 1, 1, 4, sad, None) == E_ARG
    assert L.rrin_gate_frames_u8(FAKE, FAKE, 12, 1, 2, 0, FAKE, FAKE, None) == E_SHAPE
    assert cv.scene_limit_len(1.5, 1156) == 1734 and cv.scene_limit_len(2, 7, 1023) == 14
    assert cv.scene_limit_len(0.25, 3 * 5 * 7) == cv.scene_limit(0.25, 5, 7)
    with pytest.raises(ValueError):
        cv.scene_limit_len(256, 10)


# ---- Y4M ----------------------------------------------------------------------------------------
TAGS = [("422", "422", 8), ("444", "444", 8), ("422p10", "422", 10), ("422p12", "422", 12), ("444p10", "444", 10),
        ("444p12", "444", 12)]
ALL = dict(depths=(8, 10, 12), chroma=("420", "422", "444"))


@pytest.mark.parametrize("tag,chroma,depth", TAGS)
def test_y4m_round_trip_of_the_new_tags(tag, chroma, depth):
    w, h = (6, 3) if chroma == "422" else (5, 3)                 # an odd H, and an odd W where the format allows
    samples = w * h * (2 if chroma == "422" else 3)
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 1 << depth, samples).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(3)]
    buf = io.BytesIO()
    wr = y4m.Writer(buf, w, h, 25, 1, tag, **ALL)
    assert wr.frame_bytes == samples * (2 if depth > 8 else 1)
    for f in frames:
        wr.write(f)
    raw = buf.getvalue()
    head = b"YUV4MPEG2 W%d H%d F25:1 Ip C%s\n" % (w, h, tag.encode())
    assert raw.startswith(head + b"FRAME\n") and len(raw) == len(head) + 3 * (6 + wr.frame_bytes)
    rd = y4m.Reader(io.BytesIO(raw), **ALL)
    assert (rd.width, rd.height, rd.colorspace, rd.chroma, rd.bit_depth) == (w, h, tag, chroma, depth)
    assert rd.frame_bytes == wr.frame_bytes
    got = list(rd)
    assert len(got) == 3 and all(g.dtype == f.dtype and np.array_equal(g, f) for g, f in zip(got, frames))
    with pytest.raises(ValueError):
        wr.write(frames[0][:-1])
    # asked for with the chroma format but without the depth: refused
    if depth > 8:
        with pytest.raises(ValueError, match=tag):
            y4m.Reader(io.BytesIO(raw), chroma=("420", "422", "444"))
        with pytest.raises(ValueError):
            y4m.Writer(io.BytesIO(), w, h, 25, 1, tag, chroma=("420", "422", "444"))


def test_y4m_defaults_refuse_what_they_refused():
    body = b"FRAME\n" + bytes(12)
    for tag in ("C422", "C444", "C422p10", "C444p12"):
        with pytest.raises(ValueError, match=tag) as e:
            y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 " + tag.encode() + b"\n" + body))
        assert "only 8-bit 4:2:0 is supported" in str(e.value)
        with pytest.raises(ValueError, match="only 8-bit 4:2:0 is supported"):
            y4m.Writer(io.BytesIO(), 2, 2, 24, 1, tag[1:])
        with pytest.raises(ValueError, match=r"only 4:2:0 of \(8, 10, 12\) bits"):
            y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 " + tag.encode() + b"\n" + body), depths=(8, 10, 12))
    with pytest.raises(ValueError, match="even W and H"):
        y4m.Writer(io.BytesIO(), 3, 2, 24, 1)
    # the opt-in keeps reading 4:2:0 and refusing the rest
    rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 C420jpeg\nFRAME\n" + bytes(6)), **ALL)
    assert (rd.chroma, rd.bit_depth, rd.frame_bytes) == ("420", 8, 6) and len(list(rd)) == 1
    rd = y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 C420p10\nFRAME\n" + bytes(12)), **ALL)
    assert (rd.chroma, rd.bit_depth, rd.frame_bytes) == ("420", 10, 12)
    for tag in ("Cmono", "C411", "C444alpha", "C444p16", "C422p9", "It", "Ib"):
        with pytest.raises(ValueError, match=tag):
            y4m.Reader(io.BytesIO(b"YUV4MPEG2 W2 H2 F24:1 " + tag.encode() + b"\n" + body), **ALL)
    for cs in ("mono", "411", "444alpha"):
        with pytest.raises(ValueError):
            y4m.Writer(io.BytesIO(), 2, 2, 24, 1, cs, **ALL)


def test_y4m_sizes_per_format():
    hdr = lambda w, h, tag: io.BytesIO(b"YUV4MPEG2 W%d H%d F24:1 C%s\n" % (w, h, tag))  # noqa: E731
    y4m.Reader(hdr(2, 3, b"422"), **ALL)
    y4m.Reader(hdr(3, 3, b"444"), **ALL)
    y4m.Reader(hdr(1, 1, b"444p10"), **ALL)
    y4m.Writer(io.BytesIO(), 2, 1, 24, 1, "422", **ALL)
    y4m.Writer(io.BytesIO(), 1, 1, 24, 1, "444", **ALL)
    with pytest.raises(ValueError, match="even W"):
        y4m.Reader(hdr(3, 2, b"422"), **ALL)
    with pytest.raises(ValueError, match="even W"):
        y4m.Writer(io.BytesIO(), 3, 2, 24, 1, "422p10", **ALL)
    with pytest.raises(ValueError, match="even W and H"):
        y4m.Reader(hdr(2, 3, b"420"), **ALL)
    with pytest.raises(ValueError, match="even W and H"):
        y4m.Writer(io.BytesIO(), 2, 3, 24, 1, "420", **ALL)
    with pytest.raises(ValueError):
        y4m.Writer(io.BytesIO(), 0, 1, 24, 1, "444", **ALL)


# ---- interpolate_y4m with a host model ----------------------------------------------------------
class HostModel(torch.nn.Module):
    """Stands in for Net: its "interpolated" frame k of a pair is f0 + k + 1 (wrapping), so that the order
    of the output frames shows; records the calls."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def _run(self, name, f0, f1, ts, layout, **kw):
        assert f0.shape == f1.shape and f0.data_ptr() + f0.stride(0) * f0.element_size() == f1.data_ptr()
        self.calls.append((name, tuple(f0.shape), f0.dtype, tuple(ts), layout, kw))
        return [(f0.to(torch.int32) + k + 1).to(torch.int16).view(torch.uint16) if f0.dtype == torch.uint16
                else f0 + (k + 1) for k in range(len(ts))]

    def interpolate_yuv(self, f0, f1, ts, layout="nv12", coef=None, **kw):
        return self._run("yuv", f0, f1, ts, layout, **kw)

    def interpolate_yuv16(self, f0, f1, ts, layout="nv12", depth=10, msb=False, coef=None, **kw):
        return self._run("yuv16", f0, f1, ts, layout, depth=depth, msb=msb, **kw)


@pytest.mark.parametrize("tag,chroma,depth", [("422p10", "422", 10), ("422", "422", 8), ("444", "444", 8)])
def test_interpolate_y4m_keeps_tag_order_and_input_frames(tag, chroma, depth):
    w, h = (6, 3) if chroma == "422" else (5, 3)
    samples = w * h * (2 if chroma == "422" else 3)
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 200, samples).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(4)]
    src = io.BytesIO()
    wr = y4m.Writer(src, w, h, 24, 1, tag, **ALL)
    for f in frames:
        wr.write(f)
    src.seek(0)
    dst = io.BytesIO()
    model = HostModel()
    sf = 2
    assert cv.interpolate_y4m(model, src, dst, sf, batch=2, log=lambda *a: None) == 10
    rd = y4m.Reader(io.BytesIO(dst.getvalue()), **ALL)
    assert (rd.width, rd.height, rd.colorspace, rd.chroma, rd.bit_depth) == (w, h, tag, chroma, depth)
    assert (rd.fps_num, rd.fps_den) == (72, 1)
    out = list(rd)
    assert len(out) == 10
    for p in range(3):
        assert np.array_equal(out[3 * p], frames[p])                       # the input frames as they were
        for k in range(sf):
            assert np.array_equal(out[3 * p + k + 1], frames[p] + k + 1)   # frame k of pair p, in order
    assert np.array_equal(out[9], frames[3])
    rows = 2 * h if chroma == "422" else 3 * h
    name = "yuv16" if depth > 8 else "yuv"
    assert [c[0] for c in model.calls] == [name, name]
    assert model.calls[0][1] == (2, rows, w) and model.calls[1][1] == (1, rows, w)
    assert all(c[4] == "i" + chroma and c[3] == (1 / 3, 2 / 3) for c in model.calls)
    if depth > 8:
        assert all(c[5]["depth"] == depth and c[5]["msb"] is False for c in model.calls)
