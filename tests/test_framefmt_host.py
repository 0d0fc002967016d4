"""rrin_amd.framefmt.FrameFormat against what the four per-path copies derived before it existed.

tests/golden/frame_formats.json was recorded from the commit before the format: per path, layout,
depth, alignment, matrix and frame size, every descriptor field (addresses as offsets from base 0),
the frame length, the output shape, the gate limits at thresholds 0, 1.5 and maxval, the Flow-reuse
tag string and the path part of the key of the cached gate sums.
"""
import json
import os

import pytest
import torch

from rrin_amd import yuv
from rrin_amd.convert import scene_limit, scene_limit_len
from rrin_amd.framefmt import ENTRIES, FrameFormat, check_depth, frame_stride

with open(os.path.join(os.path.dirname(__file__), "golden", "frame_formats.json")) as f:
    GOLDEN = json.load(f)
CASES = GOLDEN["cases"]
B0, B1, BO = 1 << 20, 5 << 20, 9 << 20   # three device addresses that are never dereferenced


def fmt_of(c) -> FrameFormat:
    if c["path"] == "u8":
        return FrameFormat.u8()
    if c["path"] == "u16":
        return FrameFormat.u16(c["depth"], "test")
    coef = yuv.coefficients(c["std"], depth=c["depth"])
    if c["path"] == "yuv":
        return FrameFormat.yuv(c["layout"], coef)
    return FrameFormat.yuv16(c["layout"], c["depth"], c["msb"], coef)


def case_id(c):
    return f"{c['path']}-{c['layout']}-{c['depth']}-{int(c['msb'])}-{c['std']}-{c['h0']}x{c['w0']}"


def test_golden_covers_the_issue_list():
    got = {(c["path"], c["layout"], c["depth"], c["msb"], c["h0"], c["w0"]) for c in CASES if c["std"] != "bt601"}
    want = set()
    for depth in (8, 9, 10, 16):
        for size in ((2, 2), (6, 10), (18, 34), (5, 7)):
            want.add(("u8" if depth == 8 else "u16", None, depth, False, *size))
    for depth, msb in ((8, False), (10, False), (10, True), (12, False), (12, True)):
        for layout in yuv.ALL_LAYOUTS:
            sizes = [(2, 2), (6, 10), (18, 34)]
            sizes += [(5, 6)] if layout in ("nv16", "i422") else []
            sizes += [(5, 7)] if layout == "i444" else []
            for size in sizes:
                want.add(("yuv" if depth == 8 else "yuv16", layout, depth, msb, *size))
    assert got == want


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fields(c):
    fmt, h0, w0, n = fmt_of(c), c["h0"], c["w0"], GOLDEN["n"]
    gf = c["fields"]
    assert fmt.path == c["path"] and fmt.entries == ENTRIES[c["path"]]
    assert fmt.entries == tuple(f"rrin_net_{c['path']}{s}_fwd" for s in ("", "_items", "_scaled"))
    assert fmt.dtype == (torch.uint8 if c["depth"] == 8 else torch.uint16)
    assert fmt.maxval == c["maxval"]
    assert fmt.wide == (None if c["depth"] == 8 else (c["depth"], 16 - c["depth"] if c["msb"] else 0))
    assert fmt.frame_len(h0, w0) == c["frame_len"]
    assert list(fmt.out_shape(n, h0, w0)) == c["out_shape"]
    # the gate's limit is over the frame's length: the rows x cols entry and the length entry agree
    assert [scene_limit_len(th, fmt.frame_len(h0, w0), fmt.maxval) for th in (0, 1.5, fmt.maxval)] == c["limits"]
    stride = c["frame_len"] + 7   # the inputs' own stride; the output is dense
    d, nd = fmt.desc(B0, B1, stride, BO, h0, w0)
    assert type(d).__name__ == {"u8": "NetU8Desc", "u16": "NetU16Desc", "yuv": "NetYuvDesc", "yuv16": "NetYuv16Desc"}[
        c["path"]]
    assert C_addr(nd) == C_addr(d.net)
    assert (d.h0, d.w0) == (gf["h0"], gf["w0"])
    if c["layout"] is None:
        out = d.out_u8 if c["depth"] == 8 else d.out_u16
        assert (d.f0 - B0, d.f1 - B1, out - BO) == (gf["f0"], gf["f1"], gf["out"])
        assert d.img_stride == stride and gf["img_stride"] == c["frame_len"]
        if c["depth"] > 8:
            assert d.depth == gf["depth"]
        return
    assert [getattr(d.coef, k) for k in yuv.Coef._fields] == gf["coef"]
    for s, base, st in ((d.f0, B0, stride), (d.f1, B1, stride), (d.out, BO, gf["img_stride"])):
        got = {"y": s.y - base, "u": s.u - base, "v": s.v - base, "img_stride": s.img_stride, "y_pitch": s.y_pitch,
               "c_pitch": s.c_pitch, "c_step": s.c_step, "chroma": s.chroma}
        if c["depth"] > 8:
            got.update(depth=s.depth, shift=s.shift)
        want = {k: v for k, v in gf.items() if k not in ("h0", "w0", "coef")}
        want["img_stride"] = st
        assert got == want
    assert d.f0.chroma == GOLDEN["chroma_codes"][yuv.chroma_of(c["layout"])]


def C_addr(x):
    import ctypes
    return ctypes.addressof(x)


def test_scene_limit_has_one_body():
    for th in (0, 0.25, 1.5, 255):
        assert scene_limit(th, 18, 34) == scene_limit_len(th, 18 * 34 * 3)
    with pytest.raises(ValueError, match="mean absolute byte difference"):
        scene_limit(256, 2, 2)
    with pytest.raises(ValueError, match="mean absolute sample difference"):
        scene_limit(1024, 2, 2, 1023)


def test_tags_equal_exactly_where_the_parents_are():
    fmts = [fmt_of(c) for c in CASES]
    tags = [f.tag for f in fmts]
    for i, a in enumerate(CASES):
        for j, b in enumerate(CASES):
            assert (tags[i] == tags[j]) == (a["tag"] == b["tag"]), (case_id(a), case_id(b))
    assert tags == [c["tag"] for c in CASES]   # stronger: the strings themselves


def test_sums_keys_separate_what_the_parents_separated():
    bounds = [(0, 1), (1, 2)]
    keys = [fmt_of(c).sums_key(2, c["h0"], c["w0"], bounds) for c in CASES]
    for i, a in enumerate(CASES):
        for j, b in enumerate(CASES):
            if a["sums_key"] != b["sums_key"]:
                assert keys[i] != keys[j], (case_id(a), case_id(b))
    f = FrameFormat.u8()
    assert f.sums_key(2, 6, 10, bounds) != f.sums_key(3, 6, 10, bounds)
    assert f.sums_key(2, 6, 10, bounds) != f.sums_key(2, 6, 10, [(0, 2)])
    # equal frame lengths, and what the lengths alone would merge
    assert f.sums_key(2, 6, 10, bounds) != FrameFormat.yuv("i444").sums_key(2, 6, 10, bounds)
    assert (FrameFormat.u16(10, "t").sums_key(2, 6, 10, bounds)
            != FrameFormat.yuv16("i444", 10).sums_key(2, 6, 10, bounds))
    assert f.sums_key(2, 6, 10, bounds) != f.sums_key(2, 10, 6, bounds)


def test_constructor_checks_in_the_forwards_order():
    with pytest.raises(ValueError, match="layout must be one of"):
        FrameFormat.yuv("yv12", coef=[1] * 3)            # the layout before the matrix
    with pytest.raises(ValueError, match="layout must be one of"):
        FrameFormat.yuv16("yv12", 11)                     # ... and before the depth
    with pytest.raises(ValueError, match="10 or 12 bits deep"):
        FrameFormat.yuv16("nv12", 11, coef=[1 << 20] * 15)   # the depth before the matrix
    with pytest.raises(ValueError, match="yuv coefficients"):
        FrameFormat.yuv("nv12", [1 << 20] * 15)
    for bad in (8, 17, True, 10.0):
        with pytest.raises(ValueError, match=r"forward_u16: depth must be an int in 9\.\.16"):
            FrameFormat.u16(bad, "forward_u16")
    assert check_depth(8, 8) == 8 and check_depth(16) == 16
    with pytest.raises(ValueError, match="depth is 8 or 9..16, got 7"):
        check_depth(7, 8, "depth is 8 or 9..16")
    assert hash(FrameFormat.yuv("i420")) == hash(FrameFormat.yuv("i420", yuv.coefficients()))


def stack(fmt, n, h0, w0):
    return torch.zeros(fmt.out_shape(n, h0, w0), dtype=fmt.dtype)


FMTS = [FrameFormat.u8(), FrameFormat.u16(10, "t"), FrameFormat.yuv("nv12"), FrameFormat.yuv("i422"),
        FrameFormat.yuv16("i420", 10), FrameFormat.yuv16("i444", 12, True)]


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.tag[:16])
def test_check_views_of_one_stack_take_no_copy(fmt):
    frames = stack(fmt, 4, 6, 10)
    f0, f1, h0, w0, stride = fmt.check(frames[:-1], frames[1:], "cpu", "test")
    assert (h0, w0) == (6, 10) and stride == frames.stride(0) == fmt.frame_len(6, 10)
    assert f0.data_ptr() == frames.data_ptr() and f1.data_ptr() == frames[1:].data_ptr()
    # every second frame of a stack: still the stack's own stride, still no copy
    f0, f1, _, _, stride = fmt.check(frames[0:3:2], frames[1:4:2], "cpu", "test")
    assert stride == 2 * frames.stride(0) and f0.data_ptr() == frames.data_ptr()
    # one frame: the dense stride whatever the view's
    assert fmt.check(frames[0:3:2][:1], frames[1:2], "cpu", "test")[4] == fmt.frame_len(6, 10)
    # unequal strides: both copied, dense
    f0, f1, _, _, stride = fmt.check(frames[0:3:2], frames[1:3], "cpu", "test")
    assert stride == fmt.frame_len(6, 10) and f0.is_contiguous() and f1.is_contiguous()


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.tag[:16])
def test_check_refusals(fmt):
    a = stack(fmt, 2, 6, 10)
    other = torch.uint16 if fmt.dtype == torch.uint8 else torch.uint8
    with pytest.raises(TypeError):
        fmt.check(torch.zeros(a.shape, dtype=other), a, "cpu", "test")    # wrong dtype
    with pytest.raises(TypeError):
        fmt.check(None, a, "cpu", "test")                                 # no tensor
    with pytest.raises(RuntimeError, match="model on"):
        fmt.check(a, a, "meta", "test")                                   # wrong device
    with pytest.raises(ValueError):
        fmt.check(a, stack(fmt, 3, 6, 10), "cpu", "test")                 # unequal shapes
    with pytest.raises(ValueError):
        fmt.check(a[:0], a[:0], "cpu", "test")                            # an empty stack
    if fmt.layout is None:
        b = torch.zeros((2, 6, 10, 4), dtype=fmt.dtype)
        with pytest.raises(ValueError, match=r"\[N,H0,W0,3\]"):
            fmt.check(b, b, "cpu", "test")                                # a last dimension other than 3
        nd = torch.zeros((2, 6, 10, 6), dtype=fmt.dtype)[..., ::2]        # a non-dense frame: copied
    else:
        nd = torch.zeros((2, a.shape[1], 20), dtype=fmt.dtype)[..., ::2]
    f0, f1, _, _, stride = fmt.check(nd, nd, "cpu", "test")
    assert f0.is_contiguous() and stride == fmt.frame_len(6, 10) and frame_stride(nd) is None


def test_check_refuses_odd_sizes():
    f420, f422 = FrameFormat.yuv("i420"), FrameFormat.yuv("nv16")
    odd_h = torch.zeros((1, 3 * 5 // 2, 6), dtype=torch.uint8)           # H0 = 5 has no 4:2:0 stack
    with pytest.raises(ValueError):
        f420.check(torch.zeros((1, 7, 6), dtype=torch.uint8), torch.zeros((1, 7, 6), dtype=torch.uint8), "cpu", "t")
    with pytest.raises(ValueError):
        f420.check(odd_h[:, :, :5], odd_h[:, :, :5], "cpu", "t")
    odd_w = torch.zeros((1, 10, 7), dtype=torch.uint8)                    # 4:2:2 needs an even W0
    with pytest.raises(ValueError, match="even W0"):
        f422.check(odd_w, odd_w, "cpu", "t")
    ok = torch.zeros((1, 10, 6), dtype=torch.uint8)                       # ... and takes any H0
    assert f422.check(ok, ok, "cpu", "t")[2:4] == (5, 6)


def test_planes_are_the_metrics_planes():
    from rrin_amd.metrics import planes_of
    assert FrameFormat.u8().planes(5, 7) == planes_of("rgb", 5, 7)
    for layout in yuv.ALL_LAYOUTS:
        assert FrameFormat.yuv16(layout, 10).planes(6, 10) == planes_of("yuv", 6, 10, layout)


def test_samples_only_format_has_no_tag_and_no_descriptor():
    f = FrameFormat.samples("i420", 10, 6)
    assert (f.path, f.wide, f.frame_len(6, 10)) == ("yuv16", (10, 6), 90)
    a = stack(f, 2, 6, 10)
    assert f.check(a, a, "cpu", "test")[2:] == (6, 10, 90)
    with pytest.raises(ValueError, match="no tag"):
        f.tag
    with pytest.raises(ValueError, match="no descriptor"):
        f.desc_for(90, 6, 10)
    with pytest.raises(ValueError, match="layout must be one of"):   # the layout is checked with the stack
        FrameFormat.samples("yv12").check(a.view(torch.uint8), a.view(torch.uint8), "cpu", "test")
    assert FrameFormat.samples(None).tag == "u8" and FrameFormat.u8() is FrameFormat.u8()


def test_descriptor_template_is_shared_and_left_unchanged():
    fmt = FrameFormat.yuv16("nv16", 12, True)
    make = fmt.desc_for(200, 5, 6)
    assert make is fmt.desc_for(200, 5, 6) and make is not fmt.desc_for(201, 5, 6)
    d1, _ = make(B0, B1, BO)
    d2, _ = make(B1, BO, B0)
    assert (d1.f0.y, d1.out.v - BO) == (B0, d2.out.v - B0) and d2.f0.y == B1
    assert bytes(fmt.desc(B0, B1, 200, BO, 5, 6)[0]) == bytes(d1)
