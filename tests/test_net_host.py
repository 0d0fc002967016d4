"""The host half of the forward schedule (the workspace plan, the scratch layout of the engine's real
conv tables, the argument checks of every launching entry and their order) against
tests/golden/net_host.json, recorded from the library before net.hip was split into net_plan.hpp,
unet_sched.hip, net.hip, net_frames.hip and prof.hip (the recording script is the fixture's header).

Nothing is launched or dereferenced: pointers are fake (tag k stands for address k << 30), and the
launching entries only ever see descriptors the recorded library rejected before any HIP call --
every recorded code of theirs is an RRIN_E_* (< 0; a HIP error would be > 0).  An "accept" case is
valid in every respect but one: its workspace (or the second plan's) is one byte short, which is the
last check before the first HIP call, so RRIN_E_WORKSPACE proves that every earlier check passed.

The descriptors are built here (accept_cases, order_cases); the fixture holds what the recorded
library answered: the workspace sizes they are built from, and the code of every case by name.
"""
import copy
import ctypes as C
import json
import os

import pytest

from rrin_amd import Net, _lib
from rrin_amd import engine as E
from rrin_amd.synthetic import keyed_state_dict
from rrin_amd.unet import UNet

with open(os.path.join(os.path.dirname(__file__), "golden", "net_host.json")) as _f:
    GOLD = json.load(_f)

E_WORKSPACE = -3
PRECS = (_lib.PREC_F32, _lib.PREC_F16X3, _lib.PREC_F16, _lib.PREC_F32R)
FORMATS = ("u8", "yuv", "u16", "yuv16")
# every launching entry of the schedule: name -> (library symbol, descriptor format)
ENTRIES = {"net": ("rrin_net_fwd", "f32"), "net_scaled": ("rrin_net_scaled_fwd", "f32"),
           "unet": ("rrin_unet_fwd", "unet")}
for _f in FORMATS:
    for _k in ("", "items_", "scaled_", "plane_"):
        ENTRIES[(_f + "_" + _k).rstrip("_")] = ("rrin_net_%s_%sfwd" % (_f, _k), _f)

# tables the descriptors point to: zeroed, alive for the module's life, never read (a table is read
# by the scratch walk alone, which needs a scratch pointer; no launching case has one)
_CONVS = (_lib.ConvWeights * 77)()
_HEADS = (_lib.HeadWeights * 4)()


def _ptr(tag):
    return (tag << 30) if tag else None


def _net(s, nd=None):
    nd = _lib.NetDesc() if nd is None else nd
    nd.n, nd.h, nd.w, nd.prec, nd.skip_flow = s["n"], s["h"], s["w"], s["prec"], s["skip_flow"]
    nd.i0, nd.i1, nd.out, nd.coef, nd.taps = (_ptr(s[k]) for k in ("i0", "i1", "out", "coef", "taps"))
    if s["convs"]:
        nd.convs = C.cast(_CONVS, C.POINTER(_lib.ConvWeights))
    if s["heads"]:
        nd.heads = C.cast(_HEADS, C.POINTER(_lib.HeadWeights))
    nd.workspace, nd.workspace_bytes = _ptr(s["workspace"]), s["workspace_bytes"]
    return nd


def _stack(s, cls):
    v = cls()
    v.y, v.u, v.v = _ptr(s["y"]), _ptr(s["u"]), _ptr(s["v"])
    for k in ("img_stride", "y_pitch", "c_pitch", "c_step", "chroma") + (("depth", "shift") if "depth" in s else ()):
        setattr(v, k, s[k])
    return v


def _coef(lib, depth):
    c = _lib.YuvCoef()
    assert lib.rrin_yuv_coef_std16(_lib.YUV_BT709, 0, depth, C.byref(c)) == 0
    return c


def frame_desc(lib, fmt, s):
    """The descriptor of format fmt ("f32": rrin_net_desc, "unet", or a byte-frame one) from its spec."""
    if fmt == "f32":
        return _net(s["net"])
    if fmt == "unet":
        d = _lib.UNetDesc()
        for k in ("n", "h", "w", "in_ch", "out_ch", "depth", "prec", "workspace_bytes"):
            setattr(d, k, s[k])
        d.x, d.y, d.workspace = _ptr(s["x"]), _ptr(s["y"]), _ptr(s["workspace"])
        d.head.w, d.head.bias = _ptr(s["head_w"]), _ptr(s["head_bias"])
        if s["convs"]:
            d.convs = C.cast(_CONVS, C.POINTER(_lib.ConvWeights))
        return d
    d = {"u8": _lib.NetU8Desc, "yuv": _lib.NetYuvDesc, "u16": _lib.NetU16Desc, "yuv16": _lib.NetYuv16Desc}[fmt]()
    _net(s["net"], d.net)
    d.h0, d.w0 = s["h0"], s["w0"]
    if fmt in ("u8", "u16"):
        d.f0, d.f1, d.img_stride = _ptr(s["f0"]), _ptr(s["f1"]), s["img_stride"]
        setattr(d, "out_" + fmt, _ptr(s["out"]))
        if fmt == "u16":
            d.depth = s["depth"]
    else:
        cls = _lib.Yuv420 if fmt == "yuv" else _lib.Yuv420x16
        d.f0, d.f1, d.out = (_stack(s[k], cls) for k in ("f0", "f1", "out"))
        d.coef = _coef(lib, s["f0"]["depth"] if fmt == "yuv16" else 8)
        if s.get("coef_y0") is not None:
            d.coef.y0 = s["coef_y0"]
    return d


def run_entry(lib, case):
    """One launching entry on the descriptor (and companions) of a case -> its return code."""
    sym, fmt = ENTRIES[case["entry"]]
    s = case["desc"]
    d = None if s is None else frame_desc(lib, fmt, s)
    args = [None if d is None else C.byref(d)]
    kind = case["entry"].split("_")[-1]
    it = fs = pa = None
    if case.get("items") is not None:
        it = _lib.Items(case["items"]["n_pairs"], 0, _ptr(case["items"]["map"]))
    if case.get("fs") is not None:
        f = case["fs"]
        fs = _lib.FlowScale()
        fs.s, fs.workspace, fs.workspace_bytes = f["s"], _ptr(f["workspace"]), f["workspace_bytes"]
        if f["convs"]:
            fs.convs = C.cast(_CONVS, C.POINTER(_lib.ConvWeights))
    if case.get("plane") is not None:
        p = case["plane"]
        pa = _lib.AuxPlane()
        pa.a0, pa.a1, pa.out, pa.scratch = (_ptr(p[k]) for k in ("a0", "a1", "out", "scratch"))
        for k in ("in_stride", "out_stride", "in_pitch", "out_pitch", "depth", "shift", "scratch_bytes"):
            setattr(pa, k, p[k])
    ref = lambda o: None if o is None else C.byref(o)  # noqa: E731
    if kind == "items" or (kind in ("scaled", "plane") and fmt != "f32"):
        args.append(ref(it))
    if kind in ("scaled", "plane"):
        args.append(ref(fs))
    if kind == "plane":
        args.append(ref(pa))
    return getattr(lib, sym)(*args, None)


# ---- the scratch layout with the engine's real tables ------------------------------------------
SCRATCH_SHAPES = ((2, 64, 96), (1, 368, 640), (16, 368, 640), (4, 720, 1280))
UNET_SHAPES = ((1, 64, 96), (1, 368, 640))


def _records(units):
    body, _ = E.unit_convs(units)
    return E.h8_records(body, Net().subpixel_max_level)


def net_records():
    """The record convs of a CPU Net with the stress weights, as the engine packs them."""
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=True), strict=True)
    return _records(E.net_units(net))


def unet_records_by_depth():
    """depth -> the record convs of a UNet(6, 4, depth) alone (its weights do not reach a table)."""
    return {depth: _records([("unet", UNet(6, 4, depth), None)]) for depth in (2, 3, 4, 5)}


@pytest.fixture(scope="module")
def records():
    return net_records()


@pytest.fixture(scope="module")
def unet_records():
    return unet_records_by_depth()


_FUSED = {}


def engine_table(records, prec, size, h, w):
    """The rrin_conv_weights table the engine builds for size class ``size`` at h x w (cfg, ksplit,
    subpixel, fuse_next; fake non-null weight pointers), on the host."""
    t = (_lib.ConvWeights * len(records))()
    if prec == _lib.PREC_F32:  # the planar path has tables of its own; its scratch query reads none
        return t
    geo = E.geom_splits(records, prec, h, w)
    cfgs = E.h8_cfgs(records, prec, size, geo)
    key = (tuple(cfgs), prec)
    if key not in _FUSED:
        _FUSED[key] = [m.fuse_next for m in E.pack_h8_host(records, cfgs, prec)[2]]
    for i, ((k, sub), cfg, fuse) in enumerate(zip(E.h8_splits(records, cfgs, geo, prec), cfgs, _FUSED[key])):
        t[i].cfg, t[i].ksplit, t[i].subpixel, t[i].fuse_next = cfg, k, sub, fuse
        t[i].whi, t[i].bias = 1 << 30, 1 << 30
        if prec == _lib.PREC_F16X3:
            t[i].wlo = 1 << 30
        if sub:
            t[i].wedge, t[i].bias_raw = 1 << 30, 1 << 30
    return t


def run_net_scratch(lib, records, prec, size, n, h, w):
    t = engine_table(records, prec, size, h, w)
    d = _lib.NetDesc()
    d.n, d.h, d.w, d.prec, d.convs = n, h, w, prec, C.cast(t, C.POINTER(_lib.ConvWeights))
    return lib.rrin_net_scratch_bytes(C.byref(d))


def run_unet_scratch(lib, unet_records, size, depth, n, h, w):
    t = engine_table(unet_records[depth], _lib.PREC_F32R, size, h, w)
    d = _lib.UNetDesc()
    d.n, d.h, d.w, d.in_ch, d.out_ch, d.depth, d.prec = n, h, w, 6, 4, depth, _lib.PREC_F32R
    d.convs = C.cast(t, C.POINTER(_lib.ConvWeights))
    return lib.rrin_unet_scratch_bytes(C.byref(d))


# ---- the descriptors of the launching entries ----------------------------------------------------
F32, X3, F16, R32 = PRECS
RECORD = (X3, F16, R32)
WS = GOLD.get("ws", {})  # "n,h,w,prec" -> the recorded rrin_net_workspace_bytes
WS_MISSING = []          # sizes the fixture lacks (recording only): taken from the loaded library


def ws_bytes(n, h, w, prec):
    key = "%d,%d,%d,%d" % (n, h, w, prec)
    if key not in WS:
        WS_MISSING.append(key)
        WS[key] = _lib.lib().rrin_net_workspace_bytes(n, h, w, prec)
    assert WS[key] > 0, key
    return WS[key]


def pad_up(v, m):
    return (v + m - 1) // m * m


def net(n, h, w, prec, f32=False):
    """rrin_net_desc of a frame forward (f32: of rrin_net_fwd), its workspace one byte short."""
    return dict(n=n, h=h, w=w, prec=prec, skip_flow=0, i0=1 if f32 else 0, i1=2 if f32 else 0,
                out=5 if f32 else 0, coef=3, taps=0, convs=1, heads=1, workspace=4,
                workspace_bytes=ws_bytes(n, h, w, prec) - 1)


def stack(h0, w0, chroma, nv12, tag, depth=None):
    cw = w0 if chroma == 2 else w0 // 2
    ch_ = h0 // 2 if chroma == 0 else h0
    step = 2 if nv12 else 1
    s = dict(y=tag, u=tag + 1, v=tag + 2, y_pitch=w0, c_pitch=cw * step, c_step=step, chroma=chroma,
             img_stride=h0 * w0 + 2 * ch_ * cw)
    if depth:
        s.update(depth=depth, shift=0)
    return s


def frame(fmt, n, h0, w0, prec=F16, mult=16, chroma=0, nv12=True, depth=10):
    """A descriptor of format fmt, valid but for its short workspace: n pairs of h0 x w0."""
    if fmt == "f32":
        return {"net": net(n, pad_up(h0, mult), pad_up(w0, mult), prec, f32=True)}
    d = {"net": net(n, pad_up(h0, mult), pad_up(w0, mult), prec), "h0": h0, "w0": w0}
    if fmt in ("u8", "u16"):
        d.update(f0=6, f1=7, out=8, img_stride=h0 * w0 * 3)
        if fmt == "u16":
            d["depth"] = depth
    else:
        dp = depth if fmt == "yuv16" else None
        d.update(f0=stack(h0, w0, chroma, nv12, 10, dp), f1=stack(h0, w0, chroma, nv12, 14, dp),
                 out=stack(h0, w0, chroma, nv12, 18, dp))
    return d


def unet(n=1, h=16, w=16, prec=R32, depth=4):
    return dict(n=n, h=h, w=w, in_ch=6, out_ch=4, depth=depth, prec=prec, x=1, y=2, convs=1, head_w=3,
                head_bias=5, workspace=4, workspace_bytes=ws_bytes(n, h, w, prec) - 1)


def flow_scale(d, s, short=0):
    nd = d["net"]
    return dict(s=s, convs=1, workspace=22,
                workspace_bytes=ws_bytes(nd["n"], nd["h"] // s, nd["w"] // s, nd["prec"]) - short)


def plane(d, depth):
    nd, h0, w0 = d["net"], d["h0"], d["w0"]
    return dict(a0=24, a1=25, out=26, in_stride=h0 * w0, out_stride=h0 * w0, in_pitch=w0, out_pitch=w0, depth=depth,
                shift=0, scratch=27, scratch_bytes=nd["n"] * nd["h"] * nd["w"] * 16)


def depth_of(fmt, d):
    return 8 if fmt in ("u8", "yuv") else d["depth"] if fmt == "u16" else d["f0"]["depth"]


def ch(d, **kw):
    """d with fields changed; "net__h"-style keys reach into a member."""
    d = copy.deepcopy(d)
    for k, v in kw.items():
        o, parts = d, k.split("__")
        for p in parts[:-1]:
            o = o[p]
        o[parts[-1]] = v
    return d


def full(d):
    """d with the whole workspace: only where the second plan's is the short one."""
    return ch(d, net__workspace_bytes=d["net"]["workspace_bytes"] + 1)


def shapes_of(fmt):
    """(name, h0, w0, frame() arguments): the smallest legal frames of the format and an odd size."""
    if fmt in ("u8", "u16"):
        return [("1x1", 1, 1, {}), ("17x33", 17, 33, {})]
    return [("420_2x2", 2, 2, dict(chroma=0)), ("422_1x2", 1, 2, dict(chroma=1, nv12=False)),
            ("444_1x1", 1, 1, dict(chroma=2, nv12=False)), ("444_17x33", 17, 33, dict(chroma=2, nv12=False)),
            ("420_18x34_i420", 18, 34, dict(chroma=0, nv12=False)), ("422_17x34_nv", 17, 34, dict(chroma=1))]


ITEMS = dict(n_pairs=2, map=9)


def accept_cases():
    """Per launching entry: descriptors valid but for a workspace (`low_short`: the second plan's) one
    byte short."""
    out = []

    def acc(entry, name, desc, **companions):
        out.append(dict(entry=entry, name=name, desc=desc, **companions))

    for prec in PRECS:
        acc("net", "p%d_16x16" % prec, frame("f32", 1, 16, 16, prec))
        acc("net", "p%d_n3_48x80" % prec, frame("f32", 3, 48, 80, prec))
    for s in (2, 4):
        for prec in RECORD:
            d = frame("f32", 2, 16 * s, 32 * s, prec)
            acc("net_scaled", "s%d_p%d_main_short" % (s, prec), d, fs=flow_scale(d, s))
            acc("net_scaled", "s%d_p%d_low_short" % (s, prec), full(d), fs=flow_scale(d, s, short=1))
    for depth in (2, 3, 4, 5):
        for prec in PRECS:
            acc("unet", "d%d_p%d" % (depth, prec), unet(prec=prec, depth=depth))
    acc("unet", "n2_48x32_in16_out2", ch(unet(n=2, h=48, w=32), in_ch=16, out_ch=2))
    for fmt in FORMATS:
        for i, (name, h0, w0, kw) in enumerate(shapes_of(fmt)):
            for prec in RECORD:
                acc(fmt, "%s_p%d" % (name, prec), frame(fmt, 1, h0, w0, prec, **kw))
            prec = RECORD[i % 3]  # the other entries: one record precision per shape, in turn
            tag = "%s_p%d" % (name, prec)
            d, d3 = frame(fmt, 1, h0, w0, prec, **kw), frame(fmt, 3, h0, w0, prec, **kw)
            acc(fmt + "_items", tag + "_3of2", d3, items=ITEMS)
            acc(fmt + "_items", tag + "_3of3_nomap", d3, items=dict(n_pairs=3, map=0))
            acc(fmt + "_plane", tag, d, plane=plane(d, depth_of(fmt, d)))
            acc(fmt + "_plane", tag + "_items", d3, items=ITEMS, plane=plane(d3, depth_of(fmt, d3)))
            for s in (2, 4):
                ds = frame(fmt, 1, h0, w0, prec, mult=16 * s, **kw)
                ds3 = frame(fmt, 3, h0, w0, prec, mult=16 * s, **kw)
                pl, pl3 = plane(ds, depth_of(fmt, ds)), plane(ds3, depth_of(fmt, ds3))
                acc(fmt + "_scaled", "%s_s%d_main_short" % (tag, s), ds, fs=flow_scale(ds, s))
                acc(fmt + "_scaled", "%s_s%d_low_short" % (tag, s), full(ds), fs=flow_scale(ds, s, short=1))
                acc(fmt + "_scaled", "%s_s%d_items_main_short" % (tag, s), ds3, items=ITEMS, fs=flow_scale(ds3, s))
                acc(fmt + "_scaled", "%s_s%d_items_low_short" % (tag, s), full(ds3), items=ITEMS,
                    fs=flow_scale(ds3, s, short=1))
                acc(fmt + "_plane", "%s_s%d_scaled" % (tag, s), ds, fs=flow_scale(ds, s), plane=pl)
                if s == 2:
                    acc(fmt + "_plane", "%s_s2_scaled_low_short" % tag, full(ds), fs=flow_scale(ds, s, short=1), plane=pl)
                else:
                    acc(fmt + "_plane", "%s_s4_items_scaled" % tag, ds3, items=ITEMS, fs=flow_scale(ds3, s), plane=pl3)
    return out


def order_cases():
    """Per launching entry: descriptors wrong in two ways at once (on a short workspace, so that none
    can reach a HIP call); the code says which check comes first."""
    out = []

    def dbl(entry, name, desc, **companions):
        out.append(dict(entry=entry, name=name, desc=desc, **companions))

    f = frame("f32", 2, 32, 48, F16)
    dbl("net", "null_i0+bad_shape", ch(f, net__i0=0, net__h=24))
    dbl("net", "bad_shape+bad_prec", ch(f, net__h=24, net__prec=4))
    dbl("net", "bad_prec+short_workspace", ch(f, net__prec=-1))
    dbl("net", "null_workspace+n_0", ch(f, net__workspace=0, net__n=0))
    g = frame("f32", 2, 64, 128, F16)
    dbl("net_scaled", "bad_s+null_workspace", ch(g, net__workspace=0), fs=ch(flow_scale(g, 2), s=3))
    dbl("net_scaled", "planar+bad_shape", ch(g, net__prec=F32, net__h=80), fs=flow_scale(g, 2))
    dbl("net_scaled", "taps+shape_not_16s", ch(g, net__taps=28, net__h=80), fs=flow_scale(g, 4))
    dbl("net_scaled", "shape_not_16s+null_i0", ch(g, net__h=80, net__i0=0), fs=flow_scale(g, 4))
    dbl("net_scaled", "null_fs_convs+n_0", ch(g, net__n=0), fs=ch(flow_scale(g, 2), convs=0))
    dbl("net_scaled", "null_desc+bad_s", None, fs=ch(flow_scale(g, 2), s=5))
    u = unet()
    dbl("unet", "null_x+bad_shape", ch(u, x=0, h=24))
    dbl("unet", "bad_shape+bad_depth", ch(u, w=8, depth=6))
    dbl("unet", "bad_in_ch+bad_prec", ch(u, in_ch=17, prec=4))
    dbl("unet", "bad_prec+short_workspace", ch(u, prec=-1))
    dbl("unet", "null_head_bias+out_ch_5", ch(u, head_bias=0, out_ch=5))
    for fmt in FORMATS:
        rgb = fmt in ("u8", "u16")
        kw = {} if rgb else dict(chroma=0)
        d = frame(fmt, 3, 18, 34, F16, **kw)
        null_f0 = dict(f0=0) if rgb else dict(f0__y=0)
        bad_stride = dict(img_stride=18 * 34 * 3 - 1) if rgb else dict(f1__img_stride=18 * 34 - 1)
        dpt = depth_of(fmt, d)
        dbl(fmt, "null_f0+bad_shape", ch(d, net__h=16, **null_f0))
        dbl(fmt, "planar+bad_frame_size", ch(d, net__prec=F32, h0=0))
        dbl(fmt, "null_coef+planar", ch(d, net__coef=0, net__prec=F32))
        dbl(fmt, "bad_frame_size+padded_mismatch", ch(d, w0=0, net__w=64))
        dbl(fmt, "padded_mismatch+bad_stride", ch(d, net__w=64, **bad_stride))
        dbl(fmt, "bad_stride+short_workspace", ch(d, **bad_stride))
        dbl(fmt, "n_0+null_workspace", ch(d, net__n=0, net__workspace=0))
        dbl(fmt + "_items", "taps+items_n_pairs_0", ch(d, net__taps=28), items=dict(n_pairs=0, map=9))
        dbl(fmt + "_items", "taps+bad_shape", ch(d, net__taps=28, net__h=16), items=ITEMS)
        dbl(fmt + "_items", "n_pairs_gt_n+bad_stride", ch(d, **bad_stride), items=dict(n_pairs=4, map=9))
        dbl(fmt + "_items", "nomap_n_pairs_ne_n+planar", ch(d, net__prec=F32), items=dict(n_pairs=2, map=0))
        dbl(fmt + "_items", "null_items+null_f0", ch(d, **null_f0))
        dbl(fmt + "_items", "null_desc+null_items", None)
        dbl(fmt + "_items", "bad_stride_for_pairs+padded_mismatch", ch(d, net__h=48, **bad_stride), items=ITEMS)
        ds = frame(fmt, 3, 18, 34, F16, mult=32, **kw)
        dbl(fmt + "_scaled", "bad_s+null_workspace", ch(ds, net__workspace=0), fs=ch(flow_scale(ds, 2), s=3))
        dbl(fmt + "_scaled", "taps+items_n_pairs_gt_n", ch(ds, net__taps=28), items=dict(n_pairs=4, map=9),
            fs=flow_scale(ds, 2))
        dbl(fmt + "_scaled", "shape_not_16s+items_n_pairs_0", ch(ds, net__h=48), items=dict(n_pairs=0, map=9),
            fs=flow_scale(ds, 2))
        dbl(fmt + "_scaled", "items_n_pairs_0+null_f0", ch(ds, **null_f0), items=dict(n_pairs=0, map=9),
            fs=flow_scale(ds, 2))
        dbl(fmt + "_scaled", "planar+null_fs_workspace", ch(ds, net__prec=F32), fs=ch(flow_scale(ds, 2), workspace=0))
        dbl(fmt + "_scaled", "padded_to_16_not_32+bad_stride", ch(ds, net__h=64, net__w=64, **bad_stride),
            fs=flow_scale(ds, 2))
        dbl(fmt + "_scaled", "null_desc+null_fs", None)
        dbl(fmt + "_plane", "plane_depth_mismatch+taps", ch(d, net__taps=28), plane=plane(d, dpt + 1))
        dbl(fmt + "_plane", "taps+items", ch(d, net__taps=28), items=ITEMS, plane=plane(d, dpt))
        dbl(fmt + "_plane", "plane_depth_mismatch+null_f0", ch(d, **null_f0), plane=plane(d, dpt + 1))
        dbl(fmt + "_plane", "plane_null_a0+plane_short_scratch", d, plane=ch(plane(d, dpt), a0=0, scratch_bytes=16))
        dbl(fmt + "_plane", "plane_small_pitch+bad_s", ds, fs=ch(flow_scale(ds, 2), s=3),
            plane=ch(plane(ds, dpt), in_pitch=1))
        dbl(fmt + "_plane", "plane_in_stride_for_pairs+n_pairs_gt_n", d, items=dict(n_pairs=4, map=9),
            plane=ch(plane(d, dpt), in_stride=1))
        dbl(fmt + "_plane", "plane_in_stride_for_pairs+short_workspace", d, items=ITEMS,
            plane=ch(plane(d, dpt), in_stride=1))
    return out


def case_id(c):
    return "%s-%s" % (c["entry"], c["name"])


ACCEPT, ORDER = accept_cases(), order_cases()


def test_fixture_covers_every_entry():
    assert len(GOLD["recorded_from"]) == 40 and len(ENTRIES) == 19
    assert not WS_MISSING  # every workspace size of a descriptor is the recorded library's
    for cases in (ACCEPT, ORDER):
        assert {c["entry"] for c in cases} == set(ENTRIES)
        assert len({case_id(c) for c in cases}) == len(cases)
    assert GOLD["accept"] == {"count": len(ACCEPT), "ret": E_WORKSPACE}
    assert sorted(GOLD["order"]) == sorted(case_id(c) for c in ORDER)
    assert len(GOLD["workspace"]) == 3 * 7 * 4 + 5
    # the double faults return more than one code: the order of the checks is what they pin
    assert set(GOLD["order"].values()) >= {-1, -2}


def test_workspace_bytes():
    lib = _lib.lib()
    for n, h, w, prec, want in GOLD["workspace"]:
        assert lib.rrin_net_workspace_bytes(n, h, w, prec) == want, (n, h, w, prec)
    for key, want in GOLD["ws"].items():
        assert lib.rrin_net_workspace_bytes(*map(int, key.split(","))) == want, key


@pytest.mark.parametrize("prec", PRECS)
def test_net_scratch_bytes_of_the_engine_tables(records, prec):
    lib = _lib.lib()
    got = [[size, n, h, w, run_net_scratch(lib, records, prec, size, n, h, w)]
           for size in E.WINO_SIZES for n, h, w in SCRATCH_SHAPES]
    want = GOLD["net_scratch"][str(prec)]
    assert got == want
    if prec != _lib.PREC_F32R:
        assert all(c[4] == 0 for c in want)
    else:
        assert any(c[4] > 0 for c in want)


def test_unet_scratch_bytes_of_the_engine_tables(unet_records):
    lib = _lib.lib()
    got = [[size, depth, n, h, w, run_unet_scratch(lib, unet_records, size, depth, n, h, w)]
           for size in ("small", "large") for depth in (2, 3, 4, 5) for n, h, w in UNET_SHAPES]
    assert got == GOLD["unet_scratch"]


@pytest.mark.parametrize("case", ACCEPT, ids=case_id)
def test_entries_accept_up_to_the_workspace_check(case):
    assert GOLD["accept"]["ret"] == E_WORKSPACE
    assert run_entry(_lib.lib(), case) == E_WORKSPACE


@pytest.mark.parametrize("case", ORDER, ids=case_id)
def test_check_order_of_double_faults(case):
    want = GOLD["order"][case_id(case)]
    assert want < 0  # an RRIN_E_*: the recorded library returned before its first HIP call
    assert run_entry(_lib.lib(), case) == want


