"""CPU: the extra plane of the byte-frame forwards (rrin_amd/plane.py) -- the definition against a
literal restatement of the reference forward with a fourth channel, the byte mappings against the byte
paths' own, the argument refusals of the Python layer and of the C ABI (all returned before any launch),
the ctypes structure against the header, and the folder pipeline's refusal on the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_net
from rrin_amd import Net, _lib
from rrin_amd import convert as cv
from rrin_amd import plane as P
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rrin_hip.h")
E_SHAPE, E_ARG = -1, -2


@pytest.fixture(scope="module")
def oracle_case():
    """One oracle forward per t on 2 x 3 x 32 x 48 frames, shared and left unchanged."""
    sd = keyed_state_dict(Net().state_dict(), stress=True)
    i0, i1 = synthetic_batch(2, 32, 48)
    g = torch.Generator().manual_seed(5)
    a0, a1 = torch.rand(2, 1, 32, 48, generator=g), torch.rand(2, 1, 32, 48, generator=g)
    out = {}
    for t in (0.5, 0.25):
        taps = {}
        with torch.no_grad():
            ref_net.net_forward(sd, i0, i1, t, taps)
        out[t] = taps
    return i0, i1, a0, a1, out


@pytest.mark.parametrize("t", [0.5, 0.25])
def test_definition_is_the_forward_with_a_fourth_channel(oracle_case, t):
    """model.py:46-55 restated literally on (I0 | A0) and (I1 | A1): channels 0-2 are the oracle's own blend,
    channel 3, clamped, is plane.reference on the oracle's flows and logits within the fp32 forward's own
    error (1e-5: the warp's 7.3e-6 plus the blend's 2.9e-7 of tests/glue_ref.py, rounded up)."""
    i0, i1, a0, a1, taps = oracle_case
    tp = taps[t]
    xt1 = ref_net.warp(torch.cat((i0, a0), 1), tp["ft0"])
    xt2 = ref_net.warp(torch.cat((i1, a1), 1), tp["ft1"])
    m = torch.sigmoid(tp["mask_logits"])
    w1, w2 = (1 - t) * m[:, 0:1], t * m[:, 1:2]
    out4 = (w1 * xt1 + w2 * xt2) / (w1 + w2 + 1e-8)
    assert torch.equal(out4[:, 0:3], tp["blend"])
    want = out4[:, 3:4].clamp(0, 1)
    got = P.reference(tp, a0, a1, t)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want.double()).abs().max()) <= 1e-5
    assert float(got.max()) > 0.5
    # from the raw outputs of the two U-Nets, as Net.forward(taps=) names them
    raw = {"Flow": tp["Flow"], "refine_flow": tp["refine"], "Mask": tp["mask_logits"]}
    assert float((P.reference(raw, a0, a1, t) - got).abs().max()) <= 1e-5
    per_image = P.reference(tp, a0, a1, [t, t])
    assert torch.equal(per_image, got)


@pytest.mark.parametrize("flow_scale", [1, 2])
def test_byte_mappings_are_the_byte_paths_on_one_channel(flow_scale):
    rng = np.random.default_rng(3)
    h0, w0 = 17, 33
    a = torch.from_numpy(rng.integers(0, 256, (2, h0, w0), dtype=np.uint8))
    grey = a.unsqueeze(-1).expand(2, h0, w0, 3)
    f = P.plane_to_float(a, flow_scale=flow_scale)
    assert torch.equal(f, cv.frames_u8_to_float(grey, flow_scale)[:, 0:1])
    q = torch.rand(2, 1, f.shape[-2], f.shape[-1])
    assert torch.equal(P.float_to_plane(q, h0, w0), cv.frames_float_to_u8(q.expand(2, 3, -1, -1), h0, w0)[..., 0])
    w = torch.from_numpy(rng.integers(0, 1 << 16, (2, h0, w0)).astype(np.uint16).view(np.int16)).view(torch.uint16)
    g16 = torch.stack([w.view(torch.int16)] * 3, -1).view(torch.uint16)
    assert torch.equal(P.plane_to_float(w, 10, 0, flow_scale), cv.frames_u16_to_float(g16, 10, flow_scale)[:, 0:1])
    got = P.float_to_plane(q, h0, w0, 10, 0)
    want = cv.frames_float_to_u16(q.expand(2, 3, -1, -1), h0, w0, 10)[..., 0]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the sample in the high bits: read >> shift, stored << shift
    s6 = P.samples(w, 10, 6)
    assert torch.equal(s6, ((w.view(torch.int16).to(torch.int32) & 0xFFFF) >> 6))
    back = P.float_to_plane(P.plane_to_float(w, 10, 6), h0, w0, 10, 6)
    assert torch.equal((back.view(torch.int16).to(torch.int32) & 0xFFFF), s6 << 6)


def test_python_refusals():
    a = torch.zeros((2, 16, 16), dtype=torch.uint8)
    cpu = torch.device("cpu")
    assert P.check_planes((a, a), 2, 16, 16, torch.uint8, cpu, False)[0] is a
    assert P.check_planes(torch.zeros((3, 16, 16), dtype=torch.uint8), 2, 16, 16, torch.uint8, cpu, True)[1].shape[0] == 2
    for bad in (a, (a,), (a, a, a), (a, None), None.__class__):
        with pytest.raises(TypeError):
            P.check_planes(bad, 2, 16, 16, torch.uint8, cpu, False)
    with pytest.raises(TypeError):
        P.check_planes((a, a), 2, 16, 16, torch.uint16, cpu, False)
    with pytest.raises(TypeError):
        P.check_planes((a, a), 2, 16, 16, torch.uint8, cpu, True)
    for shape in ((1, 16, 16), (2, 8, 16), (2, 16, 16, 1)):
        with pytest.raises(ValueError):
            P.check_planes((a, torch.zeros(shape, dtype=torch.uint8)), 2, 16, 16, torch.uint8, cpu, False)
    with pytest.raises(ValueError):
        P.check_planes(a, 2, 16, 16, torch.uint8, cpu, True)  # [P+1] frames wanted
    for depth, shift in ((7, 0), (17, 0), (8, 1), (10, 7), (True, 0), (10, -1)):
        with pytest.raises(ValueError):
            P.check_format(depth, shift)
    with pytest.raises(TypeError):
        P.samples(a, 10, 0)


def header_struct(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_lib_structure_matches_the_header():
    ctype_of = {"const void*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
    want = [(n, ctype_of[t]) for n, t in header_struct("rrin_aux_plane")]
    assert [(n, t) for n, t in _lib.AuxPlane._fields_] == want
    assert C.sizeof(_lib.AuxPlane) == 72  # 3 pointers, 2 int64, 4 int32, a pointer, an int64: no padding
    lib = _lib.lib()
    new = ["rrin_plane_scratch_bytes", "rrin_plane_warp_h8", "rrin_plane_blend_h8"] + [
        f"rrin_net_{p}_plane_fwd" for p in ("u8", "u16", "yuv", "yuv16")]
    for name in new:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.rrin_abi_version() == 25
    assert lib.rrin_plane_scratch_bytes(2, 32, 48) == 2 * 32 * 48 * 16
    assert lib.rrin_plane_scratch_bytes(2, 0, 48) == E_SHAPE


def test_abi_refusals_come_before_any_launch():
    """rrin_net_u8_plane_fwd on a descriptor of made-up addresses: every refusal below is decided on the
    host, so nothing is dereferenced.  (A call that would pass is never made here.)"""
    lib = _lib.lib()
    fake = 1 << 30
    n, h0, w0, h, w = 2, 17, 33, 32, 48
    convs, heads = (_lib.ConvWeights * 1)(), (_lib.HeadWeights * 1)()

    def desc(prec=_lib.PREC_F32R, taps=None):
        d = _lib.NetU8Desc()
        d.f0, d.f1, d.out_u8, d.img_stride, d.h0, d.w0 = fake, fake, fake, h0 * w0 * 3, h0, w0
        nd = d.net
        nd.n, nd.h, nd.w, nd.prec, nd.taps = n, h, w, prec, taps
        nd.coef, nd.workspace, nd.workspace_bytes = fake, fake, 0
        nd.convs, nd.heads = convs, heads
        return d

    def plane(**kw):
        ap = _lib.AuxPlane()
        ap.a0, ap.a1, ap.out, ap.scratch = fake, fake, fake, fake
        ap.in_stride = ap.out_stride = h0 * w0
        ap.in_pitch = ap.out_pitch = w0
        ap.depth, ap.shift, ap.scratch_bytes = 8, 0, 16 * n * h * w
        for k, v in kw.items():
            setattr(ap, k, v)
        return ap

    def call(d, ap):
        return lib.rrin_net_u8_plane_fwd(C.byref(d), None, None, C.byref(ap), None)

    assert call(desc(prec=_lib.PREC_F32), plane()) == E_ARG           # the planar precision
    assert call(desc(), plane(depth=10)) == E_ARG                     # not the frames' depth
    assert call(desc(), plane(in_stride=h0 * w0 - 1)) == E_ARG        # overlapping input frames
    assert call(desc(), plane(out_stride=h0 * w0 - 1)) == E_ARG       # overlapping output frames
    assert call(desc(), plane(in_pitch=w0 - 1)) == E_ARG
    assert call(desc(taps=fake), plane()) == E_ARG                    # taps
    assert call(desc(), plane(scratch=None)) == E_ARG
    assert call(desc(), plane(scratch_bytes=16 * n * h * w - 1)) == E_ARG
    # with every companion NULL the entry is rrin_net_u8_fwd: the same code for the same bad descriptor
    bad = desc()
    bad.net.h = h + 16
    assert lib.rrin_net_u8_plane_fwd(C.byref(bad), None, None, None, None) == lib.rrin_net_u8_fwd(C.byref(bad), None) == E_SHAPE
    d16 = _lib.NetU16Desc()
    assert lib.rrin_net_u16_plane_fwd(C.byref(d16), None, None, C.byref(plane()), None) == E_ARG
    assert lib.rrin_plane_warp_h8(None, C.byref(plane()), n, h0, w0, None, n, _lib.PREC_F32R, None) == E_ARG


def test_folder_alpha_needs_the_byte_pipeline(tmp_path):
    """alpha=True on the CPU (no device, so no byte pipeline) and with u8=False raises the documented
    ValueError before any frame is read or written; world > 1 too."""
    from PIL import Image
    src, dest = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(1)
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, (16, 16, 4), dtype=np.uint8), "RGBA").save(src / f"{k:03d}.png")

    class Model:
        def interpolate(self, i0, i1, ts):
            return [(i0 + i1) / 2 for _ in ts]

        def interpolate_u8(self, f0, f1, ts, **kw):
            raise AssertionError("not reached")

    for kw in ({}, {"u8": False}, {"u8": True, "world": 2}):
        with pytest.raises(ValueError, match="alpha"):
            cv.interpolate_folder(Model(), str(src), str(dest), 1, alpha=True, **kw)
    assert not dest.exists()
    # the RGBA loader: the file's alpha, or 255 for a file without one
    t, meta = cv.load_frame_rgba(str(src / "000.png"))
    assert tuple(t.shape) == (16, 16, 4) and meta["out_filetype"] == ".png"
    Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), "RGB").save(src / "rgb.png")
    t, _ = cv.load_frame_rgba(str(src / "rgb.png"))
    assert bool((t[..., 3] == 255).all())
    # and without the flag the float pipeline still runs and writes RGB
    assert cv.interpolate_folder(Model(), str(src), str(dest), 1, log=lambda *_: None) > 0
