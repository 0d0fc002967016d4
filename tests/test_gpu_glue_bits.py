"""GPU: every non-conv kernel of the record path (rrin_amd/csrc/glue_h8.hip) bit for bit against
digests recorded before the kernels were unified over the record formats (rec_fmt.hpp).

tests/golden/glue_bits.json holds, per case and record precision, the SHA-256 of everything the
call may write: the destination's raw storage taken whole -- both planes, padding, the groups
outside the view and the guard bands of record_ref.GuardedH8 -- and for the heads also raw_out,
out / out_u8 / the 4:2:0 planes, the kept raw flow and the range flag.  The other GPU tests say what
the right values are; this one says that none of those bytes moved.  Inputs are seeded, at
glue_ref.SHAPES (8-bit frames: 5 rows and 7 columns smaller, so narrower than the padded width;
rrin_unet_fwd, which alone reaches clear_channels: the two shapes that are multiples of 16).

    python3 -m tests.test_gpu_glue_bits OUT.json    records the digests with the loaded library
"""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

from rrin_amd import _lib
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from tests import glue_ref as G
from tests import hip_helpers as H
from tests import record_ref as R

pytestmark = pytest.mark.gpu
PREC = {"R32": _lib.PREC_F32R, "F16X3": _lib.PREC_F16X3, "F16": _lib.PREC_F16}
PRECISION = {"R32": "fp32", "F16X3": "fp32_split16", "F16": "fp16"}
MODE = {"plain": _lib.HEAD_PLAIN, "flow": _lib.HEAD_FLOW, "refine": _lib.HEAD_REFINE, "mask": _lib.HEAD_MASK,
        "final": _lib.HEAD_FINAL}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue_bits.json")


def digest(*parts):
    """SHA-256 of the bytes of tensors / guarded storage, in order."""
    sha = hashlib.sha256()
    for p in parts:
        for t in (p.raw if isinstance(p, R.GuardedH8) else [p]):
            sha.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return sha.hexdigest()


def coef(n, dev):
    return t_coefficients(torch.tensor(G.T_PER_IMAGE[:n]), n).to(dev)


def net_buffer(dev, prec, n, h, w, seed=1):
    """g16 in guarded storage: pattern everywhere, then the frames of glue_ref.case in channels 0-5."""
    c = G.case(n, h, w)
    g = R.GuardedH8(n, G.G16_CHANNELS, h, w, dev, prec, seed=seed)
    g.load(c["x0"].to(dev), 0)
    g.load(c["x1"].to(dev), 3)
    return g, c


# ---- the cases: name -> fn(dev, prec, n, h, w) -> digest -------------------------------------------
def up2x(dev, prec, n, h, w):
    """Groups 1-2 of a 4-group source into groups 2-3 of a 6-group destination."""
    cpr = _lib.chans_per_record(prec)
    src = R.GuardedH8(n, 4 * cpr, h // 2, w // 2, dev, prec, seed=11)
    dst = R.GuardedH8(n, 6 * cpr, h, w, dev, prec, seed=12)
    sv, dv = src.view(cpr, 2 * cpr), dst.view(2 * cpr, 2 * cpr)
    _lib.check(_lib.lib().rrin_upsample2x_h8(C.byref(sv), C.byref(dv), n, prec, H.stream(dev)))
    return digest(dst, src)


def nchw_to_records(dev, prec, n, h, w):
    t = R.GuardedH8(n, 24, h, w, dev, prec, seed=13)
    t.load((G.pattern((n, 11, h, w), 14) * 37).to(dev), 3)
    return digest(t)


def records_to_nchw(dev, prec, n, h, w):
    t = R.GuardedH8(n, 24, h, w, dev, prec, seed=15)
    return digest(t.to_nchw(3, 11), t)


def pack_g16(dev, prec, n, h, w):
    t = R.GuardedH8(n, 24, h, w, dev, prec, seed=16)
    i0, i1 = (G.pattern((n, 3, h, w), s).abs().mul(0.5).to(dev) for s in (17, 18))
    v = t.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_h8(i0.data_ptr(), i1.data_ptr(), n, C.byref(v), prec, H.stream(dev)))
    return digest(t)


def pack_g16_u8(dev, prec, n, h, w):
    """Frames of (h - 5) x (w - 7) into the g16 of their padded size."""
    h0, w0 = h - 5, w - 7
    t = R.GuardedH8(n, 24, (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16, dev, prec, seed=19)
    gen = torch.Generator().manual_seed(20)
    f0, f1 = (torch.randint(0, 256, (n, h0, w0, 3), generator=gen, dtype=torch.uint8).to(dev) for _ in range(2))
    v = t.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_u8_h8(f0.data_ptr(), f1.data_ptr(), h0 * w0 * 3, n, h0, w0, C.byref(v), prec,
                                              H.stream(dev)))
    return digest(t)


def tblend(dev, prec, n, h, w):
    g, _ = net_buffer(dev, prec, n, h, w, seed=21)
    fr = R.GuardedH8(n, 4, h, w, dev, prec, seed=22)
    frv, gv, cf = fr.view(0, 4), g.view(0, g.c), coef(n, dev)
    _lib.check(_lib.lib().rrin_flow_tblend_h8(C.byref(frv), C.byref(gv), cf.data_ptr(), n, prec, H.stream(dev)))
    return digest(g, fr)


def head(stage, scale=1.0, cout=None, out=None):
    """One rrin_head_h8_fwd case.  out: None, "f32", "u8" (a crop with top > 0, w0 < w), "nv12", "i420"."""

    def run(dev, prec, n, h, w):
        g, c = net_buffer(dev, prec, n, h, w)
        wt, b = G.keyed_head("flow" if stage == "plain" else stage, scale)
        wt, b = wt[:cout], b[:cout]
        src = H8Tensor.from_nchw(c["flow" if stage == "plain" else stage].to(dev), prec)
        raw = torch.full((n, wt.shape[0], h, w), float("nan"), device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _lib.HeadH8Desc()
        d.n, d.cin, d.cout, d.mode, d.prec = n, 32, wt.shape[0], MODE[stage], prec
        d.src, d.g16 = src.view(0, 32), g.view(0, g.c)
        wd, bd, cf = wt.contiguous().to(dev), b.contiguous().to(dev), coef(n, dev)
        d.w, d.bias, d.coef, d.raw_out, d.status = wd.data_ptr(), bd.data_ptr(), cf.data_ptr(), raw.data_ptr(), status.data_ptr()
        outs = [raw, status]
        if stage == "flow":
            fr = R.GuardedH8(n, 4, h, w, dev, prec, seed=7)
            d.flow_raw = fr.view(0, 4)
            outs.append(fr)
        if out == "f32":
            outs.append(torch.full((n, 3, h, w), float("nan"), device=dev))
            d.out = outs[-1].data_ptr()
        elif out == "u8":
            d.h0, d.w0, d.top = h - 5, w - 7, 5
            outs.append(torch.full((n, d.h0, d.w0, 3), 0xA5, dtype=torch.uint8, device=dev))
            d.out_u8 = outs[-1].data_ptr()
        elif out is not None:
            d.h0, d.w0, d.top = h - 6, w - 8, 6
            planes = [torch.full((n, d.h0 * d.w0), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
            o = d.out_yuv
            o.y, o.u, o.img_stride, o.y_pitch = planes[0].data_ptr(), planes[1].data_ptr(), d.h0 * d.w0, d.w0
            if out == "nv12":
                o.v, o.c_pitch, o.c_step = planes[1].data_ptr() + 1, d.w0, 2
            else:
                o.v, o.c_pitch, o.c_step = planes[2].data_ptr(), d.w0 // 2, 1
            from rrin_amd import yuv
            d.yuv_coef = _lib.YuvCoef(*yuv.coefficients())
            outs += planes
        _lib.check(_lib.lib().rrin_head_h8_fwd(C.byref(d), H.stream(dev)), "rrin_head_h8_fwd")
        return digest(g, src.hi, *outs)

    return run


def clear_channels(dev, prec, n, h, w):
    """rrin_unet_fwd of a 1 -> 4 channel U-Net, twice: the second call clears channels 1-3, which
    the first call's PLAIN head wrote (a range that starts inside a record).  Both outputs and
    the whole workspace."""
    from rrin_amd import UNet
    from rrin_amd.synthetic import keyed_state_dict
    net = UNet(1, 4, depth=2)
    net.load_state_dict(keyed_state_dict(net.state_dict()))
    net = net.to(dev).eval()
    net.precision = PRECISION[{v: k for k, v in PREC.items()}[prec]]
    gen = torch.Generator().manual_seed(23)
    with torch.no_grad():
        ys = [net(torch.rand(n, 1, h, w, generator=gen).to(dev)).clone() for _ in range(2)]
    return digest(*ys, net._hip_engine().workspace(n, h, w, slot=100))


CASES = {"up2x": up2x, "nchw_to_records": nchw_to_records, "records_to_nchw": records_to_nchw, "pack_g16": pack_g16,
         "pack_g16_u8": pack_g16_u8, "tblend": tblend, "clear_channels": clear_channels,
         "head_plain2": head("plain", cout=2), "head_plain3": head("plain", cout=3), "head_plain4": head("plain", cout=4),
         "head_mask": head("mask")}
for _s in G.SCALES:
    CASES[f"head_flow_x{_s:g}"] = head("flow", _s)
    CASES[f"head_refine_x{_s:g}"] = head("refine", _s)
for _o in ("f32", "u8", "nv12", "i420"):
    CASES[f"head_final_{_o}"] = head("final", out=_o)


def shapes(name):
    return [s for s in G.SHAPES if name != "clear_channels" or s[1] % 16 == 0]


def run(name, dev, prec, n, h, w):
    d = CASES[name](dev, PREC[prec], n, h, w)
    torch.cuda.synchronize(dev)
    return d


def key(name, prec, n, h, w):
    return f"{name}/{prec}/{n}x{h}x{w}"


ALL = [(name, prec, *s) for name in CASES for prec in G.PRECS for s in shapes(name)]


@pytest.mark.parametrize("name,prec,n,h,w", ALL, ids=[key(*a) for a in ALL])
def test_bits(gpu, name, prec, n, h, w):
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"][key(name, prec, n, h, w)]
    assert run(name, gpu, prec, n, h, w) == want


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    got = {key(*a): run(a[0], dev, *a[1:]) for a in ALL}
    again = {key(*a): run(a[0], dev, *a[1:]) for a in ALL}
    moved = [k for k in got if got[k] != again[k]]
    print(f"{len(got)} digests, {len(moved)} differ between two runs: {moved}")
    with open(sys.argv[1], "w") as f:
        json.dump({"sha256": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    sys.exit(1 if moved else 0)
