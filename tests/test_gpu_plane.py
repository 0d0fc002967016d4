"""GPU: the extra plane of the byte-frame forwards (rrin_amd/plane.py is the definition).

Kernels alone through the C ABI -- rrin_plane_warp_h8 on Net buffers whose channels 6-9 hold flows the
test chose, rrin_plane_blend_h8 on a scratch the test filled -- in the three record precisions and at
uint8, uint16 depth 10 shift 6, depth 16 shift 0 (and depth 10 shift 0, the only one of these formats in
which a word can lie above maxval).  Then the whole forward with ``plane=`` on the four frame paths.

Tolerances are not new numbers.  The warp is held to glue_ref.A_WARP, what tests/test_gpu_glue.py grants
REFINE's warped channels (the scratch is fp32: no storage rounding term), against float64 over the flows
decoded from the stored record bits.  The blend is held to glue_ref.A_MASK = eps on the float value,
which on the stored code reads: at most 1 code from trunc(ref * maxval) everywhere, and equal wherever
ref * maxval lies farther than eps * maxval from an integer; that exact class is asserted to be at least
half of the samples.  The whole forward adds the two: eps = A_WARP + A_MASK, since the blend is a convex
combination of the two warped values (weights w1 / den + w2 / den <= 1), so a warp error passes through
it undiminished at most."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib
from rrin_amd import convert as cv
from rrin_amd import plane as P
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from rrin_amd.synthetic import keyed_state_dict
from tests import glue_ref as G
from tests import hip_helpers as H

pytestmark = pytest.mark.gpu
PREC = {"R32": _lib.PREC_F32R, "F16X3": _lib.PREC_F16X3, "F16": _lib.PREC_F16}
FORMATS = [(8, 0), (10, 6), (16, 0), (10, 0)]
FMT_IDS = [f"d{d}s{s}" for d, s in FORMATS]
E_SHAPE, E_ARG = -1, -2


def np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def i32(x):
    """The words of a uint8 / uint16 tensor as int32."""
    return x.to(torch.int32) if x.dtype == torch.uint8 else x.view(torch.int16).to(torch.int32) & 0xFFFF


def flip0(x):
    return x.flip(0) if x.dtype == torch.uint8 else x.view(torch.int16).flip(0).view(torch.uint16)


def as_torch(a):
    """numpy uint8 / uint16 -> torch of the same bits."""
    return torch.from_numpy(a) if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).view(torch.uint16)


def plane_data(n, h0, w0, depth, shift, seed):
    """[n,h0,w0] words: random samples << shift with junk in the low bits, and 0, maxval and (where the
    format has room) a word above maxval at fixed places."""
    rng = np.random.default_rng(seed)
    maxval = (1 << depth) - 1
    a = rng.integers(0, maxval + 1, (n, h0, w0)).astype(np.int64) << shift
    if shift:
        a |= rng.integers(0, 1 << shift, a.shape)
    a[:, 0, 0], a[:, 0, 1], a[:, -1, -1], a[:, -1, 0] = 0, maxval << shift, maxval << shift, 0
    if depth + shift < 16:
        a[:, 1, 1] = 0xFFFF  # above maxval: reads as maxval
        a[:, h0 // 2, w0 // 2] = maxval + 1
    return as_torch(a.astype(np_dtype(depth)))


def strided(stack, gap, fill, dev):
    """The frames of ``stack`` [n, ...] in a device buffer with ``gap`` elements between frames: (view, buffer)."""
    n, flen = stack.shape[0], stack[0].numel()
    buf = torch.empty((n, flen + gap), dtype=torch.int16 if stack.dtype == torch.uint16 else stack.dtype)
    buf.fill_(fill)
    buf = buf.view(stack.dtype).to(dev)
    view = buf[:, :flen].view(stack.shape)
    raw = (lambda x: x) if stack.dtype == torch.uint8 else (lambda x: x.view(torch.int16))
    raw(view).copy_(raw(stack.to(dev)))
    return view, buf


def aux_plane(a0, a1, out, in_stride, out_stride, in_pitch, out_pitch, depth, shift, scratch):
    ap = _lib.AuxPlane()
    ap.a0, ap.a1, ap.out = a0.data_ptr(), a1.data_ptr(), out.data_ptr()
    ap.in_stride, ap.out_stride, ap.in_pitch, ap.out_pitch = in_stride, out_stride, in_pitch, out_pitch
    ap.depth, ap.shift = depth, shift
    ap.scratch, ap.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    return ap


def make_flows(n, h, w, h0, w0):
    """[n,4,h,w] flows (Ft0 u, v, Ft1 u, v).  The warp samples padded position (x + u - 0.5, y + v - 0.5).
    Background: multiples of 0.5 in [-3, 3] (zero, integers, +-0.5) on half of the pixels, general values
    on the rest; then, at fixed pixels of every image: positions exactly on the padded border and one
    step outside it, +-1e4, and pulls into the replicated padding (rows above ``top``, columns >= w0)."""
    g = torch.Generator().manual_seed(101 * h + w)
    grid = torch.randint(-6, 7, (n, 4, h, w), generator=g).float() * 0.5
    free = torch.randn(n, 4, h, w, generator=g) * 2.5
    f = torch.where(torch.rand(n, 1, h, w, generator=g) < 0.5, grid, free)
    top = h - h0
    special = [
        (0, 0, 0.0, 0.0), (1, 2, 0.5, -0.5), (2, 3, 1.0, 2.0),
        (3, 5, -5 + 0.5, 0.5),                # ix = 0 exactly
        (3, 6, -6 - 0.5, 0.5),                # ix = -1 exactly: one tap column outside, weight 0 inside
        (4, 5, (w - 1) - 5 + 0.5, 0.5),       # ix = w - 1 exactly
        (4, 6, w - 6 + 0.5, 0.5),             # ix = w: both tap columns outside
        (5, 1, 0.5, -5 + 0.5),                # iy = 0 exactly
        (5, 2, 0.5, (h - 1) - 5 + 0.5),       # iy = h - 1 exactly
        (6, 1, 1e4, 0.0), (6, 2, 0.0, -1e4), (6, 3, -1e4, 1e4),
        (h - 1, 0, (w - 1) + 0.25, -(h - 1) + 0.25),   # into the top-right corner of the padding
        (h - 2, 1, float(max(w0 - 1, 0)) + 0.75, -float(h - 2) + max(top - 1, 0) + 0.75),
    ]
    for y, x, u, v in special:
        f[:, 0, y, x], f[:, 1, y, x] = u, v
        f[:, 2, y, x], f[:, 3, y, x] = u, v
    return f


@pytest.mark.parametrize("depth,shift", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("h0,w0", [(17, 33), (16, 16)])
@pytest.mark.parametrize("prec", G.PRECS)
def test_warp_kernel(gpu, prec, h0, w0, depth, shift):
    """rrin_plane_warp_h8 against float64 over the stored flows, every padded pixel within A_WARP; the
    logits half of the scratch, the planes and the gaps between their frames stay bit for bit; two runs
    give the same bits; with a map image k reads frame map[k]."""
    lib, n, pr = _lib.lib(), 2, PREC[prec]
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    g16 = H8Tensor(n, G.G16_CHANNELS, h, w, gpu, pr)
    for k, a in enumerate([g16.hi] + ([g16.lo] if g16.lo is not None else [])):
        a.copy_(G.pattern(a.shape, 3 + k, a.dtype))
    g16.load(make_flows(n, h, w, h0, w0).to(gpu), 6)
    flows = g16.to_nchw(6, 4).cpu()  # as the record bits decode
    p0, p1 = plane_data(n, h0, w0, depth, shift, 1), plane_data(n, h0, w0, depth, shift, 2)
    gap = 7
    a0, b0 = strided(p0, gap, 0x5A, gpu)
    a1, b1 = strided(p1, gap, 0x5A, gpu)
    snap = (b0.clone(), b1.clone())
    out = torch.zeros((n, h0, w0), dtype=p0.dtype, device=gpu)
    view = g16.view(0, g16.c)
    hw = h * w

    def run(map_=None):
        sc = torch.full((4 * n * hw,), float("nan"), device=gpu)
        ap = aux_plane(a0, a1, out, h0 * w0 + gap, h0 * w0, w0, w0, depth, shift, sc)
        rc = lib.rrin_plane_warp_h8(C.byref(view), C.byref(ap), n, h0, w0, map_.data_ptr() if map_ is not None else None,
                                    n, pr, H.stream(gpu))
        torch.cuda.synchronize(gpu)
        assert rc == 0, rc
        return sc.cpu()

    sc = run()
    assert bool(torch.isnan(sc[2 * n * hw:]).all()), "the logits half of the scratch was written"
    got = sc[:2 * n * hw].view(n, 2, h, w)
    ref = torch.cat([P.warp(P.plane_to_float(p0, depth, shift).double(), flows[:, 0:2]),
                     P.warp(P.plane_to_float(p1, depth, shift).double(), flows[:, 2:4])], 1)
    assert float(ref.max()) > 0.9 and bool((ref == 0).any())
    err = (got.double() - ref).abs()
    print(f"warp {prec} {h0}x{w0} d{depth}s{shift}: max err {float(err.max()):.3e} (limit {G.A_WARP:.1e})")
    assert bool((err <= G.A_WARP).all()), f"{int((err > G.A_WARP).sum())} of {err.numel()} past A_WARP"
    assert torch.equal(sc.view(torch.int32), run().view(torch.int32)), "two runs differ"
    assert torch.equal(b0.view(torch.uint8), snap[0].view(torch.uint8)) and torch.equal(
        b1.view(torch.uint8), snap[1].view(torch.uint8)), "an input plane changed"
    # items: image 0 reads frame 1, image 1 frame 0 (and a map entry past the pairs is clamped)
    m = torch.tensor([1, -3], dtype=torch.int32, device=gpu)
    swapped = run(m)[:2 * n * hw].view(n, 2, h, w)
    ref_sw = torch.cat([P.warp(P.plane_to_float(flip0(p0), depth, shift).double(), flows[:, 0:2]),
                        P.warp(P.plane_to_float(flip0(p1), depth, shift).double(), flows[:, 2:4])], 1)
    assert bool(((swapped.double() - ref_sw).abs() <= G.A_WARP).all()), "pair_map"


def blend_inputs(n, h, w, seed):
    """at [n,2,h,w] in [0, 1] with exact 0 and 1, logits [n,2,h,w]: normal * 3 with 0, +-100 and +-1e4
    (the sigmoid saturates, expf overflows) and +-87 (the largest without an infinity) at fixed places."""
    g = torch.Generator().manual_seed(seed)
    at = torch.rand(n, 2, h, w, generator=g)
    lg = torch.randn(n, 2, h, w, generator=g) * 3
    row = h - 2  # a row of the crop
    for x, (l0, l1) in enumerate([(0, 0), (100, -100), (-100, 100), (-100, -100), (100, 100), (1e4, -1e4),
                                  (-1e4, -1e4), (87, -87), (-87, 87), (-87, -87)]):
        lg[:, 0, row, x], lg[:, 1, row, x] = l0, l1
    at[:, :, h - 1, 0], at[:, :, h - 1, 1], at[:, 0, h - 1, 2], at[:, 1, h - 1, 2] = 0.0, 1.0, 1.0, 0.0
    return at, lg


def code_check(got, ref, maxval, shift, eps, what):
    """The stored codes against the float64 value ``ref`` in [0, 1] under the +-1 / exact-class rule."""
    code = i32(got) >> shift
    assert bool(((i32(got) & ((1 << shift) - 1)) == 0).all()), f"{what}: bits below the shift"
    x = ref * maxval
    want = x.floor().to(torch.int32)
    exact = (x - x.round()).abs() > eps * maxval
    share = float(exact.float().mean())
    off = (code - want).abs()
    print(f"{what}: exact class {share:.3f}, max |code - ref code| {int(off.max())}, "
          f"mismatches in the exact class {int((off[exact] != 0).sum())}")
    assert share >= 0.5, f"{what}: exact class is {share:.3f} of the samples"
    assert int(off.max()) <= 1, f"{what}: a code is {int(off.max())} from the float64 result"
    assert not bool((off[exact] != 0).any()), f"{what}: {int((off[exact] != 0).sum())} wrong codes in the exact class"


@pytest.mark.parametrize("depth,shift", FORMATS[:3], ids=FMT_IDS[:3])
@pytest.mark.parametrize("h0,w0", [(17, 33), (16, 16)])
@pytest.mark.parametrize("prec", G.PRECS)
def test_blend_kernel(gpu, prec, h0, w0, depth, shift):
    """rrin_plane_blend_h8 against the float64 mask blend at A_MASK, for t = 0.25, 0.5 and a batch with
    per-image coefficients; nothing outside the crop is written; the range flag zeroes the plane at the
    fp16 precisions only; two runs give the same bits."""
    lib, n, pr = _lib.lib(), 2, PREC[prec]
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    top, maxval = h - h0, (1 << depth) - 1
    at, lg = blend_inputs(n, h, w, 5 * h0 + depth)
    sc = torch.cat([at.reshape(-1), lg.reshape(-1)]).to(gpu)
    sc_snap = sc.clone()
    dt = torch.uint8 if depth == 8 else torch.uint16
    pitch, gap = w0 + 3, 11
    dummy = torch.zeros(8, dtype=dt, device=gpu)

    def run(t, status=None):
        coef = t_coefficients(torch.tensor(t) if isinstance(t, list) else t, n)
        buf = torch.full((n, h0 * pitch + gap), 0xA5 if depth == 8 else 0x25A5, dtype=torch.int32).to(
            torch.uint8 if depth == 8 else torch.int16).view(dt).to(gpu)
        ap = aux_plane(dummy, dummy, buf, h0 * w0, h0 * pitch + gap, w0, pitch, depth, shift, sc)  # inputs: not read
        cd = coef.to(gpu)
        rc = lib.rrin_plane_blend_h8(C.byref(ap), cd.data_ptr(), n, h, w, h0, w0, pr,
                                     status.data_ptr() if status is not None else None, H.stream(gpu))
        torch.cuda.synchronize(gpu)
        assert rc == 0, rc
        return coef, buf.cpu()

    def crop_of(buf):
        return buf[:, :h0 * pitch].view(n, h0, pitch)[:, :, :w0]

    def outside_untouched(buf):
        keep = torch.ones(buf.shape, dtype=torch.bool)
        keep[:, :h0 * pitch].view(n, h0, pitch)[:, :, :w0] = False
        sent = 0xA5 if depth == 8 else 0x25A5
        return bool((i32(buf)[keep] == sent).all())

    for t in (0.25, 0.5, [0.3, 0.75]):
        coef, buf = run(t)
        ref = G.mask_blend(coef, lg, at[:, 0:1], at[:, 1:2]).clamp(0, 1)[:, 0, top:, :w0]
        code_check(crop_of(buf), ref, maxval, shift, G.A_MASK, f"blend {prec} {h0}x{w0} d{depth}s{shift} t={t}")
        assert outside_untouched(buf), "an element outside the crop was written"
    assert torch.equal(buf.view(torch.uint8), run([0.3, 0.75])[1].view(torch.uint8)), "two runs differ"
    assert torch.equal(sc, sc_snap), "the scratch changed"
    flagged = run(0.5, torch.ones(1, dtype=torch.int32, device=gpu))[1]
    clear = run(0.5, torch.zeros(1, dtype=torch.int32, device=gpu))[1]
    plain = run(0.5)[1]
    assert torch.equal(clear.view(torch.uint8), plain.view(torch.uint8))
    if prec == "R32":
        assert torch.equal(flagged.view(torch.uint8), plain.view(torch.uint8)), "fp32 records obey no range flag"
    else:
        assert not bool(i32(crop_of(flagged)).any()) and outside_untouched(flagged)


def test_kernel_refusals(gpu):
    """What the two kernel entries refuse, before any launch: the outputs keep their fill."""
    lib, n, h0, w0, h, w = _lib.lib(), 2, 17, 33, 32, 48
    g16 = H8Tensor(n, 16, h, w, gpu, _lib.PREC_F32R)
    view = g16.view(0, 16)
    a = torch.zeros((n + 1, h0, w0), dtype=torch.uint8, device=gpu)
    out = torch.full((n, h0, w0), 0xA5, dtype=torch.uint8, device=gpu)
    sc = torch.full((4 * n * h * w,), float("nan"), device=gpu)
    coef = t_coefficients(0.5, n).to(gpu)
    st = H.stream(gpu)

    def both(ap, prec=_lib.PREC_F32R, hh0=h0, ww0=w0):
        return (lib.rrin_plane_warp_h8(C.byref(view), C.byref(ap), n, hh0, ww0, None, n, prec, st),
                lib.rrin_plane_blend_h8(C.byref(ap), coef.data_ptr(), n, h, w, hh0, ww0, prec, None, st))

    def ap_of(**kw):
        args = dict(a0=a[:-1], a1=a[1:], out=out, in_stride=h0 * w0, out_stride=h0 * w0, in_pitch=w0, out_pitch=w0,
                    depth=8, shift=0, scratch=sc)
        args.update(kw)
        return aux_plane(**args)

    assert both(ap_of(), prec=_lib.PREC_F32) == (E_ARG, E_ARG)
    assert both(ap_of(depth=7)) == (E_ARG, E_ARG)
    assert both(ap_of(depth=10, shift=7)) == (E_ARG, E_ARG)
    assert both(ap_of(shift=1)) == (E_ARG, E_ARG)
    assert both(ap_of(in_pitch=w0 - 1)) == (E_ARG, E_ARG)
    assert both(ap_of(out_pitch=w0 - 1)) == (E_ARG, E_ARG)
    assert both(ap_of(in_stride=h0 * w0 - 1)) == (E_ARG, E_ARG)     # overlapping input frames
    assert both(ap_of(out_stride=h0 * w0 - 1)) == (E_ARG, E_ARG)    # overlapping output frames
    assert both(ap_of(scratch=sc[:-4])) == (E_ARG, E_ARG)
    assert both(ap_of(), hh0=h + 1) == (E_SHAPE, E_SHAPE)
    assert both(ap_of(), ww0=0) == (E_SHAPE, E_SHAPE)
    odd = torch.zeros(2 * (n + 1) * h0 * w0 + 2, dtype=torch.uint8, device=gpu)[1:]
    ap = ap_of(depth=10)
    ap.a0 = odd.data_ptr()
    assert both(ap) == (E_ARG, E_ARG)                               # an odd word address
    m = torch.zeros(n, dtype=torch.int32, device=gpu)
    apv = ap_of()
    assert lib.rrin_plane_warp_h8(C.byref(view), C.byref(apv), n, h0, w0, None, 1, _lib.PREC_F32R, st) == E_ARG
    assert lib.rrin_plane_warp_h8(C.byref(view), C.byref(apv), n, h0, w0, m.data_ptr(), n + 1, _lib.PREC_F32R, st) == E_ARG
    assert lib.rrin_plane_warp_h8(C.byref(g16.view(8, 8)), C.byref(apv), n, h0, w0, None, n, _lib.PREC_F32R, st) == E_SHAPE
    assert lib.rrin_plane_scratch_bytes(n, h, w) == 16 * n * h * w and lib.rrin_plane_scratch_bytes(0, h, w) < 0
    torch.cuda.synchronize(gpu)
    assert bool((out == 0xA5).all()) and bool(torch.isnan(sc).all())


# ---- the whole forward ----------------------------------------------------------------------------
_NETS = {}


def net_of(dev, precision):
    if precision not in _NETS:
        if "sd" not in _NETS:
            _NETS["sd"] = keyed_state_dict(Net().state_dict(), stress=True)
        net = Net()
        net.load_state_dict(_NETS["sd"], strict=True)
        net.precision = precision
        _NETS[precision] = net.to(dev).eval()
    return _NETS[precision]


def rgb_frames(n, h0, w0, seed, depth=8):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << depth, (n, h0, w0, 3)).astype(np_dtype(depth))
    return as_torch(a)


def yuv_frames(n, h0, w0, seed, depth=8):
    rng = np.random.default_rng(seed)
    lo, hi = (16 << (depth - 8)), (235 << (depth - 8))
    return as_torch(rng.integers(lo, hi, (n, 3 * h0 // 2, w0)).astype(np_dtype(depth)))


class Recorder:
    """The library with a record of the forward entries called through it."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("rrin_net_") or not name.endswith("_fwd"):
            return f

        def call(*a):
            self.calls.append(name)
            return f(*a)
        return call


PATHS = {
    "u8": (lambda n, h, w, s: rgb_frames(n, h, w, s), 8, {}),
    "u16": (lambda n, h, w, s: rgb_frames(n, h, w, s, 10), 10, {"depth": 10}),
    "yuv": (lambda n, h, w, s: yuv_frames(n, h, w, s), 8, {}),
    "yuv16": (lambda n, h, w, s: yuv_frames(n, h, w, s, 10), 10, {"depth": 10}),
}


@pytest.mark.parametrize("h0,w0", [(34, 50), (16, 16)])
@pytest.mark.parametrize("path", list(PATHS))
def test_forward_plane_leaves_the_frames_alone(gpu, path, h0, w0):
    """Every path once: without the keyword the call reaches the existing entry; with it, the path's
    _plane_fwd entry, the same frame bits, and a plane of the frames' dtype and size that two calls
    agree on."""
    net, n = net_of(gpu, "fp32"), 2
    make, depth, kw = PATHS[path]
    f0, f1 = make(n, h0, w0, 1).to(gpu), make(n, h0, w0, 2).to(gpu)
    a0, a1 = plane_data(n, h0, w0, depth, 0, 3).to(gpu), plane_data(n, h0, w0, depth, 0, 4).to(gpu)
    eng = net.engine()
    rec = Recorder(eng.lib)
    eng.lib = rec
    try:
        with torch.no_grad():
            fwd = getattr(net, "forward_" + path)
            want = fwd(f0, f1, 0.25, **kw)
            assert rec.calls == [f"rrin_net_{path}_fwd"] * len(rec.calls) and rec.calls, rec.calls
            rec.calls.clear()
            got, pl = fwd(f0, f1, 0.25, plane=(a0, a1), **kw)
            assert rec.calls == [f"rrin_net_{path}_plane_fwd"] * len(rec.calls) and rec.calls, rec.calls
            _, pl2 = fwd(f0, f1, 0.25, plane=(a0, a1), **kw)
    finally:
        eng.lib = rec._lib
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "plane= changed the frames"
    assert pl.dtype == a0.dtype and tuple(pl.shape) == (n, h0, w0)
    assert torch.equal(pl.view(torch.uint8), pl2.view(torch.uint8))
    assert int(i32(pl.cpu()).max()) <= (1 << depth) - 1 and bool(i32(pl.cpu()).any())


@pytest.mark.parametrize("h0,w0", [(34, 50), (16, 16)])
def test_forward_u8_plane_meets_the_definition(gpu, h0, w0):
    """precision="fp32": plane.reference on the taps of the float forward of the same frames against
    forward_u8(..., plane=), under the blend kernel's +-1 / exact-class rule at eps = A_WARP + A_MASK (module
    docstring).  The refined flows are the engine's own fp32 sums (glue_ref's fp32 twins of the two glue
    steps), so that the reference sees the flows the kernels saw."""
    net, n, t = net_of(gpu, "fp32"), 2, 0.25
    f0, f1 = rgb_frames(n, h0, w0, 11), rgb_frames(n, h0, w0, 12)
    a0, a1 = plane_data(n, h0, w0, 8, 0, 13), plane_data(n, h0, w0, 8, 0, 14)
    taps = {}
    with torch.no_grad():
        net.engine().forward(cv.frames_u8_to_float(f0).contiguous().to(gpu), cv.frames_u8_to_float(f1).contiguous().to(gpu),
                             t, streams=1, taps=taps)
        _, pl = net.forward_u8(f0.to(gpu), f1.to(gpu), t, plane=(a0.to(gpu), a1.to(gpu)))
    coef = t_coefficients(t, n)
    ft0, ft1 = G.flow_blend32(coef, taps["Flow"].cpu())
    ft = G.refine_add32(torch.cat([ft0, ft1], 1), taps["refine_flow"].cpu())
    ours = {"ft0": ft[:, 0:2], "ft1": ft[:, 2:4], "Mask": taps["Mask"].cpu()}
    stored, value = P.reference_plane(ours, a0, a1, t)
    code_check(pl.cpu(), value, 255, 0, G.A_WARP + G.A_MASK, f"forward_u8 plane {h0}x{w0}")
    assert int((stored.to(torch.int32) - pl.cpu().to(torch.int32)).abs().max()) <= 1
    # and on the engine's taps as they come: plane.refined_flows then forms the flows in float64 from
    # the raw Flow and refine_flow, where the engine rounds to fp32 three times per component (two
    # products with a sum, then the refine add), each by at most 2^-24 of a term no larger than F = the
    # largest |raw flow| + |refinement|.  A position error d moves a bilinear sample of a plane in [0, 1]
    # by at most d per axis, so eps grows by 2 * 3 * 2^-24 * F.
    raw = {k: v.cpu() for k, v in taps.items()}
    big = float(raw["Flow"].abs().max() + raw["refine_flow"].abs().max())
    eps = G.A_WARP + G.A_MASK + 6 * 2.0 ** -24 * big
    print(f"largest flow term {big:.3f}: eps {eps:.3e}")
    _, value_raw = P.reference_plane(raw, a0, a1, t)
    code_check(pl.cpu(), value_raw, 255, 0, eps, f"forward_u8 plane {h0}x{w0}, the engine's taps")


def test_items_plane_equals_single_pairs(gpu):
    """interpolate_items_u8 with pair = [0, 0, 1]: item k's plane (and frame) is bit for bit that of
    forward_u8 on that pair at that t."""
    net, h0, w0 = net_of(gpu, "fp32"), 34, 50
    fr = rgb_frames(3, h0, w0, 21).to(gpu)
    al = plane_data(3, h0, w0, 8, 0, 22).to(gpu)
    pair, ts = [0, 0, 1], [0.25, 0.75, 0.5]
    with torch.no_grad():
        out, pl = net.interpolate_items_u8(fr, pair, ts, plane=al)
        assert tuple(pl.shape) == (3, h0, w0)
        for k, (p, t) in enumerate(zip(pair, ts)):
            o1, p1 = net.forward_u8(fr[p:p + 1], fr[p + 1:p + 2], t, plane=(al[p:p + 1], al[p + 1:p + 2]))
            assert torch.equal(pl[k], p1[0]), f"item {k}: plane"
            assert torch.equal(out[k], o1[0]), f"item {k}: frame"


def test_gate_and_flow_scale(gpu):
    """flow_scale=2 with gate codes 0, 1, 2: the gated pairs' planes are the input planes' bytes, the
    other pair's is the ungated call's; the same through the item forward."""
    net, h0, w0 = net_of(gpu, "fp32"), 34, 50
    fr = rgb_frames(4, h0, w0, 31).to(gpu)
    al = plane_data(4, h0, w0, 8, 0, 32).to(gpu)
    gate = torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu)
    with torch.no_grad():
        o0, p0 = net.forward_u8(fr[:-1], fr[1:], 0.5, flow_scale=2, plane=(al[:-1], al[1:]))
        o1, p1 = net.forward_u8(fr[:-1], fr[1:], 0.5, gate=gate, flow_scale=2, plane=(al[:-1], al[1:]))
        o2, p2 = net.interpolate_items_u8(fr, [0, 1, 2], [0.5, 0.25, 0.75], gate=torch.tensor(
            [0, 2, 2], dtype=torch.int32, device=gpu), flow_scale=2, plane=al)
    assert torch.equal(p1[0], p0[0]) and torch.equal(p1[1], al[1]) and torch.equal(p1[2], al[3])
    assert torch.equal(o1[1], fr[1]) and torch.equal(o1[2], fr[3]) and torch.equal(o1[0], o0[0])
    assert not torch.equal(p0[1], al[1]) and not torch.equal(p0[2], al[3])
    # items: pair 1 is a cut at t = 0.25 (the first frame), pair 2 a cut at t = 0.75 (the second)
    assert torch.equal(p2[0], p0[0]) and torch.equal(p2[1], al[1]) and torch.equal(p2[2], al[3])
    assert torch.equal(o2[1], fr[1]) and torch.equal(o2[2], fr[3])


def test_refusals_change_no_state(gpu):
    """fp32_planar, a wrong dtype, a wrong shape and plane= on NetGraph raise; last_gate and the
    Flow-reuse state stay as they were."""
    net, h0, w0, n = net_of(gpu, "fp32"), 16, 16, 2
    f0, f1 = rgb_frames(n, h0, w0, 41).to(gpu), rgb_frames(n, h0, w0, 42).to(gpu)
    a = plane_data(n, h0, w0, 8, 0, 43).to(gpu)
    gate = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    with torch.no_grad():
        net.forward_u8(f0, f1, 0.5, gate=gate, plane=(a, a))
        eng = net.engine()
        last, valid = eng.last_gate, dict(eng._flow_valid)
        assert last is not None and valid
        with pytest.raises(TypeError):
            net.forward_u8(f0, f1, 0.5, gate=gate.clone(), plane=(a.to(torch.int16), a))
        with pytest.raises(TypeError):
            net.forward_u8(f0, f1, 0.5, gate=gate.clone(), plane=a)
        with pytest.raises(ValueError):
            net.forward_u8(f0, f1, 0.5, gate=gate.clone(), plane=(a[:, :-1], a[:, :-1]))
        with pytest.raises(ValueError):
            net.forward_u8(f0, f1, 0.5, gate=gate.clone(), plane=(a, a.cpu()))
        with pytest.raises(ValueError):
            net.interpolate_items_u8(torch.cat([f0, f1[-1:]]), [0, 1], [0.5, 0.5], plane=a)
        with pytest.raises(ValueError):
            eng.graph(n, 16, 16, plane=(a, a))
        assert eng.last_gate is last and dict(eng._flow_valid) == valid
        planar = net_of(gpu, "fp32_planar")
        with pytest.raises(RuntimeError):
            planar.forward_u8(f0, f1, 0.5, plane=(a, a))


def test_folder_round_trip_with_alpha(gpu, tmp_path):
    """interpolate_folder(alpha=True): RGBA PNGs in, RGBA PNGs out whose RGB and A are forward_u8's frame and
    plane of the files' bytes; a file without alpha counts as 255."""
    from PIL import Image
    net, h0, w0 = net_of(gpu, "fp32"), 17, 33
    src, dest = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rgba = np.random.default_rng(7).integers(0, 256, (3, h0, w0, 4), dtype=np.uint8)
    rgba[2, :, :, 3] = 255
    Image.fromarray(rgba[0], "RGBA").save(src / "000.png")
    Image.fromarray(rgba[1], "RGBA").save(src / "001.png")
    Image.fromarray(rgba[2, :, :, :3].copy(), "RGB").save(src / "002.png")
    cv.interpolate_folder(net, str(src), str(dest), 1, batch=2, device=gpu, alpha=True, log=lambda *_: None)
    st = torch.from_numpy(rgba).to(gpu)
    f, a = st[..., :3].contiguous(), st[..., 3].contiguous()
    with torch.no_grad():
        want, wa = net.forward_u8(f[:-1], f[1:], 0.5, plane=(a[:-1], a[1:]))
    for k, name in enumerate(("000000002.png", "000000004.png")):
        with Image.open(dest / name) as im:
            assert im.mode == "RGBA"
            got = np.asarray(im)
        np.testing.assert_array_equal(got[..., :3], want[k].cpu().numpy())
        np.testing.assert_array_equal(got[..., 3], wa[k].cpu().numpy())
