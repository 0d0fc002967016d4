"""GPU: the planar fp32 kernels one by one -- rrin_conv3x3_fwd (conv_mfma.hip) and the planar
entries of head.hip (rrin_head_fwd, rrin_warp_fwd, rrin_nchw_to_pp, rrin_pp_to_nchw) -- against
tests/planar_ref.py and tests/glue_ref.py.

Convs: integer data on which every summation order gives the same fp32 bits, compared with ==, at
every config x source mode x epilogue; the whole raw storage of dst and pool starts as a non-zero
pattern (NaN in the interior that must be written) and must come back bit for bit outside that
interior; every source channel outside the view holds NaN and +-inf.  Floats: the derived forward
bounds.  Warp, heads and layout kernels: guarded, patterned buffers.  Refusals: every RRIN_E_*
branch with proof that nothing was written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rrin_amd import _lib
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import PPTensor
from tests import glue_ref as G
from tests import hip_helpers as H
from tests import planar_ref as P
from tests.test_gpu_glue import CONV_TOL, assert_close, assert_only_moved, bits, fill_pattern, snapshot

pytestmark = pytest.mark.gpu
E_SHAPE, E_ARG, E_CONFIG = -1, -2, -4
NAN_BITS = 0x7FC0BEEF
GUARD = 64


class Guarded:
    """count floats inside a buffer of NAN_BITS with GUARD words on either side."""

    def __init__(self, count, gpu):
        self.count = count
        self.buf = torch.full((count + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=gpu)

    @property
    def t(self):
        return self.buf[GUARD:GUARD + self.count].view(torch.float32)

    def guards_ok(self):
        return bool((self.buf[:GUARD] == NAN_BITS).all()) and bool((self.buf[GUARD + self.count:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf == NAN_BITS).all())


# ---- A, B: exact values on whole storage ------------------------------------------------------------------
def source_raw(x, src_off, src_c, g):
    """Raw storage [n, src_c, hp, wp] of the source: NaN, +inf, -inf in turn in every channel outside
    [src_off, src_off + cin) -- padding included, and the channels that complete the last 8-channel
    chunk -- and in the view the zero padding of the layout contract around the integers."""
    n, cin, sh, sw = x.shape
    raw = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(n * src_c * g.hp * g.wp // 3 + 1)
    raw = raw[:n * src_c * g.hp * g.wp].reshape(n, src_c, g.hp, g.wp).clone()
    raw[:, src_off:src_off + cin] = 0
    raw[:, src_off:src_off + cin, 1:sh + 1, 32:32 + sw] = torch.from_numpy(x.astype(np.float32))
    return raw


@functools.lru_cache(maxsize=None)
def dst_pattern(shape, seed, off, cout, h, w):
    """Non-zero pattern over the whole storage; NaN (with a payload) in the interior the conv writes."""
    pat = G.pattern(shape, seed)
    assert bool((pat != 0).all())
    pat[:, off:off + cout, 1:h + 1, 32:32 + w] = torch.tensor([NAN_BITS], dtype=torch.int32).view(torch.float32)
    return pat


def check_storage(t, pat_d, off, cout, ref_d, what):
    """== to the reference in the interior of channels [off, off + cout); every other word of the raw
    storage bit for bit the pattern."""
    got = t.t[:, off:off + cout, 1:t.h + 1, 32:32 + t.w]
    assert not bool(torch.isnan(got).any()), f"{what}: interior not fully written"
    ne = got != ref_d
    assert not bool(ne.any()), (f"{what}: {int(ne.sum())} of {ne.numel()} values differ, first at "
                                f"{ne.nonzero()[:4].tolist()}: got {got[ne][:4].tolist()} want {ref_d[ne][:4].tolist()}")
    keep = torch.ones(t.t.shape, dtype=torch.bool, device=t.t.device)
    keep[:, off:off + cout, 1:t.h + 1, 32:32 + t.w] = False
    bad = (bits(t.t) != bits(pat_d)) & keep
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} words outside the interior changed, first at {bad.nonzero()[:4].tolist()}"


class ConvCase:
    """One (data set, source mode) on the device: the poisoned source, shared by every config and
    epilogue (it is checked after each call)."""

    def __init__(self, gpu, cin, cout, h, w, up, *, tag=0, src_off=2, src_c=None, dst_off=1, dst_c=None, perm=None):
        self.gpu, self.cin, self.cout, self.h, self.w, self.up, self.tag, self.perm = gpu, cin, cout, h, w, up, tag, perm
        self.src_off, self.dst_off = src_off, dst_off
        self.dst_c = dst_c or cout + dst_off + 1
        x, wt, b = P.int_case(cin, cout, h, w, up, tag)
        self.wt, self.b = torch.from_numpy(wt.astype(np.float32)), torch.from_numpy(b.astype(np.float32))
        sh, sw = x.shape[2:]
        self.src = PPTensor(P.N, src_c or src_off + (cin + 7) // 8 * 8 + 3, sh, sw, gpu)
        self.src_raw = source_raw(x, src_off, self.src.c, self.src.g).to(gpu)
        self.src.t.copy_(self.src_raw)

    def run(self, cfg, epi):
        h, w, cout, gpu = self.h, self.w, self.cout, self.gpu
        what = f"{self.cin}->{cout} {h}x{w} up={self.up} epi={epi} cfg={cfg}"
        dst = PPTensor(P.N, self.dst_c, h, w, gpu)
        dpat = dst_pattern(tuple(dst.t.shape), 11, self.dst_off, cout, h, w).to(gpu)
        dst.t.copy_(dpat)
        pool = None
        if epi == P.POOL:
            pool = PPTensor(P.N, cout + 1, h // 2, w // 2, gpu)
            ppat = dst_pattern(tuple(pool.t.shape), 12, 0, cout, h // 2, w // 2).to(gpu)
            pool.t.copy_(ppat)
        H.conv(self.src, self.wt, self.b, cfg, src_off=self.src_off, dst=dst, dst_off=self.dst_off, upsample=self.up,
               epi=epi, pool=pool, perm=list(self.perm) if self.perm else None, cin=self.cin, slope=0.25)
        ref, refp = P.conv_ref(self.cin, cout, h, w, self.up, epi, self.tag, self.perm)
        check_storage(dst, dpat, self.dst_off, cout, ref.to(gpu), f"dst {what}")
        if pool is not None:
            check_storage(pool, ppat, 0, cout, refp.to(gpu), f"pool {what}")
        assert torch.equal(bits(self.src.t), bits(self.src_raw)), f"source changed: {what}"


@pytest.mark.parametrize("h,w", list(P.SHAPES))
def test_conv_exact_whole_storage(gpu, h, w):
    """Every config x every case of the size: == to the int64 reference, storage outside the written
    interior unchanged, source unchanged, NaN / inf in every source channel outside the view.  18 x 34
    runs all 36 instantiations of launch_cfg (6 configs x 2 source modes x 3 epilogues)."""
    ncfg = _lib.lib().rrin_conv_cfg_count()
    ran = set()
    for up, epis in P.SHAPES[(h, w)]:
        for cin, cout in P.channel_sets(h, w):
            case = ConvCase(gpu, cin, cout, h, w, up)
            for epi in epis:
                for cfg in range(ncfg):
                    case.run(cfg, epi)
                    ran.add((cfg, up, epi))
    assert len(ran) == ncfg * sum(len(e) for _, e in P.SHAPES[(h, w)])
    if (h, w) == (18, 34):
        assert ncfg == 6 and len(ran) == 36 and ran == {(c, u, e) for c in range(6) for u in (False, True) for e in P.EPIS}


def test_conv_exact_views(gpu):
    """src.ch_off = 6 in a 16-channel buffer with the refine permutation (cin 10: the last chunk's
    channels 10-15 lie past the buffer's end and are never read); dst.ch_off = cout in a 2 cout
    buffer, with pool."""
    for cfg in range(_lib.lib().rrin_conv_cfg_count()):
        for up in (False, True):
            ConvCase(gpu, 10, 3, 18, 34, up, tag=1, src_off=6, src_c=16, perm=P.REFINE_PERM).run(cfg, P.LEAKY)
            ConvCase(gpu, 16, 40, 18, 34, up, tag=2, dst_off=40, dst_c=80).run(cfg, P.POOL)


# ---- C: forward bound on floats -----------------------------------------------------------------------------
@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("epi", P.EPIS)
def test_conv_float_bound(gpu, epi, up):
    """Random fp32 data, keyed weights at the Net's scale, slope 0.1, every config: per element within
    (K + 2) u S (DIRECT) / (K + 6) u S (UPSAMPLE2X), the pooled output within exact_ref.pool_bound
    (derivations: planar_ref.float_ref)."""
    x, wt, b = P.float_case(up)
    ref, refp, bnd, bndp, s = P.float_ref(x, wt, b, up, epi)
    for cfg in range(_lib.lib().rrin_conv_cfg_count()):
        dst, pool = H.conv(PPTensor.from_nchw(x.to(gpu)), wt, b, cfg, upsample=up, epi=epi, slope=P.NET_SLOPE)
        err = np.abs(dst.to_nchw().cpu().double().numpy() - ref)
        line = f"planar conv up={int(up)} epi={epi} cfg={cfg}: worst err / (u S) = {float((err / (P.U * s)).max()):.3f}, worst err / bound = {float((err / bnd).max()):.4f}"
        if epi == P.POOL:
            errp = np.abs(pool.to_nchw().cpu().double().numpy() - refp)
            line += f", pool worst err / bound = {float((errp / bndp).max()):.4f}"
        print(line)
        assert (err <= bnd).all(), line
        if epi == P.POOL:
            assert (errp <= bndp).all(), line


# ---- D: rrin_warp_fwd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("h,w", P.WARP_SIZES)
def test_warp(gpu, h, w, c):
    """Against the float64 backwarp within A_WARP at every finite flow of planar_ref.warp_flow; ==
    to the image at the tap where the flow is aligned (integer + 1/2: the oracle's grid un-normalises
    to gx + u - 0.5, also at an extent of 1, where zero flow gives img / 4) and the fp32 coordinate
    arithmetic is exact -- all aligned pixels at power-of-two extents; the rest of them fall under
    A_WARP; exactly 0 for +-1e9.  A flow with +-inf or NaN in either component gives NaN in every
    channel of that pixel and nowhere else: warp_taps tests validity in float, so no tap is read,
    and the weights, NaN, meet the zeros the invalid taps stand for (common.hpp warp_taps /
    warp_apply; 0 x NaN).  Output in a guarded NaN-pattern buffer; image and flow unchanged."""
    n = P.N
    img, flow, kind = P.warp_case(n, c, h, w)
    img_d, flow_d = img.to(gpu), flow.to(gpu)
    out = Guarded(n * c * h * w, gpu)
    _lib.check(_lib.lib().rrin_warp_fwd(img_d.data_ptr(), flow_d.data_ptr(), out.t.data_ptr(), n, c, h, w, H.stream(gpu)))
    torch.cuda.synchronize()
    assert out.guards_ok()
    assert torch.equal(bits(img_d.cpu()), bits(img)) and torch.equal(bits(flow_d.cpu()), bits(flow))
    got = out.t.cpu().view(n, c, h, w)
    k = kind[:, None].expand_as(got)
    assert bool(torch.isnan(got[k == P.BAD]).all()), "a non-finite flow must give NaN"
    assert not bool(torch.isnan(got[k != P.BAD]).any()), "NaN beside a non-finite flow"
    assert bool((got[k == P.HUGE] == 0).all())
    fin = torch.where(kind == P.BAD, torch.zeros(()), flow.permute(1, 0, 2, 3)).permute(1, 0, 2, 3)
    ref = G.warp(img, fin)
    ok = k != P.BAD
    err = (got.double() - ref).abs()[ok]
    print(f"warp {h}x{w} c={c}: max err {float(err.max()):.3e} (A_WARP {G.A_WARP:.1e})")
    assert bool((err <= G.A_WARP).all())
    val, exact, inside = P.shifted(img, flow, kind)
    m = exact[:, None].expand_as(got)
    assert int(exact.sum()) > 0
    assert torch.equal(got[m], val[m]), "aligned flow: not the image at the tap"


# ---- E: planar heads and layout kernels ----------------------------------------------------------------------
HEAD_SHAPES = [(2, 16, 16), (2, 16, 48), (2, 24, 40)]
MODE = {"flow": _lib.HEAD_FLOW, "refine": _lib.HEAD_REFINE, "mask": _lib.HEAD_MASK, "final": _lib.HEAD_FINAL}


class PlanarRig:
    """test_gpu_glue.Rig on the planar layout: a patterned 24-channel Net buffer, per-image t."""

    def __init__(self, dev, n, h, w):
        self.dev, self.n, self.h, self.w = dev, n, h, w
        self.c = G.case(n, h, w)
        self.coef = t_coefficients(torch.tensor(G.T_PER_IMAGE[:n]), n)
        self.coef_d = self.coef.to(dev)

    def g16(self, seed=1):
        g = PPTensor(self.n, G.G16_CHANNELS, self.h, self.w, self.dev)
        fill_pattern(g, seed)
        g.load(self.c["x0"].to(self.dev), 0)
        g.load(self.c["x1"].to(self.dev), 3)
        return g

    def head(self, stage, g16, mode, wt, b, scale=1.0, out=None):
        """One call with raw_out; the head conv within the R32 tolerance of CONV_TOL of float64, the
        32-channel source unchanged.  Returns raw_out on the CPU."""
        src = PPTensor.from_nchw(self.c[stage].to(self.dev))
        src_snap = snapshot(src)
        raw = Guarded(self.n * wt.shape[0] * self.h * self.w, self.dev)
        H.head(src, g16, wt, b, mode, self.coef_d, out=out, raw_out=raw.t)
        assert raw.guards_ok()
        assert_only_moved(src, src_snap, [], f"{stage}: source")
        rtol, atol = CONV_TOL["R32"]
        got = raw.t.cpu().view(self.n, wt.shape[0], self.h, self.w)
        np.testing.assert_allclose(got.double().numpy(), G.conv64(self.c[stage], wt, b).numpy(), rtol=rtol,
                                   atol=atol * max(scale, 1.0), err_msg=f"{stage}: head conv")
        return got


@pytest.mark.parametrize("cout", [2, 3, 4])
@pytest.mark.parametrize("n,h,w", HEAD_SHAPES)
def test_head_plain(gpu, n, h, w, cout):
    """PLAIN: channels [0, cout) of the view receive the head conv's output (== raw_out); nothing else moves."""
    rig = PlanarRig(gpu, n, h, w)
    g16 = rig.g16()
    snap = snapshot(g16)
    wt, b = G.keyed_head("flow")
    raw = rig.head("flow", g16, _lib.HEAD_PLAIN, wt[:cout].contiguous(), b[:cout].contiguous())
    assert torch.equal(g16.to_nchw(0, cout).cpu(), raw)
    assert_only_moved(g16, snap, range(cout), "PLAIN g16")


@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n,h,w", HEAD_SHAPES)
def test_head_refine(gpu, n, h, w, scale):
    """REFINE: Ft == fp32(Ft_before + raw_out); xt1 / xt2 within A_WARP of the float64 backwarp with
    those sums; channels 6-15 only."""
    rig = PlanarRig(gpu, n, h, w)
    g16 = rig.g16()
    before = g16.to_nchw(0, 16).cpu()
    snap = snapshot(g16)
    raw = rig.head("refine", g16, _lib.HEAD_REFINE, *G.keyed_head("refine", scale), scale=scale)
    s32 = G.refine_add32(before[:, 6:10], raw)
    assert torch.equal(g16.to_nchw(6, 4).cpu(), s32), "Ft != fp32(Ft + raw_out)"
    ref = torch.cat([G.warp(before[:, 0:3], s32[:, 0:2]), G.warp(before[:, 3:6], s32[:, 2:4])], 1)
    assert float(ref.abs().max()) > 0.5
    assert_close(g16.to_nchw(10, 6).cpu(), ref, G.A_WARP, "R32", f"planar REFINE warp x{scale:g}")
    assert_only_moved(g16, snap, range(6, 16), "REFINE g16")


@pytest.mark.parametrize("n,h,w", HEAD_SHAPES)
def test_head_mask(gpu, n, h, w):
    """MASK: the blend within A_MASK of float64; channels 6-8 only."""
    rig = PlanarRig(gpu, n, h, w)
    g16 = rig.g16()
    before = g16.to_nchw(0, 16).cpu()
    snap = snapshot(g16)
    raw = rig.head("mask", g16, _lib.HEAD_MASK, *G.keyed_head("mask"))
    ref = G.mask_blend(rig.coef, raw, before[:, 10:13], before[:, 13:16])
    assert_close(g16.to_nchw(6, 3).cpu(), ref, G.A_MASK, "R32", "planar MASK blend")
    assert_only_moved(g16, snap, range(6, 9), "MASK g16")


@pytest.mark.parametrize("n,h,w", HEAD_SHAPES)
def test_head_final(gpu, n, h, w):
    """FINAL: out == clamp(fp32(raw_out + blend), 0, 1), the fp32 twin; g16 is not written; out guarded."""
    rig = PlanarRig(gpu, n, h, w)
    g16 = rig.g16()
    blend = g16.to_nchw(6, 3).cpu()
    snap = snapshot(g16)
    out = Guarded(n * 3 * h * w, gpu)
    raw = rig.head("final", g16, _lib.HEAD_FINAL, *G.keyed_head("final"), out=out.t)
    q = G.final32(raw, blend)
    assert float(q.min()) == 0.0 and float(q.max()) == 1.0
    assert out.guards_ok() and torch.equal(out.t.cpu().view(n, 3, h, w), q), "out != final32(raw_out, blend)"
    assert_only_moved(g16, snap, [], "FINAL g16")


def random_bits(shape, seed):
    """Arbitrary bit patterns: NaN payloads, infinities and denormals among them."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2 ** 31, 2 ** 31, tuple(shape), generator=g, dtype=torch.int64).to(torch.int32)
    flat = v.view(-1)
    for k, word in enumerate((0x7FC12345, -0x3FEDCBB, 0x7F800001, 0x00000001, -0x7FFFFFFF, 0x007FFFFF, 0x7F800000, 0)):
        flat[(k * 7) % flat.numel()] = word
    return v


@pytest.mark.parametrize("c", [1, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 33), (23, 40)])
def test_layout_roundtrip_bitwise(gpu, h, w, c):
    """rrin_nchw_to_pp into channels [2, 2 + c) of a guarded, patterned PP buffer and rrin_pp_to_nchw
    back into a guarded buffer: the int32 words come back unchanged, only the interior of the
    addressed channels moved, the guards and the sources are intact."""
    n, off = 2, 2
    lib = _lib.lib()
    x = random_bits((n, c, h, w), 31 * h + w + c).to(gpu)
    pp = PPTensor(n, c + 4, h, w, gpu)
    store = Guarded(pp.t.numel(), gpu)
    pp.t = store.t.view(pp.t.shape)
    fill_pattern(pp, 3)
    snap = snapshot(pp)
    v = pp.view(off, c)
    assert lib.rrin_nchw_to_pp(x.data_ptr(), n, c, C.byref(v), H.stream(gpu)) == 0
    torch.cuda.synchronize()
    assert store.guards_ok()
    assert_only_moved(pp, snap, range(off, off + c), "nchw_to_pp")
    assert torch.equal(bits(pp.t[:, off:off + c, 1:h + 1, 32:32 + w]), x)
    after = snapshot(pp)
    out = Guarded(n * c * h * w, gpu)
    assert lib.rrin_pp_to_nchw(C.byref(v), n, c, out.t.data_ptr(), H.stream(gpu)) == 0
    torch.cuda.synchronize()
    assert out.guards_ok() and store.guards_ok()
    assert torch.equal(bits(out.t).view(n, c, h, w), x)
    assert_only_moved(pp, after, [], "pp_to_nchw source")


# ---- F: refusals ------------------------------------------------------------------------------------------------
def test_conv_refusals(gpu):
    """Every RRIN_E_* branch of conv_prepare; nothing is launched: dst and pool keep their pattern."""
    lib = _lib.lib()
    n, cin, cout, h, w = 2, 16, 8, 18, 34
    src = PPTensor(n, cin, h, w, gpu)
    half = PPTensor(n, cin, h // 2, w // 2, gpu)
    dst, pool = PPTensor(n, cout, h, w, gpu), PPTensor(n, cout, h // 2, w // 2, gpu)
    odd = {k: (PPTensor(n, cin, *k, gpu), PPTensor(n, cout, *k, gpu), PPTensor(n, cout, k[0] // 2, k[1] // 2, gpu))
           for k in ((17, 34), (18, 33))}
    watched = [dst, pool] + [t for v in odd.values() for t in v[1:]]
    for k, t in enumerate(watched):
        fill_pattern(t, 20 + k)
    snaps = [snapshot(t) for t in watched]
    wp, bp = H.pack(torch.ones(cout, cin, 3, 3), torch.ones(cout), 0, None, gpu)

    def desc(**kw):
        d = _lib.ConvDesc()
        d.n, d.cin, d.cout, d.cfg, d.src_mode, d.epi_mode, d.slope = n, cin, cout, 0, _lib.SRC_DIRECT, _lib.EPI_LINEAR, 0.1
        d.src, d.dst, d.pool = src.view(0, cin), dst.view(0, cout), pool.view(0, cout)
        d.wpack, d.bias = wp.data_ptr(), bp.data_ptr()
        for key, val in kw.items():
            obj, names = d, key.split("__")
            for name in names[:-1]:
                obj = getattr(obj, name)
            setattr(obj, names[-1], val)
        return d

    def call(d):
        return lib.rrin_conv3x3_fwd(C.byref(d) if d is not None else None, H.stream(gpu))

    up, pl = _lib.SRC_UPSAMPLE2X, _lib.EPI_LEAKY_POOL
    cases = [
        (None, E_ARG), (desc(src__base=None), E_ARG), (desc(dst__base=None), E_ARG), (desc(wpack=None), E_ARG),
        (desc(bias=None), E_ARG),
        (desc(cfg=-1), E_CONFIG), (desc(cfg=lib.rrin_conv_cfg_count()), E_CONFIG),
        (desc(n=0), E_ARG), (desc(cin=0), E_ARG), (desc(cout=0), E_ARG),
        (desc(src_mode=2), E_ARG), (desc(src_mode=-1), E_ARG), (desc(epi_mode=-1), E_ARG), (desc(epi_mode=3), E_ARG),
        (desc(cin=cin + 1), E_ARG), (desc(src__channels=cin - 1), E_ARG), (desc(cout=cout + 1), E_ARG),
        (desc(src=half.view(0, cin)), E_SHAPE),                              # DIRECT from a half-size source
        (desc(src_mode=up), E_SHAPE),                                        # UPSAMPLE2X from a full-size source
        (desc(src_mode=up, src=odd[(17, 34)][0].view(0, cin)), E_SHAPE),
        (desc(epi_mode=pl, pool__base=None), E_SHAPE),
        (desc(epi_mode=pl, pool=dst.view(0, cout)), E_SHAPE),                # pool of the full size
        (desc(epi_mode=pl, pool__channels=cout - 1), E_SHAPE),
        (desc(src__g__wp=src.g.wp + 32), E_SHAPE), (desc(src__g__hp=src.g.hp + 16), E_SHAPE),
        (desc(dst__g__wp=dst.g.wp + 32), E_SHAPE), (desc(dst__g__hp=dst.g.hp + 16), E_SHAPE),
        (desc(n=0x7FFFFFFF), E_SHAPE),                                       # more tiles than a grid holds
    ]
    for (hh, ww), (s, d_, p_) in odd.items():                                 # odd h, odd w under pool
        cases.append((desc(epi_mode=pl, src=s.view(0, cin), dst=d_.view(0, cout), pool=p_.view(0, cout)), E_SHAPE))
    for k, (d, code) in enumerate(cases):
        assert call(d) == code, f"case {k}"
    torch.cuda.synchronize()
    for t, s in zip(watched, snaps):
        assert_only_moved(t, s, [], "refused conv")
    for d in (desc(), desc(epi_mode=pl), desc(src_mode=up, src=half.view(0, cin))):   # the base descriptors are accepted
        assert call(d) == 0
    torch.cuda.synchronize()


def test_head_refusals(gpu):
    """Every RRIN_E_* branch of rrin_head_fwd; g16, out, raw_out and flow_raw keep their patterns."""
    lib = _lib.lib()
    n, h, w = 2, 16, 48
    src, g16, fr = PPTensor(n, 32, h, w, gpu), PPTensor(n, 24, h, w, gpu), PPTensor(n, 4, h, w, gpu)
    other = PPTensor(n, 24, h + 16, w, gpu)
    wide = PPTensor(n, 4, h, w + 32, gpu)
    for k, t in enumerate((g16, fr, other, wide)):
        fill_pattern(t, 40 + k)
    snaps = [snapshot(t) for t in (g16, fr, other, wide)]
    out, raw = Guarded(n * 4 * h * w, gpu), Guarded(n * 4 * h * w, gpu)
    wt = torch.ones(4, 32, 3, 3, device=gpu)
    b = torch.ones(4, device=gpu)
    coef = t_coefficients(torch.tensor([0.3, 0.6]), n).to(gpu)
    cout_of = {_lib.HEAD_PLAIN: 4, _lib.HEAD_FLOW: 4, _lib.HEAD_REFINE: 4, _lib.HEAD_MASK: 2, _lib.HEAD_FINAL: 3}

    def desc(mode=_lib.HEAD_FLOW, **kw):
        d = _lib.HeadDesc()
        d.n, d.cin, d.cout, d.mode = n, 32, cout_of.get(mode, 4), mode
        d.src, d.g16 = src.view(0, 32), g16.view(0, 24)
        d.w, d.bias, d.coef, d.out, d.raw_out = wt.data_ptr(), b.data_ptr(), coef.data_ptr(), out.t.data_ptr(), raw.t.data_ptr()
        for key, val in kw.items():
            obj, names = d, key.split("__")
            for name in names[:-1]:
                obj = getattr(obj, name)
            setattr(obj, names[-1], val)
        return d

    def call(d):
        return lib.rrin_head_fwd(C.byref(d) if d is not None else None, H.stream(gpu))

    PL, FL, RF, MK, FN = _lib.HEAD_PLAIN, _lib.HEAD_FLOW, _lib.HEAD_REFINE, _lib.HEAD_MASK, _lib.HEAD_FINAL
    cases = [
        (None, E_ARG), (desc(src__base=None), E_ARG), (desc(g16__base=None), E_ARG), (desc(w=None), E_ARG), (desc(bias=None), E_ARG),
        (desc(cin=16), E_ARG), (desc(n=0), E_ARG),
        (desc(g16=other.view(0, 24)), E_SHAPE), (desc(g16=PPTensor(n, 24, h, w + 32, gpu).view(0, 24)), E_SHAPE),
        (desc(src__g__wp=src.g.wp + 32), E_SHAPE), (desc(src__g__hp=src.g.hp + 16), E_SHAPE),
        (desc(g16__g__wp=g16.g.wp + 32), E_SHAPE), (desc(g16__g__hp=g16.g.hp + 16), E_SHAPE),
        (desc(src__channels=31), E_ARG),
        (desc(g16__channels=15), E_ARG), (desc(g16__ch_off=1), E_ARG), (desc(coef=None), E_ARG),
        (desc(PL, g16__channels=3), E_ARG),
        (desc(FN, out=None), E_ARG),
        (desc(FL, flow_raw=fr.view(0, 3)), E_SHAPE), (desc(FL, flow_raw=other.view(0, 4)), E_SHAPE),
        (desc(FL, flow_raw=wide.view(0, 4)), E_SHAPE), (desc(FL, flow_raw=fr.view(0, 4), flow_raw__g__wp=fr.g.wp + 32), E_SHAPE),
        (desc(PL, cout=0), E_ARG), (desc(PL, cout=5), E_ARG), (desc(FL, cout=3), E_ARG), (desc(RF, cout=3), E_ARG),
        (desc(MK, cout=3), E_ARG), (desc(MK, cout=4), E_ARG), (desc(FN, cout=2), E_ARG), (desc(FN, cout=4), E_ARG),
        (desc(5), E_ARG), (desc(-1), E_ARG),
    ]
    for k, (d, code) in enumerate(cases):
        assert call(d) == code, f"case {k}"
    torch.cuda.synchronize()
    for t, s in zip((g16, fr, other, wide), snaps):
        assert_only_moved(t, s, [], "refused head")
    assert out.untouched() and raw.untouched()
    assert call(desc(FL, flow_raw=fr.view(0, 4))) == 0                       # the base descriptor is accepted
    torch.cuda.synchronize()


def test_warp_and_layout_refusals(gpu):
    """rrin_warp_fwd, rrin_nchw_to_pp, rrin_pp_to_nchw: every RRIN_E_ARG branch, outputs untouched."""
    lib = _lib.lib()
    n, c, h, w = 2, 3, 5, 9
    st = H.stream(gpu)
    img, flow = torch.rand(n, c, h, w, device=gpu), torch.zeros(n, 2, h, w, device=gpu)
    out = Guarded(n * c * h * w, gpu)
    i, f, o = img.data_ptr(), flow.data_ptr(), out.t.data_ptr()
    for args in [(None, f, o, n, c, h, w), (i, None, o, n, c, h, w), (i, f, None, n, c, h, w), (i, f, o, 0, c, h, w),
                 (i, f, o, n, 0, h, w), (i, f, o, n, c, 0, w), (i, f, o, n, c, h, 0), (i, f, o, -1, c, h, w)]:
        assert lib.rrin_warp_fwd(*args, st) == E_ARG, args
    pp = PPTensor(n, c + 1, h, w, gpu)
    fill_pattern(pp, 9)
    snap = snapshot(pp)

    def view(**kw):
        v = pp.view(1, c)
        for key, val in kw.items():
            obj, names = v, key.split("__")
            for name in names[:-1]:
                obj = getattr(obj, name)
            setattr(obj, names[-1], val)
        return v

    bad_views = [view(base=None), view(g__wp=pp.g.wp + 32), view(g__hp=pp.g.hp + 16), view(g__plane=pp.g.plane + 1)]
    for v in bad_views:
        assert lib.rrin_nchw_to_pp(i, n, c, C.byref(v), st) == E_ARG
        assert lib.rrin_pp_to_nchw(C.byref(v), n, c, o, st) == E_ARG
    good = view()
    for nn, cc in [(0, c), (n, 0), (n, c + 1)]:
        assert lib.rrin_nchw_to_pp(i, nn, cc, C.byref(good), st) == E_ARG
        assert lib.rrin_pp_to_nchw(C.byref(good), nn, cc, o, st) == E_ARG
    assert lib.rrin_nchw_to_pp(None, n, c, C.byref(good), st) == E_ARG
    assert lib.rrin_nchw_to_pp(i, n, c, None, st) == E_ARG
    assert lib.rrin_pp_to_nchw(C.byref(good), n, c, None, st) == E_ARG
    assert lib.rrin_pp_to_nchw(None, n, c, o, st) == E_ARG
    torch.cuda.synchronize()
    assert out.untouched()
    assert_only_moved(pp, snap, [], "refused layout call")
