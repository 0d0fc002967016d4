"""GPU: what the record-layout convs, the fused level-0 block, the ring fix-up and the layout
kernels touch *outside* the pixels they compute, and the fp16 range guard at its edges.

Every destination is a tests/record_ref.GuardedH8: raw storage prefilled with a finite non-zero
pattern, one spare 2-group chunk before and after the view (img_stride exceeds the view), guard
bands around each plane.  record_ref.check_storage compares the raw storage after the call with a
snapshot: the view's interior against float64 within the project's own tol(prec, cfg), every
other element -- padding on four sides, neighbouring groups, the lo plane, the guards -- bit for
bit.  tests/test_record_ref.py shows on the CPU that the checker rejects one changed record in
each of those places.  Shapes are the smallest with ragged tiles (9 x 40: a 2 x 2-3 ragged grid;
17 x 33: one row and one column into a second 16 x 32 tile), two images."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from rrin_amd import _lib
from rrin_amd.pp import H8Tensor
from tests import glue_ref as G
from tests import hip_helpers as H
from tests import record_ref as R
from tests.test_gpu_block0 import block0, direct_cfg
from tests.test_gpu_h8 import (NO_POOL_CFGS, cfgs, conv_h8, f16_wino_cfgs, keyed_conv, replicate_ring, subpixel_upconv,
                               tol, wino_cfgs)

pytestmark = pytest.mark.gpu
X3, F16, R32 = _lib.PREC_F16X3, _lib.PREC_F16, _lib.PREC_F32R
PRECS = [R32, X3, F16]
NAME = {R32: "R32", X3: "F16X3", F16: "F16"}
N = 2
LINEAR, LEAKY, POOL, REP = _lib.EPI_LINEAR, _lib.EPI_LEAKY, _lib.EPI_LEAKY_POOL, _lib.EPI_LEAKY_REP
RAN = {}   # (prec, epilogue name) -> set of configs that ran through check_storage (test a)


def chunk(prec):
    return 2 * _lib.chans_per_record(prec)


def all_cfgs(prec, cin):
    """cfgs() of tests/test_gpu_h8.py without its co-block rule (bm <= 2 cout): cout 40 leaves the
    last co block short for every BM, BM 128 included.  Its alignment rules stay."""
    return cfgs(prec, 1 << 20, cin)


def kind(cfg):
    return _lib.lib().rrin_conv_h8_cfg_wino(cfg)


@functools.lru_cache(maxsize=None)
def inputs(n, c, h, w):
    return G.pattern((n, c, h, w), 1000 * c + 10 * h + w) * 0.5


@functools.lru_cache(maxsize=None)
def weights(cin, cout):
    return keyed_conv(cin, cout, "stor")


@functools.lru_cache(maxsize=None)
def reference(cin, cout, h, w, epi):
    """float64 reference of one case, computed once and shared: (full resolution, pooled or None)."""
    x = inputs(N, cin, h, w).double()
    wt, b = weights(cin, cout)
    if epi == "sub":
        up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        return F.conv2d(up, wt.double(), b.double(), padding=1), None
    y = F.conv2d(x, wt.double(), b.double(), padding=1)
    if epi != LINEAR:
        y = F.leaky_relu(y, 0.1)
    return y, (F.avg_pool2d(y, 2) if epi == POOL else None)


class Scratch:
    """The `alloc` of conv_h8 / subpixel_upconv: every scratch array inside guard bands (pattern),
    floats NaN, tickets zero; one array per name, reused within a case."""

    def __init__(self):
        self.arrays, self.before = {}, {}

    def __call__(self, name, numel, dtype, dev):
        a = self.arrays.get(name)
        if a is None or a.numel != numel:
            a = R.GuardedFlat(numel, dtype, dev, seed=len(self.arrays) + 3)
            self.arrays[name] = a
        if dtype == torch.float32:
            a.t.fill_(float("nan"))
        self.before[name] = a.snapshot()
        return a

    def check(self, what):
        for name, a in self.arrays.items():
            if name not in self.before:
                continue
            a.check_guards(self.before[name], f"{what}: {name}")
            if a.t.dtype == torch.int32:
                assert not bool(a.t.any()), f"{what}: {name}: a ticket is not back at zero"
            if name == "edge":
                assert not bool(torch.isnan(a.t).any()), f"{what}: edge: a ring entry was not written"
        self.before = {}


class Dst:
    """A guarded destination refilled with the same pattern before every config."""

    def __init__(self, c, h, w, dev, prec, seed):
        self.t = R.GuardedH8(N, c + 2 * chunk(prec), h, w, dev, prec, seed=seed)
        self.fill = [r.clone() for r in self.t.raw]
        self.before = self.t.snapshot()
        self.c, self.off = c, chunk(prec)

    def reset(self):
        for r, f in zip(self.t.raw, self.fill):
            r.copy_(f)

    def check(self, ref, tl, what, **kw):
        R.check_storage(self.before, self.t.snapshot(), self.t.storage(self.off, self.c), self.t.h, self.t.w, ref, tl,
                        what=what, **kw)


# ---- a. every config x every epilogue x every precision ---------------------------------------
PLAIN = [(epi, cin, cout, h, w) for epi in (LINEAR, LEAKY, REP) for cin, cout in ((16, 32), (64, 40))
         for h, w in ((9, 40), (17, 33))]
PLAIN += [(POOL, cin, cout, 18, 34) for cin, cout in ((16, 32), (64, 40))]
# the configs that keep every weight chunk resident in LDS, at the deepest K they hold: none of them
# fits cin 256 at any precision (rrin_conv_h8_cfg_fits), so the case runs at the largest of
# 256 / 192 / 128 / 96 that at least one of them fits (fp32 records and split-fp16: 96, fp16: 192)
PLAIN += [(LEAKY, "resident", 32, 9, 40)]
EPI_NAME = {LINEAR: "linear", LEAKY: "leaky", POOL: "pool", REP: "rep"}
# exclusions of the coverage assertion (test c), each with its reason
EXCLUDE = {
    "pool": lambda prec, c: c in NO_POOL_CFGS,             # one row per wave: no pool pair, RRIN_E_CONFIG
    "fold": lambda prec, c: kind(c) != 3,                  # the ring fold exists for Winograd kind 3 only
}


def resident_cfgs(prec):
    """Configs whose LDS need grows with cin (every weight chunk resident): they stop fitting."""
    lib = _lib.lib()
    return [c for c in range(lib.rrin_conv_h8_cfg_count())
            if lib.rrin_conv_h8_cfg_ok(c, prec) and not lib.rrin_conv_h8_cfg_fits(c, prec, 1 << 16)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi,cin,cout,h,w", PLAIN)
def test_conv_whole_storage(gpu, prec, epi, cin, cout, h, w):
    """LINEAR / LEAKY / LEAKY_POOL / LEAKY_REP: dst and pool through check_storage, every config."""
    resident = cin == "resident"
    if resident:
        cin = next(k for k in (256, 192, 128, 96) if set(all_cfgs(prec, k)) & set(resident_cfgs(prec)))
    x = inputs(N, cin, h, w).to(gpu)
    wt, b = weights(cin, cout)
    ref, refp = reference(cin, cout, h, w, epi)
    src = H8Tensor.from_nchw(x, prec)
    dst = Dst(cout, h, w, gpu, prec, 21)
    pool = Dst(cout, h // 2, w // 2, gpu, prec, 22) if epi == POOL else None
    todo = [c for c in all_cfgs(prec, cin) if not (epi == POOL and EXCLUDE["pool"](prec, c))]
    if resident:
        todo = [c for c in todo if c in resident_cfgs(prec)]
        assert todo
    for cfg in todo:
        dst.reset()
        if pool:
            pool.reset()
        what = f"cfg {cfg} (kind {kind(cfg)})"
        conv_h8(src, wt, b, cfg, prec, epi=epi, dst=dst.t, dst_off=dst.off, pool=pool.t if pool else None,
                pool_off=pool.off if pool else 0)
        dst.check(ref, tol(prec, cfg), what, ring="replicate" if epi == REP else None)
        if pool:
            pool.check(refp, tol(prec, cfg), what + " pool")
        if not resident:
            RAN.setdefault((prec, EPI_NAME[epi]), set()).add(cfg)


SUB = [(mode, cin, cout, sh, sw) for mode in ("fix", "inlaunch", "fold") for cin, cout in ((16, 32), (64, 40))
       for sh, sw in ((5, 9), (1, 2))]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode,cin,cout,sh,sw", SUB)
def test_subpixel_whole_storage(gpu, prec, mode, cin, cout, sh, sw):
    """EPI_SUBPIXEL with the separate fix-up, with ring_full in the launch and with the ring fold
    (kind 3): dst through check_storage; edge, part / cnt, ring_corr / ring_cnt inside guards,
    every edge entry written, tickets back at zero."""
    x = inputs(N, cin, sh, sw).to(gpu)
    wt, b = weights(cin, cout)
    ref, _ = reference(cin, cout, sh, sw, "sub")
    src = H8Tensor.from_nchw(x, prec)
    replicate_ring(src)
    dst = Dst(cout, 2 * sh, 2 * sw, gpu, prec, 23)
    todo = [c for c in all_cfgs(prec, cin) if not (mode == "fold" and EXCLUDE["fold"](prec, c))]
    sc = Scratch()
    for cfg in todo:
        dst.reset()
        subpixel_upconv(src, wt, b, cfg, prec, dst=dst.t, dst_off=dst.off, fold=mode == "fold",
                        inlaunch=mode == "inlaunch", alloc=sc, edge_split=mode == "fix" and prec == R32)
        what = f"cfg {cfg} (kind {kind(cfg)}) {mode}"
        dst.check(ref, tol(prec, cfg), what)
        sc.check(what)
        RAN.setdefault((prec, "sub_" + mode), set()).add(cfg)


@pytest.mark.parametrize("prec", [R32])
@pytest.mark.parametrize("ksplit", [2, 3])
def test_split_k_whole_storage(gpu, prec, ksplit):
    """Winograd kinds 3 and 4 with a split-K: part and cnt inside guards, tickets back at zero."""
    cin, cout, h, w = 64, 40, 17, 33
    x = inputs(N, cin, h, w).to(gpu)
    wt, b = weights(cin, cout)
    ref, _ = reference(cin, cout, h, w, LEAKY)
    src = H8Tensor.from_nchw(x, prec)
    dst = Dst(cout, h, w, gpu, prec, 24)
    sc = Scratch()
    ran = []
    for cfg in [c for c in all_cfgs(prec, cin) if kind(c) in (3, 4)]:
        dst.reset()
        conv_h8(src, wt, b, cfg, prec, epi=LEAKY, dst=dst.t, dst_off=dst.off, ksplit=ksplit, alloc=sc)
        dst.check(ref, tol(prec, cfg), f"cfg {cfg} ksplit {ksplit}")
        sc.check(f"cfg {cfg} ksplit {ksplit}")
        ran.append(kind(cfg))
    assert sorted(ran) == [3, 4]


# ---- c. coverage ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_coverage_is_every_config(prec):
    """The configs test (a) runs per precision and epilogue are every config the library offers
    (rrin_conv_h8_cfg_ok and a live id), minus EXCLUDE.  The alignment rules of cfgs() exclude
    nothing at cin 16 and 64; fp16 Winograd exists for kind 6 only (rrin_conv_h8_cfg_ok says so).
    Where test (a) ran in this session, what it recorded must be that plan."""
    lib = _lib.lib()
    offered = {c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_ok(c, prec) and kind(c) >= 0}
    assert offered
    kinds = {kind(c) for c in offered}
    assert kinds == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]
    assert {c for c in offered if kind(c) > 0} == set({R32: wino_cfgs(), X3: (), F16: f16_wino_cfgs()}[prec])
    for cin in (16, 64):
        assert set(all_cfgs(prec, cin)) == offered, (cin, offered - set(all_cfgs(prec, cin)))
    plan = {name: offered for name in ("linear", "leaky", "rep", "sub_fix", "sub_inlaunch")}
    plan["pool"] = {c for c in offered if not EXCLUDE["pool"](prec, c)}
    plan["sub_fold"] = {c for c in offered if not EXCLUDE["fold"](prec, c)}
    assert plan["pool"] == offered - set(NO_POOL_CFGS)
    assert (prec == R32) == bool(plan["sub_fold"])
    for name, want in plan.items():
        got = RAN.get((prec, name))
        print(f"{NAME[prec]} {name}: configs {sorted(want)} kinds {sorted({kind(c) for c in want})}")
        if got is not None:
            assert got == want, (name, sorted(want - got), sorted(got - want))


# ---- b. source views ------------------------------------------------------------------------------
# one direct-form config per workgroup size (h8_cfg.hpp: 128, 256, 512 threads) and one per Winograd kind
DIRECT_BY_THREADS = {128: 7, 256: 6, 512: 1}


def source_cfgs(prec, cin):
    ok = all_cfgs(prec, cin)
    out = [c for c in DIRECT_BY_THREADS.values() if c in ok]
    seen = set()
    for c in ok:
        if kind(c) > 0 and kind(c) not in seen:
            seen.add(kind(c))
            out.append(c)
    return out


def nan_source(x, prec, cin, dev, nan_tail):
    """x [n, cin, h, w] as the view [chunk, chunk + cin) of a NaN-filled guarded tensor: NaN groups
    before the view and after the whole chunks the conv may stage (chunk_view), NaN guard bands;
    the staged groups hold zero padding, and zeros past cin -- or NaN in [cin, 8 ceil(cin / 8))."""
    ck = chunk(prec)
    cview = (cin + ck - 1) // ck * ck
    src = R.GuardedH8(x.shape[0], 2 * ck + cview, x.shape[2], x.shape[3], dev, prec, nan=True)
    cpr = src.cpr
    hi, lo = R.nchw_to_records(x.cpu(), NAME[prec], cview // cpr, 0)
    if nan_tail:
        for ch in range(cin, (cin + 7) // 8 * 8):
            hi[:, ch // cpr, 1:src.h + 1, 8:8 + src.w, ch % cpr] = float("nan")
            if lo is not None:
                lo[:, ch // cpr, 1:src.h + 1, 8:8 + src.w, ch % cpr] = float("nan")
    src.put(hi, lo, slice(ck // cpr, (ck + cview) // cpr))
    return src, ck


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi,cin,cout,h,w", [(LEAKY, 16, 32, 9, 40), (LEAKY, 64, 40, 17, 33), (POOL, 16, 32, 18, 34),
                                              (REP, 64, 40, 9, 40), ("sub", 64, 40, 5, 9), ("sub", 16, 32, 1, 2)])
def test_source_view_offset_and_nan_neighbours(gpu, prec, epi, cin, cout, h, w):
    """The source as a view at g_off = one chunk of a larger tensor (img_stride exceeds the view)
    whose other groups, and whose guard bands, are NaN; the view's own padding is zero.

    What this sees: a read outside the view (a wrong g_off or image stride, a group past the
    chunk the conv is documented to stage, a row above or below the plane) whose value reaches an
    accumulator -- the output is then NaN, and the output must meet tol.  What it cannot see: a
    read whose value is discarded (a lane outside the image, a staged record no MFMA consumes)."""
    x = inputs(N, cin, h, w)
    wt, b = weights(cin, cout)
    ref, refp = reference(cin, cout, h, w, epi)
    src, off = nan_source(x, prec, cin, gpu, False)
    if epi == "sub":
        replicate_ring(SimpleView(src, off, (cin + off - 1) // off * off))
    snap = src.snapshot()
    ran = set()
    for cfg in source_cfgs(prec, cin):
        if epi == POOL and cfg in NO_POOL_CFGS:
            continue
        if epi == "sub":
            dst = subpixel_upconv(src, wt, b, cfg, prec, src_off=off)
            pool = None
        else:
            dst, pool = conv_h8(src, wt, b, cfg, prec, epi=epi, src_off=off)
        for t, r, nm in ((dst, ref, "dst"), (pool, refp, "pool")):
            if t is None:
                continue
            got = t.to_nchw().cpu().double()
            assert not bool(torch.isnan(got).any()), f"cfg {cfg}: NaN in {nm}"
            torch.testing.assert_close(got, r, **tol(prec, cfg), msg=lambda m: f"cfg {cfg} {nm}: {m}")
        ran.add(kind(cfg))
    assert ran == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]
    for a, s in zip(src.snapshot(), snap):
        assert torch.equal(R.bits(a), R.bits(s)), "the conv wrote into its source"


class SimpleView:
    """The groups of a view as the object replicate_ring() of tests/test_gpu_h8.py edits."""

    def __init__(self, t, ch_off, c):
        g0, g1 = ch_off // t.cpr, (ch_off + c + t.cpr - 1) // t.cpr
        self.h, self.w = t.h, t.w
        self.hi = t.hi[:, g0:g1]
        self.lo = t.lo[:, g0:g1] if t.lo is not None else None


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin", [6, 10])
def test_source_channel_tail_is_never_read(gpu, prec, cin):
    """tail_finite = 0: the channels [cin, 8 ceil(cin / 8)) of the source are NaN, for every config
    that accepts an unaligned cin (the direct-form tiles; the Winograd tiles stage whole records
    and are excluded by the alignment rules of cfgs()).  Sees and cannot see what the test above
    does; here a tail value that met a zero weight would also show (NaN x 0)."""
    cout, h, w = 32, 9, 40
    x = inputs(N, cin, h, w)
    wt, b = weights(cin, cout)
    ref, _ = reference(cin, cout, h, w, LINEAR)
    src, off = nan_source(x, prec, cin, gpu, True)
    todo = all_cfgs(prec, cin)
    assert todo and all(kind(c) == 0 for c in todo)
    lib = _lib.lib()
    assert set(todo) == {c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_ok(c, prec) and kind(c) == 0}
    for cfg in todo:
        dst, _ = conv_h8(src, wt, b, cfg, prec, src_off=off, cin=cin)
        got = dst.to_nchw().cpu().double()
        assert not bool(torch.isnan(got).any()), f"cfg {cfg}: NaN in dst"
        torch.testing.assert_close(got, ref, **tol(prec, cfg), msg=lambda m: f"cfg {cfg}: {m}")


# ---- d. fused level-0 block and the ring fix-up ----------------------------------------------------
@pytest.mark.parametrize("cin", [6, 16])
@pytest.mark.parametrize("h,w", [(9, 40), (18, 34)])
def test_block0_whole_storage(gpu, cin, h, w):
    """rrin_conv_block0_h8_fwd (fp16): dst and pool (even sizes) through check_storage."""
    x = inputs(N, cin, h, w)
    wa, ba = keyed_conv(cin, 32, "stor0a")
    wb, bb = keyed_conv(32, 32, "stor0b")
    mid = F.leaky_relu(F.conv2d(x.double(), wa.double(), ba.double(), padding=1), 0.1)
    ref = F.leaky_relu(F.conv2d(mid, wb.double(), bb.double(), padding=1), 0.1)
    pooled = h % 2 == 0
    # channels [cin, 16) of the source are zeros: finite, as tail_finite promises
    src = H8Tensor.from_nchw(x.to(gpu), F16)
    dst = Dst(32, h, w, gpu, F16, 31)
    pool = Dst(32, h // 2, w // 2, gpu, F16, 32) if pooled else None
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    block0(src, cin, wa, ba, direct_cfg(cin, 32), wb, bb, direct_cfg(32, 32), pooled, dst=dst.t, dst_off=dst.off,
           status=status, tail_finite=1 if cin % 8 else 0, pl=pool.t if pool else None, pool_off=pool.off if pool else 0)
    assert int(status.item()) == 0
    dst.check(ref, tol(F16, 0), "block0")
    if pool:
        pool.check(F.avg_pool2d(ref, 2), tol(F16, 0), "block0 pool")


@pytest.mark.parametrize("prec,split", [(R32, False), (R32, True), (X3, False), (F16, False)])
@pytest.mark.parametrize("full", [False, True])
def test_edge_fix_writes_only_the_ring(gpu, prec, split, full):
    """rrin_subpixel_edge_fix_h8, correction and from scratch, with and without the K split at cin
    128: it writes only ring pixels of the view's groups -- the interior keeps the bits the conv
    left (correction) or the pattern (full), like everything else -- and the ring meets tol."""
    cin, cout, sh, sw = 128, 40, 5, 9
    x = inputs(N, cin, sh, sw).to(gpu)
    wt, b = weights(cin, cout)
    ref, _ = reference(cin, cout, sh, sw, "sub")
    src = H8Tensor.from_nchw(x, prec)
    replicate_ring(src)
    cfg = next(c for c in all_cfgs(prec, cin) if prec != R32 or kind(c) == 3)
    dst = Dst(cout, 2 * sh, 2 * sw, gpu, prec, 33)
    sc = Scratch()
    if not full:
        subpixel_upconv(src, wt, b, cfg, prec, dst=dst.t, dst_off=dst.off, alloc=sc, fix=False)
        dst.before = dst.t.snapshot()       # what the conv left
        edge = sc.arrays["edge"]
        sc.arrays = {"edge": edge}
        keep_edge = edge.t.clone()
        alloc = lambda name, numel, dtype, dev: (edge if name == "edge" else sc(name, numel, dtype, dev))  # noqa: E731
        subpixel_upconv(src, wt, b, cfg, prec, dst=dst.t, dst_off=dst.off, alloc=alloc, conv=False, edge_split=split)
        assert torch.equal(edge.t, keep_edge), "the fix-up wrote into edge"
    else:
        subpixel_upconv(src, wt, b, cfg, prec, dst=dst.t, dst_off=dst.off, alloc=sc, full=True, conv=False,
                        edge_split=split)
    ringpix = torch.zeros(2 * sh, 2 * sw, dtype=torch.bool)
    ringpix[0], ringpix[-1], ringpix[:, 0], ringpix[:, -1] = True, True, True, True
    dst.check(ref, tol(prec, cfg), f"edge fix full={full} split={split}", interior_mask=ringpix)
    if split:
        assert "fix_part" in sc.arrays and "fix_cnt" in sc.arrays
    sc.before.pop("edge", None)
    for name in ("fix_part", "fix_cnt"):
        if name in sc.arrays:
            sc.arrays[name].check_guards(sc.before[name], name)
    if "fix_cnt" in sc.arrays:
        assert not bool(sc.arrays["fix_cnt"].t.any())


# ---- e. layout kernels against the CPU codec -------------------------------------------------------
def assert_planes_equal(t, want, what):
    for p, (a, wnt) in enumerate(zip(t.planes(), want)):
        bad = R.bits(a.cpu()) != R.bits(wnt)
        assert not bool(bad.any()), f"{what}: plane {p}: first difference at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", [3, 11, 16])
@pytest.mark.parametrize("off_groups", [0, 1])
def test_nchw_to_h8_is_the_cpu_encoder(gpu, prec, c, off_groups):
    """rrin_nchw_to_h8 into pattern-filled guarded storage: the c channels' interior elements are
    bitwise the CPU encoder's, and nothing else changes -- the other channels of a partly covered
    record included (the kernel stores one element per value, never a whole record)."""
    h, w = 9, 40
    t = R.GuardedH8(N, 24, h, w, gpu, prec, seed=41)
    before = t.snapshot()
    x = G.pattern((N, c, h, w), 77) * 37
    ch_off = off_groups * t.cpr
    t.load(x.to(gpu), ch_off)
    torch.cuda.synchronize()
    enc = R.nchw_to_records(x, NAME[prec], t.groups, ch_off)
    want = []
    for k, e in enumerate(e for e in enc if e is not None):
        wnt = before[k][t.guard:t.guard + t.hi.numel()].view(t.hi.shape).clone()
        for ch in range(ch_off, ch_off + c):
            sel = (slice(None), ch // t.cpr, slice(1, h + 1), slice(8, 8 + w), ch % t.cpr)
            wnt[sel] = e[sel]
        want.append(wnt)
    assert_planes_equal(t, want, "nchw_to_h8")
    R.check_storage(before, t.snapshot(), t.storage(ch_off, c), h, w, G.store_round(x, NAME[prec]).double(),
                    dict(rtol=0.0, atol=0.0), what="nchw_to_h8")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ch_off,c", [(0, 24), (3, 11), (8, 5)])
def test_h8_to_nchw_is_the_cpu_decoder(gpu, prec, ch_off, c):
    """rrin_h8_to_nchw of pattern-filled storage (garbage in the padding and in the neighbouring
    groups) is bitwise glue_ref.records_to_nchw, and writes nothing into the records."""
    h, w = 9, 40
    t = R.GuardedH8(N, 24, h, w, gpu, prec, seed=43)
    before = t.snapshot()
    got = t.to_nchw(ch_off, c).cpu()
    want = G.records_to_nchw(t.hi.cpu(), t.lo.cpu() if t.lo is not None else None, ch_off, c, h, w)
    assert torch.equal(R.bits(got), R.bits(want))
    for a, s in zip(t.snapshot(), before):
        assert torch.equal(R.bits(a), R.bits(s))


@pytest.mark.parametrize("prec", PRECS)
def test_pack_g16_against_the_cpu_encoder(gpu, prec):
    """rrin_pack_g16_h8: channels 0-5 bitwise the encoder's, channels 6-15 zero (whole-record
    stores), the padding and the groups past channel 15 untouched."""
    h, w = 9, 40
    t = R.GuardedH8(N, 24, h, w, gpu, prec, seed=45)
    before = t.snapshot()
    i0, i1 = G.pattern((N, 3, h, w), 5).abs() * 0.5, G.pattern((N, 3, h, w), 6).abs() * 0.5
    v = t.view(0, 16)
    a, b_ = i0.to(gpu), i1.to(gpu)
    _lib.check(_lib.lib().rrin_pack_g16_h8(a.data_ptr(), b_.data_ptr(), N, C.byref(v), prec, H.stream(gpu)))
    torch.cuda.synchronize()
    x = torch.cat([i0, i1, torch.zeros(N, 10, h, w)], 1)
    enc = R.nchw_to_records(x, NAME[prec], t.groups, 0)
    want = []
    g16 = 16 // t.cpr
    for k, e in enumerate(e for e in enc if e is not None):
        wnt = before[k][t.guard:t.guard + t.hi.numel()].view(t.hi.shape).clone()
        wnt[:, :g16, 1:h + 1, 8:8 + w] = e[:, :g16, 1:h + 1, 8:8 + w]
        want.append(wnt)
    assert_planes_equal(t, want, "pack_g16")
    R.check_storage(before, t.snapshot(), t.storage(0, 16), h, w, G.store_round(x, NAME[prec]).double(),
                    dict(rtol=0.0, atol=0.0), what="pack_g16")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sh,sw", [(5, 7), (1, 1)])
def test_upsample_whole_storage(gpu, prec, sh, sw):
    """rrin_upsample2x_h8 into a view of guarded storage: the interior within test_h8_upsample's
    tolerance of float64 F.interpolate, everything else bitwise untouched."""
    c = 16
    x = inputs(N, c, sh, sw)
    src = H8Tensor.from_nchw(x.to(gpu), prec)
    dst = Dst(c, 2 * sh, 2 * sw, gpu, prec, 47)
    sv, dv = src.view(), dst.t.view(dst.off, c)
    _lib.check(_lib.lib().rrin_upsample2x_h8(C.byref(sv), C.byref(dv), N, prec, H.stream(gpu)))
    torch.cuda.synchronize()
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    dst.check(ref, dict(rtol=0.0, atol=2e-3 if prec == F16 else 1e-6), "upsample2x")


# ---- f. the fp16 range guard at its edges -----------------------------------------------------------
F16MAX = 65504.0


def one_tap(cin, cout, co, ky, kx, bias=0.0):
    wt, b = torch.zeros(cout, cin, 3, 3), torch.zeros(cout)
    wt[co, 0, ky, kx] = 1.0
    b[co] = bias
    return wt, b


def guard_cfgs(prec):
    """Every config that runs at prec; cin 8, or 16 where the config stages 16-channel chunks (the
    fp16 Winograd kind 6) -- the extra channels are zero, the construction stays exact."""
    return [(c, 8) for c in all_cfgs(prec, 8)] + [(c, 16) for c in all_cfgs(prec, 16) if c not in all_cfgs(prec, 8)]


def run_guard(gpu, prec, cfg, cin, x, wt, b, epi, status=None):
    status = torch.zeros(1, dtype=torch.int32, device=gpu) if status is None else status
    xx = torch.zeros(x.shape[0], cin, *x.shape[2:])
    xx[:, :x.shape[1]] = x
    dst, pool = conv_h8(H8Tensor.from_nchw(xx.to(gpu), prec), wt, b, cfg, prec, epi=epi, status=status, cin=cin)
    return int(status.item()), dst, pool


def expect_flag(prec, over):
    return int(over and prec != R32)   # exact fp32 records never set it


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_range_guard_threshold(gpu, prec, sign):
    """x = +-65504 under the centre tap: the flag stays clear and the stored value is +-65504;
    with bias +-16 (65520, which rounds to inf) it is set (R32: never).  LINEAR; output = x + bias
    exactly (an 11-bit by 1-bit product in fp32, inv_wscale a power of two)."""
    n, h, w, cout = 2, 17, 33, 40
    x = torch.zeros(n, 1, h, w)
    x[1, 0, 8, 16] = sign * F16MAX
    for cfg, cin in guard_cfgs(prec):
        wt, b = one_tap(cin, cout, 39, 1, 1)
        flag, dst, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, LINEAR)
        got = dst.to_nchw().cpu()
        assert flag == 0, f"cfg {cfg}: false alarm at {sign * F16MAX}"
        if prec == R32:
            torch.testing.assert_close(got[1, 39, 8, 16].double(), torch.tensor(sign * F16MAX).double(), **tol(prec, cfg))
        else:
            assert float(got[1, 39, 8, 16]) == sign * F16MAX, f"cfg {cfg}"
        wt, b = one_tap(cin, cout, 39, 1, 1, sign * 16.0)
        flag, _, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, LINEAR)
        assert flag == expect_flag(prec, True), f"cfg {cfg}: {sign * 65520.0} not flagged"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi", [LINEAR, LEAKY, REP])
def test_range_guard_placement(gpu, prec, epi):
    """One offending value (65520) at pixel (h - 1, w - 1), the last real channel of cout 40, the
    last image, 17 x 33: every direct-form config (the wide whole-record stores of conv_h8.hip's
    kWide path at fp16 / split-fp16, BM 32, 64 and 128) and every Winograd kind of the precision.
    A set flag is not cleared by a later in-range call into the same status."""
    n, h, w, cout = 2, 17, 33, 40
    x = torch.zeros(n, 1, h, w)
    x[1, 0, h - 1, w - 1] = F16MAX
    for cfg, cin in guard_cfgs(prec):
        wt, b = one_tap(cin, cout, 39, 1, 1, 16.0)
        status = torch.zeros(1, dtype=torch.int32, device=gpu)
        flag, _, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, epi, status)
        assert flag == expect_flag(prec, True), f"cfg {cfg}"
        wt, b = one_tap(cin, cout, 39, 1, 1, 0.0)
        flag, _, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, epi, status)
        assert flag == expect_flag(prec, True), f"cfg {cfg}: an in-range call cleared the flag"
        flag, _, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, epi)
        assert flag == 0, f"cfg {cfg}: false alarm"


@pytest.mark.parametrize("prec", PRECS)
def test_range_guard_pool(gpu, prec):
    """LEAKY_POOL: (i) one full-resolution value of 65520 in the last 2 x 2 block -- its pooled value
    16380 is in range, the flag is set by the full-resolution store; (ii) all four values of the
    block 65504 -- the pooled value is exactly 65504, nothing exceeds the range, the flag stays 0.
    (ii) reaches 65504 as 16376 x 1 + 49128: the fp16 Winograd tile (kind 6) forms sums of up to
    four neighbouring inputs in fp16 in its input transform, so four adjacent inputs of 65504
    overflow there, before any store ("Whole-storage tests")."""
    n, h, w, cout = 2, 18, 34, 40
    for cfg, cin in guard_cfgs(prec):
        if cfg in NO_POOL_CFGS:
            continue
        x = torch.zeros(n, 1, h, w)
        x[1, 0, h - 1, w - 1] = F16MAX
        flag, _, pool = run_guard(gpu, prec, cfg, cin, x, *one_tap(cin, cout, 39, 1, 1, 16.0), POOL)
        assert flag == expect_flag(prec, True), f"cfg {cfg} (i)"
        x[1, 0, h - 2:, w - 2:] = 16376.0
        flag, dst, pool = run_guard(gpu, prec, cfg, cin, x, *one_tap(cin, cout, 39, 1, 1, 49128.0), POOL)
        assert flag == 0, f"cfg {cfg} (ii): false alarm"
        if prec != R32:
            assert float(dst.to_nchw().cpu()[1, 39, -1, -1]) == F16MAX, f"cfg {cfg}"
            assert float(pool.to_nchw().cpu()[1, 39, -1, -1]) == F16MAX, f"cfg {cfg}"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ["column_w", "row_h", "channels_past_cout"])
def test_range_guard_no_false_alarm_from_discarded_lanes(gpu, prec, case):
    """Values the kernel computes and discards must not raise the flag.  column_w: the only weight
    is the left tap (kx = 0) and the only input 65504 at pixel (h - 1, w - 1), plus a bias of 16:
    the out-of-range 65520 exists only in column w, outside the image (every real output is
    16).  row_h: the same with the top tap (ky = 0): 65520 only in row h.
    channels_past_cout: cout 40 on the BM 64 / 128 configs, whose co block computes channels 40 up
    to BM - 1 from zero weights and the zero bias tail rrin_pack_bias_floats leaves; the real
    channels sit at exactly 65504."""
    n, h, w, cout = 2, 17, 33, 40
    x = torch.zeros(n, 1, h, w)
    x[1, 0, h - 1, w - 1] = F16MAX
    lib = _lib.lib()
    for cfg, cin in guard_cfgs(prec):
        wt, b = torch.zeros(cout, cin, 3, 3), torch.zeros(cout)
        if case == "column_w":
            wt[:, 0, 1, 0] = 1.0      # out(y, x) = in(y, x - 1) + 16: 65520 at (h - 1, w) only
            b[:] = 16.0
        elif case == "row_h":
            wt[:, 0, 0, 1] = 1.0      # out(y, x) = in(y - 1, x) + 16: 65520 at (h, w - 1) only
            b[:] = 16.0
        else:
            if lib.rrin_conv_h8_cfg_bm(cfg) < 64:
                continue
            wt[:, 0, 1, 1] = 1.0
        for epi in (LINEAR, LEAKY):
            flag, dst, _ = run_guard(gpu, prec, cfg, cin, x, wt, b, epi)
            assert flag == 0, f"cfg {cfg} epi {epi}: false alarm"
        if prec != R32:
            got = dst.to_nchw().cpu()
            want = F16MAX if case == "channels_past_cout" else 16.0
            assert float(got[1, 39, h - 1, w - 1]) == want, f"cfg {cfg}"


@pytest.mark.parametrize("prec", PRECS)
def test_range_guard_subpixel(gpu, prec):
    """EPI_SUBPIXEL (the half-record store4 path of the direct-form tiles) and the ring fix-up, each
    with a flag of its own.  The low-resolution source is 65504 at its last pixel (and in that
    pixel's replicated ring), channel 0, last image; the original weight is the centre tap of
    output channel 39.  Then, exactly (products of 65504 = 2047 x 32 with k / 16):
    the corner ring pixel (H - 1, W - 1) = 65504 + bias, the interior pixel (H - 2, W - 2) =
    0.5625 x 65504 + bias = 36846 + bias, and nothing is larger.
      bias 0: both flags stay 0;  bias 16: only the fix-up's (65520 on the ring);
      bias 28674: both (the interior reaches 65520).
    Direct-form configs: a single 65504 next to its replicated copies overflows fp16 inside the
    input transform of the fp16 Winograd tile (d1 + d2 = 131008), which is not a store."""
    n, sh, sw, cin, cout = 2, 5, 9, 16, 40
    x = torch.zeros(n, cin, sh, sw)
    x[1, 0, sh - 1, sw - 1] = F16MAX
    src = H8Tensor.from_nchw(x.to(gpu), prec)
    replicate_ring(src)
    for cfg in [c for c in all_cfgs(prec, cin) if kind(c) == 0 or prec == R32]:
        for bias, want in ((0.0, (0, 0)), (16.0, (0, 1)), (28674.0, (1, 1))):
            wt, b = one_tap(cin, cout, 39, 1, 1, bias)
            st = torch.zeros(2, dtype=torch.int32, device=gpu)
            dst = subpixel_upconv(src, wt, b, cfg, prec, status=st[0:1], fix_status=st[1:2])
            got = tuple(int(v) for v in st.cpu())
            assert got == tuple(expect_flag(prec, v) for v in want), f"cfg {cfg} bias {bias}: flags {got}"
            if prec != R32 and bias == 0.0:
                o = dst.to_nchw().cpu()
                inner = float(G.store_round(torch.tensor([36846.0]), NAME[prec]))   # fp16 holds 36832
                assert float(o[1, 39, -1, -1]) == F16MAX and float(o[1, 39, -2, -2]) == inner, f"cfg {cfg}"
