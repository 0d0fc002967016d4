"""GPU: the record-layout convs held to equality on data where every summation order gives the
same bits (tests/exact_ref.py; DESIGN.md §8b, "Exact values").

Inputs and weights are +-1 / +-2, the bias +-1..3, the slope 1/4; split-fp16 carries +-2^-12 in a
quarter of its lo halves and is held to the exact hx*hw + hx*lw + lx*hw; kind 14 takes the weights
times 48 (its G has 1/24).  The comparison is == on every interior element; at split-fp16 the hi
and lo planes equal the CPU record encoder's of the reference bit for bit; under LEAKY_REP the
ring equals the replicated border.  Every destination's interior starts as NaN.  The
representability of each case's data (fp16 results, fp32 sums below 2^24, packed weights equal to
their rational values) is asserted in tests/test_exact_ref.py without a GPU, and where cheap here.

Kind 14 is held to equality like every other kind: exact_ref.wino_fits (every intermediate
below 2^24 grid steps, worst case over the data's magnitudes) holds for each of its cases, the
sub-pixel conv at cin 64 (U on a grid of 1/8) and cin 256 included, and is asserted before each run.

Part B (test_conv_float_bound): random floats the storage holds exactly, against float64 within a
derived per-element forward bound (exact_ref.bound), the observed worst ratio printed;
test_subpixel_float_bound does the same for the sub-pixel up conv, its ring pixels under
exact_ref.ring_bound (the operation count of the fix-up, per ring mode)."""
import functools

import numpy as np
import pytest
import torch

from rrin_amd import _lib
from rrin_amd.pp import H8Tensor
from tests import exact_ref as E
from tests import record_ref as R
from tests.test_gpu_block0 import block0, direct_cfg
from tests.test_gpu_h8 import NO_POOL_CFGS, cfgs, conv_h8, pack_h8, replicate_ring, subpixel_upconv

pytestmark = pytest.mark.gpu
X3, F16, R32 = _lib.PREC_F16X3, _lib.PREC_F16, _lib.PREC_F32R
PRECS = [R32, X3, F16]
NAME = {R32: "R32", X3: "F16X3", F16: "F16"}
LINEAR, LEAKY, POOL, REP = _lib.EPI_LINEAR, _lib.EPI_LEAKY, _lib.EPI_LEAKY_POOL, _lib.EPI_LEAKY_REP
EPI_NAME = {LINEAR: "linear", LEAKY: "leaky", POOL: "pool", REP: "rep"}
N = 2
RAN = {}                  # (prec, epilogue name) -> configs that ran


def kind(cfg):
    return _lib.lib().rrin_conv_h8_cfg_wino(cfg)


def all_cfgs(prec, cin):
    return cfgs(prec, 1 << 20, cin)


def resident_cfgs(prec):
    lib = _lib.lib()
    return [c for c in range(lib.rrin_conv_h8_cfg_count())
            if lib.rrin_conv_h8_cfg_ok(c, prec) and not lib.rrin_conv_h8_cfg_fits(c, prec, 1 << 16)]


def wmul(cfg):
    return 48 if kind(cfg) == 14 else 1


def source(x, prec, dev, c_alloc=None, ch_off=0):
    """x (float64 numpy, fp32-exact) as an H8Tensor through the CPU record encoder; the channels
    before ch_off are NaN."""
    n, c, h, w = x.shape
    t = H8Tensor(n, c_alloc or c, h, w, dev, prec)
    assert E.f32_exact(x)
    hi, lo = R.nchw_to_records(torch.from_numpy(np.ascontiguousarray(x)).float(), NAME[prec], t.groups, ch_off)
    t.hi.copy_(hi.to(dev))
    if lo is not None:
        t.lo.copy_(lo.to(dev))
    if ch_off:
        t.hi[:, :ch_off // t.cpr] = float("nan")
        if t.lo is not None:
            t.lo[:, :ch_off // t.cpr] = float("nan")
    return t


def fresh(t):
    """Zero padding, NaN interior of the groups that hold the c channels: an element the conv does
    not write fails the comparison.  The spare group of the last 2-group chunk stays zero."""
    for a in (t.hi, t.lo):
        if a is not None:
            a.zero_()
            a[:, :(t.c + t.cpr - 1) // t.cpr, 1:t.h + 1, 8:8 + t.w] = float("nan")


def assert_equal(t, off, c, ref, prec, what):
    """The decoded channels [off, off + c) of t == ref (float64) everywhere; split-fp16: both
    planes bit for bit the CPU encoder's."""
    got = t.to_nchw(off, c).cpu().double().numpy()
    bad = ~(got == ref)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at (image, channel, y, x) {i}: "
                             f"got {got[i]!r}, exact {ref[i]!r}")
    if prec == X3:
        hi, lo = E.records(ref, "F16X3", c // 8)
        g0 = off // 8
        sel = (slice(None), slice(g0, g0 + c // 8), slice(1, t.h + 1), slice(8, 8 + t.w))
        isel = (slice(None), slice(None), slice(1, t.h + 1), slice(8, 8 + t.w))
        assert torch.equal(R.bits(t.hi[sel].cpu()), R.bits(hi[isel])), f"{what}: hi plane is not the encoder's"
        assert torch.equal(R.bits(t.lo[sel].cpu()), R.bits(lo[isel])), f"{what}: lo plane is not the encoder's"


def assert_ring(t, what):
    """LEAKY_REP: the ring equals the replicated border, the rest of the padding is zero."""
    want = H8Tensor(t.n, t.c, t.h, t.w, t.hi.device, t.prec)
    for a, b_ in ((want.hi, t.hi), (want.lo, t.lo)):
        if a is not None:
            a[:, :, 1:t.h + 1, 8:8 + t.w] = b_[:, :, 1:t.h + 1, 8:8 + t.w]
    replicate_ring(want)
    assert torch.equal(R.bits(t.hi), R.bits(want.hi)), f"{what}: ring"
    if t.lo is not None:
        assert torch.equal(R.bits(t.lo), R.bits(want.lo)), f"{what}: ring (lo)"


def tensors(wt, b, ow, prec, mul):
    """fp32 torch weights and bias of a case: mul wt (+ ow 2^-12 at split-fp16), mul b."""
    w64 = mul * wt.astype(np.float64) + (ow / E.LO if prec == X3 else 0.0)
    assert E.f32_exact(w64)
    return torch.from_numpy(w64).float(), torch.from_numpy((mul * b).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(n, cin, cout, h, w, mags, split, mul, epi):
    """(full resolution, pooled or None) float64, exact; computed once per case."""
    x, wt, b, ox, ow = E.split_case(n, cin, cout, h, w, mags) if split else E.int_case(n, cin, cout, h, w, mags)
    if epi == "sub":
        r = E.pre_sub_split(x, wt, b, ox) if split else E.pre_sub(x, wt, b, mul)
        return r.f64(), None
    r = E.pre_split(x, wt, b, ox, ow) if split else E.pre_int(x, wt, b, mul)
    if epi != LINEAR:
        pre = r.units
        assert (pre > 0).any() and (pre < 0).any()            # both sides of y > 0 ...
        assert (pre == 0).sum() >= 2                          # ... and 0 itself (split-fp16: split_case keeps them)
        r = E.leaky(r)
    return r.f64(), (E.pool(r).f64() if epi == POOL else None)


def run_plain(gpu, prec, epi, n, cin, cout, h, w, mags, todo, ksplit=0, record=True):
    split = prec == X3
    x, wt, b, ox, ow = E.split_case(n, cin, cout, h, w, mags) if split else E.int_case(n, cin, cout, h, w, mags)
    xf = x.astype(np.float64) + (ox / E.LO if split else 0.0)
    src = source(xf, prec, gpu)
    if split:
        assert bool(src.lo.any())
    dst = H8Tensor(n, cout, h, w, gpu, prec)
    pool = H8Tensor(n, cout, h // 2, w // 2, gpu, prec) if epi == POOL else None
    ran = []
    for cfg in todo:
        mul = wmul(cfg)
        what = f"{NAME[prec]} {EPI_NAME[epi]} cin {cin} {h}x{w} cfg {cfg} (kind {kind(cfg)}) ksplit {ksplit}"
        if kind(cfg) > 0:   # F(2x2) too: every intermediate below 2^24 (fp16 kind 6: its fp32 accumulator)
            k = 14 if kind(cfg) == 14 else 1
            assert E.wino_fits(k, mul * wt, 1, cin, max(mags))[0], what
        else:
            assert E.direct_sum_units(x, wt, b) * (E.LO + 2 if split else 1) < E.P24   # + 2: the two hi*lo classes
        wt_t, b_t = tensors(wt, b, ow, prec, mul)
        packed = pack_h8(wt_t, b_t, cfg, prec, gpu)
        if split:
            assert bool(packed[1].any()), "wlo blob is zero"
        ref, refp = reference(n, cin, cout, h, w, mags, split, mul, epi)
        fresh(dst)
        if pool is not None:
            fresh(pool)
        conv_h8(src, wt_t, b_t, cfg, prec, epi=epi, dst=dst, pool=pool, packed=packed, slope=E.SLOPE, ksplit=ksplit)
        assert_equal(dst, 0, cout, ref, prec, what)
        if pool is not None:
            assert_equal(pool, 0, cout, refp, prec, what + " pool")
        if epi == REP:
            assert_ring(dst, what)
        ran.append(cfg)
        if record:
            RAN.setdefault((prec, EPI_NAME[epi]), set()).add(cfg)
    return ran


# ---- A. every config x epilogue x precision -------------------------------------------------------
PLAIN = [(epi, cin, cout, h, w) for epi in (LINEAR, LEAKY, REP) for cin, cout in ((16, 32), (64, 40))
         for h, w in ((9, 40), (17, 33))]
PLAIN += [(POOL, cin, cout, 18, 34) for cin, cout in ((16, 32), (64, 40))]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi,cin,cout,h,w", PLAIN)
def test_conv_exact(gpu, prec, epi, cin, cout, h, w):
    """LINEAR / LEAKY / LEAKY_REP / LEAKY_POOL at every config: == the int64 reference.  The pool
    cases use +-1 alone: the pooled value sits on a grid of 1/16 and must stay an fp16 number."""
    mags = (1,) if epi == POOL else (1, 2)
    todo = [c for c in all_cfgs(prec, cin) if not (epi == POOL and c in NO_POOL_CFGS)]
    assert run_plain(gpu, prec, epi, N, cin, cout, h, w, mags, todo)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("which", ["cin256", "resident"])
def test_conv_exact_deep_k(gpu, prec, which):
    """n 1, 9 x 40, +-1, LEAKY: cin 256 (32 K chunks of 8) for the streaming configs, and the
    weight-resident ones at the deepest cin one of them holds (96; fp16: 192)."""
    if which == "cin256":
        cin, todo = 256, all_cfgs(prec, 256)
    else:
        cin = next(k for k in (256, 192, 128, 96) if set(all_cfgs(prec, k)) & set(resident_cfgs(prec)))
        todo = [c for c in all_cfgs(prec, cin) if c in resident_cfgs(prec)]
    assert todo
    ran = run_plain(gpu, prec, LEAKY, 1, cin, 32, 9, 40, (1,), todo, record=False)
    if which == "cin256":
        assert {kind(c) for c in ran} == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]


@pytest.mark.parametrize("ksplit", [2, 3, 8])
def test_split_k_exact(gpu, ksplit):
    """Winograd kinds 3 and 4 with 2, 3 and 8 K slices at cin 64 (8 chunks): a slice added twice
    or left out moves every output of its co block."""
    todo = [c for c in all_cfgs(R32, 64) if kind(c) in (3, 4)]
    ran = run_plain(gpu, R32, LEAKY, N, 64, 40, 17, 33, (1, 2), todo, ksplit=ksplit, record=False)
    assert sorted(kind(c) for c in ran) == [3, 4]


@pytest.mark.parametrize("prec", PRECS)
def test_source_offset_and_perm_exact(gpu, prec):
    """The source as the view [16, 32) of a 32-channel tensor whose first 16 channels are NaN, with
    an input permutation in the pack: == conv(x, w[:, perm]), one config per kind."""
    n, cin, cout, h, w = N, 16, 32, 9, 40
    x, wt, b, ox, ow = E.int_case(n, cin, cout, h, w, (1, 2), tag=1)
    perm = [(5 * c + 3) % cin for c in range(cin)]
    split = prec == X3
    src = source(x.astype(np.float64) + (ox / E.LO if split else 0.0), prec, gpu, c_alloc=32, ch_off=16)
    wp, owp = wt[:, perm], ow[:, perm]
    r = E.pre_split(x, wp, b, ox, owp) if split else None
    seen = set()
    for cfg in all_cfgs(prec, cin):
        if kind(cfg) in seen:
            continue
        seen.add(kind(cfg))
        mul = wmul(cfg)
        wt_t, b_t = tensors(wt, b, ow, prec, mul)
        packed = pack_h8(wt_t, b_t, cfg, prec, gpu, perm)
        ref = (r if split else E.pre_int(x, wp, b, mul)).f64()
        dst = H8Tensor(n, cout, h, w, gpu, prec)
        fresh(dst)
        conv_h8(src, wt_t, b_t, cfg, prec, dst=dst, packed=packed, src_off=16, slope=E.SLOPE)
        assert_equal(dst, 0, cout, ref, prec, f"{NAME[prec]} offset + perm cfg {cfg}")
    assert seen == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]


# 3 x 33: output rows of 66 px, two fix-up tiles of 32 and a ragged third; 18 x 3: columns of 34 px
SUB_SHAPES = ((5, 9), (1, 2), (3, 33), (18, 3))
SUB = [(mode, cin, cout, sh, sw) for mode in ("fix", "inlaunch", "fold") for cin, cout in ((16, 32), (64, 40))
       for sh, sw in SUB_SHAPES]
RAN_SUB = {}              # (prec, mode, cin, sh, sw) -> configs that ran


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode,cin,cout,sh,sw", SUB)
def test_subpixel_exact(gpu, prec, mode, cin, cout, sh, sw):
    """conv3x3(upsample_x2(x)) as the sub-pixel conv with the separate fix-up (fp32: with its K
    split), with ring_full in the launch and with the ring fold (kind 3): == the int64 reference in
    sixteenths, ring pixels included.  +-1 data (an fp16 result on a grid of 1/16 stays below
    128).  Split-fp16 carries the +-2^-12 offsets in the source alone (lo plane asserted non-zero):
    the phase-combined weights k / 16 w are fp16 numbers, lx*hw is exact and the reference linear in
    x; an offset on w would give k / 16 (w + lo), which does not split into the integer's and the
    offset's share, so the wlo side of the three-product form is held by the plain convs."""
    n = N
    split = prec == X3
    x, wt, b, ox, ow = E.split_case(n, cin, cout, sh, sw, (1,)) if split else E.int_case(n, cin, cout, sh, sw, (1,))
    src = source(x.astype(np.float64) + (ox / E.LO if split else 0.0), prec, gpu)
    if split:
        assert bool(src.lo.any())
    replicate_ring(src)
    dst = H8Tensor(n, cout, 2 * sh, 2 * sw, gpu, prec)
    wsub = E.subpixel_weights_int(wt)
    todo = [c for c in all_cfgs(prec, cin) if not (mode == "fold" and kind(c) != 3)]
    for cfg in todo:
        mul = wmul(cfg)
        what = f"{NAME[prec]} sub {mode} cin {cin} {sh}x{sw} cfg {cfg} (kind {kind(cfg)})"
        if kind(cfg) > 0:
            assert E.wino_fits(14 if kind(cfg) == 14 else 1, mul * wsub, 16, cin, 1)[0], what
        wt_t, b_t = tensors(wt, b, 0 * ow, R32, mul)
        ref, _ = reference(n, cin, cout, sh, sw, (1,), split, mul, "sub")
        if prec == F16:   # one rounding of the exact fp32 value (the identity while sixteenths fit 11 bits)
            ref = E.f16_round(ref)
        fresh(dst)
        subpixel_upconv(src, wt_t, b_t, cfg, prec, dst=dst, fold=mode == "fold", inlaunch=mode == "inlaunch",
                        edge_split=mode == "fix" and prec == R32)
        assert_equal(dst, 0, cout, ref, prec, what)
        RAN.setdefault((prec, "sub_" + mode), set()).add(cfg)
        RAN_SUB.setdefault((prec, mode, cin, sh, sw), set()).add(cfg)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cin", [128, 256])
def test_subpixel_exact_deep_k(gpu, prec, cin):
    """cin 128 and 256, cout 32, from 3 x 33: the fix-up's K groups (2; 4 at fp16 and cin 256) and,
    fp32 records, its runs of one chunk per group with the cross-workgroup split.  First the standalone
    fix-up from scratch (launched before a direct-form conv), then the correction form behind every
    config whose sums stay below 2^24 (exact_ref.wino_fits, direct_sum_units): the direct-form ones
    all do.  +-1 data and the int64 reference in sixteenths; fp16 stores np.float16(exact), one
    rounding of an exact fp32 value.  Split-fp16 runs on the integers (a zero lo plane): with the
    +-2^-12 offsets a partial sum of 6 cin joined values no longer fits 24 bits; the lo reads of the
    ring are held at cin 16 and 64."""
    n, cout, sh, sw = N, 32, 3, 33
    x, wt, b, _, ow = E.int_case(n, cin, cout, sh, sw, (1,))
    src = source(x.astype(np.float64), prec, gpu)
    replicate_ring(src)
    dst = H8Tensor(n, cout, 2 * sh, 2 * sw, gpu, prec)
    wsub, up = E.subpixel_weights_int(wt), E.up2_int(x)
    ks = E.edge_split(cin, NAME[prec], "fix")[0]
    assert ks == (4 if prec == F16 and cin == 256 else 2)
    direct = [c for c in all_cfgs(prec, cin) if kind(c) == 0]
    assert direct
    ran = []
    for mode, todo in (("full", direct[:1]), ("fix", all_cfgs(prec, cin))):
        for cfg in todo:
            mul = wmul(cfg)
            what = f"{NAME[prec]} sub {mode} cin {cin} {sh}x{sw} cfg {cfg} (kind {kind(cfg)})"
            if kind(cfg) > 0:
                if not E.wino_fits(14 if kind(cfg) == 14 else 1, mul * wsub, 16, cin, 1)[0]:
                    continue
            else:
                assert E.direct_sum_units(up, wt, 16 * b, mul) < E.P24, what
            wt_t, b_t = tensors(wt, b, 0 * ow, R32, mul)
            ref, _ = reference(n, cin, cout, sh, sw, (1,), False, mul, "sub")
            if prec == F16:
                ref = E.f16_round(ref)
            fresh(dst)
            subpixel_upconv(src, wt_t, b_t, cfg, prec, dst=dst, full=mode == "full", edge_split=prec == R32)
            assert_equal(dst, 0, cout, ref, prec, what)
            if mode == "fix":
                ran.append(cfg)
    print(f"{NAME[prec]} cin {cin}: fix-up K groups {ks}, configs {ran} (kinds {sorted({kind(c) for c in ran})})")
    assert set(direct) <= set(ran)


@pytest.mark.parametrize("cin", [6, 32])
@pytest.mark.parametrize("h,w", [(9, 40), (17, 33), (10, 40), (18, 34), (2, 2), (2, 66)])
def test_block0_exact(gpu, cin, h, w):
    """rrin_conv_block0_h8_fwd at fp16 on exact_ref.block0_case: == leaky(conv b(leaky(conv a))),
    the intermediate an fp16 number.  The even sizes run with the pool: conv a is a multiple of 4,
    so out sits on a grid of 1/4 and the pooled mean on one of 1/16; the fp32 sum of four and the
    multiply by 1/4 are exact, so the pooled store is one round-to-nearest-even of a known rational
    and must be np.float16(exact) bit for bit -- ties at the 1/8 spacing above 128 included
    (tests/test_exact_ref.py)."""
    pooled = h % 2 == 0
    x, wa, ba, wb, bb = E.block0_case(N, cin, h, w)
    mid, out = E.block0_ref(x, wa, ba, wb, bb)
    assert E.f16_exact(mid.f64()) and E.f16_exact(out.f64())
    ref = out.f64()
    ca = 16 if cin < 16 else cin
    xa = np.zeros((N, ca, h, w))
    xa[:, :cin] = x
    src = source(xa, F16, gpu)
    t = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    dst = H8Tensor(N, 32, h, w, gpu, F16)
    fresh(dst)
    pl = None
    if pooled:
        pl = H8Tensor(N, 32, h // 2, w // 2, gpu, F16)
        fresh(pl)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    block0(src, cin, t(wa), t(ba), direct_cfg(cin, 32), t(wb), t(bb), direct_cfg(32, 32), pooled, dst=dst,
           status=status, tail_finite=1 if cin % 8 else 0, slope=E.SLOPE, pl=pl)
    assert int(status.item()) == 0
    assert_equal(dst, 0, 32, ref, F16, f"block0 cin {cin} {h}x{w}")
    if pooled:
        assert_equal(pl, 0, 32, E.f16_round(E.pool(out).f64()), F16, f"block0 cin {cin} {h}x{w} pool")


# ---- B. representable floats: derived forward bounds ------------------------------------------------
FLOAT = [(LINEAR, 16, 32, 9, 40), (LEAKY, 64, 40, 17, 33), (REP, 16, 32, 17, 33), (POOL, 16, 32, 18, 34)]
WORST = {}   # (precision, kind) -> largest observed err / (2^-24 S)


def within(got, ref, bnd, s, what):
    """|got - ref| <= bnd per element; prints and returns the largest err / (2^-24 S)."""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - ref)
    ratio = float((err / (E.U * s)).max())
    print(f"{what}: max err / (2^-24 S) = {ratio:.2f}, bound / (2^-24 S) >= {float((bnd / (E.U * s)).min()):.2f}")
    bad = ~(err <= bnd)
    assert not bad.any(), (what, int(bad.sum()), ratio, float((err / bnd).max()))
    return ratio


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi,cin,cout,h,w", FLOAT)
def test_conv_float_bound(gpu, prec, epi, cin, cout, h, w):
    """Random floats the storage holds exactly (exact_ref.float_case), every config, one shape per
    epilogue: |got - float64| within exact_ref.bound per element -- the derived (K + 2) 2^-24 S forms
    for the direct tiles, 4 x the measured ratio of the numpy emulation for the Winograd kinds -- and
    the pooled value within exact_ref.pool_bound.  Integer data cannot see a wrong final rounding or
    precision lost inside an accumulation; this does.  Slope 1/4.  The sub-pixel conv is not here."""
    name = NAME[prec]
    x, wt, b = E.float_case(N, cin, cout, h, w, name)
    s = E.s_of(x, wt, b)
    pre = E.conv64(x, wt, b)
    ref = pre if epi == LINEAR else E.leaky64(pre)
    refp = E.pool64(ref) if epi == POOL else None
    src = source(x, prec, gpu)
    dst = H8Tensor(N, cout, h, w, gpu, prec)
    pool = H8Tensor(N, cout, h // 2, w // 2, gpu, prec) if epi == POOL else None
    wt_t, b_t = torch.from_numpy(wt).float(), torch.from_numpy(b).float()
    for cfg in [c for c in all_cfgs(prec, cin) if not (epi == POOL and c in NO_POOL_CFGS)]:
        k = kind(cfg)
        ratio = E.wino_ratio(N, cin, cout, h, w, name, 14 if k == 14 else 1) if k else None
        bnd = E.bound(name, 9 * cin, s, ref, ratio)
        what = f"{name} {EPI_NAME[epi]} cin {cin} {h}x{w} cfg {cfg} (kind {k})"
        fresh(dst)
        if pool is not None:
            fresh(pool)
        conv_h8(src, wt_t, b_t, cfg, prec, epi=epi, dst=dst, pool=pool, slope=E.SLOPE)
        r = within(dst.to_nchw(0, cout).cpu().double().numpy(), ref, bnd, s, what)
        WORST[(name, k)] = max(WORST.get((name, k), 0.0), r)
        if pool is not None:
            within(pool.to_nchw(0, cout).cpu().double().numpy(), refp, E.pool_bound(name, bnd, ref, refp), E.pool64(s), what + " pool")
        if epi == REP:
            assert_ring(dst, what)
    print("worst err / (2^-24 S) so far:", {k_: round(v, 2) for k_, v in sorted(WORST.items())})


SUB_WORST = {}    # (precision, kind, mode, "interior" | "ring") -> largest observed err / (2^-24 S)
FLOAT_RAN = {}    # (prec, mode, cin, sh, sw) -> configs that ran


@functools.lru_cache(maxsize=None)
def sub_float_reference(n, cin, cout, sh, sw, name):
    """(x, wt, b, float64 reference, exact_ref.sub_terms): computed once per case and precision."""
    x, wt, b = E.sub_float_case(n, cin, cout, sh, sw, name)
    return x, wt, b, E.sub_ref64(x, wt, b), E.sub_terms(x, wt, b)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode,cin,cout,sh,sw", SUB)
def test_subpixel_float_bound(gpu, prec, mode, cin, cout, sh, sw):
    """The sub-pixel up conv on random floats the storage and the packs hold exactly
    (exact_ref.sub_float_case: w = m 2^-8, so the phase weights are exact), against float64
    conv(upsample(x)) + b over the whole 2h x 2w output, every config, the three ring modes.
    Interior pixels: exact_ref.bound with K = 9 cin and S of the pixel's phase over the
    edge-replicated x (Winograd: 4 x exact_ref.sub_wino_ratio).  Ring pixels: exact_ref.ring_bound,
    derived from the operation count of the fix-up per mode.  The worst err / (2^-24 S) is printed,
    interior and ring apart."""
    name = NAME[prec]
    x, wt, b, ref, terms = sub_float_reference(N, cin, cout, sh, sw, name)
    ring = E.ring_mask(2 * sh, 2 * sw)
    s_ring = terms[1] if mode == "inlaunch" else terms[0] + terms[2]
    src = source(x, prec, gpu)
    replicate_ring(src)
    dst = H8Tensor(N, cout, 2 * sh, 2 * sw, gpu, prec)
    wt_t, b_t = torch.from_numpy(wt).float(), torch.from_numpy(b).float()
    for cfg in [c for c in all_cfgs(prec, cin) if not (mode == "fold" and kind(c) != 3)]:
        k = kind(cfg)
        ratio = E.sub_wino_ratio(N, cin, cout, sh, sw, name, 14 if k == 14 else 1) if k else None
        inner = E.bound(name, 9 * cin, terms[0], ref, ratio)
        edge = E.ring_bound(name, mode, cin, terms, ref, b, ratio)
        what = f"{name} sub {mode} cin {cin} {sh}x{sw} cfg {cfg} (kind {k})"
        fresh(dst)
        subpixel_upconv(src, wt_t, b_t, cfg, prec, dst=dst, fold=mode == "fold", inlaunch=mode == "inlaunch",
                        edge_split=mode == "fix" and prec == R32)
        got = dst.to_nchw(0, cout).cpu().double().numpy()
        assert np.all(np.isfinite(got)), what
        for part, m, bnd, s in (("interior", ~ring, inner, terms[0]), ("ring", ring, edge, s_ring)):
            if m.any():
                r = within(got[:, :, m], ref[:, :, m], bnd[:, :, m], s[:, :, m], f"{what} {part}")
                key = (name, k, mode, part)
                SUB_WORST[key] = max(SUB_WORST.get(key, 0.0), r)
        FLOAT_RAN.setdefault((prec, mode, cin, sh, sw), set()).add(cfg)
    for key, v in sorted(SUB_WORST.items()):
        if key[0] == name and key[2] == mode:
            print(f"SUBPIXEL_WORST {key[0]} kind {key[1]} {key[2]} {key[3]}: err / (2^-24 S) <= {v:.2f}")


# ---- coverage -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_exact_coverage_is_every_config(prec):
    """Per precision and epilogue the configs held to equality are every config the library offers
    (rrin_conv_h8_cfg_ok), minus the two exclusions of tests/test_gpu_h8_storage.py: configs 4 and
    16 under pool, the fold for kinds other than 3.  Where the tests above ran in this session,
    what they recorded must be that plan."""
    lib = _lib.lib()
    offered = {c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_ok(c, prec) and kind(c) >= 0}
    assert offered
    assert {kind(c) for c in offered} == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]
    for cin in (16, 64):
        assert set(all_cfgs(prec, cin)) == offered
    plan = {name: offered for name in ("linear", "leaky", "rep", "sub_fix", "sub_inlaunch")}
    plan["pool"] = offered - set(NO_POOL_CFGS)
    plan["sub_fold"] = {c for c in offered if kind(c) == 3}
    assert (prec == R32) == bool(plan["sub_fold"])
    for name, want in plan.items():
        got = RAN.get((prec, name))
        print(f"{NAME[prec]} {name}: configs {sorted(want)}")
        if got is not None:
            assert got == want, (name, sorted(want - got), sorted(got - want))
    # the sub-pixel shapes -- the multi-tile ring lines among them -- are each required of every config
    for mode in ("fix", "inlaunch", "fold"):
        for cin in (16, 64):
            for sh, sw in SUB_SHAPES:
                got = RAN_SUB.get((prec, mode, cin, sh, sw))
                if got is not None:
                    assert got == plan["sub_" + mode], (mode, cin, sh, sw, sorted(plan["sub_" + mode] - got))
                for ran in (FLOAT_RAN.get((prec, mode, cin, sh, sw)),):
                    if ran is not None:
                        assert ran == plan["sub_" + mode], ("float", mode, cin, sh, sw, sorted(plan["sub_" + mode] - ran))
    assert len(SUB) == 3 * 2 * len(SUB_SHAPES) and {(3, 33), (18, 3)} <= set(SUB_SHAPES)
