"""CPU: the tests of tests/exact_ref.py, on which tests/test_gpu_h8_exact.py rests -- the int64
references against float64 torch, the mutations that equality must reject, the representability
of every case's data and results, and the packed weight blobs against their rational values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rrin_amd import _lib
from tests import exact_ref as E
from tests.test_gpu_h8 import pack_h8

X3, F16, R32 = _lib.PREC_F16X3, _lib.PREC_F16, _lib.PREC_F32R
# (n, cin, cout, h, w, mags) of tests/test_gpu_h8_exact.py: plain, pool, deep K (cin 256; resident 96 / 192)
PLAIN = [(2, cin, cout, h, w, (1, 2)) for cin, cout in ((16, 32), (64, 40)) for h, w in ((9, 40), (17, 33))]
POOLED = [(2, cin, cout, 18, 34, (1,)) for cin, cout in ((16, 32), (64, 40))]
DEEP = [(1, cin, 32, 9, 40, (1,)) for cin in (256, 192, 96)]
SUB = [(2, cin, cout, sh, sw, (1,)) for cin, cout in ((16, 32), (64, 40)) for sh, sw in ((5, 9), (1, 2))]
T = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731


@pytest.mark.parametrize("case", PLAIN[:2] + POOLED[:1] + DEEP[2:])
def test_int_references_equal_float64_torch(case):
    x, wt, b, ox, ow = E.int_case(*case)
    y = F.conv2d(T(x), T(wt), T(b), padding=1)
    assert np.array_equal(E.pre_int(x, wt, b).f64(), y.numpy())
    assert np.array_equal(E.pre_int(x, wt, b, 48).f64(), F.conv2d(T(x), 48 * T(wt), 48 * T(b), padding=1).numpy())
    ly = F.leaky_relu(y, E.SLOPE)
    assert np.array_equal(E.leaky(E.pre_int(x, wt, b)).f64(), ly.numpy())
    if x.shape[2] % 2 == 0:
        assert np.array_equal(E.pool(E.leaky(E.pre_int(x, wt, b))).f64(), F.avg_pool2d(ly, 2).numpy())
    # split-fp16: the three product classes, without lo*lo
    xf, wf = T(x) + T(ox) / E.LO, T(wt) + T(ow) / E.LO
    full = F.conv2d(xf, wf, T(b), padding=1) - F.conv2d(T(ox) / E.LO, T(ow) / E.LO, None, padding=1)
    assert np.array_equal(E.pre_split(x, wt, b, ox, ow).f64(), full.numpy())


@pytest.mark.parametrize("case", SUB)
def test_subpixel_reference_equals_float64_torch(case):
    x, wt, b, _, _ = E.int_case(*case)
    up = F.interpolate(T(x), scale_factor=2, mode="bilinear", align_corners=False)
    assert np.array_equal(E.up2_int(x) / 16.0, up.numpy())
    assert np.array_equal(E.pre_sub(x, wt, b).f64(), F.conv2d(up, T(wt), T(b), padding=1).numpy())
    r = E.pre_sub(x, wt, b).f64()
    assert E.f16_exact(r), float(np.abs(r).max())     # sixteenths below 128


@pytest.mark.parametrize("case", PLAIN + POOLED + DEEP)
def test_mutations_break_equality(case):
    """A dropped tap of one channel at one pixel, a K chunk added twice for one co block, a zero lo
    and two exchanged output rows: each changes the reference of every data set, the pooled one too."""
    x, wt, b, ox, ow = E.split_case(*case)
    assert not (x == 0).any() and not (wt == 0).any() and not (b == 0).any()
    for r, mul in ((E.pre_int(x, wt, b), 1), (E.pre_int(x, wt, b, 48), 48), (E.pre_split(x, wt, b, ox, ow), 1)):
        epis = (lambda q: q, E.leaky) + ((lambda q: E.pool(E.leaky(q)),) if case in POOLED else ())
        for k, epi in enumerate(epis):
            good = epi(r).units
            # pooled: rows 2 and 3 share a pool pair (their exchange is invisible, rightly); rows 1 and 2 do not
            for bad in (E.drop_one_tap(r, x, wt, mul), E.chunk_twice(r, x, wt, mul), E.swap_rows(r, 1 if k == 2 else 2)):
                assert not np.array_equal(epi(bad).units, good)
    assert (ox != 0).any() and (ow != 0).any()
    assert not np.array_equal(E.pre_split(x, wt, b, ox, ow, zero_lo=True).units, E.pre_split(x, wt, b, ox, ow).units)


@pytest.mark.parametrize("case", PLAIN + POOLED + DEEP)
def test_results_are_representable(case):
    """fp16: the result and its pooled value are fp16 numbers; split-fp16: the result in units of
    2^-14 (2^-16 pooled) stays below 2^24, so the fp32 the kernel splits is exact; fp32 records:
    every direct-form partial sum below 2^24."""
    x, wt, b, ox, ow = E.split_case(*case)
    assert (E.pre_split(x, wt, b, ox, ow).units == 0).sum() >= 2 and (E.pre_int(x, wt, b).units == 0).sum() >= 2
    pooled = case in POOLED
    for r in (E.pre_int(x, wt, b), E.leaky(E.pre_int(x, wt, b))):
        assert E.f16_exact(r.f64()), float(np.abs(r.f64()).max())
    s = E.leaky(E.pre_split(x, wt, b, ox, ow))
    assert int(np.abs(s.units).max()) < E.P24 and E.f32_exact(s.f64())
    if pooled:
        assert E.f16_exact(E.pool(E.leaky(E.pre_int(x, wt, b))).f64())
        p = E.pool(s)
        assert int(np.abs(p.units).max()) < E.P24 and E.f32_exact(p.f64())
    assert E.direct_sum_units(x, wt, b) * (E.LO + 2) < E.P24
    assert E.direct_sum_units(x, wt, b, 48) < E.P24


def _cfg(prec, want_kind, bm=None):
    lib = _lib.lib()
    return next(c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_ok(c, prec)
                and lib.rrin_conv_h8_cfg_wino(c) == want_kind and (bm is None or lib.rrin_conv_h8_cfg_bm(c) == bm))


@pytest.mark.parametrize("case", PLAIN[::2] + DEEP[:1] + SUB[::2])
def test_packed_weights_are_their_rational_values(case):
    """Every blob the GPU tests hand to a kernel, decoded: fp32 direct = w; fp32 U = G g G^T
    (F(2x2): quarters; kind 14 with w x 48: integers); fp16 U and the direct hi / lo halves times
    the power-of-two scale.  Sub-pixel cases: the phase-combined weights are sixteenths."""
    lib = _lib.lib()
    x, wt, b, _, ow = E.int_case(*case)
    cout, cin = wt.shape[:2]
    sub = case in SUB
    if sub:
        ws = np.empty((4 * cout, cin, 3, 3), np.float32)
        bs = np.empty(4 * cout, np.float32)
        w32, b32 = wt.astype(np.float32), b.astype(np.float32)
        _lib.check(lib.rrin_subpixel_weights(w32.ctypes.data, b32.ctypes.data, cout, cin, ws.ctypes.data, bs.ctypes.data))
        assert np.array_equal(ws.astype(np.float64) * 16, E.subpixel_weights_int(wt).astype(np.float64))
        wu, den, cout, ow = E.subpixel_weights_int(wt), 16, 4 * cout, 0 * E.subpixel_weights_int(wt)
        bq = bs.astype(np.float64)
    else:
        wu, den, bq = wt, 1, b.astype(np.float64)
    w64 = wu.astype(np.float64) / den
    tw, tb = torch.from_numpy(w64).float(), torch.from_numpy(bq).float()
    # fp32 records, direct form
    c = _cfg(R32, 0)
    bm = lib.rrin_conv_h8_cfg_bm(c)
    assert np.array_equal(E.unpack_direct(pack_h8(tw, tb, c, R32, "cpu")[0].numpy(), cout, cin, bm, 4), w64.reshape(cout, cin, 9))
    # fp32 Winograd F(2x2) (BM 32 and 64) and kind 14 (weights x 48)
    for k in (3, 6):
        c = _cfg(R32, k)
        bm = lib.rrin_conv_h8_cfg_bm(c)
        u = E.wino_u(wu, 1) / den
        assert E.f32_exact(u) and E.wino_fits(1, wu, den, cin, max(case[5]))[0]
        assert np.array_equal(E.unpack_wino(pack_h8(tw, tb, c, R32, "cpu")[0].numpy(), cout, cin, bm, 4, 16), u.reshape(cout, cin, 16))
    c = _cfg(R32, 14)
    u = E.wino_u(48 * wu, 14) / den
    assert E.f32_exact(u)
    assert np.array_equal(E.unpack_wino(pack_h8(48 * tw, tb, c, R32, "cpu")[0].numpy(), cout, cin, 32, 4, 24), u.reshape(cout, cin, 24))
    fits, worst, coarse, grid = E.wino_fits(14, 48 * wu, den, cin, max(case[5]))
    print(f"kind 14 cin {cin} sub {sub}: grid {grid}, worst {worst:.3g}, coarse bound {coarse:.3g}, 2^24 = {E.P24}")
    assert fits, (worst, coarse)
    # the coarser cin max|U| max|V| rowsum(A^T) pairs the largest U with the largest A^T coefficient,
    # which never meet at one point.  It holds for every F(2x2) case and for kind 14 at cin 16; it
    # cannot hold for kind 14 at cin 64 (2.1e7 with |x| <= 2, |w| <= 96), at cin 256 and for the
    # sub-pixel conv at cin 64 (both already +-1: no smaller data exists), so one bound, the per-point
    # one -- itself a worst case over the magnitudes -- is asserted for every case
    assert E.wino_fits(1, wu, den, cin, max(case[5]))[2] < E.P24
    assert (coarse < E.P24) == (cin == 16), (cin, sub, coarse)
    if not sub:
        assert grid == 1.0
    # fp16 Winograd kind 6 (16-channel chunks): fp16(U 2^s) exact
    c = _cfg(F16, 6)
    whi, _, _, inv = pack_h8(tw, tb, c, F16, "cpu")
    u = E.wino_u(wu, 1) / den
    assert np.array_equal(E.unpack_wino(E.halves(whi), cout, cin, 64, 8, 16) * inv, u.reshape(cout, cin, 16))
    # direct hi / lo halves: fp16 (hi alone) and split-fp16 on w + ow 2^-12
    c = _cfg(F16, 0)
    bm = lib.rrin_conv_h8_cfg_bm(c)
    whi, _, _, inv = pack_h8(tw, tb, c, F16, "cpu")
    assert np.array_equal(E.unpack_direct(E.halves(whi), cout, cin, bm, 8) * inv, w64.reshape(cout, cin, 9))
    c = _cfg(X3, 0)
    bm = lib.rrin_conv_h8_cfg_bm(c)
    wf = w64 + ow / E.LO
    assert E.f32_exact(wf)
    whi, wlo, _, inv = pack_h8(torch.from_numpy(wf).float(), tb, c, X3, "cpu")
    assert np.array_equal(E.unpack_direct(E.halves(whi), cout, cin, bm, 8) * inv, w64.reshape(cout, cin, 9))
    assert np.array_equal(E.unpack_direct(E.halves(wlo), cout, cin, bm, 8) * inv / 2048, (ow / E.LO).reshape(cout, cin, 9))
    assert sub or bool(wlo.any())


@pytest.mark.parametrize("case", PLAIN + POOLED + SUB)
def test_source_records_split_as_intended(case):
    """x + ox 2^-12 through the CPU record encoder: hi is the integer, lo the offset (x 2^11)."""
    x, _, _, ox, _ = E.split_case(*case)
    hi, lo = E.records(x + ox / E.LO, "F16X3", (x.shape[1] + 15) // 16 * 2)
    from tests import glue_ref as G
    n, c, h, w = x.shape
    assert np.array_equal(G.records_to_nchw(hi, None, 0, c, h, w).double().numpy(), x.astype(np.float64))
    assert np.array_equal(G.records_to_nchw(lo, None, 0, c, h, w).double().numpy(), ox / 2.0)
    assert bool(lo.any())


@pytest.mark.parametrize("cin", [6, 32])
@pytest.mark.parametrize("h,w", [(9, 40), (17, 33)])
def test_block0_data_is_representable(cin, h, w):
    x, wa, ba, wb, bb = E.block0_case(2, cin, h, w)
    assert not (x == 0).any() and not (wa == 0).any() and not (wb == 0).any()
    mid, out = E.block0_ref(x, wa, ba, wb, bb)
    assert E.f16_exact(mid.f64()) and E.f16_exact(out.f64()), (np.abs(mid.units).max(), np.abs(out.f64()).max())
    ref = F.leaky_relu(F.conv2d(F.leaky_relu(F.conv2d(T(x), T(wa), T(ba), padding=1), E.SLOPE), T(wb), T(bb), padding=1), E.SLOPE)
    assert np.array_equal(out.f64(), ref.numpy())
    ya = E.conv_int(x, wa) + ba[None, :, None, None]
    assert (ya > 0).any() and (ya < 0).any()
    # mutations of conv a (a dropped tap, a K chunk twice) and of conv b, and exchanged rows, reach the result
    def out_of(ya_, wb_=wb, extra=0):
        mid_ = np.where(ya_ > 0, ya_, ya_ // 4) if not (ya_ % 4).any() else None
        if mid_ is None:
            return None   # conv a left its grid of 4: the result is not even an fp16-exact integer form
        return E.leaky(E.Ref(E.conv_int(mid_, wb_) + bb[None, :, None, None] + extra, 1)).units
    good = out_of(ya)
    assert np.array_equal(good, out.units)
    r = E.Ref(ya, 1)
    for bad in (E.drop_one_tap(r, x, wa), E.chunk_twice(r, x, wa, c0=0, width=min(8, cin))):
        o = out_of(bad.units)
        assert o is None or not np.array_equal(o, good)
    rb = E.Ref(E.conv_int(mid.units, wb) + bb[None, :, None, None], 1)
    yy, xq = (int(v) for v in np.argwhere(mid.units[0, 1, :h - 1, 1:] != 0)[0])   # conv a can be 0 there: a product that is not
    for bad in (E.drop_one_tap(rb, mid.units, wb, at=(0, 1, yy + 1, xq)), E.chunk_twice(rb, mid.units, wb), E.swap_rows(rb)):
        assert not np.array_equal(E.leaky(bad).units, good)


BLOCK0_POOLED = [(cin, h, w) for cin in (6, 32) for h, w in ((10, 40), (18, 34), (2, 2), (2, 66))]


def test_block0_pooled_store_is_one_rounding():
    """The fused block with its pool: conv a is a multiple of 4, so mid is an integer, out sits on a
    grid of 1/4 and is an fp16 number, and the pooled mean on a grid of 1/16.  The fp32 sum of four
    such values (below 2^24 units) and the multiply by 1/4 are exact: the pooled store is one
    round-to-nearest-even of a known rational, np.float16(exact).  The cases hold pooled values that
    are no fp16 numbers and, between them, exact ties (odd sixteenths at the 1/8 spacing above
    128), so they pin the rounding mode; a dropped tap of conv b and a chunk added twice reach the
    rounded pooled value."""
    ties = 0
    for cin, h, w in BLOCK0_POOLED:
        x, wa, ba, wb, bb = E.block0_case(2, cin, h, w)
        mid, out = E.block0_ref(x, wa, ba, wb, bb)
        assert out.scale == 4 and E.f16_exact(mid.f64()) and E.f16_exact(out.f64())
        p = E.pool(out)
        assert p.scale == 16 and p.units.shape[2:] == (h // 2, w // 2)
        a = np.abs(out.units)
        assert int((a[:, :, 0::2, 0::2] + a[:, :, 0::2, 1::2] + a[:, :, 1::2, 0::2] + a[:, :, 1::2, 1::2]).max()) < E.P24
        assert np.abs(p.f64()).max() <= 752
        ref = F.avg_pool2d(T(out.f64()), 2).numpy()
        assert np.array_equal(p.f64(), ref)
        want = E.f16_round(p.f64())
        inexact = want != p.f64()
        # a tie: the exact value halfway between two neighbouring fp16 numbers
        up_, dn = np.nextafter(want.astype(np.float16), np.float16(np.inf)).astype(np.float64), \
            np.nextafter(want.astype(np.float16), np.float16(-np.inf)).astype(np.float64)
        tie = inexact & ((np.abs(p.f64() - want) == np.abs(up_ - p.f64())) | (np.abs(p.f64() - want) == np.abs(p.f64() - dn)))
        print(f"cin {cin} {h}x{w}: {inexact.mean():.1%} of the pooled values are no fp16 numbers, {int(tie.sum())} ties")
        assert inexact.any() or (h, w) == (2, 2)   # 64 pooled values: the union below covers it
        ties += int(tie.sum())
        rb = E.Ref(E.conv_int(mid.units, wb) + bb[None, :, None, None], 1)
        yy, xq = (int(v) for v in np.argwhere(mid.units[0, 1, :h - 1, 1:] != 0)[0])
        for bad in (E.drop_one_tap(rb, mid.units, wb, at=(0, 1, yy + 1, xq)), E.chunk_twice(rb, mid.units, wb)):
            assert not np.array_equal(E.f16_round(E.pool(E.leaky(bad)).f64()), want)
    assert ties > 0


@pytest.mark.parametrize("case", SUB)
def test_subpixel_mutations_break_equality(case):
    """The mutations on the sub-pixel references (integer and split-fp16 with offsets on x), applied
    to conv(upsample(x), w); the 1 x 2 source has 2 x 4 outputs: rows 0 and 1 are exchanged."""
    x, wt, b, ox, _ = E.split_case(*case)
    up = E.up2_int(x)
    for r, mul in ((E.pre_sub(x, wt, b), 1), (E.pre_sub(x, wt, b, 48), 48), (E.pre_sub_split(x, wt, b, ox), 1)):
        at, rs = (0, 1, 1, 2), r.scale // 16     # products are in sixteenths: up carries the 16
        bads = (E.drop_one_tap(E.Ref(r.units, rs), up, wt, mul, at=at, tap=(0, 2)), E.chunk_twice(E.Ref(r.units, rs), up, wt, mul),
                E.swap_rows(r, 0))
        for bad in bads:
            assert not np.array_equal(bad.units, r.units)
    assert (ox != 0).any()
    assert not np.array_equal(E.pre_sub_split(x, wt, b, 0 * ox).units, E.pre_sub_split(x, wt, b, ox).units)
    s = E.pre_sub_split(x, wt, b, ox)
    assert int(np.abs(s.units).max()) < E.P24 and E.f32_exact(s.f64())
    # float64 torch on x + ox 2^-12 (w has no offset: nothing is dropped)
    upf = F.interpolate(T(x) + T(ox) / E.LO, scale_factor=2, mode="bilinear", align_corners=False)
    assert np.array_equal(s.f64(), F.conv2d(upf, T(wt), T(b), padding=1).numpy())


SUB_RING = [(2, cin, cout, sh, sw, (1,)) for cin, cout in ((16, 32), (64, 40)) for sh, sw in ((3, 33), (18, 3))]
SUB_DEEP = [(2, cin, 32, 3, 33, (1,)) for cin in (128, 256)]


@pytest.mark.parametrize("case", SUB_RING + SUB_DEEP)
def test_subpixel_ring_cases(case):
    """The sub-pixel cases with ring lines of two tiles and a ragged third (3 x 33: 66 px rows; 18 x 3:
    34 px columns) and with fix-up K groups 2 and 4 (cin 128, 256).  Every direct-form partial sum
    stays below 2^24 sixteenths, so the fp32 accumulator holds the exact value and the fp16 store is
    its single rounding, exact_ref.f16_round; fp32 records hold it as it is, split-fp16 as hi + lo.
    The mutations -- a dropped tap, a chunk added twice, exchanged rows, a ring pixel moved across the
    32-pixel seam, a K group left out of the ring sums -- break the equality, after the fp16
    rounding too."""
    deep = case in SUB_DEEP
    x, wt, b, ox, _ = E.int_case(*case) if deep else E.split_case(*case)
    n, cin, h, w = x.shape
    up = E.up2_int(x)
    r = E.pre_sub(x, wt, b)
    upf = F.interpolate(T(x), scale_factor=2, mode="bilinear", align_corners=False)
    assert np.array_equal(r.f64(), F.conv2d(upf, T(wt), T(b), padding=1).numpy())
    assert E.direct_sum_units(up, wt, 16 * b) < E.P24 and E.direct_sum_units(up, wt, 16 * b, 48) < E.P24
    assert E.f32_exact(r.f64()) and E.own_split(r.f64())
    inexact = int((E.f16_round(r.f64()) != r.f64()).sum())
    print(case, f"max |v| {np.abs(r.f64()).max()}, not fp16 numbers: {inexact} of {r.units.size}")
    assert deep or not inexact         # only cin 128 and 256 may leave the range where sixteenths fit 11 bits
    if not deep:
        s = E.pre_sub_split(x, wt, b, ox)
        assert int(np.abs(s.units).max()) < E.P24 and E.f32_exact(s.f64()) and E.own_split(s.f64()) and (ox != 0).any()
        upo = F.interpolate(T(x) + T(ox) / E.LO, scale_factor=2, mode="bilinear", align_corners=False)
        assert np.array_equal(s.f64(), F.conv2d(upo, T(wt), T(b), padding=1).numpy())
        assert not np.array_equal(E.pre_sub_split(x, wt, b, 0 * ox).units, s.units)
    left = w < 17
    refs = [(r, 1), (E.pre_sub(x, wt, b, 48), 48)] + ([] if deep else [(E.pre_sub_split(x, wt, b, ox), 1)])
    for q, mul in refs:
        rs = E.Ref(q.units, q.scale // 16)
        bads = [E.drop_one_tap(rs, up, wt, mul, at=(0, 1, 1, 2), tap=(0, 2)), E.chunk_twice(rs, up, wt, mul),
                E.swap_rows(q, 0), E.seam_shift(q, left)]
        bads += [E.ring_groups_miscounted(q, up, wt, mul, ks) for ks in (2, 4) if cin % (32 * ks) == 0]
        assert len(bads) == 4 + (cin >= 64) + (cin >= 128)
        for bad in bads:
            assert not np.array_equal(bad.units, q.units)
            if mul == 1:
                assert not np.array_equal(E.f16_round(bad.units / q.scale), E.f16_round(q.f64()))


# ---- part B ------------------------------------------------------------------------------------------
FLOAT = [(2, 16, 32, 9, 40), (2, 64, 40, 17, 33), (2, 16, 32, 17, 33), (2, 16, 32, 18, 34)]
# worst err / (2^-24 S) of exact_ref.wino_emulate against float64 on float_case: (F(2x2) fp32, kind 14, fp16 kind 6)
RATIOS = {FLOAT[0]: (1.81, 10.5, 6000.0), FLOAT[1]: (1.63, 5.86, 2881.3), FLOAT[2]: (1.76, 7.42, 5894.0), FLOAT[3]: (1.99, 9.36, 6392.7)}


@pytest.mark.parametrize("case", FLOAT)
def test_wino_emulation_ratios_are_the_recorded_ones(case):
    """The measured amplification of the Winograd transforms, which the GPU bound multiplies by 4:
    it fails if a ratio moves from the recorded value (to its printed precision)."""
    got = (E.wino_ratio(*case, "R32", 1), E.wino_ratio(*case, "R32", 14), E.wino_ratio(*case, "F16", 6))
    print(case, [round(g, 2) for g in got])
    for g, want in zip(got, RATIOS[case]):
        assert abs(g - want) <= 0.006 * max(want, 1.0), (got, RATIOS[case])
    # and the emulation is the conv: float64 operands through the same code reproduce float64 to 1e-12 ... in fp32 to its ratio
    x, wt, b = E.float_case(*case, "R32")
    assert np.abs(E.wino_emulate(x, wt, b, 14) - E.conv64(x, wt, b)).max() < 1e-4


@pytest.mark.parametrize("case", FLOAT)
@pytest.mark.parametrize("prec", ["R32", "F16", "F16X3"])
def test_float_data_is_held_exactly(case, prec):
    """fp16: x and the packed w 2^s are fp16 numbers; split-fp16: x and w 2^s equal their hi + lo;
    the blobs decode to w exactly."""
    lib = _lib.lib()
    x, wt, b = E.float_case(*case, prec)
    cout, cin = wt.shape[:2]
    assert E.f32_exact(x) and E.f32_exact(wt)
    tw, tb = torch.from_numpy(wt).float(), torch.from_numpy(b).float()
    if prec == "F16":
        assert E.f16_exact(x) and E.f16_exact(wt)
        c = _cfg(F16, 0)
        whi, _, _, inv = pack_h8(tw, tb, c, F16, "cpu")
        assert np.array_equal(E.unpack_direct(E.halves(whi), cout, cin, lib.rrin_conv_h8_cfg_bm(c), 8) * inv, wt.reshape(cout, cin, 9))
    if prec == "F16X3":
        hi, lo = E.split16_f64(x)
        assert np.array_equal(hi + lo, x) and lo.any()
        c = _cfg(X3, 0)
        whi, wlo, _, inv = pack_h8(tw, tb, c, X3, "cpu")
        bm = lib.rrin_conv_h8_cfg_bm(c)
        joined = (E.unpack_direct(E.halves(whi), cout, cin, bm, 8) + E.unpack_direct(E.halves(wlo), cout, cin, bm, 8) / 2048) * inv
        assert np.array_equal(joined, wt.reshape(cout, cin, 9)) and bool(wlo.any())


# ---- the sub-pixel conv on floats: data, emulation, ring bounds --------------------------------------
SUBF = [(2, cin, cout, sh, sw) for cin, cout in ((16, 32), (64, 40)) for sh, sw in ((5, 9), (1, 2), (3, 33), (18, 3))]
# worst err / (2^-24 S) of wino_emulate on the phase weights (exact_ref.sub_wino_ratio): (F(2x2) fp32, kind 14, fp16 kind 6)
SUB_RATIOS = {
    (2, 16, 32, 5, 9): (1.94, 9.63, 4824.3), (2, 16, 32, 1, 2): (1.20, 1.49, 2856.5),
    (2, 16, 32, 3, 33): (2.12, 8.34, 4493.1), (2, 16, 32, 18, 3): (1.64, 3.15, 4420.4),
    (2, 64, 40, 5, 9): (1.68, 7.16, 2616.5), (2, 64, 40, 1, 2): (1.25, 1.44, 1148.2),
    (2, 64, 40, 3, 33): (2.03, 8.55, 2205.7), (2, 64, 40, 18, 3): (1.95, 2.94, 2153.3)}


@pytest.mark.parametrize("case", SUBF)
@pytest.mark.parametrize("prec", ["R32", "F16", "F16X3"])
def test_subpixel_float_data_is_held_exactly(case, prec):
    """w = m 2^-8: the phase weights are multiples of 2^-12 of at most 49 x 31 < 2^11 steps (the
    centre tap of a phase gathers coefficients (1 + 3 + 3)^2 = 49 sixteenths), rrin_subpixel_weights
    gives them exactly and the direct packs of every precision decode to them (split-fp16: hi alone,
    lo zero); the phase form equals conv(upsample(x)) off the ring."""
    lib = _lib.lib()
    x, wt, b = E.sub_float_case(*case, prec)
    cout, cin = wt.shape[:2]
    wp = E.phase_weights64(wt)
    steps = wp * 4096
    assert np.array_equal(steps, np.rint(steps)) and np.abs(steps).max() <= 49 * 31 < 2 ** 11
    assert E.f16_exact(wp * 2.0 ** 4)
    rows = E.phase_rows(wp)
    ws, bs = np.empty((4 * cout, cin, 3, 3), np.float32), np.empty(4 * cout, np.float32)
    w32, b32 = wt.astype(np.float32), b.astype(np.float32)
    _lib.check(lib.rrin_subpixel_weights(w32.ctypes.data, b32.ctypes.data, cout, cin, ws.ctypes.data, bs.ctypes.data))
    assert np.array_equal(ws.astype(np.float64), rows)
    tw, tb = torch.from_numpy(ws), torch.from_numpy(bs)
    want = rows.reshape(4 * cout, cin, 9)
    if prec == "R32":
        c = _cfg(R32, 0)
        assert np.array_equal(E.unpack_direct(pack_h8(tw, tb, c, R32, "cpu")[0].numpy(), 4 * cout, cin, lib.rrin_conv_h8_cfg_bm(c), 4), want)
    else:
        p = F16 if prec == "F16" else X3
        c = _cfg(p, 0)
        whi, wlo, _, inv = pack_h8(tw, tb, c, p, "cpu")
        assert np.array_equal(E.unpack_direct(E.halves(whi), 4 * cout, cin, lib.rrin_conv_h8_cfg_bm(c), 8) * inv, want)
        assert prec == "F16" or not bool(wlo.any())
    assert np.array_equal(E.up_emulate(x, np.float64), F.interpolate(T(x), scale_factor=2, mode="bilinear", align_corners=False).numpy())
    ref = E.sub_ref64(x, wt, b)
    off = ~E.ring_mask(*ref.shape[2:])
    s = E.sub_terms(x, wt, b)[0]
    assert (np.abs(E.phase64(x, wp, b) - ref)[:, :, off] <= 2.0 ** -50 * s[:, :, off]).all()


def _ring_got(case, prec, mode, mutate=None, cin_case=None):
    x, wt, b = E.sub_float_case(*case, prec)
    cin = case[1]
    ks, nsl = E.edge_split(cin, prec, "fix" if mode == "full" else mode)
    pre = E.phase_emulate(x, E.phase_weights64(wt)) if mode in ("fix", "fold") else None
    v = E.edge_emulate(x, wt, b, "full" if mode in ("full", "inlaunch") else "corr", ks, nsl, pre, mutate)
    ref = E.sub_ref64(x, wt, b)
    bnd = E.ring_bound(prec, mode, cin, E.sub_terms(x, wt, b), ref, b)
    m = E.ring_mask(*ref.shape[2:])
    return np.abs(E.store_emulate(v, prec) - ref)[:, :, m], bnd[:, :, m], E.sub_terms(x, wt, b), m


@pytest.mark.parametrize("case", SUBF)
@pytest.mark.parametrize("prec", ["R32", "F16", "F16X3"])
@pytest.mark.parametrize("mode", ["fix", "full", "inlaunch", "fold"])
def test_ring_emulation_is_inside_the_derived_bound(case, prec, mode):
    if mode == "fold" and prec != "R32":
        return
    err, bnd, terms, m = _ring_got(case, prec, mode)
    assert np.isfinite(err).all() and (err <= bnd).all(), float((err / bnd).max())
    s = (terms[1] if mode in ("full", "inlaunch") else terms[0] + terms[2])[:, :, m]
    print(case, prec, mode, f"worst err / (u S) {float((err / (E.U * s)).max()):.2f}, err / bound {float((err / bnd).max()):.3f}")


@pytest.mark.parametrize("prec", ["R32", "F16", "F16X3"])
def test_ring_bound_rejects_wrong_rings(prec):
    """A corner's extra taps dropped, an align_corners=True upsample on the ring line, one K group's
    sum added twice at cin 128 and a ring pixel taken from x + 1 across the tile seam."""
    wide, corner = (2, 16, 32, 3, 33), (2, 16, 32, 5, 9)
    for case, mode, mutate in ((corner, "fix", "no_extras"), (corner, "fix", "align_corners"), (corner, "full", "align_corners"),
                               (wide, "fix", "seam"), (wide, "full", "seam"), ((1, 128, 32, 3, 33), "fix", "group_twice"),
                               ((1, 128, 32, 3, 33), "full", "group_twice")):
        err, bnd, _, _ = _ring_got(case, prec, mode)
        assert (err <= bnd).all()
        err, bnd, _, _ = _ring_got(case, prec, mode, mutate)
        assert (err > bnd).any(), (case, mode, mutate)
    assert E.edge_split(128, prec, "fix")[0] == 2


@pytest.mark.parametrize("case", SUBF)
def test_subpixel_wino_ratios_are_the_recorded_ones(case):
    got = (E.sub_wino_ratio(*case, "R32", 1), E.sub_wino_ratio(*case, "R32", 14), E.sub_wino_ratio(*case, "F16", 6))
    print(case, [round(g, 2) for g in got])
    for g, want in zip(got, SUB_RATIOS[case]):
        assert abs(g - want) <= 0.006 * max(want, 1.0), (got, SUB_RATIOS[case])


def test_split_bound_rejects_a_dropped_hi_lo_class():
    """got = float64 without the hx*lw products: past the split-fp16 bound somewhere (cin 16)."""
    case = FLOAT[0]
    x, wt, b = E.float_case(*case, "F16X3")
    ref, s = E.conv64(x, wt, b), E.s_of(x, wt, b)
    bnd = E.bound("F16X3", 9 * case[1], s, ref)
    assert (np.abs(ref - ref) <= bnd).all()
    hx, _ = E.split16_f64(x)
    _, lw = E.split16_f64(wt)
    got = ref - E.conv64(hx, lw)
    assert (np.abs(got - ref) > bnd).any()
    # ... while the lo*lo class the design drops stays inside
    _, lx = E.split16_f64(x)
    assert (np.abs(E.conv64(lx, lw)) <= 2.0 ** -22 * s).all()


def test_fp16_bound_rejects_a_second_rounding():
    """got = f16(f16(conv) + b): the sum rounded to fp16 before the bias and again after it."""
    case = FLOAT[0]
    x, wt, b = E.float_case(*case, "F16")
    ref, s = E.conv64(x, wt, b), E.s_of(x, wt, b)
    bnd = E.bound("F16", 9 * case[1], s, ref)
    once = T(ref).half().double().numpy()
    assert (np.abs(once - ref) <= bnd).all()
    twice = (T(E.conv64(x, wt)).half().double() + T(b).view(1, -1, 1, 1)).half().double().numpy()
    assert (np.abs(twice - ref) > bnd).any()


# ---- launch paths (tests/test_gpu_h8_paths.py): ladder, ranges, mutations ----------------------------
ALL_PATH_SHAPES = sorted(set(E.LADDER) | set(E.K14_TALL) | {E.K14_TALL_AUTO}
                         | {(n, cin, cout, h, w) for n, cout, h, w in E.K14_PERSIST[:1] for cin in E.K14_PERSIST_CIN}
                         | {(n, cin, cout, h, w) for n, cout, h, w in E.K14_PERSIST[1:] for cin in E.K14_PERSIST_CIN[:3]})


def test_ladder_is_ordered_and_bounded():
    """Cheapest first within each cin; nothing beyond 96 x 640 x 4 pixels, n 2-6, cout of the four widths."""
    for ladder, cins in ((E.LADDER, (16, 64)), (E.LADDER_SUB, (32,))):
        for cin in cins:
            cost = [n * cout * h * w for n, c, cout, h, w in ladder if c == cin]
            assert cost and cost == sorted(cost)
        for n, cin, cout, h, w in ladder:
            assert 2 <= n <= 6 and n * h * w <= 4 * 96 * 640 and cout in (32, 40, 64, 128, 256) and cin in cins
            assert h % 16 == 1 and w % 32 == 1        # one past a tile multiple: ragged last tiles of every geometry


@pytest.mark.parametrize("shape", ALL_PATH_SHAPES)
def test_path_shapes_stay_in_the_exact_range(shape):
    """Every ladder and fixed shape keeps its reference exactly representable: the direct form's sums
    below 2^24 grid steps at the worst signs (split-fp16: in units of 2^-12, two hi*lo classes), the
    stored values fp16 numbers where the fp16 precisions store them, and the Winograd forms inside
    exact_ref.wino_fits with +-1 / +-2, or with +-1 alone where the test falls back to it."""
    n, cin, cout, h, w = shape
    if shape in E.LADDER:      # the shapes split-fp16 runs; the kind-14 shapes run on fp32 records alone
        assert (9 * cin * 4 + 3) * (E.LO + 2) < E.P24
    assert 48 * (9 * cin * 4 + 3) < E.P24
    x, wt, b, _, _ = E.int_case(n, cin, cout, h, w, (1, 2))
    for k, mul in ((1, 1), (14, 48)):
        fits = E.wino_fits(k, mul * wt, 1, cin, 2)[0]
        if not fits:
            assert E.wino_fits(k, mul * E.int_case(n, cin, cout, h, w, (1,))[1], 1, cin, 1)[0], (k, shape)
    if shape in E.LADDER:
        r = E.leaky(E.pre_int(x, wt, b))
        assert E.f16_exact(r.f64()) and E.f32_exact(48 * r.f64())
        hp, wp = h + 1, w + 1
        x1, w1, b1, _, _ = E.int_case(n, cin, cout, hp, wp, (1,))
        assert E.f16_exact(E.pool(E.leaky(E.pre_int(x1, w1, b1))).f64())


@pytest.mark.parametrize("shape", list(E.LADDER_SUB) + E.K14_PERSIST_SUB)
def test_sub_shapes_stay_in_the_exact_range(shape):
    """Every sub-pixel ladder entry and kind 14's persistent sub-pixel shapes, +-1 data: sums in
    sixteenths (split-fp16: x 2^12) below 2^24 at the worst signs, both Winograd forms inside
    wino_fits, and the values of one image fp16 numbers after one rounding at most 2048."""
    n, cin, cout, h, w = shape
    assert (9 * cin * 16 + 16 * 3) * (E.LO + 2) // E.LO * E.LO < E.P24 * E.LO and 48 * (9 * cin * 16 + 48) < E.P24
    x, wt, b, _, _ = E.int_case(n, cin, cout, h, w, (1,))
    wsub = E.subpixel_weights_int(wt)
    assert E.wino_fits(1, wsub, 16, cin, 1)[0] and E.wino_fits(14, 48 * wsub, 16, cin, 1)[0]
    r = E.pre_sub(x[:1], wt, b)
    assert E.f32_exact(r.f64()) and np.abs(r.f64()).max() < 2048


@pytest.mark.parametrize("shape", [E.COB_SHAPE, E.COB_SHAPE_F16])
def test_cob_shapes_stay_in_the_exact_range(shape):
    """cin 256 on +-1 data: the F(2x2) forms and kind 14 inside wino_fits, the stored values fp16 numbers."""
    n, cin, cout, h, w = shape
    x, wt, b, _, _ = E.int_case(n, cin, cout, h, w, (1,))
    assert E.wino_fits(1, wt, 1, cin, 1)[0] and E.wino_fits(14, 48 * wt, 1, cin, 1)[0]
    assert E.f16_exact(E.leaky(E.pre_int(x, wt, b)).f64())


@pytest.mark.parametrize("n,cin,h,w", E.BLOCK0_PATHS)
def test_block0_path_shapes_stay_fp16(n, cin, h, w):
    x, wa, ba, wb, bb = E.block0_case(n, cin, h, w)
    mid, out = E.block0_ref(x, wa, ba, wb, bb)
    assert E.f16_exact(mid.f64()) and E.f16_exact(out.f64())


def test_tile_walk_mutations_break_equality():
    """At a multi-tile shape (5 x 40 x 17 x 65: 90 tiles of 32 co x 32 px x 8 rows) the slips of a
    tile walk each break ==: a tile's outputs taken from another tile, a tile computed with the
    previous tile's bias, the last tiles % grid tiles never written."""
    n, cin, cout, h, w = E.LADDER[0]
    x, wt, b, _, _ = E.int_case(n, cin, cout, h, w)
    pre = E.pre_int(x, wt, b)
    ref = E.leaky(pre).f64()
    boxes = E.tile_boxes(n, cout, h, w, 32, 8)
    assert len(boxes) == 90 and len({bx[2] - bx[1] for bx in boxes}) == 2      # a ragged second co block
    grid = 32
    size = lambda bx: (bx[2] - bx[1], bx[4] - bx[3], bx[6] - bx[5])  # noqa: E731
    # a workgroup's third tile (k = bid + 2 grid) computed at its second tile's coordinates
    k = next(i for i in range(2 * grid, len(boxes)) if size(boxes[i]) == size(boxes[i - grid]))
    assert not np.array_equal(E.leaky(E.tile_from_other(pre, boxes, k, k - grid)).f64(), ref)
    # the tile after a tile of the other co block keeps that tile's bias (two full co blocks: cout 64)
    other = E.tile_boxes(n, 64, h, w, 32, 8)
    x2, w2, b2, _, _ = E.int_case(n, cin, 64, h, w)
    pre2 = E.pre_int(x2, w2, b2)
    assert other[5][1] != other[4][1] and not np.array_equal(b2[:32], b2[32:])
    assert not np.array_equal(E.leaky(E.tile_with_previous_bias(pre2, other, 5, 4, b2)).f64(), E.leaky(pre2).f64())
    left = E.last_tiles_unwritten(ref, boxes, grid)
    assert len(boxes) % grid == 26 and np.isnan(left).sum() > 0 and not np.array_equal(left, ref)
    assert not (left == ref).all()
