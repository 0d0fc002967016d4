"""No GPU: the references of tests/planar_ref.py against float64 torch, the 2^24 range of every
case, the mutations each reference must notice, the float bounds and their fp32 emulation, the
packed blob of rrin_pack_conv3x3 and the float64 backwarp at integer flows."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rrin_amd import _lib
from tests import exact_ref as E
from tests import glue_ref as G
from tests import planar_ref as P

SIZES = list(P.SHAPES)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def torch_ref(x, wt, b, up, epi):
    xin = _t(x)
    if up:
        xin = F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=False)
    y = F.conv2d(xin, _t(wt), _t(b), padding=1)
    if epi != P.LINEAR:
        y = F.leaky_relu(y, E.SLOPE)
    return y, (F.avg_pool2d(y, 2) if epi == P.POOL else None)


def test_the_cases_cover_every_instantiation():
    """6 configs x 2 source modes x 3 epilogues: 18 x 34 alone runs all of them, and every size
    of a pool case is even."""
    assert {(up, epi) for up, epi, _, _ in P.combos(18, 34)} == {(u, e) for u in (False, True) for e in P.EPIS}
    for (h, w) in SIZES:
        for up, epi, _, _ in P.combos(h, w):
            assert not (epi == P.POOL or up) or (h % 2 == 0 and w % 2 == 0)
    assert _lib.lib().rrin_conv_cfg_count() == 6
    assert sorted({_lib.lib().rrin_conv_cfg_bm(c) for c in range(6)}) == list(P.BMS)


@pytest.mark.parametrize("h,w", SIZES)
def test_int_references_equal_float64_torch_and_stay_below_2_24(h, w):
    for up, epi, cin, cout in P.combos(h, w):
        x, wt, b = P.int_case(cin, cout, h, w, up)
        assert not (x == 0).any() and not (wt == 0).any() and not (b == 0).any()
        steps = P.worst_steps(x, wt, b, up, epi)
        assert steps < E.P24, (h, w, up, epi, cin, cout, steps)
        got = P.epilogue(P.pre_ref(x, wt, b, up), epi)
        for r, t in zip(got, torch_ref(x, wt, b, up, epi)):
            assert (r is None) == (t is None)
            if r is not None:
                assert np.array_equal(r.f64(), t.numpy()) and E.f32_exact(r.f64())
        dst, pool = P.conv_ref(cin, cout, h, w, up, epi)
        assert dst.shape == (P.N, cout, h, w) and (pool is None or pool.shape == (P.N, cout, h // 2, w // 2))


def test_shrinking_rule():
    """No case needs +-1 data (the deepest, 256 channels upsampled and pooled, is 9 x 256 x 4 + 3 in
    units of 1, x 256 steps: 2.4e6), and data that would not fit is refused rather than used."""
    for (h, w) in SIZES:
        for up, epi, cin, cout in P.combos(h, w):
            x, wt, _ = P.int_case(cin, cout, h, w, up)
            assert int(np.abs(x).max()) == 2 and int(np.abs(wt).max()) == 2
    x, wt, b = P.int_case(256, 32, 18, 34, True)
    assert P.worst_steps(x, wt, b, True, P.POOL) <= (9 * 256 * 4 + 3) * 256 < E.P24
    assert P.worst_steps(x * 16, wt, b, True, P.POOL) >= E.P24


def test_permuted_view_reference():
    """The refine permutation: buffer channel c meets the weights of channel perm[c]."""
    x, wt, b = P.int_case(10, 3, 18, 34, False, tag=1)
    dst, _ = P.conv_ref(10, 3, 18, 34, False, P.LINEAR, 1, P.REFINE_PERM)
    ref_in = np.empty_like(x)
    ref_in[:, list(P.REFINE_PERM)] = x
    assert np.array_equal(dst.double().numpy(), torch_ref(ref_in, wt, b, False, P.LINEAR)[0].numpy())


@pytest.mark.parametrize("h,w", SIZES)
def test_mutations_break_equality(h, w):
    seen = set()
    for up, epi, cin, cout in P.combos(h, w):
        x, wt, b = P.int_case(cin, cout, h, w, up)
        good = P.epilogue(P.pre_ref(x, wt, b, up), epi)
        for bm in P.BMS:
            for name, bad in P.mutants(x, wt, b, up, epi, bm).items():
                same = all(g is None or np.array_equal(g.units * (m.scale // g.scale), m.units) for g, m in zip(good, bad))
                assert not same, (name, h, w, up, epi, cin, cout, bm)
                seen.add(name)
    want = {"drop_tap", "chunk_twice"} | ({"rows_swapped"} if h >= 2 else set())
    if any(up for up, _ in P.SHAPES[(h, w)]) and w >= 4:
        want.add("bilinear_swapped")
    if h >= 4 and any(P.POOL in e for _, e in P.SHAPES[(h, w)]):
        want.add("pool_rows")
    assert seen == want, (seen, want)


@pytest.mark.parametrize("cin,cout", P.CHANNELS + [P.DEEP])
def test_packed_weights_are_their_rational_values(cin, cout):
    """rrin_pack_conv3x3 at every BM, with and without a permutation: the blob decodes to the
    integers that went in, zero everywhere else."""
    lib = _lib.lib()
    _, wt, b = P.int_case(cin, cout, 18, 34, False)
    rot = tuple((c + 4) % cin for c in range(cin))
    for bm in P.BMS:
        for perm in (None, rot):
            w32 = np.ascontiguousarray(wt, np.float32)
            b32 = np.ascontiguousarray(b, np.float32)
            wp = np.full(lib.rrin_pack_conv3x3_floats(cout, cin, bm), np.nan, np.float32)
            bp = np.full(lib.rrin_pack_bias_floats(cout, bm), np.nan, np.float32)
            assert wp.size == -(-cout // bm) * bm * -(-cin // 8) * 72 and bp.size == -(-cout // bm) * bm
            pa = np.asarray(perm, np.int32) if perm else None
            assert lib.rrin_pack_conv3x3(w32.ctypes.data, b32.ctypes.data, cout, cin, bm,
                                         pa.ctypes.data if perm else None, wp.ctypes.data, bp.ctypes.data) == 0
            got_w, got_b = P.unpack_planar(wp, bp, cout, cin, bm)
            want = wt[:, list(perm)] if perm else wt
            assert np.array_equal(got_w, want.reshape(cout, cin, 9).astype(np.float64))
            assert np.array_equal(got_b, b.astype(np.float64))


# ---- float bounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [False, True])
def test_fp32_emulation_is_inside_the_bound(up):
    """The numpy fp32 restatement of the kernel (UPSAMPLE2X: its LDS expansion, every product and sum
    rounded on its own) stays inside the derived bound against float64; each staged value is within
    UP_ROUNDINGS u of the upsample of |x|.  Worst err / (u S) on this data: 3.83 DIRECT, 1.98
    UPSAMPLE2X (the bounds are K + 2 = 146 and K + 6 = 150: worst case, not typical)."""
    x, wt, b = P.float_case(up)
    xin = x.numpy()
    if up:
        xin = P.up_emulate(x)
        err_up = np.abs(xin.astype(np.float64) - P.up64(x).numpy())
        assert (err_up <= P.UP_ROUNDINGS * P.U * P.up64(x.abs()).numpy()).all()
        assert err_up.max() > 0
    got = P.conv_emulate(xin, wt, b)
    for epi in P.EPIS:
        ref, refp, bnd, bndp, s = P.float_ref(x, wt, b, up, epi)
        v = got if epi == P.LINEAR else P.leaky64(torch.from_numpy(got)).numpy()
        err = np.abs(v - ref)
        ratio = float((err / (P.U * s)).max())
        print(f"emulation up={up} epi={epi}: worst err / (u S) = {ratio:.2f}")
        assert (err <= bnd).all() and 0.5 < ratio < 8
        if epi == P.POOL:
            assert (np.abs(E.pool64(v) - refp) <= bndp).all()


def test_bound_rejects_a_chunk_summed_twice():
    cin = P.FLOAT_SHAPE[0]
    assert cin == 16
    for up in (False, True):
        x, wt, b = P.float_case(up)
        xin = P.up64(x) if up else x.double()
        extra = F.conv2d(xin[:, 8:], wt.double()[:, 8:], None, padding=1)
        for epi in P.EPIS:
            ref, refp, bnd, bndp, _ = P.float_ref(x, wt, b, up, epi)
            pre = F.conv2d(xin, wt.double(), b.double(), padding=1) + extra
            bad = (pre if epi == P.LINEAR else P.leaky64(pre)).numpy()
            assert (np.abs(bad - ref) > bnd).mean() > 0.9
            if epi == P.POOL:
                assert (np.abs(E.pool64(bad) - refp) > bndp).mean() > 0.9


def test_bound_rejects_align_corners_true():
    x, wt, b = P.float_case(True)
    for epi in P.EPIS:
        ref, refp, bnd, bndp, _ = P.float_ref(x, wt, b, True, epi)
        bad, badp, _, _, _ = P.float_ref(x, wt, b, True, epi, align_corners=True)
        assert (np.abs(bad - ref) > bnd).mean() > 0.9
        if epi == P.POOL:
            assert (np.abs(badp - refp) > bndp).mean() > 0.9


# ---- backwarp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", P.WARP_SIZES)
def test_warp_reference_is_the_shifted_image_at_aligned_flows(h, w):
    """The oracle's normalisation is defined at an extent of 1 (align_corners=False divides by W, not
    by W - 1) and un-normalises to gx + u - 0.5, so zero flow is the mean of four taps, three of them
    outside a 1 x 1 frame (img / 4), and the flows that give the shifted image are the integers plus
    one half.  There the float64 backwarp is the image at the tap (to the 1e-13 that (x / W) W costs
    in double; exactly at power-of-two extents), and exactly 0 for +-1e9.  The fp32 coordinate
    arithmetic is exact at power-of-two extents only: elsewhere part of these pixels have weights a
    few 1e-6 off 1 and 0, and the GPU test holds those to A_WARP."""
    for c in (1, 3):
        img, flow, kind = P.warp_case(P.N, c, h, w)
        val, exact, inside = P.shifted(img, flow, kind)
        fin = torch.where(kind == P.BAD, torch.zeros(()), flow.permute(1, 0, 2, 3)).permute(1, 0, 2, 3)
        ref = G.warp(img, fin)
        m = inside[:, None].expand_as(ref)
        pow2 = (h, w) in ((1, 1), (16, 32))
        assert float((ref[m] - val.double()[m]).abs().max()) <= (0.0 if pow2 else 1e-13)
        assert int(inside.sum()) > 0 and bool((ref[(kind == P.HUGE)[:, None].expand_as(ref)] == 0).all())
        if h * w >= 23:
            assert sorted(kind.unique().tolist()) == [0, 1, 2, 3, 4]
        zero = (kind == P.ZERO)[:, None].expand_as(ref)
        if (h, w) == (1, 1):
            assert torch.equal(ref[zero], img.double()[zero] / 4)
        if pow2:
            assert torch.equal(exact, inside)
        if (h, w) == (17, 50):
            assert 0 < int(exact.sum()) < int(inside.sum())


def test_entry_points_take_pointers():
    """ctypes signatures the GPU tests rely on when they pass None for a descriptor."""
    assert _lib.SIGNATURES["rrin_conv3x3_fwd"][1][0] == C.POINTER(_lib.ConvDesc)
    assert _lib.SIGNATURES["rrin_head_fwd"][1][0] == C.POINTER(_lib.HeadDesc)
