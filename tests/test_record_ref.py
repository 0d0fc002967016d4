"""CPU: the record codec of tests/record_ref.py against the hand values of the layout, and
check_storage against synthetic corruptions of an otherwise correct storage -- the evidence that
tests/test_gpu_h8_storage.py fails on a kernel that writes one record too many."""
import pytest
import torch

from tests import glue_ref as G
from tests import record_ref as R

PRECS = G.PRECS
TOL0 = dict(rtol=0.0, atol=0.0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ch_off,c", [(0, 3), (4, 11), (8, 16), (5, 6)])
def test_codec_round_trips(prec, ch_off, c):
    n, h, w = 2, 9, 40
    x = G.pattern((n, c, h, w), 11) * 37
    hi, lo = R.nchw_to_records(x, prec, 4 if prec != "R32" else 8, ch_off)
    hp, wp = G.record_geom(h, w)
    assert hi.shape == (n, 4 if prec != "R32" else 8, hp, wp, R.CPR[prec]) and (lo is None) == (prec != "F16X3")
    back = G.records_to_nchw(hi, lo, ch_off, c, h, w)
    assert torch.equal(back, G.store_round(x, prec))
    # zero everywhere else: padding on four sides, the other channels
    for a in (hi, lo):
        if a is None:
            continue
        assert not a[:, :, 0].any() and not a[:, :, h + 1:].any() and not a[:, :, :, :8].any() and not a[:, :, :, 8 + w:].any()
        mask = torch.ones(a.shape[1] * a.shape[-1], dtype=torch.bool)
        mask[ch_off:ch_off + c] = False
        assert not a.permute(0, 2, 3, 1, 4).reshape(n, hp, wp, -1)[..., mask].any()


def test_codec_places_pixel_0_0_at_record_1_8():
    for prec in PRECS:
        x = torch.zeros(1, 9, 3, 5)
        x[0, 6, 0, 0] = 1.5
        x[0, 8, 2, 4] = -2.0
        hi, _ = R.nchw_to_records(x, prec, 4, 0)
        cpr = R.CPR[prec]
        assert float(hi[0, 6 // cpr, 1, 8, 6 % cpr]) == 1.5 and float(hi[0, 8 // cpr, 3, 12, 8 % cpr]) == -2.0
        assert int((hi != 0).sum()) == 2


def test_codec_hand_values():
    """The hand values of test_glue_ref.test_store_round_is_the_record_layout through the encoder."""
    b16 = lambda t: int(t.view(torch.int16).item()) & 0xFFFF  # noqa: E731
    cases = [(1.0, 0x3C00, 0x0000), (1 + 2.0 ** -12, 0x3C00, 0x3800), (1 + 2.0 ** -11, 0x3C00, 0x3C00),
             (1 + 2.0 ** -11 + 2.0 ** -20, 0x3C01, 0xBBFC), (2.0 ** -20 + 2.0 ** -31 + 2.0 ** -33, 0x0010, 0x0014),
             (-0.375, 0xB600, 0x0000), (65504.0, 0x7BFF, 0x0000), (65512.0, 0x7BFF, 0x7400), (-65519.0, 0xFBFF, 0xF780)]
    for v, hb, lb in cases:
        x = torch.full((1, 1, 1, 1), v, dtype=torch.float32)
        hi, lo = R.nchw_to_records(x, "F16X3", 2, 9)
        assert (b16(hi[0, 1, 1, 8, 1]), b16(lo[0, 1, 1, 8, 1])) == (hb, lb), v
        h16, none = R.nchw_to_records(x, "F16", 2, 9)
        assert none is None and b16(h16[0, 1, 1, 8, 1]) == hb
        r32, _ = R.nchw_to_records(x, "R32", 4, 9)
        assert float(r32[0, 2, 1, 8, 1]) == v


# ---- check_storage ------------------------------------------------------------------------------
N, H, W, GROUPS_ALLOC = 2, 9, 40, 6   # the view: 2 record groups from group 2; groups 0-1 before, 4-5 after


def correct(prec, ring=None):
    """(before, after, view, ref): pattern-filled raw planes with guard bands, and the same with the
    view's interior (and ring) holding the stored form of ref."""
    cpr = R.CPR[prec]
    hp, wp = G.record_geom(H, W)
    guard = 2 * wp * cpr
    ch_off, c = 2 * cpr, 2 * cpr
    ref = (G.pattern((N, c, H, W), 5) * 3).double()
    ehi, elo = R.nchw_to_records(ref, prec, GROUPS_ALLOC, ch_off)
    numel = N * GROUPS_ALLOC * hp * wp * cpr
    shape = (N, GROUPS_ALLOC, hp, wp, cpr)
    before, after = [], []
    for k, enc in enumerate(e for e in (ehi, elo) if e is not None):
        b = G.pattern((numel + 2 * guard,), 40 + k, R.DTYPE[prec])
        a = b.clone()
        a5 = a[guard:guard + numel].view(shape)
        a5[:, 2:4, 1:H + 1, 8:8 + W] = enc[:, 2:4, 1:H + 1, 8:8 + W]
        if ring:
            a5[:, 2:4] = R._replicated(a5[:, 2:4], H, W)
        before.append(b)
        after.append(a)
    return before, after, R.StorageView(N, GROUPS_ALLOC, cpr, guard, ch_off, c), ref


def tol_of(prec):
    return dict(rtol=G.STORE_REL[prec], atol=0.0)


def at(view, plane, i, g, y, x, e):
    hp, wp = G.record_geom(H, W)
    return view.guard + ((((i * view.groups + g) * hp + y) * wp + x) * view.cpr + e)


@pytest.mark.parametrize("ring", [None, "replicate"])
@pytest.mark.parametrize("prec", PRECS)
def test_check_storage_accepts_correct(prec, ring):
    before, after, view, ref = correct(prec, ring)
    R.check_storage(before, after, view, H, W, ref, tol_of(prec), ring=ring)
    if ring:  # without ring="replicate" the written ring is a stray write
        with pytest.raises(AssertionError, match="outside the view's interior"):
            R.check_storage(before, after, view, H, W, ref, tol_of(prec))


# name -> (ring, plane, (image, group, row, column, element) or a flat raw index, expected words)
CORRUPT = {
    "right padding": (None, 0, (1, 3, 4, 8 + W, 0), "group 3, record row 4, column 48"),
    "bottom padding": (None, 0, (0, 2, H + 1, 20, 1), f"group 2, record row {H + 1}, column 20"),
    "row h+2 under replicate": ("replicate", 0, (1, 2, H + 2, 8, 0), f"record row {H + 2}, column 8"),
    "group before the view": (None, 0, (0, 1, 3, 10, 2), "image 0, group 1, record row 3, column 10"),
    "group after the view": (None, 0, (1, 4, 3, 10, 2), "image 1, group 4, record row 3, column 10"),
    "lo plane only": (None, 1, (0, 2, 0, 9, 3), "plane lo, image 0, group 2, record row 0, column 9"),
    "leading guard band": (None, 0, 5, "leading guard band"),
    "trailing guard band": (None, 0, -3, "trailing guard band"),
}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(CORRUPT))
def test_check_storage_rejects(prec, name):
    ring, plane, where, words = CORRUPT[name]
    if plane == 1 and prec != "F16X3":
        prec = "F16X3"  # the only precision with a lo plane
    before, after, view, ref = correct(prec, ring)
    k = where if isinstance(where, int) else at(view, plane, *where)
    after[plane][k] = -after[plane][k]     # still finite, still non-zero: one value, one sign bit
    with pytest.raises(AssertionError, match=words):
        R.check_storage(before, after, view, H, W, ref, tol_of(prec), ring=ring)


@pytest.mark.parametrize("prec", PRECS)
def test_check_storage_rejects_zero_over_pattern(prec):
    """A kernel that writes zeros into a neighbouring group or the padding passes a zero-filled
    tensor read through to_nchw; here it changes a pattern value."""
    before, after, view, ref = correct(prec)
    for where in [(0, 0, 5, 12, 0), (1, 2, 5, 3, 1), (1, 5, 17, 79, view.cpr - 1)]:
        a = [p.clone() for p in after]
        assert float(a[0][at(view, 0, *where)]) != 0.0
        a[0][at(view, 0, *where)] = 0.0
        with pytest.raises(AssertionError, match="outside the view's interior"):
            R.check_storage(before, a, view, H, W, ref, tol_of(prec))


def test_check_storage_rejects_wrong_interior_and_bad_split():
    """The interior: a value past the tolerance (with its position), NaN, and at F16X3 a lo that no
    split16 makes (more than half an ulp of hi) although the join is within the tolerance."""
    for prec in PRECS:
        before, after, view, ref = correct(prec)
        bad = ref.clone()
        bad[1, 3, 8, 39] += 1.0
        with pytest.raises(AssertionError, match="image 1, group 2, record row 9, column 47, element 3"):
            R.check_storage(before, after, view, H, W, bad, tol_of(prec))
        a = [p.clone() for p in after]
        a[0][at(view, 0, 0, 2, 1, 8, 0)] = float("nan")
        with pytest.raises(AssertionError, match="past the tolerance"):
            R.check_storage(before, a, view, H, W, ref, tol_of(prec))
    before, after, view, ref = correct("F16X3")
    k = at(view, 0, 0, 3, 2, 9, 1)
    hi = after[0][k].clone()
    up, _ = R._f16_neighbours(hi.view(1))
    step = float(up) - float(hi)
    after[0][k] = up[0]                                  # hi one ulp up, lo 2^11 x one ulp down: the same join
    after[1][k] = torch.tensor((float(after[1][k]) / G.LO_SCALE - step) * G.LO_SCALE, dtype=torch.float16)
    with pytest.raises(AssertionError, match="split16 partner"):
        R.check_storage(before, after, view, H, W, ref, dict(rtol=1e-4, atol=1e-4))


def test_check_storage_interior_mask():
    """interior_mask (the ring fix-up): only the masked pixels may change."""
    prec = "R32"
    before, after, view, ref = correct(prec)
    ringpix = torch.zeros(H, W, dtype=torch.bool)
    ringpix[0], ringpix[-1], ringpix[:, 0], ringpix[:, -1] = True, True, True, True
    with pytest.raises(AssertionError, match="outside the view's interior"):
        R.check_storage(before, after, view, H, W, ref, tol_of(prec), interior_mask=ringpix)
    hp, wp = G.record_geom(H, W)
    numel = N * GROUPS_ALLOC * hp * wp * view.cpr
    b5 = before[0][view.guard:view.guard + numel].view(N, GROUPS_ALLOC, hp, wp, view.cpr)
    a5 = after[0][view.guard:view.guard + numel].view(N, GROUPS_ALLOC, hp, wp, view.cpr)
    a5[:, 2:4, 2:H, 9:7 + W] = b5[:, 2:4, 2:H, 9:7 + W]   # the inner pixels back to what they were
    R.check_storage(before, after, view, H, W, ref, tol_of(prec), interior_mask=ringpix)
