"""CPU: the references and case tables of the whole-forward contract tests (tests/net_contract.py),
the host-side rejections of rrin_unet_fwd / rrin_unet_scratch_bytes (nothing is launched) and the
host schedule of every (in_ch, depth) of the U-Net table in every precision."""
import ctypes as C

import pytest
import torch

from rrin_amd import _lib
from rrin_amd import engine as E
from rrin_amd.unet import UNet
from tests import net_contract as NC

FAKE = 1 << 30  # a fabricated non-null device pointer: never dereferenced
E_SHAPE, E_ARG = -1, -2
SANITY = 1e-4  # float64 reference vs fp32 oracle: the stress gate 1e-3 with a factor 10 to spare


def test_unet_table_covers_the_contract():
    cases = set(NC.UNET_CASES)
    assert len(cases) == len(NC.UNET_CASES) and 18 <= len(cases) <= 24
    for d in (2, 3, 4, 5):
        assert {co for _, co, dd in cases if dd == d} == {2, 3, 4}
    for d in (2, 5):
        assert {ci for ci, _, dd in cases if dd == d} == set(NC.UNET_IN_CH)


@pytest.mark.parametrize("ci,co,d", NC.UNET_CASES)
def test_unet_reference_sanity_and_scale(ci, co, d):
    """float64 reference == fp32 oracle within 1e-4 at every size (and for the second input of the
    reuse check); every scaled reference has max|ref| in [0.5, 2], so the tolerance relative to
    max(1, max|ref|) is a relative one."""
    for n, h, w in NC.UNET_SIZES:
        for which in (0, 1):
            ref = NC.unet_ref(ci, co, d, n, h, w, which)
            assert ref.dtype == torch.float64 and tuple(ref.shape) == (n, co, h, w)
            top = float(ref.abs().max())
            assert 0.5 <= top <= 2.0, f"({ci},{co},{d}) {n}x{h}x{w} input {which}: max|ref| {top:.3f}"
            err = NC.maxabs(NC.unet_oracle32(ci, co, d, n, h, w, which), ref)
            assert err <= SANITY, f"({ci},{co},{d}) {n}x{h}x{w}: oracle vs float64 {err:.3e}"


@pytest.mark.parametrize("which", NC.NET_WEIGHTS)
def test_net_reference_sanity(which):
    for n, h, w in NC.NET_SIZES:
        for tname in NC.NET_T:
            ref, taps = NC.net_ref(which, n, h, w, tname)
            assert ref.dtype == torch.float64 and tuple(ref.shape) == (n, 3, h, w)
            assert set(NC.TAP_KEYS.values()) <= set(taps)
            err = NC.maxabs(NC.net_oracle32(which, n, h, w, tname), ref)
            assert err <= SANITY, f"{which} {n}x{h}x{w} t={tname}: oracle vs float64 {err:.3e}"


def test_net_t_cases():
    assert NC.net_t("0", 2) == 0.0 and NC.net_t("1", 2) == 1.0
    t = NC.net_t("tensor", 3)
    assert tuple(t.shape) == (3, 1, 1, 1) and t.flatten().tolist() == [0.0, 1.0, 0.5]
    assert NC.net_t("tensor", 2).flatten().tolist() == [0.0, 1.0]
    # the coefficient table at the ends: one blend weight (columns 4, 5: 1 - t, t) exactly zero
    c = E.t_coefficients(t, 3)
    assert c[0].tolist() == [0, 0, 1, 0, 1, 0, 0, 0] and c[1].tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
    assert E.t_coefficients(0.0, 1)[0].tolist() == [0, 0, 1, 0, 1, 0, 0, 0]
    assert E.t_coefficients(1.0, 1)[0].tolist() == [0, 1, 0, 0, 0, 1, 0, 0]


def test_poisoned_pair_is_all_nan_in_the_oracle():
    """The history tests' worst predecessor: frame 0 scaled by 3e38 (finite fp32) overflows inside
    the first U-Net and the oracle's output is NaN everywhere."""
    from oracle.ref_net import net_forward
    i0, i1 = NC.net_frames(3, 32, 48)
    bad = i0 * 3e38
    assert torch.isfinite(bad).all() and float(bad.max()) > 1e38
    with torch.no_grad():
        out = net_forward(NC.net_state_dict("stress"), bad, i1, 0.5)
    assert torch.isnan(out).all()


# ---- host rejections ------------------------------------------------------------------------

def _unet_desc(in_ch=6, out_ch=4, depth=5, h=32, w=48, n=1, prec=_lib.PREC_F32R, x=FAKE):
    d = _lib.UNetDesc()
    d.n, d.h, d.w, d.in_ch, d.out_ch, d.depth, d.prec = n, h, w, in_ch, out_ch, depth, prec
    d.x, d.y = x, FAKE
    d.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.head.w = d.head.bias = FAKE
    d.workspace, d.workspace_bytes = FAKE, 1 << 40
    return d


REJECTS = [
    (dict(in_ch=0), E_ARG), (dict(in_ch=17), E_ARG),
    (dict(out_ch=1), E_ARG), (dict(out_ch=5), E_ARG),
    (dict(depth=1), E_ARG), (dict(depth=6), E_ARG),
    (dict(h=0), E_SHAPE), (dict(h=8), E_SHAPE), (dict(w=8), E_SHAPE),
    (dict(h=24), E_SHAPE), (dict(w=40), E_SHAPE), (dict(h=17), E_SHAPE), (dict(w=-16), E_SHAPE),
    (dict(n=0), E_SHAPE),
    (dict(prec=-1), E_ARG), (dict(prec=4), E_ARG),
]


@pytest.mark.parametrize("kw,code", REJECTS, ids=[f"{k}={v}" for kw, _ in REJECTS for k, v in kw.items()])
def test_unet_entries_reject_before_any_launch(kw, code):
    """Outside the documented contract (in_ch 1..16, out_ch 2..4, depth 2..5, h and w multiples of
    16 from 16 up) both entries return the documented code before any HIP call: the pointers are
    fabricated and this machine may have no GPU."""
    L = _lib.lib()
    assert L.rrin_unet_fwd(C.byref(_unet_desc(**kw)), None) == code
    assert L.rrin_unet_scratch_bytes(C.byref(_unet_desc(**kw))) == code


def test_unet_entries_reject_null():
    L = _lib.lib()
    assert L.rrin_unet_fwd(None, None) == E_ARG and L.rrin_unet_scratch_bytes(None) == E_ARG
    assert L.rrin_unet_fwd(C.byref(_unet_desc(x=None)), None) == E_ARG
    for depth, want in ((1, E_ARG), (2, 8), (3, 13), (4, 18), (5, 23), (6, E_ARG)):  # 5d - 2
        assert L.rrin_unet_conv_count(depth) == want


# ---- host schedule --------------------------------------------------------------------------

@pytest.mark.parametrize("ci,d", sorted({(ci, d) for ci, _, d in NC.UNET_CASES}))
def test_unet_host_schedule(ci, d):
    """The conv table the engine builds for UNet(ci, ., d) -- unit_convs -> h8_records ->
    geom_splits -> h8_cfgs -> h8_splits, at every size of the table and in every size class a
    forced class could ask for -- has rrin_unet_conv_count(d) entries, every config exists at the
    precision and takes the conv's cin (rrin_conv_h8_cfg_fits); the planar packing likewise."""
    L = _lib.lib()
    count = L.rrin_unet_conv_count(d)
    body, heads = E.unit_convs([("unet", UNet(ci, 2, d), None)])
    assert len(body) == count and len(heads) == 1
    assert body[0][2] == ci and [c[5] for c in body[:2 * d]] == [k // 2 for k in range(2 * d)]
    _, meta = E.pack_planar_host(body)
    assert len(meta) == count and all(0 <= m[2] < L.rrin_conv_cfg_count() for m in meta)
    records = E.h8_records(body, 2)
    assert len(records) == count
    for precision in NC.RECORD_PRECISIONS:
        prec = _lib.PRECISIONS[precision]
        for n, h, w in NC.UNET_SIZES:
            geo = E.geom_splits(records, prec, h, w)
            for size in ("small", "large"):
                cfgs = E.h8_cfgs(records, prec, size, geo)
                splits = E.h8_splits(records, cfgs, geo, prec)
                assert len(cfgs) == len(splits) == count
                for (_, _, cin, _, _, _, edge), cfg, (k, sub) in zip(records, cfgs, splits):
                    assert 0 <= cfg < L.rrin_conv_h8_cfg_count()
                    assert L.rrin_conv_h8_cfg_fits(cfg, prec, cin), (precision, size, cin, cfg)
                    assert (sub != 0) == (edge is not None)
                    assert k == 0 or (prec == _lib.PREC_F32R and L.rrin_conv_h8_cfg_wino(cfg) in (3, 4))
