"""CPU: pin tests/glue_ref.py (the float64 reference of the per-kernel glue tests) to the
oracle, its ``store_round`` to the documented record layout, and the tolerance A of
tests/test_gpu_glue.py to the fp32 oracle's own deviation on that file's inputs."""
import numpy as np
import torch

from oracle.ref_net import net_forward
from oracle.ref_net import warp as oracle_warp
from rrin_amd import Net
from rrin_amd.engine import t_coefficients
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch
from tests import glue_ref as G


def _dev(a, b):
    return float((a.double() - b.double()).abs().max())


def test_stages_match_oracle():
    """The float64 stages, fed the oracle's U-Net outputs (taps Flow, refine, mask_logits,
    final_unet) on synthetic_batch(2, 64, 96) with the stress weights at t = 0.5, against the
    oracle's own glue (taps ft0, ft1, xt1, xt2, blend, final_pre and the returned frame).

    The oracle computes in fp32, so the bound is its rounding.  Measured max-abs here:
    ft0 3.0e-7, ft1 3.6e-7 (flows up to 4 px), xt1 5.1e-6, xt2 5.0e-6 (position rounding at
    w = 96 times the frame's gradient), blend 4.1e-6, final_pre 4.1e-6, output 4.1e-6.
    Bounds: 4 x the measured value, and never above 1e-5."""
    sd = keyed_state_dict(Net().state_dict(), stress=True)
    i0, i1 = synthetic_batch(2, 64, 96)
    taps = {}
    with torch.no_grad():
        out = net_forward(sd, i0, i1, 0.5, taps)
    coef = G.coefficients(0.5, 2)
    ft0, ft1 = G.flow_blend(coef, taps["Flow"])
    ft0, ft1, xt1, xt2 = G.refine(ft0, ft1, taps["refine"], i0, i1)
    blend = G.mask_blend(coef, taps["mask_logits"], xt1, xt2)
    pre = taps["final_unet"].double() + blend
    got = {"ft0": ft0, "ft1": ft1, "xt1": xt1, "xt2": xt2, "blend": blend, "final_pre": pre}
    bound = {"ft0": 1.5e-6, "ft1": 1.5e-6, "xt1": 1e-5, "xt2": 1e-5, "blend": 1e-5, "final_pre": 1e-5}
    for k, v in got.items():
        d = _dev(v, taps[k])
        print(f"{k}: max-abs vs oracle {d:.3e}")
        assert d <= bound[k], (k, d)
    d = _dev(G.final(taps["final_unet"], blend), out)
    print(f"output: max-abs vs oracle {d:.3e}")
    assert d <= 1e-5, d
    # the kernels' fp32 coefficient table is the float64 one rounded
    assert torch.equal(G.coefficients(0.5, 2).float(), t_coefficients(0.5, 2))
    tt = torch.tensor([0.3, 0.75])
    np.testing.assert_allclose(G.coefficients(tt, 2).numpy(), t_coefficients(tt, 2).double().numpy(), rtol=3e-7, atol=0)


def test_fp32_twins_are_the_float64_stages_rounded():
    """The twins differ from the float64 stages by fp32 rounding only (3 roundings per value)."""
    n, h, w = 2, 24, 40
    coef = t_coefficients(torch.tensor(G.T_PER_IMAGE[:n]), n)
    raw = G.pattern((n, 4, h, w), 3) * 100
    a32 = torch.cat(G.flow_blend32(coef, raw), 1)
    a64 = torch.cat(G.flow_blend(coef, raw), 1)
    assert bool(((a32.double() - a64).abs() <= 3 * 2.0 ** -24 * 200).all())
    acc, base = G.pattern((n, 3, h, w), 4), G.pattern((n, 3, h, w), 5)
    q = G.final32(acc, base)
    assert float(q.min()) == 0.0 and float(q.max()) == 1.0      # both clamps reached
    assert _dev(q, G.final(acc, base)) <= 2.0 ** -24 * 4
    assert torch.equal(G.to_u8(torch.tensor([0.0, 0.999999, 1.0, 0.5, 1 / 255])),
                       torch.tensor([0, 254, 255, 127, 1], dtype=torch.uint8))


def test_store_round_is_the_record_layout():
    """include/rrin_hip.h: F16X3 holds v as hi = f16(v), lo = f16((v - hi) * 2^11) and reads
    hi + lo 2^-11; F16 holds f16(v); fp32 records hold v.  Hand values, tiny and near 65504."""
    bits = lambda t: int(t.view(torch.int16).item()) & 0xFFFF  # noqa: E731
    cases = [
        # v, hi bits, lo bits, F16X3 value, F16 value
        (1.0, 0x3C00, 0x0000, 1.0, 1.0),
        (1 + 2.0 ** -12, 0x3C00, 0x3800, 1 + 2.0 ** -12, 1.0),           # lo = 0.5: 2^-12 * 2^11
        (1 + 2.0 ** -11, 0x3C00, 0x3C00, 1 + 2.0 ** -11, 1.0),           # fp16 tie: to even
        (1 + 2.0 ** -11 + 2.0 ** -20, 0x3C01, 0xBBFC, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -10),
        # tiny: hi a subnormal fp16; v - hi = 2^-31 + 2^-33 would vanish in an unscaled fp16 lo
        (2.0 ** -20 + 2.0 ** -31 + 2.0 ** -33, 0x0010, 0x0014, 2.0 ** -20 + 2.0 ** -31 + 2.0 ** -33, 2.0 ** -20),
        (-0.375, 0xB600, 0x0000, -0.375, -0.375),
        (65504.0, 0x7BFF, 0x0000, 65504.0, 65504.0),
        (65512.0, 0x7BFF, 0x7400, 65512.0, 65504.0),                     # lo = 8 * 2^11 = 16384
        (-65519.0, 0xFBFF, 0xF780, -65519.0, -65504.0),                  # lo = -15 * 2^11 = -30720
    ]
    for v, hb, lb, x3, f16 in cases:
        t = torch.tensor([v], dtype=torch.float32)
        assert float(t) == v                                             # the hand value is an fp32
        hi, lo = G.split16(t)
        assert (bits(hi), bits(lo)) == (hb, lb), (v, hex(bits(hi)), hex(bits(lo)))
        assert float(G.store_round(t, "F16X3")) == x3, v
        assert float(G.store_round(t, "F16")) == f16, v
        assert float(G.store_round(t, "R32")) == v
        if abs(v) >= 2.0 ** -14:                                         # S holds where hi is a normal fp16
            assert abs(x3 - v) <= G.STORE_REL["F16X3"] * abs(v) and abs(f16 - v) <= G.STORE_REL["F16"] * abs(v)
    # past the fp16 range (the range guard's business): 65520 rounds to inf
    over = torch.tensor([65520.0])
    assert torch.isinf(G.store_round(over, "F16")).all() and not torch.isfinite(G.store_round(over, "F16X3")).any()
    # float64 in: rounded to fp32 first
    assert float(G.store_round(torch.tensor([1 + 2.0 ** -30], dtype=torch.float64), "R32")) == 1.0
    # records_to_nchw reads what split16 wrote
    v = G.pattern((1, 8), 9) * 37
    hi, lo = G.split16(v)
    st_hi, st_lo = torch.zeros(1, 1, 3, 10, 8, dtype=torch.float16), torch.zeros(1, 1, 3, 10, 8, dtype=torch.float16)
    st_hi[0, 0, 1, 8], st_lo[0, 0, 1, 8] = hi[0], lo[0]
    assert torch.equal(G.records_to_nchw(st_hi, st_lo, 0, 8, 1, 1).view(1, 8), G.store_round(v, "F16X3"))


def test_tolerance_A_is_the_fp32_oracles_deviation():
    """A of tests/test_gpu_glue.py's tolerance A + S |ref| (REFINE's warps, MASK's blend) is
    4 x the deviation of the fp32 oracle from the float64 stage on that file's inputs (fp32
    records; the head conv in float64 rounded to fp32 stands in for the kernel's), capped at 1e-5.

    Measured: warp 7.2e-6 (n=3, 16x80, x1 flows; 2.5e-6 at 24x40, 8.0e-7 at 16x32; x300 flows
    3.3e-6 / 1.6e-6 / 4.1e-7): 4 x that is above the cap, so A_WARP = 1e-5, and the deviation is
    position rounding at the frame's width, which a smaller flow scale does not lower (x1 is the
    larger of the two).  Mask blend 2.9e-7 (2.4e-7 at 16x32; 1e-7 in the +-100 logit case):
    A_MASK = 1.16e-6."""
    warp_dev, mask_dev = 0.0, 0.0

    def blend32(coef, logits, xt):
        m = torch.sigmoid(logits)
        w1, w2 = coef[:, 4].view(-1, 1, 1, 1) * m[:, 0:1], coef[:, 5].view(-1, 1, 1, 1) * m[:, 1:2]
        return (w1 * xt[:, :3] + w2 * xt[:, 3:]) / (w1 + w2 + 1e-8)

    for n, h, w in G.SHAPES:
        c = G.case(n, h, w)
        hp, wp = G.record_geom(h, w)
        pat = G.pattern((n, G.G16_CHANNELS // 4, hp, wp, 4), 1)
        ft, xt = G.records_to_nchw(pat, None, 6, 4, h, w), G.records_to_nchw(pat, None, 10, 6, h, w)
        coef = t_coefficients(torch.tensor(G.T_PER_IMAGE[:n]), n)
        for scale in G.SCALES:
            s32 = G.refine_add32(ft, G.conv64(c["refine"], *G.keyed_head("refine", scale)).float())
            for img, fl in ((c["x0"], s32[:, :2]), (c["x1"], s32[:, 2:])):
                d = _dev(oracle_warp(img, fl), G.warp(img, fl))
                print(f"warp {n}x{h}x{w} x{scale:g}: {d:.3e}")
                warp_dev = max(warp_dev, d)
        logits = G.conv64(c["mask"], *G.keyed_head("mask")).float()
        d = _dev(blend32(coef, logits, xt), G.mask_blend(coef, logits, xt[:, :3], xt[:, 3:]))
        print(f"mask {n}x{h}x{w}: {d:.3e}")
        mask_dev = max(mask_dev, d)
    n, h, w = 2, 16, 32
    c = G.case(n, h, w)
    hp, wp = G.record_geom(h, w)
    xt = G.records_to_nchw(G.pattern((n, G.G16_CHANNELS // 4, hp, wp, 4), 1), None, 10, 6, h, w)
    coef = t_coefficients(torch.tensor([0.0, 1.0]), n)
    for bias in G.MASK_EDGE_BIAS:
        logits = G.conv64(c["mask"], G.keyed_head("mask")[0], torch.tensor(bias)).float()
        d = _dev(blend32(coef, logits, xt), G.mask_blend(coef, logits, xt[:, :3], xt[:, 3:]))
        print(f"mask +-100 {bias}: {d:.3e}")
        mask_dev = max(mask_dev, d)
    assert 0.75 * G.DEV_WARP <= warp_dev <= G.DEV_WARP, warp_dev
    assert 0.75 * G.DEV_MASK <= mask_dev <= G.DEV_MASK, mask_dev
    assert G.A_WARP == min(4 * G.DEV_WARP, 1e-5) and G.A_MASK == min(4 * G.DEV_MASK, 1e-5)
