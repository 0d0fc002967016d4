"""GPU: exact values and whole storage on the launch paths the small exact suites never take
("Launch paths").

tests/test_gpu_h8_exact.py and tests/test_gpu_h8_storage.py run a few tiles: every launcher takes
one workgroup per tile.  Here the launch-shape query (rrin_conv_h8_launch_info, the launchers' own
decision) picks, per precision and config, the first shape of exact_ref.LADDER at which
  * a config with a capped grid walks tiles: grid < tiles, tiles % grid != 0, tiles > 2 grid --
    workgroups with two and with three or more tiles;
  * a config that launches one workgroup per tile has grid >= 64 and grid % 8 != 0 -- the XCD remap
    with a remainder;
and kind 14 runs its 16 x 16 tile (policy 2, and policy 0 where it picks it) and its persistent
32 x 8 form (policy 0, asserted from the query).  Data and references are §8b's integers; the
comparison is == on the decoded interior, split-fp16 planes bit for bit the encoder's, and every
word of the guarded, patterned storage outside the NaN-prefilled interior must keep its bits.  A
second call on the dirtied tensors and tickets must give the same bits.  The launch helpers hand
back the launch shape of the descriptor they launched (info=), which must be the one the case was
picked for.  test_paths_float_bound holds one float case per (precision, kind, launch form) to
exact_ref.bound; test_cob_group_walk_exact starts the co-block group walk."""
import ctypes as C

import numpy as np
import pytest
import torch

from rrin_amd import _lib
from rrin_amd.pp import H8Tensor
from tests import exact_ref as E
from tests import record_ref as R
from tests.test_gpu_block0 import block0, direct_cfg
from tests.test_gpu_h8 import NO_POOL_CFGS, conv_h8, pack_h8, replicate_ring, subpixel_upconv
from tests.test_gpu_h8_exact import all_cfgs, kind, reference, source, tensors, within, wmul
from tests.test_gpu_h8_storage import Scratch, chunk, nan_source

pytestmark = pytest.mark.gpu
X3, F16, R32 = _lib.PREC_F16X3, _lib.PREC_F16, _lib.PREC_F32R
PRECS = [R32, X3, F16]
NAME = {R32: "R32", X3: "F16X3", F16: "F16"}
LINEAR, LEAKY, POOL, REP, SUBPIXEL = (_lib.EPI_LINEAR, _lib.EPI_LEAKY, _lib.EPI_LEAKY_POOL, _lib.EPI_LEAKY_REP,
                                      _lib.EPI_SUBPIXEL)
EPI_NAME = {LINEAR: "linear", LEAKY: "leaky", POOL: "pool", REP: "rep"}
FAKE = 1 << 30        # a non-null pointer for descriptors that are only validated
# what ran: (precision, config, variant, epilogue) -> (shape, tiles, grid, extra); the coverage test reads it
RAN = {}
DONE = set()          # the test functions that ran; the coverage test is strict once all of them did
WORST = {}            # (precision, kind, variant) -> largest observed err / (2^-24 S) of the float cases
# combinations left out, each with its reason (test_paths_coverage)
EXCLUDE = {
    "pool": "configs 4 and 16 (one row per wave) reject LEAKY_POOL: RRIN_E_CONFIG",
    "sub_fold": "the ring fold exists for Winograd kind 3 alone",
    "k14_sub_cin256": "kind 14's sub-pixel conv at cin 256 leaves the 2^24 range even on +-1 data (wino_fits: 26.5 M grid "
                      "steps); cin 256 runs the four other epilogues, the sub-pixel conv cin 16 and 64",
}


# ---- the launch-shape query -------------------------------------------------------------------------
def _view(prec, h, w, channels):
    cpr = _lib.chans_per_record(prec)
    g = _lib.geom_h8(h, w)
    groups = -(-channels // (2 * cpr)) * 2
    return _lib.H8(FAKE, FAKE if prec == X3 else None, groups * g.plane, 0, groups, g)


def launch_info(prec, cfg, n, cin, cout, h, w, epi=LEAKY, mode=None, ksplit=0):
    """rrin_conv_h8_launch_info of a descriptor with this shape (validated, never dereferenced).
    SUBPIXEL: (h, w) is the low-res source, cout the up conv's; mode "fix" / "inlaunch" / "fold"."""
    d = _lib.ConvH8Desc()
    sub = epi == SUBPIXEL
    d.n, d.cin, d.cout, d.cfg, d.prec = n, cin, 4 * cout if sub else cout, cfg, prec
    d.epi_mode, d.slope, d.inv_wscale = epi, E.SLOPE, 1.0
    d.src = _view(prec, h, w, cin)
    d.dst = _view(prec, 2 * h, 2 * w, cout) if sub else _view(prec, h, w, cout)
    if epi == POOL:
        d.pool = _view(prec, h // 2, w // 2, cout)
    d.whi, d.wlo, d.bias = FAKE, FAKE if prec == X3 else None, FAKE
    if sub:
        d.edge = FAKE
    if ksplit:
        d.ksplit, d.part, d.cnt = ksplit, FAKE, FAKE
    e = _lib.EdgeFixDesc()
    if mode == "fold":
        d.ring_w = d.ring_bias = d.ring_corr = d.ring_cnt = FAKE
    elif mode == "inlaunch":
        e.n, e.cin, e.cout, e.prec, e.epi_mode, e.slope, e.full = n, cin, cout, prec, LINEAR, E.SLOPE, 1
        e.src, e.dst, e.wedge, e.bias = d.src, d.dst, FAKE, FAKE
        d.ring_full = C.addressof(e)
    out = _lib.LaunchInfo()
    _lib.check(_lib.lib().rrin_conv_h8_launch_info(C.byref(d), None, C.byref(out)), "rrin_conv_h8_launch_info")
    return out


def same_launch(real, picked, what):
    """The descriptor that was launched reports the launch shape the case was picked for."""
    a, b_ = ((i.tiles, i.grid, i.extra, i.variant) for i in (real, picked))
    assert a == b_, f"{what}: launched (tiles, grid, extra, variant) {a}, picked for {b_}"


def poison(src, off, cin):
    """+-inf beside the NaN in every group outside the view [off, off + cin) of a nan_source."""
    g0, g1 = off // src.cpr, (off + cin + src.cpr - 1) // src.cpr
    for a in src.planes():
        for g in list(range(0, g0)) + list(range(-(-g1 // 2) * 2, a.shape[1])):
            a[:, g, :, 0::3] = float("inf")
            a[:, g, :, 1::3] = float("-inf")


def can_loop(info):
    return info.grid < info.tiles


def wanted(info, loops):
    if loops:
        return info.grid < info.tiles and info.tiles % info.grid != 0 and info.tiles > 2 * info.grid
    return info.grid == info.tiles and info.grid % 8 != 0 and info.grid >= 64


def ladder_pick(prec, cfg, ladder, cin, loops=None, **kw):
    """The first ladder entry of this cin whose query reports the wanted branch; whether the config's
    grid is capped at all is read from the largest entry (loops None).  No entry: the test fails."""
    big = max(ladder, key=lambda s: s[0] * s[2] * s[3] * s[4])
    if loops is None:
        loops = can_loop(launch_info(prec, cfg, *big, **kw))
    for s in ladder:
        if s[1] != cin:
            continue
        info = launch_info(prec, cfg, *s, **kw)
        if wanted(info, loops):
            return s, info, loops
    raise AssertionError(f"{NAME[prec]} cfg {cfg} (kind {kind(cfg)}): no ladder entry gives the "
                         f"{'tile walk' if loops else 'grid % 8 != 0, >= 64'} branch")


# ---- guarded destinations, checked on the device --------------------------------------------------------
def ibits(a):
    return R.bits(a)


class Dst:
    """A tests/record_ref.GuardedH8 of c_total channels whose view [off, off + c) has a NaN interior
    and pattern everywhere else; check() compares on the device."""

    def __init__(self, n, c_total, off, c, h, w, dev, prec, seed):
        self.t = R.GuardedH8(n, c_total, h, w, dev, prec, seed=seed)
        self.off, self.c, self.prec = off, c, prec
        t = self.t
        assert off % t.cpr == 0 and c % t.cpr == 0
        self.g0, self.g1 = off // t.cpr, (off + c) // t.cpr
        numel = t.hi.numel()
        self.may, self.ring = [], []
        for a, raw in zip(t.planes(), t.raw):
            a[:, self.g0:self.g1, 1:h + 1, 8:8 + w] = float("nan")
            m = torch.zeros(raw.shape, dtype=torch.bool, device=dev)
            m[t.guard:t.guard + numel].view(a.shape)[:, self.g0:self.g1, 1:h + 1, 8:8 + w] = True
            rm = torch.zeros(raw.shape, dtype=torch.bool, device=dev)
            rv = rm[t.guard:t.guard + numel].view(a.shape)[:, self.g0:self.g1]
            rv[:, :, 0, 7:9 + w] = rv[:, :, h + 1, 7:9 + w] = True
            rv[:, :, 0:h + 2, 7] = rv[:, :, 0:h + 2, 8 + w] = True
            self.may.append(m)
            self.ring.append(rm)
        self.fill = [r.clone() for r in t.raw]

    def reset(self):
        for r, f in zip(self.t.raw, self.fill):
            r.copy_(f)

    def raw_bits(self):
        return [ibits(r).clone() for r in self.t.raw]

    def check(self, ref, what, rep=False):
        """ref: float64 numpy [n, c, h, w]."""
        t = self.t
        want = torch.from_numpy(np.ascontiguousarray(ref)).to(t.hi.device)
        got = t.to_nchw(self.off, self.c).double()
        bad = ~(got == want)
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at (image, channel, y, x) "
                                 f"{i}: got {float(got[i])!r}, exact {float(want[i])!r}")
        for p, (raw, f, m, rm) in enumerate(zip(t.raw, self.fill, self.may, self.ring)):
            changed = (ibits(raw) != ibits(f)) & ~(m | rm if rep else m)
            if bool(changed.any()):
                raise AssertionError(f"{what}: plane {p}: {int(changed.sum())} words outside the written interior changed, "
                                     f"first at flat element {int(changed.nonzero()[0])} (guard {t.guard})")
        if rep:
            for a in t.planes():
                v = a[:, self.g0:self.g1]
                assert torch.equal(ibits(v), ibits(R._replicated(v, t.h, t.w))), f"{what}: the ring is not the replicated border"
        if self.prec == X3:   # both planes are the encoder's records of the reference (rrin_nchw_to_h8 is bitwise
            enc = H8Tensor.from_nchw(want.float(), X3)   # the CPU encoder: tests/test_gpu_h8_storage.py)
            sel = (slice(None), slice(0, self.g1 - self.g0), slice(1, t.h + 1), slice(8, 8 + t.w))
            mine = (slice(None), slice(self.g0, self.g1), slice(1, t.h + 1), slice(8, 8 + t.w))
            assert torch.equal(ibits(t.hi[mine]), ibits(enc.hi[sel])), f"{what}: hi plane is not the encoder's"
            assert torch.equal(ibits(t.lo[mine]), ibits(enc.lo[sel])), f"{what}: lo plane is not the encoder's"


def case(prec, shape, mags):
    n, cin, cout, h, w = shape
    split = prec == X3
    x, wt, b, ox, ow = E.split_case(n, cin, cout, h, w, mags) if split else E.int_case(n, cin, cout, h, w, mags)
    return split, x, wt, b, ox, ow


def mags_for(cfg, wt_of, cin, den=1):
    """+-1 / +-2; +-1 alone where a Winograd form would leave the 2^24 range (exact_ref.wino_fits)."""
    if kind(cfg) <= 0:
        return (1, 2)
    k = 14 if kind(cfg) == 14 else 1
    return (1, 2) if E.wino_fits(k, wmul(cfg) * wt_of((1, 2)), den, cin, 2)[0] else (1,)


def record(prec, cfg, variant, epi, shape, info):
    RAN[(prec, cfg, variant, epi)] = (shape, info.tiles, info.grid, info.extra)
    print(f"LAUNCH_PATH {NAME[prec]} cfg {cfg} kind {kind(cfg)} variant {variant} {epi}: shape {shape} tiles {info.tiles} "
          f"grid {info.grid} extra {info.extra}")


def run_plain(gpu, prec, cfg, epi, shape, info, variant=0, ksplit=0, cache=None, mags=None):
    """One config at one shape and epilogue: exact values, whole storage, and the same bits again
    on the dirtied destination.  cache: a dict that keeps the source and the destinations of a
    shape across the configs of one test."""
    n, cin, cout, h, w = shape
    if mags is None:
        mags = (1,) if epi == POOL else mags_for(cfg, lambda m: E.int_case(n, cin, cout, h, w, m)[1], cin)
    cache = {} if cache is None else cache
    key = (shape, mags)
    if key not in cache:
        cache.clear()       # one shape's tensors at a time
        split, x, wt, b, ox, ow = case(prec, shape, mags)
        ck = chunk(prec)
        cache[key] = (split, x, wt, b, ox, ow, source(x.astype(np.float64) + (ox / E.LO if split else 0.0), prec, gpu),
                      Dst(n, cout + 2 * ck, ck, cout, h, w, gpu, prec, 51),
                      Dst(n, 2 * cout, cout, cout, h // 2, w // 2, gpu, prec, 52) if epi == POOL else None)
    split, x, wt, b, ox, ow, src, dst, pool = cache[key]
    dst.reset()
    if pool:
        pool.reset()
    mul = wmul(cfg)
    if kind(cfg) > 0:
        assert E.wino_fits(14 if kind(cfg) == 14 else 1, mul * wt, 1, cin, max(mags))[0]
    wt_t, b_t = tensors(wt, b, ow, prec, mul)
    packed = pack_h8(wt_t, b_t, cfg, prec, gpu)
    ref, refp = reference(n, cin, cout, h, w, mags, split, mul, epi)
    what = f"{NAME[prec]} {EPI_NAME[epi]} {shape} cfg {cfg} (kind {kind(cfg)}) tiles {info.tiles} grid {info.grid}"
    sc = Scratch()
    first = None
    for rnd in range(2):
        real = _lib.LaunchInfo()
        conv_h8(src, wt_t, b_t, cfg, prec, epi=epi, dst=dst.t, dst_off=dst.off, pool=pool.t if pool else None,
                pool_off=pool.off if pool else 0, packed=packed, slope=E.SLOPE, ksplit=ksplit, alloc=sc, info=real)
        same_launch(real, info, what)
        dst.check(ref, f"{what} call {rnd}", rep=epi == REP)
        if pool:
            pool.check(refp, f"{what} pool call {rnd}")
        sc.check(what)
        bits = dst.raw_bits() + (pool.raw_bits() if pool else [])
        if first is None:
            first = bits
        else:
            assert all(torch.equal(a, b_) for a, b_ in zip(first, bits)), f"{what}: the second call differs"
    record(prec, cfg, variant, EPI_NAME[epi] + (f"_k{ksplit}" if ksplit else ""), shape, info)


def pool_shape(s):
    """(h + 1, w + 1): even sizes with the tile counts of the odd ladder entry."""
    return s[:3] + (s[3] + 1, s[4] + 1)


# ---- (a) the multi-tile walk, every config of every kind -----------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("epi", [LINEAR, LEAKY, REP, POOL])
def test_walk_exact(gpu, prec, epi):
    """Every config at cin 16 on its ladder entry: LINEAR / LEAKY / LEAKY_REP on the odd shape,
    LEAKY_POOL on (h + 1, w + 1) into the view at channel cout of a 2 cout tensor."""
    DONE.add("walk")
    ladder = [pool_shape(s) for s in E.LADDER] if epi == POOL else list(E.LADDER)
    todo = [c for c in all_cfgs(prec, 16) if not (epi == POOL and c in NO_POOL_CFGS)]
    assert todo
    picks = sorted(((ladder_pick(prec, cfg, ladder, 16, epi=epi)[:2], cfg) for cfg in todo), key=lambda p: (p[0][0], p[1]))
    cache = {}
    for (shape, info), cfg in picks:
        run_plain(gpu, prec, cfg, epi, shape, info, variant=info.variant, cache=cache)


@pytest.mark.parametrize("prec", PRECS)
def test_walk_exact_cin64(gpu, prec):
    """cin 64 (8 K chunks of 8; 4 of 16), LEAKY: one config per kind and, for the direct form, one
    per grid form (capped / one workgroup per tile)."""
    DONE.add("cin64")
    seen = set()
    big = max(E.LADDER, key=lambda s: s[0] * s[2] * s[3] * s[4])
    for cfg in all_cfgs(prec, 64):
        key = (kind(cfg), can_loop(launch_info(prec, cfg, *big)))
        if key in seen:
            continue      # the first config of each kind and grid form; no ladder entry for it fails the test
        seen.add(key)
        shape, info, loops = ladder_pick(prec, cfg, E.LADDER, 64)
        assert loops == key[1]
        run_plain(gpu, prec, cfg, LEAKY, shape, info, variant=info.variant)
        RAN[(prec, cfg, info.variant, "leaky_cin64")] = (shape, info.tiles, info.grid, info.extra)
    assert {k for k, _ in seen} == {R32: {0, 1, 3, 4, 6, 7, 14}, X3: {0}, F16: {0, 6}}[prec]
    assert (0, True) in seen and (0, False) in seen


@pytest.mark.parametrize("ksplit", [2, 3])
def test_walk_split_k(gpu, ksplit):
    """Kinds 3 and 4 with 2 and 3 K slices at cin 64 on a grid with a remainder mod 8: part / cnt
    inside guards, the tickets back at zero, the second call on them the same bits."""
    DONE.add("split_k")
    ran = []
    for cfg in [c for c in all_cfgs(R32, 64) if kind(c) in (3, 4)]:
        shape = next(s for s in E.LADDER if s[1] == 64)
        info = launch_info(R32, cfg, *shape, ksplit=ksplit)
        plain = launch_info(R32, cfg, *shape)
        assert info.tiles == ksplit * plain.tiles and info.grid == info.tiles and info.grid >= 64
        run_plain(gpu, R32, cfg, LEAKY, shape, info, ksplit=ksplit)
        ran.append(kind(cfg))
    assert sorted(ran) == [3, 4]


@pytest.mark.parametrize("prec", PRECS)
def test_walk_source_view_nan_neighbours(gpu, prec):
    """The source as a view at a channel offset with NaN and +-inf in every group beside it and NaN
    in the guard bands, on the ladder entry of one config per kind and grid form: a tile of the walk
    that read another image's or group's records would store a non-finite value."""
    DONE.add("nan_source")
    seen = set()
    for cfg in all_cfgs(prec, 16):
        shape, info, loops = ladder_pick(prec, cfg, E.LADDER, 16)
        if (kind(cfg), loops) in seen:
            continue
        seen.add((kind(cfg), loops))
        n, cin, cout, h, w = shape
        mags = mags_for(cfg, lambda m: E.int_case(n, cin, cout, h, w, m)[1], cin)
        split, x, wt, b, ox, ow = case(prec, shape, mags)
        xf = torch.from_numpy(x.astype(np.float64) + (ox / E.LO if split else 0.0)).float()
        src, off = nan_source(xf, prec, cin, gpu, False)
        poison(src, off, cin)
        mul = wmul(cfg)
        wt_t, b_t = tensors(wt, b, ow, prec, mul)
        ck = chunk(prec)
        dst = Dst(n, cout + 2 * ck, ck, cout, h, w, gpu, prec, 53)
        real = _lib.LaunchInfo()
        conv_h8(src, wt_t, b_t, cfg, prec, epi=LEAKY, dst=dst.t, dst_off=dst.off, src_off=off, slope=E.SLOPE, info=real)
        same_launch(real, info, f"nan source cfg {cfg}")
        dst.check(reference(n, cin, cout, h, w, mags, split, mul, LEAKY)[0], f"{NAME[prec]} nan source cfg {cfg} {shape}")
        record(prec, cfg, info.variant, "leaky_nan_source", shape, info)


SUB_MODES = ("fix", "inlaunch", "fold")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", SUB_MODES)
def test_walk_subpixel(gpu, prec, mode):
    """EPI_SUBPIXEL on each config's entry of exact_ref.LADDER_SUB in the three ring modes.  The
    in-launch modes must report their ring workgroups (extra > 0) wherever the tile runs the ring
    in its launch; the ring must be exact and every ticket back at zero (Scratch.check)."""
    DONE.add("sub")
    todo = [c for c in all_cfgs(prec, 32) if not (mode == "fold" and kind(c) != 3)]
    for cfg in todo:
        shape, info, _ = ladder_pick(prec, cfg, E.LADDER_SUB, 32, epi=SUBPIXEL, mode=None if mode == "fix" else mode)
        n, cin, cout, sh, sw = shape
        # ring_full runs in the launch of the tiles of 256 and 512 threads (cin a multiple of 32): the
        # direct form but its two-wave tiles, kinds 6 and 7 on fp32 records; elsewhere it is a second launch
        in_launch = mode == "fold" or (kind(cfg) in (6, 7) and prec == R32) or (kind(cfg) == 0 and cfg not in TWO_WAVE_CFGS)
        if mode == "fix" or not in_launch:
            assert info.extra == 0, (cfg, info.extra)
        else:
            assert info.extra > 0 and info.extra % 8 == 0, (cfg, info.extra)
        split, x, wt, b, ox, ow = case(prec, shape, (1,))
        mul = wmul(cfg)
        if kind(cfg) > 0:
            assert E.wino_fits(14 if kind(cfg) == 14 else 1, mul * E.subpixel_weights_int(wt), 16, cin, 1)[0]
        src = source(x.astype(np.float64) + (ox / E.LO if split else 0.0), prec, gpu)
        replicate_ring(src)
        ck = chunk(prec)
        dst = Dst(n, cout + 2 * ck, ck, cout, 2 * sh, 2 * sw, gpu, prec, 54)
        wt_t, b_t = tensors(wt, b, 0 * ow, R32, mul)
        ref, _ = reference(n, cin, cout, sh, sw, (1,), split, mul, "sub")
        if prec == F16:
            ref = E.f16_round(ref)
        what = f"{NAME[prec]} sub {mode} {shape} cfg {cfg} (kind {kind(cfg)}) tiles {info.tiles} grid {info.grid} extra {info.extra}"
        sc = Scratch()
        first = None
        for rnd in range(2):
            real = _lib.LaunchInfo()
            subpixel_upconv(src, wt_t, b_t, cfg, prec, dst=dst.t, dst_off=dst.off, fold=mode == "fold",
                            inlaunch=mode == "inlaunch", alloc=sc, edge_split=mode == "fix" and prec == R32, info=real)
            same_launch(real, info, what)
            dst.check(ref, f"{what} call {rnd}")
            sc.check(what)
            bits = dst.raw_bits()
            if first is None:
                first = bits
            else:
                assert all(torch.equal(a, b_) for a, b_ in zip(first, bits)), f"{what}: the second call differs"
        record(prec, cfg, info.variant, "sub_" + mode, shape, info)


TWO_WAVE_CFGS = (7, 17)     # the direct-form tiles of 128 threads (h8_cfg.hpp's table, NW 2)


# ---- (b), (c) kind 14's other two geometries -------------------------------------------------------------
@pytest.fixture
def geom():
    lib = _lib.lib()
    try:
        yield lib.rrin_conv_h8_set_wino42_geom
    finally:
        lib.rrin_conv_h8_set_wino42_geom(0)


def cfg14():
    lib = _lib.lib()
    return next(c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_wino(c) == 14)


EPIS5 = [LINEAR, LEAKY, REP, POOL, SUBPIXEL]


def run_k14(gpu, shape, epi, variant):
    """Kind 14 at one shape and epilogue under the policy in force; the variant is asserted."""
    cfg = cfg14()
    n, cin, cout, h, w = shape
    if epi == SUBPIXEL:   # (h, w) the low-res source, cout the up conv's (4 cout phase channels)
        info = launch_info(R32, cfg, n, cin, cout, h, w, epi=SUBPIXEL)
        assert info.variant == variant, (shape, info.variant, info.tiles, info.grid)
        split, x, wt, b, ox, ow = case(R32, (n, cin, cout, h, w), (1,))
        assert E.wino_fits(14, 48 * E.subpixel_weights_int(wt), 16, cin, 1)[0]
        src = source(x.astype(np.float64), R32, gpu)
        replicate_ring(src)
        dst = Dst(n, cout + 16, 8, cout, 2 * h, 2 * w, gpu, R32, 55)
        wt_t, b_t = tensors(wt, b, 0 * ow, R32, 48)
        ref, _ = reference(n, cin, cout, h, w, (1,), False, 48, "sub")
        sc = Scratch()
        real = _lib.LaunchInfo()
        subpixel_upconv(src, wt_t, b_t, cfg, R32, dst=dst.t, dst_off=dst.off, alloc=sc, edge_split=True, info=real)
        same_launch(real, info, f"kind 14 sub {shape}")
        dst.check(ref, f"kind 14 variant {variant} sub {shape}")
        sc.check(f"kind 14 sub {shape}")
        record(R32, cfg, variant, "sub_fix", (n, cin, cout, h, w), info)
        return
    if epi == POOL:
        h, w = h + (h & 1), w + (w & 1)
    s = (n, cin, cout, h, w)
    info = launch_info(R32, cfg, *s, epi=epi)
    assert info.variant == variant, (s, info.variant, info.tiles, info.grid)
    run_plain(gpu, R32, cfg, epi, s, info, variant=variant)
    return info


@pytest.mark.parametrize("epi", EPIS5)
def test_kind14_one_workgroup_per_tile(gpu, geom, epi):
    """Policy 3: 32 x 8 tiles, one workgroup each, on the first ladder entry with grid >= 64 and
    grid % 8 != 0 (under policy 0 the ladder's kind-14 entries are the persistent form)."""
    DONE.add("k14_v0")
    geom(3)
    if epi == SUBPIXEL:
        shape, _, _ = ladder_pick(R32, cfg14(), E.LADDER_SUB, 32, loops=False, epi=SUBPIXEL)
    else:
        shape, _, _ = ladder_pick(R32, cfg14(), [pool_shape(s) for s in E.LADDER] if epi == POOL else E.LADDER, 16,
                                  loops=False, epi=epi)
    run_k14(gpu, shape, epi, 0)


@pytest.mark.parametrize("epi", EPIS5)
def test_kind14_tall_tile_exact(gpu, geom, epi):
    """Policy 2: the 16 x 16 tile at the exact suites' small shapes (ragged in both directions at
    17 x 33 and 18 x 34), cin 16, 64 and 256, every epilogue."""
    DONE.add("k14_tall")
    geom(2)
    for shape in E.K14_TALL:
        if epi == SUBPIXEL and shape[1] == 256:
            continue      # EXCLUDE["k14_sub_cin256"]
        run_k14(gpu, shape, epi, 1)


@pytest.mark.parametrize("epi", EPIS5)
def test_kind14_tall_tile_chosen_by_itself(gpu, geom, epi):
    """Policy 0 at 80 x 45 with co_blocks n = 32: 576 tiles of 32 x 8 need two rounds of 512
    workgroups, 480 of 16 x 16 one, so the launcher takes the tall tile unforced."""
    DONE.add("k14_auto")
    geom(0)
    n, cin, cout, h, w = E.K14_TALL_AUTO
    if epi == SUBPIXEL:
        cout //= 4       # the same 8 co blocks from the 4 phases
    if epi == POOL:
        h += 1           # even, and still 6 rows of 32 x 8 tiles against 3 of 16 x 16
    info = launch_info(R32, cfg14(), n, cin, cout, h, w, epi=epi)
    assert (info.tiles, info.grid) == (480, 480), (info.tiles, info.grid)     # 32 x 3 x 5; 32 x 8 tiles: 32 x 3 x 6 = 576
    run_k14(gpu, (n, cin, cout, h, w), epi, 1)


@pytest.mark.parametrize("epi", EPIS5)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_kind14_persistent_exact(gpu, geom, epi, which):
    """Policy 0, the persistent 32 x 8 form (variant 2 asserted): 768 tiles on 384 workgroups, 2 x 780
    on 512 with a ragged second co block, 1131 on 512 (two, three and four tiles each); cin 8, 16, 24 (and
    64 at the first shape): the nch 1, 2, > 2 and 8-chunk prefetch branches.  The source is a view
    with NaN beyond its last image and NaN and +-inf in the groups beside it (nan_source, poison): the prefetch of the next
    tile and the dummy re-issue after the last must not let one reach an output."""
    DONE.add("k14_persist")
    geom(0)
    cfg = cfg14()
    n, cout, h, w = E.K14_PERSIST[which]
    if epi == SUBPIXEL:
        return _persist_sub(gpu, which)
    for cin in E.K14_PERSIST_CIN:
        if cin == 64 and which:
            continue
        hh, ww = (h + (h & 1), w + (w & 1)) if epi == POOL else (h, w)
        shape = (n, cin, cout, hh, ww)
        info = launch_info(R32, cfg, *shape, epi=epi)
        tiles = -(-cout // 32) * n * -(-hh // 8) * -(-ww // 32)
        assert (info.variant, info.tiles, info.grid) == (2, tiles, min(512, tiles // 2)), (shape, info.tiles, info.grid)
        # 780 tile positions x 2 co blocks at cout 40
        assert (info.tiles, info.grid) == ((768, 384), (1560, 512), (1131, 512))[which]
        mags = (1,) if epi == POOL else mags_for(cfg, lambda m: E.int_case(*shape, m)[1], cin)
        _, x, wt, b, _, ow = case(R32, shape, mags)
        src, off = nan_source(torch.from_numpy(x.astype(np.float64)).float(), R32, cin, gpu, False)
        poison(src, off, cin)
        wt_t, b_t = tensors(wt, b, ow, R32, 48)
        dst = Dst(n, cout + 16, 8, cout, hh, ww, gpu, R32, 56)
        pool = Dst(n, 2 * cout, cout, cout, hh // 2, ww // 2, gpu, R32, 57) if epi == POOL else None
        ref, refp = reference(n, cin, cout, hh, ww, mags, False, 48, epi)
        what = f"kind 14 persistent {EPI_NAME[epi]} {shape} tiles {info.tiles} grid {info.grid}"
        for rnd in range(2):      # the second call on the written destination
            real = _lib.LaunchInfo()
            conv_h8(src, wt_t, b_t, cfg, R32, epi=epi, dst=dst.t, dst_off=dst.off, pool=pool.t if pool else None,
                    pool_off=pool.off if pool else 0, src_off=off, slope=E.SLOPE, info=real)
            same_launch(real, info, what)
            dst.check(ref, f"{what} call {rnd}", rep=epi == REP)
            if pool:
                pool.check(refp, f"{what} pool call {rnd}")
        record(R32, cfg, 2, EPI_NAME[epi] + f"_cin{cin}", shape, info)
        RAN[(R32, cfg, 2, EPI_NAME[epi])] = (shape, info.tiles, info.grid, info.extra)


def _persist_sub(gpu, which):
    """SUBPIXEL on the persistent form: the low-res source of half the size, 4 x the co blocks."""
    shape = E.K14_PERSIST_SUB[which]
    info = launch_info(R32, cfg14(), *shape, epi=SUBPIXEL)
    assert info.variant == 2 and info.grid == min(512, info.tiles // 2), (info.tiles, info.grid)
    run_k14(gpu, shape, SUBPIXEL, 2)


# ---- (d) the fused level-0 block -----------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,h,w", E.BLOCK0_PATHS)
def test_block0_paths_exact(gpu, n, cin, h, w):
    """rrin_conv_block0_h8_fwd with a grid that leaves a remainder mod 8 (the XCD split q, r of its
    block-id remap).  The launcher always starts one workgroup per tile (its query reports grid ==
    tiles at every shape: the kernel's walk never takes a second tile), so grid < tiles cannot be
    had; the condition is grid % 8 != 0 with more than 8 tiles.  test_block0_exact's check: bit for
    bit np.float16(exact); the even shape pooled."""
    DONE.add("block0")
    pooled = h % 2 == 0
    d = _lib.Block0Desc()
    d.n, d.cin, d.cfg_a, d.cfg_b, d.slope = n, cin, direct_cfg(cin, 32), direct_cfg(32, 32), E.SLOPE
    d.inv_wscale_a = d.inv_wscale_b = 1.0
    d.src, d.dst = _view(F16, h, w, cin), _view(F16, h, w, 32)
    if pooled:
        d.pool = _view(F16, h // 2, w // 2, 32)
    d.whi_a = d.bias_a = d.whi_b = d.bias_b = FAKE
    info = _lib.LaunchInfo()
    _lib.check(_lib.lib().rrin_conv_block0_h8_launch_info(C.byref(d), None, C.byref(info)))
    assert info.grid == info.tiles == n * -(-h // 8) * -(-w // 62) and info.grid % 8 != 0 and info.grid > 8
    x, wa, ba, wb, bb = E.block0_case(n, cin, h, w)
    mid, out = E.block0_ref(x, wa, ba, wb, bb)
    assert E.f16_exact(mid.f64()) and E.f16_exact(out.f64())
    ca = 16 if cin < 16 else cin
    xa = np.zeros((n, ca, h, w))
    xa[:, :cin] = x
    src = source(xa, F16, gpu)
    t = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    dst = Dst(n, 64, 16, 32, h, w, gpu, F16, 58)
    pl = Dst(n, 64, 32, 32, h // 2, w // 2, gpu, F16, 59) if pooled else None
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    block0(src, cin, t(wa), t(ba), d.cfg_a, t(wb), t(bb), d.cfg_b, pooled, dst=dst.t, dst_off=dst.off, status=status,
           slope=E.SLOPE, pl=pl.t if pl else None, pool_off=pl.off if pl else 0)
    assert int(status.item()) == 0
    dst.check(out.f64(), f"block0 cin {cin} {h}x{w} grid {info.grid}")
    if pooled:
        pl.check(E.f16_round(E.pool(out).f64()), f"block0 cin {cin} {h}x{w} pool")
    RAN[(F16, "block0", 0, "pool" if pooled else "leaky")] = ((n, cin, 32, h, w), info.tiles, info.grid, 0)
    print(f"LAUNCH_PATH block0 cin {cin} {h}x{w}: tiles {info.tiles} grid {info.grid}")


# ---- the co-block group walk -------------------------------------------------------------------------------
COB_BUDGET = 2048 * 1024        # RRIN_WINO*_UGROUP_KB: U of a co-block group within 2 MB (an XCD's L2 share)


def cob_group(co_blocks, per_cob):
    """wino_cob_group (wino_tile.hpp) restated: 0 while U of all co blocks fits the budget, else the
    largest power of two of co blocks (below the count) whose U fits."""
    if co_blocks * per_cob <= COB_BUDGET:
        return 0
    g = 1
    while 2 * g < co_blocks and 2 * g * per_cob <= COB_BUDGET:
        g *= 2
    return g


def u_bytes_per_cob(k, prec, cin):
    """U of one co block, as each launcher states it: 16 KB per 8-channel chunk for the BM 32 tiles of
    kinds 3, 4 and 7, 32 KB for kind 6's BM 64 (fp16: per 16-channel chunk), 24 KB for kind 14."""
    if k == 14:
        return cin // 8 * 1536 * 16
    if k == 6:
        return (cin // 16 if prec == F16 else cin // 8) * 32 * 64 * 16
    return cin // 8 * 1024 * 16


@pytest.mark.parametrize("prec", [R32, F16])
def test_cob_group_walk_exact(gpu, prec):
    """cin 256 at 17 x 65, three images: U of all co blocks passes 2 MB, so kinds 3, 4, 6, 7 and 14
    walk their tiles in co-block groups (wino_tile_pos) -- with a short last group: 5 co blocks in
    groups of 4 (kinds 3, 4, 7) or 2 (kind 14), 3 in groups of 2 (kind 6); fp16 kind 6 at cout 320.
    Kind 1 has no groups.  == and whole storage, twice."""
    DONE.add("cob")
    ran = {}
    for cfg in all_cfgs(prec, 256):
        k = kind(cfg)
        if k in (0, 1) or k in ran:
            continue
        shape = E.COB_SHAPE_F16 if prec == F16 else E.COB_SHAPE
        cob = -(-shape[2] // _lib.lib().rrin_conv_h8_cfg_bm(cfg))
        g = cob_group(cob, u_bytes_per_cob(k, prec, shape[1]))
        assert g > 0 and cob % g != 0, (k, cob, g)
        info = launch_info(prec, cfg, *shape)
        assert info.grid == info.tiles
        run_plain(gpu, prec, cfg, LEAKY, shape, info, variant=info.variant, mags=(1,))   # +-1: fp16 numbers at K = 2304
        RAN[(prec, cfg, info.variant, "leaky_cob_group")] = (shape, info.tiles, info.grid, g)
        ran[k] = g
    assert ran == ({3: 4, 4: 4, 6: 2, 7: 4, 14: 2} if prec == R32 else {6: 4}), ran


# ---- (e) floats -----------------------------------------------------------------------------------------
def run_float(gpu, prec, cfg, shape, info, variant):
    """LEAKY on exact_ref.float_case at one shape: |got - float64| within exact_ref.bound per element --
    (K + 2) u S for the direct form, 4 x exact_ref.wino_ratio for the Winograd kinds."""
    n, cin, cout, h, w = shape
    name, k = NAME[prec], kind(cfg)
    x, wt, b = E.float_case(n, cin, cout, h, w, name)
    s = E.s_of(x, wt, b)
    ref = E.leaky64(E.conv64(x, wt, b))
    ratio = E.wino_ratio(n, cin, cout, h, w, name, 14 if k == 14 else 1) if k else None
    bnd = E.bound(name, 9 * cin, s, ref, ratio)
    src = source(x, prec, gpu)
    dst = H8Tensor(n, cout, h, w, gpu, prec)
    for a in (dst.hi, dst.lo):
        if a is not None:
            a[:, :, 1:h + 1, 8:8 + w] = float("nan")
    real = _lib.LaunchInfo()
    conv_h8(src, torch.from_numpy(wt).float(), torch.from_numpy(b).float(), cfg, prec, epi=LEAKY, dst=dst, slope=E.SLOPE,
            info=real)
    what = f"{name} float {shape} cfg {cfg} (kind {k}) variant {variant} tiles {info.tiles} grid {info.grid}"
    same_launch(real, info, what)
    r = within(dst.to_nchw(0, cout).cpu().double().numpy(), ref, bnd, s, what)
    key = (name, k, variant if k == 14 else ("walk" if info.grid < info.tiles else "tile"))
    WORST[key] = max(WORST.get(key, 0.0), r)
    print(f"PATH_WORST {name} kind {k} variant {key[2]} {shape}: err / (2^-24 S) <= {r:.2f}")
    RAN[(prec, cfg, variant, "float")] = (shape, info.tiles, info.grid, info.extra)


@pytest.mark.parametrize("prec", PRECS)
def test_paths_float_bound(gpu, geom, prec):
    """One float case per (kind, launch form) at its smallest qualifying ladder shape: the first config
    of each kind with a one-workgroup-per-tile grid (grid >= 64, grid % 8 != 0) and the first with a
    capped grid (the unequal walk); kind 14 apart -- one workgroup per 32 x 8 tile (policy 3), the
    16 x 16 tile at 17 x 33 (policy 2), the persistent form at its smallest shape, cin 8 (policy 0)."""
    DONE.add("float")
    geom(0)
    seen = set()
    big = max(E.LADDER, key=lambda s: s[0] * s[2] * s[3] * s[4])
    for cfg in all_cfgs(prec, 16):
        key = (kind(cfg), can_loop(launch_info(prec, cfg, *big)))
        if kind(cfg) == 14 or key in seen:
            continue
        seen.add(key)
        shape, info, _ = ladder_pick(prec, cfg, E.LADDER, 16)
        run_float(gpu, prec, cfg, shape, info, info.variant)
    assert {k for k, _ in seen} == {R32: {0, 1, 3, 4, 6, 7}, X3: {0}, F16: {0, 6}}[prec]
    assert (0, True) in seen and (0, False) in seen
    if prec != R32:
        return
    c14 = cfg14()
    n, cout, h, w = E.K14_PERSIST[0]
    for policy, variant, shape in ((3, 0, None), (2, 1, E.K14_TALL[3]), (0, 2, (n, 8, cout, h, w))):
        geom(policy)
        if shape is None:
            shape, info, _ = ladder_pick(R32, c14, E.LADDER, 16, loops=False)
        else:
            info = launch_info(R32, c14, *shape)
        assert info.variant == variant
        run_float(gpu, R32, c14, shape, info, variant)


# ---- (f) coverage ----------------------------------------------------------------------------------------
def test_paths_coverage():
    """What ran (where the tests above ran in this session) is every combination the library offers:
    per precision every config x {linear, leaky, rep, pool, sub_fix, sub_inlaunch, sub_fold} minus
    EXCLUDE, and the 15 kind-14 instantiations: five epilogues x {32 x 8, 16 x 16, persistent}."""
    lib = _lib.lib()
    assert set(EXCLUDE) == {"pool", "sub_fold", "k14_sub_cin256"}
    if not RAN:
        return
    strict = DONE >= {"walk", "cin64", "split_k", "nan_source", "sub", "k14_v0", "k14_tall", "k14_auto", "k14_persist",
                      "block0", "cob", "float"}     # the whole file ran: nothing may be missing
    for prec in PRECS:
        offered = {c for c in range(lib.rrin_conv_h8_cfg_count()) if lib.rrin_conv_h8_cfg_ok(c, prec) and kind(c) >= 0}
        assert set(all_cfgs(prec, 16)) == offered
        plan = {name: offered for name in ("linear", "leaky", "rep", "sub_fix", "sub_inlaunch")}
        plan["pool"] = offered - set(NO_POOL_CFGS)
        plan["sub_fold"] = {c for c in offered if kind(c) == 3}
        for name, want in plan.items():
            got = {c for (p, c, _, e) in RAN if p == prec and e == name}
            if got or (strict and want):
                assert got >= want, (NAME[prec], name, sorted(want - got))
            print(f"{NAME[prec]} {name}: configs {sorted(want)}")
    c14 = cfg14()
    k14 = {(v, e) for (p, c, v, e) in RAN if p == R32 and c == c14 and e in ("linear", "leaky", "rep", "pool", "sub_fix")}
    if strict or any(v for v, _ in k14):
        want = {(v, e) for v in (0, 1, 2) for e in ("linear", "leaky", "rep", "pool", "sub_fix")}
        assert k14 == want, sorted(want - k14)
    if strict:
        eps = {e for (_, _, _, e) in RAN}
        assert {"leaky_k2", "leaky_k3", "leaky_nan_source", "leaky_cin64", "leaky_cob_group", "float"} <= eps, eps
        assert {e for (p, c, _, e) in RAN if c == "block0"} == {"leaky", "pool"}
        for cin in E.K14_PERSIST_CIN:      # the nch 1, 2, > 2 and 8-chunk prefetch branches of the persistent form
            assert {e for (_, _, v, e) in RAN if v == 2 and e.endswith(f"_cin{cin}")} == {f"{e}_cin{cin}" for e in EPI_NAME.values()}
        for prec in PRECS:                 # both grid forms of the direct configs, exact and float
            for e in ("leaky", "float"):
                forms = {RAN[k][2] < RAN[k][1] for k in RAN if k[0] == prec and k[3] == e and isinstance(k[1], int) and kind(k[1]) == 0}
                assert forms == {True, False}, (NAME[prec], e, forms)
        assert {k[:3] for k in WORST} >= {("R32", 14, 0), ("R32", 14, 1), ("R32", 14, 2), ("R32", 0, "walk"), ("F16X3", 0, "walk"),
                                          ("F16", 0, "walk"), ("F16", 6, "tile")}
    for key, val in sorted(RAN.items(), key=str):
        print("RAN", key, val)
