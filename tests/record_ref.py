"""CPU side of the whole-storage tests of the record layout (include/rrin_hip.h): an encoder that
is independent of the library (``nchw_to_records``, the inverse of glue_ref.records_to_nchw, from
glue_ref.record_geom and glue_ref.split16 alone), storage with guard bands (``GuardedH8``,
``GuardedFlat``) and ``check_storage``, which compares the *raw* storage after a call -- both
planes, the padding on all four sides, the groups outside the view, the guard bands -- with a
snapshot taken before it and a float64 reference of the view's interior.

No torch.cuda call and no library call happens at import or in the codec and the checker, so
tests/test_record_ref.py runs them without a GPU; ``GuardedH8`` needs the library's geometry
query only (host code)."""
from dataclasses import dataclass

import torch

from tests import glue_ref as G

CPR = {"R32": 4, "F16X3": 8, "F16": 8}
DTYPE = {"R32": torch.float32, "F16X3": torch.float16, "F16": torch.float16}


def nchw_to_records(x, prec, groups, ch_off):
    """(hi, lo) raw record storage [n, groups, hp, wp, cpr] holding the channels of the NCHW
    tensor x at [ch_off, ch_off + c), everything else zero; lo is None unless prec is F16X3.
    R32 stores the fp32 value, F16 f16(v), F16X3 the two halves of glue_ref.split16."""
    n, c, h, w = x.shape
    cpr = CPR[prec]
    assert ch_off >= 0 and ch_off + c <= groups * cpr
    hp, wp = G.record_geom(h, w)
    v = x.float()
    hi = torch.zeros(n, groups, hp, wp, cpr, dtype=DTYPE[prec])
    lo = torch.zeros_like(hi) if prec == "F16X3" else None
    if prec == "R32":
        a, b = v, None
    else:
        a, b = G.split16(v)
    for k in range(c):
        ch = ch_off + k
        hi[:, ch // cpr, 1:h + 1, 8:8 + w, ch % cpr] = a[:, k]
        if lo is not None:
            lo[:, ch // cpr, 1:h + 1, 8:8 + w, ch % cpr] = b[:, k]
    return hi, lo


def bits(a):
    """The storage as integers of its own width: comparisons that see -0.0 and NaN payloads."""
    return a.view({torch.float32: torch.int32, torch.float16: torch.int16, torch.int32: torch.int32}[a.dtype])


def fill(raw, seed, nan=False):
    """Prefill raw storage: glue_ref.pattern (finite, non-zero), or NaN where reads must show."""
    if nan:
        raw.fill_(float("nan"))
    else:
        raw.copy_(G.pattern(raw.shape, seed, raw.dtype))


class GuardedFlat:
    """A flat scratch array (fp32 or int32: edge, part, ring_corr, the ticket arrays, status) as a
    slice ``t`` of a larger allocation ``raw`` with ``guard`` elements before and after it."""

    def __init__(self, numel, dtype, device, guard=64, seed=1, nan=False, zero=False):
        self.guard, self.numel = guard, numel
        self.raw = torch.empty(numel + 2 * guard, dtype=dtype, device=device)
        if dtype == torch.int32:
            self.raw.copy_(torch.arange(1, self.raw.numel() + 1, dtype=torch.int32) * 7919)
        else:
            fill(self.raw, seed, nan)
        self.t = self.raw[guard:guard + numel]
        if zero or dtype == torch.int32:
            self.t.zero_()

    def data_ptr(self):
        return self.t.data_ptr()

    def snapshot(self):
        return self.raw.detach().cpu().clone()

    def check_guards(self, before, what):
        after = self.raw.detach().cpu()
        g = self.guard
        for name, sl in (("leading", slice(0, g)), ("trailing", slice(g + self.numel, None))):
            bad = bits(after[sl]) != bits(before[sl])
            assert not bool(bad.any()), f"{what}: {name} guard band changed at element {int(bad.nonzero()[0])}"


@dataclass
class StorageView:
    """What check_storage needs to know of raw storage: the allocation ([n, groups, hp, wp, cpr]
    behind ``guard`` leading elements of each flat plane) and the channels [ch_off, ch_off + c)
    the call may write."""
    n: int
    groups: int
    cpr: int
    guard: int
    ch_off: int
    c: int


class GuardedH8:
    """An rrin_amd.pp.H8Tensor look-alike whose ``hi`` / ``lo`` are slices of larger flat
    allocations (``raw``): ``guard_rows`` plane rows (wp records each) before and after the
    tensor.  Everything is prefilled with glue_ref.pattern, or with NaN; ``zero_padding`` zeroes
    the padding of every plane (a conv's source: the padding is its zero padding).  ``view`` and
    ``chunk_view`` are H8Tensor's, on data_ptr() of the slices."""

    def __init__(self, n, c, h, w, device, prec, seed=1, nan=False, guard_rows=2):
        from rrin_amd import _lib
        from rrin_amd.pp import H8Tensor
        self._cls = H8Tensor
        self.n, self.c, self.h, self.w, self.prec = n, c, h, w, prec
        self.g = _lib.geom_h8(h, w)
        assert (self.g.hp, self.g.wp) == G.record_geom(h, w)
        self.cpr = _lib.chans_per_record(prec)
        self.groups = (c + 2 * self.cpr - 1) // (2 * self.cpr) * 2
        shape = (n, self.groups, self.g.hp, self.g.wp, self.cpr)
        numel = n * self.groups * self.g.hp * self.g.wp * self.cpr
        self.guard = guard_rows * self.g.wp * self.cpr
        dt = torch.float32 if prec == _lib.PREC_F32R else torch.float16
        self.raw = []
        for k in range(2 if prec == _lib.PREC_F16X3 else 1):
            r = torch.empty(numel + 2 * self.guard, dtype=dt, device=device)
            fill(r, seed + 17 * k, nan)
            self.raw.append(r)
        planes = [r[self.guard:self.guard + numel].view(shape) for r in self.raw]
        self.hi = planes[0]
        self.lo = planes[1] if len(planes) == 2 else None

    def view(self, ch_off=0, channels=None):
        return self._cls.view(self, ch_off, channels)

    def chunk_view(self, ch_off=0, channels=None):
        return self._cls.chunk_view(self, ch_off, channels)

    def to_nchw(self, ch_off=0, channels=None):
        return self._cls.to_nchw(self, ch_off, channels)

    def load(self, x, ch_off=0):
        return self._cls.load(self, x, ch_off)

    def planes(self):
        return [a for a in (self.hi, self.lo) if a is not None]

    def zero_padding(self):
        for a in self.planes():
            a[:, :, 0] = 0
            a[:, :, self.h + 1:] = 0
            a[:, :, :, :8] = 0
            a[:, :, :, 8 + self.w:] = 0

    def put(self, hi, lo=None, groups=None):
        """Copy CPU records (nchw_to_records) into the record groups `groups` (a slice)."""
        groups = slice(None) if groups is None else groups
        self.hi[:, groups] = hi.to(self.hi.device)
        if self.lo is not None:
            self.lo[:, groups] = lo.to(self.lo.device)

    def snapshot(self):
        return [r.detach().cpu().clone() for r in self.raw]

    def storage(self, ch_off=0, channels=None):
        channels = self.c - ch_off if channels is None else channels
        return StorageView(self.n, self.groups, self.cpr, self.guard, ch_off, channels)


def replicate_ring_mask(shape, h, w):
    """The padding elements EPI_LEAKY_REP writes (replicate_ring of tests/test_gpu_h8.py): row 0 and
    row h + 1 over columns 7 .. 8 + w, columns 7 and 8 + w over rows 0 .. h + 1."""
    m = torch.zeros(shape, dtype=torch.bool)
    m[:, :, 0, 7:9 + w] = True
    m[:, :, h + 1, 7:9 + w] = True
    m[:, :, 0:h + 2, 7] = True
    m[:, :, 0:h + 2, 8 + w] = True
    return m


def _replicated(a, h, w):
    """a with its ring overwritten by the replicated border, in replicate_ring's order."""
    a = a.clone()
    a[:, :, 0, 8:8 + w] = a[:, :, 1, 8:8 + w]
    a[:, :, h + 1, 8:8 + w] = a[:, :, h, 8:8 + w]
    a[:, :, 0:h + 2, 7] = a[:, :, 0:h + 2, 8]
    a[:, :, 0:h + 2, 8 + w] = a[:, :, 0:h + 2, 7 + w]
    return a


def _where(idx, plane):
    i, g, y, x, e = (int(v) for v in idx)
    return f"plane {('hi', 'lo')[plane]}, image {i}, group {g}, record row {y}, column {x}, element {e}"


def _f16_neighbours(hi):
    """The fp16 values next to hi on both sides (by magnitude bits; zero: the smallest subnormals)."""
    b = hi.view(torch.int16).to(torch.int32) & 0xFFFF
    sign, mag = b & 0x8000, b & 0x7FFF

    def half(u):  # 16 bits held in an int32 -> fp16
        return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16).view(torch.float16)

    up = half(sign | (mag + 1).clamp(max=0x7C00))
    down = half(torch.where(mag > 0, sign | (mag - 1), (sign ^ 0x8000) | 1))
    return up, down


def check_storage(before, after, view, h, w, expect_nchw, tol, ring=None, what="storage", interior_mask=None):
    """before / after: the raw flat planes ([hi] or [hi, lo], guard bands included, CPU) around a
    call that may write the interior pixels of view's channels; expect_nchw: float64 [n, c, h, w].

    * the interior of the view's channels, decoded with glue_ref.records_to_nchw, is within
      tol (rtol, atol: |got - ref| <= atol + rtol |ref|) of expect_nchw; F16X3 through the join of
      both planes, and hi must be a nearest fp16 of that join -- the pairs glue_ref.split16 makes
      (its lo is at most half an ulp of hi; a tie may have gone either way);
    * every other element is bitwise what it was: the padding on all four sides, the groups
      outside the view, both guard bands, in both planes;
    * ring="replicate": the one-pixel ring around the interior of the view's channels must equal
      the replicated border (replicate_ring of tests/test_gpu_h8.py), nothing else in the padding
      may change;
    * interior_mask (bool [h, w], optional): only these interior pixels may change and are
      compared (the ring fix-up); the other interior pixels must keep their bits too.

    The message of a failure names plane, image, group, record row and column of the first
    offending element."""
    hp, wp = G.record_geom(h, w)
    shape = (view.n, view.groups, hp, wp, view.cpr)
    numel = view.n * view.groups * hp * wp * view.cpr
    assert len(before) == len(after)
    for b, a in zip(before, after):
        assert b.shape == a.shape == (numel + 2 * view.guard,), (b.shape, a.shape, numel, view.guard)
    may = torch.zeros(shape, dtype=torch.bool)
    chans = range(view.ch_off, view.ch_off + view.c)
    for ch in chans:
        if interior_mask is None:
            may[:, ch // view.cpr, 1:h + 1, 8:8 + w, ch % view.cpr] = True
        else:
            may[:, ch // view.cpr, 1:h + 1, 8:8 + w, ch % view.cpr] = interior_mask
    ringm = None
    if ring is not None:
        assert ring == "replicate", ring
        chm = torch.zeros(shape, dtype=torch.bool)
        for ch in chans:
            chm[:, ch // view.cpr, :, :, ch % view.cpr] = True
        ringm = replicate_ring_mask(shape, h, w) & chm
    g = view.guard
    planes = []
    for p, (b, a) in enumerate(zip(before, after)):
        for name, sl in (("leading", slice(0, g)), ("trailing", slice(g + numel, None))):
            bad = bits(a[sl]) != bits(b[sl])
            assert not bool(bad.any()), (f"{what}: plane {('hi', 'lo')[p]}: the {name} guard band changed, first at "
                                         f"element {int(bad.nonzero()[0])} of {int(bad.numel())}")
        a5, b5 = a[g:g + numel].view(shape), b[g:g + numel].view(shape)
        fixed = ~may if ringm is None else ~(may | ringm)
        bad = (bits(a5) != bits(b5)) & fixed
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements outside the view's interior changed, first: "
                                     f"{_where(bad.nonzero()[0], p)}")
        if ringm is not None:
            bad = (bits(a5) != bits(_replicated(a5, h, w))) & ringm
            assert not bool(bad.any()), (f"{what}: the ring is not the replicated border, first: "
                                         f"{_where(bad.nonzero()[0], p)}")
        planes.append(a5)
    hi, lo = planes[0], planes[1] if len(planes) == 2 else None
    got = G.records_to_nchw(hi, lo, view.ch_off, view.c, h, w).double()
    ref = expect_nchw.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    lim = tol["atol"] + tol["rtol"] * ref.abs()
    bad = ~(err <= lim)  # NaN fails
    if interior_mask is not None:
        bad &= interior_mask
    if bool(bad.any()):
        i, k, y, x = (int(v) for v in bad.nonzero()[0])
        ch = view.ch_off + k
        raise AssertionError(f"{what}: {int(bad.sum())} interior values past the tolerance, first: image {i}, group "
                             f"{ch // view.cpr}, record row {y + 1}, column {x + 8}, element {ch % view.cpr}: got "
                             f"{float(got[i, k, y, x])!r}, reference {float(ref[i, k, y, x])!r}")
    if lo is not None:
        for k, ch in enumerate(chans):
            sel = (slice(None), ch // view.cpr, slice(1, h + 1), slice(8, 8 + w), ch % view.cpr)
            hh, ll = hi[sel], lo[sel]
            v = hh.double() + ll.double() / G.LO_SCALE
            up, down = _f16_neighbours(hh)
            d0 = (v - hh.double()).abs()
            bad = (d0 > (v - up.double()).abs()) | (d0 > (v - down.double()).abs())
            if interior_mask is not None:
                bad &= interior_mask
            if bool(bad.any()):
                i, y, x = (int(t) for t in bad.nonzero()[0])
                raise AssertionError(f"{what}: lo is not the split16 partner of hi, first: plane lo, image {i}, group "
                                     f"{ch // view.cpr}, record row {y + 1}, column {x + 8}, element {ch % view.cpr}")
