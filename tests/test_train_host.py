"""CPU: argument validation of the training entry points (csrc/train.hip, rrin_t*).  Every case
here is rejected before the entry makes any HIP call, so nothing is launched and the pointers
(one small host buffer) are never dereferenced."""
import ctypes as C

import pytest

from rrin_amd import _lib

E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3

_BUF = (C.c_float * 16)()
P = C.addressof(_BUF)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _tconv(**kw):
    d = _lib.TConvDesc(n=1, cin=2, cout=3, h=4, w=5, mode=_lib.TCONV_FWD, leaky=0, slope=0.1, x=P, y=None, wt=P,
                       bias=None, out=P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _twgrad(**kw):
    d = _lib.TWgradDesc(n=1, cin=2, cout=3, h=4, w=5, leaky=0, slope=0.1, x=P, g=P, y=None, gw=P, gb=P, work=P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_tconv3x3_rejects(lib):
    f = lambda **kw: lib.rrin_tconv3x3(C.byref(_tconv(**kw)), None)
    assert lib.rrin_tconv3x3(None, None) == E_ARG
    for k in ("x", "wt", "out"):
        assert f(**{k: None}) == E_ARG, k
    for k in ("n", "cin", "cout", "h", "w"):
        assert f(**{k: 0}) == E_ARG and f(**{k: -1}) == E_ARG, k
    for slope in (0.0, -0.1, 1.5, float("nan")):
        assert f(leaky=1, slope=slope) == E_ARG, slope
        assert f(mode=_lib.TCONV_DGRAD, leaky=1, y=P, slope=slope) == E_ARG, slope
    assert f(mode=_lib.TCONV_DGRAD, leaky=1, y=None) == E_ARG
    for mode in (2, 3, -1):     # 2: the weight gradient is rrin_tconv3x3_wgrad, not a mode of this entry
        assert f(mode=mode) == E_ARG, mode
    # h w > 2^31 - 1: the pixel index of a plane is an int
    assert f(h=65536, w=32768) == E_SHAPE
    assert f(h=1, w=2 ** 31 - 1, mode=7) == E_ARG    # the largest h w passes the shape check


def test_tconv3x3_wgrad_rejects(lib):
    f = lambda **kw: lib.rrin_tconv3x3_wgrad(C.byref(_twgrad(**kw)), None)
    assert lib.rrin_tconv3x3_wgrad(None, None) == E_ARG
    for k in ("x", "g", "gw", "work"):
        assert f(**{k: None}) == E_ARG, k
    assert f(leaky=1, y=None) == E_ARG
    for k in ("n", "cin", "cout", "h", "w"):
        assert f(**{k: 0}) == E_ARG and f(**{k: -3}) == E_ARG, k
    for slope in (0.0, -1.0, 1.0001):
        assert f(leaky=1, y=P, slope=slope) == E_ARG, slope


def _slices(n, cin, cout, h):
    """twgrad_slices: whole rows per slice so that about 1024 tile workgroups run."""
    ct = 2 if cout % 64 == 0 else 1
    per = ((cin + 31) // 32) * ((cout + 32 * ct - 1) // (32 * ct))
    rows = n * h
    sl = max(1, min(rows, (1024 + per - 1) // per))
    rps = (rows + sl - 1) // sl
    return rps, (rows + rps - 1) // rps


@pytest.mark.parametrize("shape,rps,slices", [
    ((1, 65, 96, 151, 5), 2, 76),      # 9 tile workgroups -> 114 wanted, 2 rows each, the last slice 1 row
    ((3, 65, 96, 50, 8), 2, 75),       # 75 full slices across the image boundaries
    ((1, 1, 1, 1, 1), 1, 1),
    ((2, 16, 128, 6, 12), 1, 12),      # CT = 2: one slice per row
    ((2, 512, 512, 40, 7), 10, 8),     # 128 tile workgroups -> 8 slices of 10 rows
    ((1, 32, 64, 1500, 3), 2, 750),    # 1 tile workgroup, 1024 wanted < 1500 rows
])
def test_wgrad_work_floats(lib, shape, rps, slices):
    n, cin, cout, h, w = shape
    assert _slices(n, cin, cout, h) == (rps, slices)
    assert lib.rrin_tconv3x3_wgrad_work_floats(*shape) == slices * cout * (9 * cin + 1)


def test_wgrad_work_floats_rejects(lib):
    for i in range(5):
        for bad in (0, -1):
            a = [1, 2, 3, 4, 5]
            a[i] = bad
            assert lib.rrin_tconv3x3_wgrad_work_floats(*a) < 0, a


@pytest.mark.parametrize("name", ["rrin_tpool2_fwd", "rrin_tpool2_bwd"])
def test_tpool2_rejects(lib, name):
    f = getattr(lib, name)
    assert f(None, P, 1, 2, 2, None) == E_ARG and f(P, None, 1, 2, 2, None) == E_ARG
    for nc, h, w in ((0, 2, 2), (1, 3, 2), (1, 2, 3), (1, 1, 2), (1, 2, 1), (1, 0, 2), (1, 2, 0), (1, -2, 2),
                     (-1, 2, 2), (1, 5, 5)):
        assert f(P, P, nc, h, w, None) == E_ARG, (nc, h, w)


@pytest.mark.parametrize("name", ["rrin_tup2_fwd", "rrin_tup2_bwd"])
def test_tup2_rejects(lib, name):
    f = getattr(lib, name)
    assert f(None, P, 1, 1, 1, None) == E_ARG and f(P, None, 1, 1, 1, None) == E_ARG
    for nc, h, w in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        assert f(P, P, nc, h, w, None) == E_ARG, (nc, h, w)


def test_tpack_wino_rejects(lib):
    f = lib.rrin_tpack_wino
    assert f(None, 4, 4, 32, 0, P, None) == E_ARG and f(P, 4, 4, 32, 0, None, None) == E_ARG
    for bm in (0, 16, 33, 48, 128, -32):
        assert f(P, 4, 4, bm, 0, P, None) == E_ARG, bm
    for mode in (2, -1):
        assert f(P, 4, 4, 64, mode, P, None) == E_ARG, mode
    assert f(P, 0, 4, 32, 0, P, None) == E_ARG and f(P, 4, 0, 32, 1, P, None) == E_ARG


def test_twarp_bwd_workspace(lib):
    wb = lib.rrin_twarp_bwd_work_bytes
    assert wb(2, 3, 17, 23) == 2 * 3 * 17 * 23 * 8 + 256    # one 64-bit sum per element + the max
    assert wb(1, 1, 1, 1) == 264
    for i in range(4):
        for bad in (0, -1):
            a = [2, 3, 17, 23]
            a[i] = bad
            assert wb(*a) < 0, a
            assert lib.rrin_twarp_bwd(P, P, P, P, P, P, 1 << 40, *a, None) == E_ARG, a
    need = wb(2, 3, 17, 23)
    assert lib.rrin_twarp_bwd(P, P, P, P, P, P, need - 1, 2, 3, 17, 23, None) == E_WORKSPACE
    assert lib.rrin_twarp_bwd(P, P, P, P, P, P, 0, 2, 3, 17, 23, None) == E_WORKSPACE
    for k in range(6):
        a = [P] * 6
        a[k] = None
        assert lib.rrin_twarp_bwd(*a, need, 2, 3, 17, 23, None) == E_ARG, k
