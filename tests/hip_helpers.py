"""Test helpers: drive single kernels of librrin_hip.so through the C ABI."""
import ctypes as C

import numpy as np
import torch

from rrin_amd import _lib
from rrin_amd.pp import H8Tensor, PPTensor


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def pack(w: torch.Tensor, b: torch.Tensor, cfg: int, perm=None, dev="cuda"):
    lib = _lib.lib()
    w = w.detach().cpu().float().contiguous().numpy()
    b = b.detach().cpu().float().contiguous().numpy()
    cout, cin = w.shape[:2]
    bm = lib.rrin_conv_cfg_bm(cfg)
    wp = np.empty(lib.rrin_pack_conv3x3_floats(cout, cin, bm), np.float32)
    bp = np.empty(lib.rrin_pack_bias_floats(cout, bm), np.float32)
    pa = np.asarray(perm, np.int32) if perm is not None else None
    _lib.check(lib.rrin_pack_conv3x3(w.ctypes.data, b.ctypes.data, cout, cin, bm,
                                     pa.ctypes.data if pa is not None else None, wp.ctypes.data,
                                     bp.ctypes.data))
    return torch.from_numpy(wp).to(dev), torch.from_numpy(bp).to(dev)


def conv(src: PPTensor, w, b, cfg, *, src_off=0, dst=None, dst_off=0, upsample=False, epi=_lib.EPI_LINEAR,
         pool=None, perm=None, cin=None, slope=0.1):
    """Run rrin_conv3x3_fwd; returns (dst PPTensor, pool PPTensor or None)."""
    dev = src.t.device
    cout, cin_w = w.shape[:2]
    cin = cin or cin_w
    h, wd = (src.h * 2, src.w * 2) if upsample else (src.h, src.w)
    if dst is None:
        dst = PPTensor(src.n, cout + dst_off, h, wd, dev)
    if epi == _lib.EPI_LEAKY_POOL and pool is None:
        pool = PPTensor(src.n, cout, h // 2, wd // 2, dev)
    wp, bp = pack(w, b, cfg, perm, dev)
    d = _lib.ConvDesc()
    d.n, d.cin, d.cout, d.cfg = src.n, cin, cout, cfg
    d.src_mode = _lib.SRC_UPSAMPLE2X if upsample else _lib.SRC_DIRECT
    d.epi_mode = epi
    d.slope = slope
    d.src = src.view(src_off, cin)
    d.dst = dst.view(dst_off, cout)
    if pool is not None:
        d.pool = pool.view(0, cout)
    d.wpack, d.bias = wp.data_ptr(), bp.data_ptr()
    _lib.check(_lib.lib().rrin_conv3x3_fwd(C.byref(d), stream(dev)), "rrin_conv3x3_fwd")
    torch.cuda.synchronize(dev)
    return dst, pool


def head(src: PPTensor, g16: PPTensor, w, b, mode, coef=None, out=None, flow_raw: PPTensor = None, raw_out=None):
    dev = src.t.device
    d = _lib.HeadDesc()
    d.n, d.cin, d.cout, d.mode = src.n, 32, w.shape[0], mode
    d.src = src.view(0, 32)
    d.g16 = g16.view(0, g16.c)
    wd = w.detach().float().contiguous().to(dev)
    bd = b.detach().float().contiguous().to(dev)
    d.w, d.bias = wd.data_ptr(), bd.data_ptr()
    if coef is not None:
        d.coef = coef.data_ptr()
    if out is not None:
        d.out = out.data_ptr()
    if flow_raw is not None:
        d.flow_raw = flow_raw.view(0, 4)
    if raw_out is not None:
        d.raw_out = raw_out.data_ptr()
    _lib.check(_lib.lib().rrin_head_fwd(C.byref(d), stream(dev)), "rrin_head_fwd")
    torch.cuda.synchronize(dev)


def head_h8(src: H8Tensor, dst: H8Tensor, w, b, mode, coef=None, out=None, prec=_lib.PREC_F16X3, *,
            flow_raw: H8Tensor = None, raw_out=None, status=None, out_u8=None, crop=None, rc=False):
    """Run rrin_head_h8_fwd on the record layout.  crop = (h0, w0, top) of out_u8; rc=True
    returns the entry's code instead of raising on it."""
    dev = src.hi.device
    w_d = w.detach().float().contiguous().to(dev)
    b_d = b.detach().float().contiguous().to(dev)
    d = _lib.HeadH8Desc()
    d.n, d.cin, d.cout, d.mode, d.prec = src.n, 32, w.shape[0], mode, prec
    d.src, d.g16 = src.view(0, 32), dst.view(0, dst.c)
    d.w, d.bias = w_d.data_ptr(), b_d.data_ptr()
    d.coef = coef.data_ptr() if coef is not None else None
    d.out = out.data_ptr() if out is not None else None
    if flow_raw is not None:
        d.flow_raw = flow_raw.view(0, 4)
    d.raw_out = raw_out.data_ptr() if raw_out is not None else None
    d.status = status.data_ptr() if status is not None else None
    d.out_u8 = out_u8.data_ptr() if out_u8 is not None else None
    if crop is not None:
        d.h0, d.w0, d.top = crop
    code = _lib.lib().rrin_head_h8_fwd(C.byref(d), stream(dev))
    torch.cuda.synchronize(dev)
    if rc:
        return code
    _lib.check(code, "rrin_head_h8_fwd")


# ---- training entry points (csrc/train.hip): contiguous NCHW fp32 device tensors ----
def nans(shape, dev):
    """An output buffer no kernel has written: an element left out stays NaN and fails."""
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype in (torch.float32, torch.uint8) and t.is_contiguous()
    return t.data_ptr()


def tconv(x, wt, bias=None, *, dgrad=False, leaky=False, slope=0.1, y=None):
    """rrin_tconv3x3: FWD conv3x3(x, wt) + bias [, leaky]; dgrad: x is g [n][cout][h][w], y the
    forward output of the leaky mask."""
    cout, cin = wt.shape[:2]
    n, _, h, w = x.shape
    assert x.shape[1] == (cout if dgrad else cin)
    out = nans((n, cin if dgrad else cout, h, w), x.device)
    d = _lib.TConvDesc(n=n, cin=cin, cout=cout, h=h, w=w, mode=_lib.TCONV_DGRAD if dgrad else _lib.TCONV_FWD,
                       leaky=int(leaky), slope=slope, x=_p(x), y=_p(y), wt=_p(wt), bias=_p(bias), out=_p(out))
    _lib.check(_lib.lib().rrin_tconv3x3(C.byref(d), stream(x.device)), "rrin_tconv3x3")
    torch.cuda.synchronize(x.device)
    return out


def twgrad(x, g, *, y=None, leaky=False, slope=0.1, bias_grad=True):
    """rrin_tconv3x3_wgrad -> (gw, gb or None); the work buffer starts as NaN too."""
    n, cin, h, w = x.shape
    cout = g.shape[1]
    nw = int(_lib.lib().rrin_tconv3x3_wgrad_work_floats(n, cin, cout, h, w))
    assert nw > 0
    work = nans((nw,), x.device)
    gw = nans((cout, cin, 3, 3), x.device)
    gb = nans((cout,), x.device) if bias_grad else None
    d = _lib.TWgradDesc(n=n, cin=cin, cout=cout, h=h, w=w, leaky=int(leaky), slope=slope, x=_p(x), g=_p(g),
                        y=_p(y), gw=_p(gw), gb=_p(gb), work=_p(work))
    _lib.check(_lib.lib().rrin_tconv3x3_wgrad(C.byref(d), stream(x.device)), "rrin_tconv3x3_wgrad")
    torch.cuda.synchronize(x.device)
    return gw, gb


def tresample(name, src, out_shape):
    """rrin_tpool2_fwd / _bwd, rrin_tup2_fwd / _bwd on [nc][h][w]; h, w are the sizes of the
    entry's argument list (pool: the full size, up: the low-resolution size)."""
    big = src.shape if (src.shape[1] * src.shape[2] > out_shape[1] * out_shape[2]) else out_shape
    nc, h, w = big if "pool" in name else (big[0], big[1] // 2, big[2] // 2)
    out = nans(out_shape, src.device)
    _lib.check(getattr(_lib.lib(), name)(_p(src), _p(out), nc, h, w, stream(src.device)), name)
    torch.cuda.synchronize(src.device)
    return out


def twarp_bwd(img, flow, gout):
    """rrin_twarp_bwd -> (gimg, gflow)."""
    n, c, h, w = img.shape
    nb = int(_lib.lib().rrin_twarp_bwd_work_bytes(n, c, h, w))
    work = torch.full((nb,), 0xFF, dtype=torch.uint8, device=img.device)
    gimg, gflow = nans(img.shape, img.device), nans(flow.shape, img.device)
    _lib.check(_lib.lib().rrin_twarp_bwd(_p(img), _p(flow), _p(gout), _p(gimg), _p(gflow), _p(work), nb, n, c, h, w,
                                         stream(img.device)), "rrin_twarp_bwd")
    torch.cuda.synchronize(img.device)
    return gimg, gflow
