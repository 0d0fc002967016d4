"""ctypes binding of ``librrin_hip.so`` (C ABI declared in include/rrin_hip.h).

The library is built in-tree (``make`` or ``__graft_entry__.build()``) and
loaded from ``rrin_amd/librrin_hip.so``.  There is no fallback: if the library
is missing or its ABI version differs, ``lib()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

ABI_VERSION = 25
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "librrin_hip.so")
# A/B sessions only (tools/sessions/): another build of the same library, e.g. ab/librrin_hip_X.so
if os.environ.get("RRIN_LIB_AB"):
    LIB_PATH = os.path.abspath(os.environ["RRIN_LIB_AB"])

# enums (rrin_hip.h)
SRC_DIRECT, SRC_UPSAMPLE2X = 0, 1
EPI_LINEAR, EPI_LEAKY, EPI_LEAKY_POOL, EPI_LEAKY_REP, EPI_SUBPIXEL = 0, 1, 2, 3, 4
KIND_CONV, KIND_HEAD, KIND_LAYOUT, KIND_EDGE = 0, 1, 2, 3
HEAD_PLAIN, HEAD_FLOW, HEAD_REFINE, HEAD_MASK, HEAD_FINAL = 0, 1, 2, 3, 4
PREC_F32, PREC_F16X3, PREC_F16, PREC_F32R = 0, 1, 2, 3
# "fp32": exact fp32 on the record layout (F32R); "fp32_planar": exact fp32 on the
# planar PP layout (the first implementation, kept for A/B); "fp32_split16":
# fp32-emulated (fp16 hi+lo x3); "fp16"
PRECISIONS = {"fp32": PREC_F32R, "fp32_planar": PREC_F32, "fp32_split16": PREC_F16X3, "fp16": PREC_F16}
RECORD_PRECS = (PREC_F16X3, PREC_F16, PREC_F32R)


def chans_per_record(prec: int) -> int:
    """Channels of one 16-B record of the record layout: 4 fp32 or 8 halves."""
    return 4 if prec == PREC_F32R else 8


class Geom(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32),
                ("plane", C.c_int64)]


class PP(C.Structure):
    _fields_ = [("base", C.c_void_p), ("img_stride", C.c_int64), ("ch_off", C.c_int32),
                ("channels", C.c_int32), ("g", Geom)]


class ConvDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("cfg", C.c_int32),
                ("src_mode", C.c_int32), ("epi_mode", C.c_int32), ("slope", C.c_float),
                ("src", PP), ("dst", PP), ("pool", PP), ("wpack", C.c_void_p), ("bias", C.c_void_p)]


class HeadDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("mode", C.c_int32),
                ("src", PP), ("g16", PP), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("coef", C.c_void_p), ("out", C.c_void_p), ("flow_raw", PP), ("raw_out", C.c_void_p)]


class ConvWeights(C.Structure):
    _fields_ = [("wpack", C.c_void_p), ("bias", C.c_void_p), ("cfg", C.c_int32), ("inv_wscale", C.c_float),
                ("whi", C.c_void_p), ("wlo", C.c_void_p), ("subpixel", C.c_int32), ("ksplit", C.c_int32),
                ("wedge", C.c_void_p), ("bias_raw", C.c_void_p), ("fuse_next", C.c_int32), ("pad_", C.c_int32)]


class H8(C.Structure):
    _fields_ = [("hi", C.c_void_p), ("lo", C.c_void_p), ("img_stride", C.c_int64), ("g_off", C.c_int32),
                ("groups", C.c_int32), ("g", Geom)]


class ConvH8Desc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("cfg", C.c_int32),
                ("prec", C.c_int32), ("epi_mode", C.c_int32), ("slope", C.c_float), ("inv_wscale", C.c_float),
                ("tail_finite", C.c_int32), ("pad_", C.c_int32), ("src", H8), ("dst", H8), ("pool", H8), ("whi", C.c_void_p), ("wlo", C.c_void_p),
                ("bias", C.c_void_p), ("edge", C.c_void_p), ("status", C.c_void_p), ("ksplit", C.c_int32),
                ("pad2_", C.c_int32), ("part", C.c_void_p), ("cnt", C.c_void_p), ("ring_w", C.c_void_p),
                ("ring_bias", C.c_void_p), ("ring_corr", C.c_void_p), ("ring_cnt", C.c_void_p),
                ("ring_full", C.c_void_p)]


class Block0Desc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cfg_a", C.c_int32), ("cfg_b", C.c_int32),
                ("slope", C.c_float), ("inv_wscale_a", C.c_float), ("inv_wscale_b", C.c_float),
                ("tail_finite", C.c_int32), ("src", H8), ("dst", H8), ("pool", H8), ("whi_a", C.c_void_p),
                ("bias_a", C.c_void_p), ("whi_b", C.c_void_p), ("bias_b", C.c_void_p), ("status", C.c_void_p)]


class LaunchInfo(C.Structure):
    """rrin_launch_info: the launch shape a conv would take (rrin_conv_h8_launch_info)."""
    _fields_ = [("tiles", C.c_int64), ("grid", C.c_int64), ("extra", C.c_int64), ("variant", C.c_int32),
                ("pad_", C.c_int32)]


class EdgeFixDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("prec", C.c_int32),
                ("epi_mode", C.c_int32), ("slope", C.c_float), ("src", H8), ("dst", H8),
                ("edge", C.c_void_p), ("wedge", C.c_void_p), ("bias", C.c_void_p), ("status", C.c_void_p),
                ("part", C.c_void_p), ("cnt", C.c_void_p), ("part_floats", C.c_int64), ("cnt_len", C.c_int32),
                ("full", C.c_int32)]


class Yuv420(C.Structure):
    """rrin_yuv420: one stack of 8-bit YUV frames (NV12: v == u + 1, c_step 2; I420: c_step 1); ``chroma`` is
    CHROMA_420 (zero, the default), CHROMA_422 or CHROMA_444."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("img_stride", C.c_int64),
                ("y_pitch", C.c_int32), ("c_pitch", C.c_int32), ("c_step", C.c_int32), ("chroma", C.c_int32)]


CHROMA_420, CHROMA_422, CHROMA_444 = 0, 1, 2   # enum rrin_chroma


class YuvCoef(C.Structure):
    """rrin_yuv_coef: the 15 Q14 integers of the colour conversion (rrin_amd.yuv.Coef order)."""
    _fields_ = [(k, C.c_int32) for k in ("y0", "ay", "rv", "gu", "gv", "bu", "yr", "yg", "yb", "ur", "ug", "ub",
                                         "vr", "vg", "vb")]


YUV_BT709, YUV_BT601 = 0, 1


class YuvPlanes(C.Structure):
    """rrin_yuv_planes: the geometry of one YUV frame in elements, for rrin_mean_frames_yuv_lut."""
    _fields_ = [("u_off", C.c_int64), ("v_off", C.c_int64), ("y_pitch", C.c_int32), ("c_pitch", C.c_int32),
                ("c_step", C.c_int32), ("chroma", C.c_int32), ("depth", C.c_int32), ("shift", C.c_int32)]


class Yuv420x16(C.Structure):
    """rrin_yuv420_16: one stack of 4:2:0 frames of 16-bit words (pitches and strides in samples; depth 10 or
    12; shift 0: the sample in the low bits, 16 - depth: in the high bits)."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("img_stride", C.c_int64),
                ("y_pitch", C.c_int32), ("c_pitch", C.c_int32), ("c_step", C.c_int32), ("depth", C.c_int32),
                ("shift", C.c_int32), ("chroma", C.c_int32)]


class HeadH8Desc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("mode", C.c_int32),
                ("prec", C.c_int32), ("pad_", C.c_int32), ("src", H8), ("g16", H8), ("w", C.c_void_p),
                ("bias", C.c_void_p), ("coef", C.c_void_p), ("out", C.c_void_p), ("flow_raw", H8),
                ("raw_out", C.c_void_p), ("status", C.c_void_p), ("out_u8", C.c_void_p), ("h0", C.c_int32),
                ("w0", C.c_int32), ("top", C.c_int32), ("pad2_", C.c_int32), ("out_yuv", Yuv420),
                ("yuv_coef", YuvCoef), ("pad3_", C.c_int32), ("out_u16", C.c_void_p), ("u16_depth", C.c_int32),
                ("pad4_", C.c_int32), ("out_yuv16", Yuv420x16)]


class HeadWeights(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p)]


class NetDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("pad_", C.c_int32),
                ("i0", C.c_void_p), ("i1", C.c_void_p), ("out", C.c_void_p), ("coef", C.c_void_p),
                ("convs", C.POINTER(ConvWeights)), ("heads", C.POINTER(HeadWeights)),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("skip_flow", C.c_int32), ("prec", C.c_int32), ("prof", C.c_void_p), ("taps", C.c_void_p),
                ("status", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class NetU8Desc(C.Structure):
    _fields_ = [("net", NetDesc), ("f0", C.c_void_p), ("f1", C.c_void_p), ("img_stride", C.c_int64),
                ("out_u8", C.c_void_p), ("h0", C.c_int32), ("w0", C.c_int32)]


class NetYuvDesc(C.Structure):
    _fields_ = [("net", NetDesc), ("f0", Yuv420), ("f1", Yuv420), ("out", Yuv420), ("coef", YuvCoef),
                ("h0", C.c_int32), ("w0", C.c_int32), ("pad_", C.c_int32)]


class NetU16Desc(C.Structure):
    _fields_ = [("net", NetDesc), ("f0", C.c_void_p), ("f1", C.c_void_p), ("img_stride", C.c_int64),
                ("out_u16", C.c_void_p), ("h0", C.c_int32), ("w0", C.c_int32), ("depth", C.c_int32),
                ("pad_", C.c_int32)]


class NetYuv16Desc(C.Structure):
    _fields_ = [("net", NetDesc), ("f0", Yuv420x16), ("f1", Yuv420x16), ("out", Yuv420x16), ("coef", YuvCoef),
                ("h0", C.c_int32), ("w0", C.c_int32), ("pad_", C.c_int32)]


class Items(C.Structure):
    """rrin_items: the pairs of an item forward and the device int32 map item -> pair."""
    _fields_ = [("n_pairs", C.c_int32), ("pad_", C.c_int32), ("pair_map", C.c_void_p)]


class FlowScale(C.Structure):
    """rrin_flow_scale: the second plan (Flow U-Net at (h / s, w / s)) of a flow_scale forward."""
    _fields_ = [("s", C.c_int32), ("pad_", C.c_int32), ("convs", C.POINTER(ConvWeights)),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_int64)]


class Plane(C.Structure):
    """rrin_plane: sample (r, c) of a frame's plane is element ``off + r*pitch + c*step`` (rrin_amd.metrics.planes_of)."""
    _fields_ = [("off", C.c_int64), ("pitch", C.c_int64), ("step", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("pad", C.c_int32)]


class AuxPlane(C.Structure):
    """rrin_aux_plane: the extra plane (alpha, depth, ID) of a byte-frame forward (rrin_amd.plane); strides and
    pitches in elements, ``scratch`` of rrin_plane_scratch_bytes."""
    _fields_ = [("a0", C.c_void_p), ("a1", C.c_void_p), ("out", C.c_void_p), ("in_stride", C.c_int64),
                ("out_stride", C.c_int64), ("in_pitch", C.c_int32), ("out_pitch", C.c_int32), ("depth", C.c_int32),
                ("shift", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class TConvDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("mode", C.c_int32), ("leaky", C.c_int32), ("slope", C.c_float), ("x", C.c_void_p),
                ("y", C.c_void_p), ("wt", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p)]


class TWgradDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("leaky", C.c_int32), ("slope", C.c_float), ("pad_", C.c_int32), ("x", C.c_void_p),
                ("g", C.c_void_p), ("y", C.c_void_p), ("gw", C.c_void_p), ("gb", C.c_void_p),
                ("work", C.c_void_p)]


TCONV_FWD, TCONV_DGRAD = 0, 1


class UNetDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("in_ch", C.c_int32), ("out_ch", C.c_int32),
                ("depth", C.c_int32), ("prec", C.c_int32), ("pad_", C.c_int32), ("x", C.c_void_p), ("y", C.c_void_p),
                ("convs", C.POINTER(ConvWeights)), ("head", HeadWeights), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("prof", C.c_void_p), ("status", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


# every symbol include/rrin_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "rrin_make_geom": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Geom)]),
    "rrin_conv_cfg_count": (C.c_int, []),
    "rrin_conv_cfg_bm": (C.c_int, [C.c_int32]),
    "rrin_conv_cfg_th": (C.c_int, [C.c_int32]),
    "rrin_conv3x3_fwd": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "rrin_pack_conv3x3_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_pack_bias_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "rrin_head_fwd": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p]),
    "rrin_nchw_to_pp": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PP), C.c_void_p]),
    "rrin_pp_to_nchw": (C.c_int, [C.POINTER(PP), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_warp_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_net_conv_count": (C.c_int, []),
    "rrin_net_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rrin_net_scratch_bytes": (C.c_int64, [C.POINTER(NetDesc)]),
    "rrin_tpack_wino": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_unet_scratch_bytes": (C.c_int64, [C.POINTER(UNetDesc)]),
    "rrin_make_geom_h8": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Geom)]),
    "rrin_conv_h8_cfg_count": (C.c_int, []),
    "rrin_conv_h8_cfg_bm": (C.c_int, [C.c_int32]),
    "rrin_conv_h8_cfg_th": (C.c_int, [C.c_int32]),
    "rrin_conv_h8_cfg_ok": (C.c_int, [C.c_int32, C.c_int32]),
    "rrin_conv_h8_cfg_fits": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_conv3x3_h8_fwd": (C.c_int, [C.POINTER(ConvH8Desc), C.c_void_p]),
    "rrin_conv_block0_h8_fwd": (C.c_int, [C.POINTER(Block0Desc), C.c_void_p]),
    "rrin_conv_h8_cfg_wino": (C.c_int, [C.c_int32]),
    "rrin_conv_h8_split_floats": (C.c_int64, [C.c_void_p, C.c_void_p]),
    "rrin_conv_h8_ring_floats": (C.c_int64, [C.c_void_p, C.c_void_p]),
    "rrin_edge_fix_split_floats": (C.c_int64, [C.c_void_p, C.c_void_p]),
    "rrin_pack_conv3x3_wino_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3_wino_bm_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3_wino_bm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "rrin_pack_conv3x3_wino": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "rrin_pack_conv3x3_wino42_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "rrin_conv_h8_set_wino42_geom": (C.c_int, [C.c_int32]),
    "rrin_conv_h8_launch_info": (C.c_int, [C.POINTER(ConvH8Desc), C.c_void_p, C.POINTER(LaunchInfo)]),
    "rrin_conv_block0_h8_launch_info": (C.c_int, [C.POINTER(Block0Desc), C.c_void_p, C.POINTER(LaunchInfo)]),
    "rrin_pack_conv3x3_wino42": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rrin_pack_conv3x3_wino_h8_halves": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3_wino_h8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "rrin_pack_conv3x3_h8_halves": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3_h8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "rrin_pack_conv3x3_r32_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_pack_conv3x3_r32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "rrin_subpixel_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p]),
    "rrin_ring_pixels": (C.c_int64, [C.c_int32, C.c_int32]),
    "rrin_subpixel_edge_fix_h8": (C.c_int, [C.POINTER(EdgeFixDesc), C.c_void_p]),
    "rrin_upsample2x_h8": (C.c_int, [C.POINTER(H8), C.POINTER(H8), C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_pack_g16_h8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(H8), C.c_int32, C.c_void_p]),
    "rrin_pack_g16_u8_h8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(H8), C.c_int32, C.c_void_p]),
    "rrin_yuv_coef_std": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(YuvCoef)]),
    "rrin_pack_g16_yuv_h8": (C.c_int, [C.POINTER(Yuv420), C.POINTER(Yuv420), C.POINTER(YuvCoef), C.c_int32,
                                       C.c_int32, C.c_int32, C.POINTER(H8), C.c_int32, C.c_void_p]),
    "rrin_pack_g16_u16_h8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(H8), C.c_int32, C.c_void_p]),
    "rrin_yuv_coef_std16": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(YuvCoef)]),
    "rrin_pack_g16_yuv16_h8": (C.c_int, [C.POINTER(Yuv420x16), C.POINTER(Yuv420x16), C.POINTER(YuvCoef), C.c_int32,
                                         C.c_int32, C.c_int32, C.POINTER(H8), C.c_int32, C.c_void_p]),
    "rrin_nchw_to_h8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(H8), C.c_int32,
                                  C.c_void_p]),
    "rrin_h8_to_nchw": (C.c_int, [C.POINTER(H8), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p]),
    "rrin_head_h8_fwd": (C.c_int, [C.POINTER(HeadH8Desc), C.c_void_p]),
    "rrin_flow_tblend_fwd": (C.c_int, [C.POINTER(PP), C.POINTER(PP), C.c_void_p, C.c_int32, C.c_void_p]),
    "rrin_flow_tblend_h8": (C.c_int, [C.POINTER(H8), C.POINTER(H8), C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p]),
    "rrin_flow_tblend_items_h8": (C.c_int, [C.POINTER(H8), C.POINTER(H8), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_void_p]),
    "rrin_net_u8_items_fwd": (C.c_int, [C.POINTER(NetU8Desc), C.POINTER(Items), C.c_void_p]),
    "rrin_net_yuv_items_fwd": (C.c_int, [C.POINTER(NetYuvDesc), C.POINTER(Items), C.c_void_p]),
    "rrin_net_u16_items_fwd": (C.c_int, [C.POINTER(NetU16Desc), C.POINTER(Items), C.c_void_p]),
    "rrin_net_yuv16_items_fwd": (C.c_int, [C.POINTER(NetYuv16Desc), C.POINTER(Items), C.c_void_p]),
    "rrin_g16_downscale_h8": (C.c_int, [C.POINTER(H8), C.POINTER(H8), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_flow_upscale_h8": (C.c_int, [C.POINTER(H8), C.POINTER(H8), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p]),
    "rrin_net_scaled_fwd": (C.c_int, [C.POINTER(NetDesc), C.POINTER(FlowScale), C.c_void_p]),
    "rrin_net_u8_scaled_fwd": (C.c_int, [C.POINTER(NetU8Desc), C.POINTER(Items), C.POINTER(FlowScale), C.c_void_p]),
    "rrin_net_yuv_scaled_fwd": (C.c_int, [C.POINTER(NetYuvDesc), C.POINTER(Items), C.POINTER(FlowScale),
                                          C.c_void_p]),
    "rrin_net_u16_scaled_fwd": (C.c_int, [C.POINTER(NetU16Desc), C.POINTER(Items), C.POINTER(FlowScale),
                                          C.c_void_p]),
    "rrin_net_yuv16_scaled_fwd": (C.c_int, [C.POINTER(NetYuv16Desc), C.POINTER(Items), C.POINTER(FlowScale),
                                            C.c_void_p]),
    "rrin_plane_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "rrin_plane_warp_h8": (C.c_int, [C.POINTER(H8), C.POINTER(AuxPlane), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_plane_blend_h8": (C.c_int, [C.POINTER(AuxPlane), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_net_u8_plane_fwd": (C.c_int, [C.POINTER(NetU8Desc), C.POINTER(Items), C.POINTER(FlowScale),
                                        C.POINTER(AuxPlane), C.c_void_p]),
    "rrin_net_u16_plane_fwd": (C.c_int, [C.POINTER(NetU16Desc), C.POINTER(Items), C.POINTER(FlowScale),
                                         C.POINTER(AuxPlane), C.c_void_p]),
    "rrin_net_yuv_plane_fwd": (C.c_int, [C.POINTER(NetYuvDesc), C.POINTER(Items), C.POINTER(FlowScale),
                                         C.POINTER(AuxPlane), C.c_void_p]),
    "rrin_net_yuv16_plane_fwd": (C.c_int, [C.POINTER(NetYuv16Desc), C.POINTER(Items), C.POINTER(FlowScale),
                                           C.POINTER(AuxPlane), C.c_void_p]),
    "rrin_mean_frames": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_mean_frames_lut": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rrin_mean_frames_yuv_lut": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                           C.POINTER(YuvPlanes), C.POINTER(YuvCoef), C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "rrin_gate_items_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "rrin_gate_frames_items_u8_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rrin_net_fwd": (C.c_int, [C.POINTER(NetDesc), C.c_void_p]),
    "rrin_net_u8_fwd": (C.c_int, [C.POINTER(NetU8Desc), C.c_void_p]),
    "rrin_net_yuv_fwd": (C.c_int, [C.POINTER(NetYuvDesc), C.c_void_p]),
    "rrin_net_u16_fwd": (C.c_int, [C.POINTER(NetU16Desc), C.c_void_p]),
    "rrin_net_yuv16_fwd": (C.c_int, [C.POINTER(NetYuv16Desc), C.c_void_p]),
    "rrin_pair_sad_u16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_pair_sad_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "rrin_gate_from_sad_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_gate_frames_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "rrin_pair_sad_u8_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                       C.c_void_p]),
    "rrin_pair_sad_u16_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p]),
    "rrin_gate_frames_u8_len": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "rrin_frame_metrics_workspace_bytes": (C.c_int64, [C.c_int32, C.POINTER(Plane), C.c_int32, C.c_int32]),
    "rrin_frame_metrics_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Plane),
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_void_p]),
    "rrin_frame_metrics_u16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Plane),
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_void_p]),
    "rrin_frame_metrics_tile": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rrin_triplet_crop_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Plane), C.POINTER(C.c_int32),
                                       C.c_int32, C.c_int32, C.c_int32, C.POINTER(YuvCoef), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "rrin_triplet_crop_u16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(Plane), C.POINTER(C.c_int32),
                                        C.c_int32, C.c_int32, C.c_int32, C.POINTER(YuvCoef), C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rrin_tloss_workspace_bytes": (C.c_int64, [C.c_int64]),
    "rrin_tloss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_float,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rrin_trelu_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rrin_trelu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "rrin_tmaxpool2_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_tmaxpool2_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p]),
    "rrin_tfeatdist_workspace_bytes": (C.c_int64, [C.c_int64]),
    "rrin_tfeatdist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p]),
    "rrin_unet_conv_count": (C.c_int64, [C.c_int32]),
    "rrin_unet_fwd": (C.c_int, [C.POINTER(UNetDesc), C.c_void_p]),
    "rrin_prof_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "rrin_prof_destroy": (C.c_int, [C.c_void_p]),
    "rrin_prof_reset": (C.c_int, [C.c_void_p]),
    "rrin_prof_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.POINTER(C.c_int32)]),
    "rrin_prof_read_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.POINTER(C.c_int32)]),
    "rrin_tconv3x3": (C.c_int, [C.POINTER(TConvDesc), C.c_void_p]),
    "rrin_tconv3x3_wgrad_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rrin_tconv3x3_wgrad": (C.c_int, [C.POINTER(TWgradDesc), C.c_void_p]),
    "rrin_tpool2_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_tpool2_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_tup2_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_tup2_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_twarp_bwd_work_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rrin_twarp_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "rrin_abi_version": (C.c_int, []),
    "rrin_strerror": (C.c_char_p, [C.c_int]),
}

_LIB = None


class RRINError(RuntimeError):
    pass


def build_id(path: str = LIB_PATH) -> str:
    """First 16 hex digits of the SHA-256 of the library file: names the build a
    measurement came from (profiles/pmc_traffic.json entries carry it; bench.py only
    reports a PMC traffic figure measured on the library it runs)."""
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def lib():
    """Load (once) and return the library; raises if it is absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RRINError(f"{LIB_PATH} not built: run `make -j16` (or __graft_entry__.build()); "
                            "rrin_amd has no non-HIP fallback")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(h, name, None)
            if f is None and os.environ.get("RRIN_LIB_AB"):
                continue  # an A/B build from before the symbol was added
            if f is None:
                raise RRINError(f"{LIB_PATH} lacks {name}: rebuild it (`make -j16`)")
            f.restype = res
            f.argtypes = args
        # an A/B build of an earlier ABI whose changes since are appends only (RRIN_LIB_AB_ABI=16)
        ok = {ABI_VERSION} | ({int(os.environ.get("RRIN_LIB_AB_ABI", ABI_VERSION))} if os.environ.get("RRIN_LIB_AB") else set())
        if h.rrin_abi_version() not in ok:
            raise RRINError(f"librrin_hip ABI {h.rrin_abi_version()} != expected {ABI_VERSION}")
        _LIB = h
    return _LIB


def check(rc: int, what: str = "rrin"):
    if rc != 0:
        msg = lib().rrin_strerror(rc)
        raise RRINError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def geom(h: int, w: int) -> Geom:
    g = Geom()
    check(lib().rrin_make_geom(h, w, C.byref(g)), "rrin_make_geom")
    return g


def geom_h8(h: int, w: int) -> Geom:
    g = Geom()
    check(lib().rrin_make_geom_h8(h, w, C.byref(g)), "rrin_make_geom_h8")
    return g
