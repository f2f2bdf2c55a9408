"""lanczos_hls_amd -- Python plumbing over the C ABI (include/lanczos_hip.h).

The product is liblanczos_hip.so (HIP kernels for gfx950 + the extern "C" boundary).  This module
only loads it with ctypes and mirrors the reference's call surface so tests and the benchmark read like
the reference's testbench:

    lanczos(img_hwc, scale_n, scale_d, a)   <- lanczos(stream_in, stream_out)   lanczos.h:121-126
    lanczos_kernel(x, a)                    <- double lanczos_kernel(double)    full_TB.h:51-53

There is NO CPU fallback: if the shared library is missing or no GPU is present the calls raise.
Nothing here imports anything under oracle/.
"""
import collections
import ctypes
import os
import subprocess
from functools import cached_property as _cached_property

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LANCZOS_LIB: load another build of the same C ABI (A/B experiments); default is the in-tree product build
LIB_PATH = os.environ.get("LANCZOS_LIB") or os.path.join(_HERE, "liblanczos_hip.so")

OK, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_RCCL = range(7)   # include/lanczos_hip.h:43-49
MODE_LSB1, MODE_EXACT, MODE_HLS = 0, 1, 2
KERNEL_NONE, KERNEL_GENERIC, KERNEL_FAST, KERNEL_HLS = 0, 1, 2, 3
KERNEL_RESIZE_FUSED, KERNEL_RESIZE_TWO_PASS, KERNEL_RESIZE_NEAREST = 4, 5, 6
# lanczos_last_route: the main kernel and the route of the in-place prefix rows (include/lanczos_hip.h LANCZOS_ROUTE_*)
ROUTE_MAIN_NONE, ROUTE_MAIN_MARCH, ROUTE_MAIN_TILE, ROUTE_MAIN_RATP, ROUTE_MAIN_RAT, ROUTE_MAIN_GENERIC, ROUTE_MAIN_HLS = range(7)
ROUTE_PREFIX_NONE, ROUTE_PREFIX_RIDING, ROUTE_PREFIX_FRONT, ROUTE_PREFIX_BEHIND, ROUTE_PREFIX_STREAMED = range(5)
ROUTE_MAIN_NAMES = ("none", "march", "tile", "ratp", "rat", "generic", "hls")
ROUTE_PREFIX_NAMES = ("none", "riding", "front", "behind", "streamed")
RESIZE_AUTO, RESIZE_FUSED, RESIZE_TWO_PASS, RESIZE_CONVERT = 0, 1, 2, 3   # lanczos_resize_force
RESIZE_ALPHA = 1   # flag of lanczos_resize_desc.reserved[0]: channel 3 of 4 is straight alpha (Pillow's RGBA mode)
RESIZE_U16 = 4     # flag of lanczos_resize_desc.reserved[0]: native-endian uint16 samples (Pillow's I;16 arithmetic)
RESIZE_F32 = 16    # flag of lanczos_resize_desc.reserved[0]: float samples (Pillow's mode F arithmetic); with no other flag
# the filter of a resize (Image.resize's `resample`), bits 8..11 of lanczos_resize_desc.reserved[0]
FILTER_LANCZOS, FILTER_BOX, FILTER_BILINEAR, FILTER_HAMMING, FILTER_BICUBIC, FILTER_NEAREST = range(6)
FILTER_NAMES = ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest")
TENSOR_FUSED, TENSOR_CONVERTED = 1, 2   # lanczos_last_tensor_route: who wrote the floats of the last tensor call
TENSOR_BF16, TENSOR_F16 = 1, 2          # the formats of lanczos_tensor_lut_convert16 / lanczos_tensor16_lut_normalize
_TENSOR16_FORMATS = {"bfloat16": TENSOR_BF16, "float16": TENSOR_F16}
TENSOR_F32 = 3                          # ... and the third element format of lanczos_tensor_norm
TENSOR_CHW, TENSOR_HWC = 0, 1           # the layouts of lanczos_tensor_norm_init
_TENSOR_NORM_FORMATS = {"float32": TENSOR_F32, "bfloat16": TENSOR_BF16, "float16": TENSOR_F16}
SOURCE_INTERLEAVED, SOURCE_PLANAR = 0, 1   # the layouts of lanczos_resize_source_init
SOURCE_DIRECT, SOURCE_PACKED = 1, 2        # lanczos_last_source_route: who read the source of the last call that had one
DEST_INTERLEAVED, DEST_PLANAR = 0, 1       # the layouts of lanczos_resize_dest_init
DEST_DIRECT, DEST_UNPACKED = 1, 2          # lanczos_last_dest_route: who stored into the destination of the last call that had one

# every symbol include/lanczos_hip.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = [
    "lanczos_desc_init", "lanczos_validate", "lanczos_inplace_rows", "lanczos_strip_input_rows",
    "lanczos_in_frame_bytes", "lanczos_out_frame_bytes", "lanczos_kernel", "lanczos_kernel_idx",
    "lanczos_taps_host", "lanczos_create", "lanczos_destroy", "lanczos_host_alloc", "lanczos_host_free",
    "lanczos_resample_host",
    "lanczos_resample_device", "lanczos_planar_to_interleaved_device", "lanczos_interleaved_to_planar_device",
    "lanczos_resample_planar_device", "lanczos_u8", "lanczos_timing_enable", "lanczos_timing_read",
    "lanczos_last_kernel", "lanczos_last_route", "lanczos_last_march_table", "lanczos_last_hip_error", "lanczos_force_kernel", "lanczos_strerror",
    "lanczos_version",
    "lanczos_partition_frames", "lanczos_partition_rows", "lanczos_multi_create", "lanczos_multi_destroy",
    "lanczos_multi_devices", "lanczos_resample_multi_host", "lanczos_resample_multi_root",
    "lanczos_multi_last_error", "lanczos_multi_exchange_plan", "lanczos_multi_exchange_selftest", "lanczos_device_alloc", "lanczos_device_free",
    "lanczos_device_copy",
    "lanczos_resize_desc_init", "lanczos_resize_desc_init_ex", "lanczos_resize_desc_init_filter", "lanczos_resize_validate", "lanczos_resize_taps_host",
    "lanczos_resize_taps_f64_host", "lanczos_resize_device",
    "lanczos_resize_host", "lanczos_resize_force", "lanczos_resize_plan_host",
    "lanczos_resize_opts_init", "lanczos_resize_taps_host_ex", "lanczos_resize_taps_f64_host_ex",
    "lanczos_resize_plan_host_ex", "lanczos_resize_device_ex", "lanczos_resize_host_ex",
    "lanczos_reduce_size", "lanczos_reduce_device", "lanczos_reduce_host",
    "lanczos_resize_tensor_validate", "lanczos_tensor_lut_normalize", "lanczos_resize_tensor_device",
    "lanczos_resize_tensor_host", "lanczos_last_tensor_route",
    "lanczos_resize_tensor16_validate", "lanczos_tensor_lut_convert16", "lanczos_tensor16_lut_normalize",
    "lanczos_resize_tensor16_device", "lanczos_resize_tensor16_host",
    "lanczos_resize_window_init", "lanczos_resize_window_validate", "lanczos_resize_window_source",
    "lanczos_resize_window_plan_host", "lanczos_resize_window_device", "lanczos_resize_window_host",
    "lanczos_resize_tensor_window_validate", "lanczos_resize_tensor16_window_validate",
    "lanczos_resize_tensor_window_device", "lanczos_resize_tensor_window_host",
    "lanczos_resize_tensor16_window_device", "lanczos_resize_tensor16_window_host",
    "lanczos_tensor_view_init", "lanczos_resize_tensor_view_validate", "lanczos_resize_tensor_view_device",
    "lanczos_resize_tensor_view_host",
    "lanczos_resize_crops_validate", "lanczos_resize_crops_plan_host", "lanczos_resize_tensor_crops_validate",
    "lanczos_resize_tensor_crops_device", "lanczos_resize_tensor_crops_host",
    "lanczos_resize_source_init", "lanczos_resize_source_validate", "lanczos_resize_source_device",
    "lanczos_resize_tensor_source_device", "lanczos_resize_source_host", "lanczos_resize_tensor_source_host",
    "lanczos_last_source_route",
    "lanczos_resize_dest_init", "lanczos_resize_dest_validate", "lanczos_resize_dest_device", "lanczos_resize_dest_host",
    "lanczos_last_dest_route",
    "lanczos_tensor_norm_init", "lanczos_resize_tensor_norm_validate", "lanczos_resize_tensor_norm_device",
    "lanczos_resize_tensor_norm_host",
    "lanczos_ycc_source_init", "lanczos_ycc_source_validate", "lanczos_ycc_table", "lanczos_resize_ycc_device",
    "lanczos_resize_ycc_tensor_device", "lanczos_resize_ycc_host", "lanczos_resize_ycc_tensor_host", "lanczos_last_ycc_info",
    "lanczos_ycc_dest_init", "lanczos_ycc_dest_validate", "lanczos_ycc_table_forward", "lanczos_resize_ycc_out",
    "lanczos_last_ycc_out_info",
    "lanczos_ycc16_matrix_init", "lanczos_ycc16_matrix_validate", "lanczos_ycc16_source_init", "lanczos_ycc16_source_validate",
    "lanczos_ycc16_dest_init", "lanczos_ycc16_dest_validate", "lanczos_ycc16_request_validate", "lanczos_resize_ycc16",
    "lanczos_last_ycc16_info",
]
SPLIT_FRAMES, SPLIT_ROWS = 0, 1
YCC_PLANAR, YCC_NV12, YCC_NV21 = 0, 1, 2   # lanczos_ycc_source.layout
YCC_JFIF, YCC_BT601, YCC_BT709 = 0, 1, 2   # the standards of lanczos_ycc_table
MEM_DEVICE, MEM_HOST = 0, 1                 # lanczos_ycc_out_request.memory
YCC_STANDARDS = {"jfif": YCC_JFIF, "bt601": YCC_BT601, "bt709": YCC_BT709}
# the frame layouts Context.resize_ycc knows by name: (layout, sub_x, sub_y)
YCC_LAYOUTS = {"nv12": (YCC_NV12, 1, 1), "nv21": (YCC_NV21, 1, 1), "i420": (YCC_PLANAR, 1, 1), "i422": (YCC_PLANAR, 1, 0),
               "i444": (YCC_PLANAR, 0, 0)}
# ... and what the 16-bit entry (lanczos_resize_ycc16) adds: a fourth standard for ycc16_matrix, and the names of the frames of
# word pairs -- "p010" / "p016" have the nv12 shape, "p210" / "p216" (and "nv16") the 4:2:2 one
YCC_BT2020 = 3
YCC16_STANDARDS = dict(YCC_STANDARDS, bt2020=YCC_BT2020)
YCC16_LAYOUTS = dict(YCC_LAYOUTS, p010=(YCC_NV12, 1, 1), p016=(YCC_NV12, 1, 1), nv16=(YCC_NV12, 1, 0), p210=(YCC_NV12, 1, 0),
                     p216=(YCC_NV12, 1, 0))


class Route(collections.namedtuple("Route", "main prefix launches prefix_seen")):
    """lanczos_last_route, unpacked: ROUTE_MAIN_* and ROUTE_PREFIX_* of the last launch of the call, the number of launches,
    and the set of ROUTE_PREFIX_* that any launch of the call took."""

    def __str__(self):
        seen = "+".join(ROUTE_PREFIX_NAMES[r] for r in sorted(self.prefix_seen))
        return f"{ROUTE_MAIN_NAMES[self.main]}+{ROUTE_PREFIX_NAMES[self.prefix]} x{self.launches} (prefix routes seen: {seen})"


MARCH_TABLE_NONE, MARCH_TABLE_A, MARCH_TABLE_B = 0, 1, 2   # lanczos_march_table_info.mode


class MarchTableInfoC(ctypes.Structure):   # include/lanczos_hip.h: lanczos_march_table_info
    _fields_ = [(n, ctypes.c_int32) for n in ("workgroups", "segs", "mode", "rank_aware", "strips", "frames", "m_lo", "m_hi",
                                               "wg_per_cu", "cus")] + [("reserved", ctypes.c_int32 * 6)]


class MarchTableInfo(collections.namedtuple("MarchTableInfo", "workgroups segs mode rank_aware strips frames m_lo m_hi wg_per_cu cus")):
    """lanczos_last_march_table's info: the shape of the workgroup table the last k_march launch used (mode: MARCH_TABLE_*)."""

    def __str__(self):
        return (f"mode {'-AB'[self.mode]}, {'rank-aware' if self.rank_aware else 'equal'}: {self.workgroups} workgroups x {self.segs} "
                f"segment(s) for {self.strips} strips x {self.frames} frames, rows [{self.m_lo}, {self.m_hi}), "
                f"{self.wg_per_cu} workgroups/CU x {self.cus} CUs")


class LanczosError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = _lib().lanczos_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__(f"{what}: {msg} (code {code})")


class Desc(ctypes.Structure):
    """lanczos_desc -- the run-time form of params.h (lanczos.h:9-31)."""
    _fields_ = [
        ("in_w", ctypes.c_int32), ("in_h", ctypes.c_int32),
        ("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32),
        ("channels", ctypes.c_int32), ("bytes_per_sample", ctypes.c_int32),
        ("scale_n", ctypes.c_int32), ("scale_d", ctypes.c_int32),
        ("a", ctypes.c_int32), ("mode", ctypes.c_int32),
        ("out_row0", ctypes.c_int32), ("out_rows", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class ResizeDesc(ctypes.Structure):
    """lanczos_resize_desc -- resize to any size with Pillow's Lanczos contract (include/lanczos_hip.h)."""
    _fields_ = [
        ("in_w", ctypes.c_int32), ("in_h", ctypes.c_int32),
        ("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32),
        ("channels", ctypes.c_int32), ("a", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class ResizePlan(ctypes.Structure):
    """lanczos_resize_plan -- what lanczos_resize_device would launch (lanczos_resize_plan_host, diagnostic)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("fused", "K", "strips", "rows_per_chunk", "chunks", "ring_rows", "stage_rows",
                                              "stage_dw", "lds_bytes")]


class ResizeOpts(ctypes.Structure):
    """lanczos_resize_opts -- the source box and reducing_gap of a resize (Pillow's other two arguments)."""
    _fields_ = [("box", ctypes.c_double * 4), ("reducing_gap", ctypes.c_double), ("reserved", ctypes.c_int32 * 4)]


class ResizePlanEx(ctypes.Structure):
    """lanczos_resize_plan_ex -- how a request with options resolves (lanczos_resize_plan_host_ex, diagnostic)."""
    _fields_ = [("fx", ctypes.c_int32), ("fy", ctypes.c_int32), ("safe_box", ctypes.c_int32 * 4),
                ("reduced_w", ctypes.c_int32), ("reduced_h", ctypes.c_int32),
                ("pass_h", ctypes.c_int32), ("pass_v", ctypes.c_int32),
                ("mid_row0", ctypes.c_int32), ("mid_rows", ctypes.c_int32),
                ("inner_box", ctypes.c_double * 4), ("inner", ResizePlan)]


class ResizeWindow(ctypes.Structure):
    """lanczos_resize_window -- the window (x0, y0, w, h) of the output, in output pixels, that a call computes and stores."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


class TensorOut(ctypes.Structure):
    """lanczos_tensor_out -- the table and the float layout of a tensor request: out[c * chan_stride + y * row_stride +
    x * pix_stride] = lut[c * 256 + byte], strides in floats."""
    _fields_ = [("d_lut", ctypes.c_void_p), ("chan_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("pix_stride", ctypes.c_int64), ("reserved", ctypes.c_int32 * 4)]


class TensorOut16(ctypes.Structure):
    """lanczos_tensor16_out -- TensorOut for 16-bit elements (bfloat16 or float16 words): the table is channels * 256 16-bit
    words, strides in elements."""
    _fields_ = TensorOut._fields_


class TensorView(ctypes.Structure):
    """lanczos_tensor_view -- a tensor request of either element width with a channel map and flips:
    out[oc * chan_stride + Y * row_stride + X * pix_stride] = lut[oc * 256 + byte of source channel src_channel[oc]], X and Y
    mirrored per frame by bits 0 and 1 of flip ^ d_flip[f]."""
    _fields_ = [("d_lut", ctypes.c_void_p), ("chan_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("pix_stride", ctypes.c_int64), ("elem_bytes", ctypes.c_int32), ("out_channels", ctypes.c_int32),
                ("src_channel", ctypes.c_int32 * 4), ("flip", ctypes.c_int32), ("d_flip", ctypes.c_void_p),
                ("reserved", ctypes.c_int32 * 4)]


class TensorNorm(ctypes.Structure):
    """lanczos_tensor_norm -- a tensor request of 16-bit or float samples: out[oc * chan_stride + Y * row_stride +
    X * pix_stride] = cvt(((float)sample of source channel src_channel[oc] / div[oc] - mean[oc]) / std[oc]), three IEEE float
    operations, X and Y mirrored per frame as in TensorView; format TENSOR_F32 / TENSOR_BF16 / TENSOR_F16."""
    _fields_ = [("div", ctypes.c_float * 4), ("mean", ctypes.c_float * 4), ("std", ctypes.c_float * 4),
                ("chan_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64), ("pix_stride", ctypes.c_int64),
                ("format", ctypes.c_int32), ("out_channels", ctypes.c_int32), ("src_channel", ctypes.c_int32 * 4),
                ("flip", ctypes.c_int32), ("d_flip", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 4)]


class ResizeCrops(ctypes.Structure):
    """lanczos_resize_crops -- one window size (w, h) for every frame and a pointer to `frames` pairs (x0, y0) of int32, the
    window's origin per frame in output pixels of the full request; read, and clamped into the output, when the kernels run."""
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("d_origin", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 4)]


class ResizeSource(ctypes.Structure):
    """lanczos_resize_source -- where the samples of a source frame lie: sample (y, x, c) at byte c * chan_stride +
    y * row_stride + x * pix_stride of its frame.  Interleaved with pitched rows, or planar (8-bit)."""
    _fields_ = [("row_stride", ctypes.c_int64), ("chan_stride", ctypes.c_int64), ("pix_stride", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class ResizeDest(ctypes.Structure):
    """lanczos_resize_dest -- where the samples of a result frame go: sample (y, x, c) to byte c * chan_stride +
    y * row_stride + x * pix_stride of its frame.  Interleaved with pitched rows, or planar (8-bit)."""
    _fields_ = [("row_stride", ctypes.c_int64), ("chan_stride", ctypes.c_int64), ("pix_stride", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class YccSource(ctypes.Structure):
    """lanczos_ycc_source -- where the planes of a YCbCr frame lie: in_w x in_h luma samples at the frame base, rows
    y_row_stride bytes apart, and chroma subsampled by 2^sub_x x 2^sub_y at cb_offset / cr_offset, rows c_row_stride bytes apart
    (YCC_PLANAR), or interleaved in one plane at cb_offset == cr_offset (YCC_NV12: Cb first, YCC_NV21: Cr first)."""
    _fields_ = [("y_row_stride", ctypes.c_int64), ("c_row_stride", ctypes.c_int64), ("cb_offset", ctypes.c_int64),
                ("cr_offset", ctypes.c_int64), ("layout", ctypes.c_int32), ("sub_x", ctypes.c_int32), ("sub_y", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class YccInfoC(ctypes.Structure):   # include/lanczos_hip.h: lanczos_ycc_info
    _fields_ = [(n, ctypes.c_int32) for n in ("luma_kernel", "chroma_kernel", "split", "launches")] + [("reserved", ctypes.c_int32 * 4)]


class YccInfo(collections.namedtuple("YccInfo", "luma_kernel chroma_kernel split launches")):
    """lanczos_last_ycc_info: KERNEL_* of the luma and of the chroma resize of the last resize_ycc call (KERNEL_NONE: a copy),
    whether the interleaved chroma was split into planes first, and the number of launches of the call."""


class YccDest(ctypes.Structure):
    """lanczos_ycc_dest -- where the planes of a YCbCr result frame go: the fields of YccSource, for the stored frame (the
    window) of w x h luma samples and chroma planes of ((w + sub_x) >> sub_x) x ((h + sub_y) >> sub_y) samples."""
    _fields_ = YccSource._fields_


class YccOutRequest(ctypes.Structure):
    """lanczos_ycc_out_request -- one call of lanczos_resize_ycc_out.  The pointer fields are addresses: whoever fills them in
    keeps the structs they name alive (ycc_out_request does, on the request itself)."""
    _fields_ = [("d", ctypes.c_void_p), ("opts", ctypes.c_void_p), ("win", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("dst", ctypes.c_void_p), ("table", ctypes.c_void_p), ("in_", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("frames", ctypes.c_int32), ("memory", ctypes.c_int32), ("in_frame_stride", ctypes.c_size_t),
                ("out_frame_stride", ctypes.c_size_t), ("stream", ctypes.c_void_p), ("reserved", ctypes.c_int32 * 4)]


class YccOutInfoC(ctypes.Structure):   # include/lanczos_hip.h: lanczos_ycc_out_info
    _fields_ = [(n, ctypes.c_int32) for n in ("luma_kernel", "chroma_kernel", "split", "join", "encode", "launches")] + [
        ("reserved", ctypes.c_int32 * 2)]


class YccOutInfo(collections.namedtuple("YccOutInfo", "luma_kernel chroma_kernel split join encode launches")):
    """lanczos_last_ycc_out_info: KERNEL_* of the luma and of the chroma resize of the last resize_*_to_ycc call (KERNEL_NONE: a
    copy; from RGB luma_kernel is the RGB resize's), whether k_rs_ycc_split, k_rs_ycc_join and k_rs_ycc_encode ran, and the
    number of launches of the call."""


class Ycc16Matrix(ctypes.Structure):
    """lanczos_ycc16_matrix -- the colour conversion of 16-bit YCbCr words, passed by value:
    out[c] = clamp((k[c][0] * (y - sub[0]) + k[c][1] * (cb - sub[1]) + k[c][2] * (cr - sub[2]) + rnd) >> shift, 0, max), the sum
    in int64, rnd = 1 << (shift - 1) (0 for shift 0).  |k| < 2^24, sub and max in 0 .. 65535, shift in 0 .. 30."""
    _fields_ = [("k", (ctypes.c_int32 * 3) * 3), ("sub", ctypes.c_int32 * 3), ("shift", ctypes.c_int32), ("max", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


class Ycc16Request(ctypes.Structure):
    """lanczos_ycc16_request -- one call of lanczos_resize_ycc16.  The pointer fields are addresses: whoever fills them in keeps
    the structs they name alive (ycc16_request does, on the request itself).  dst alone: wide YCbCr out; matrix alone: packed
    RGB words; matrix and norm: tensor elements."""
    _fields_ = [("d", ctypes.c_void_p), ("opts", ctypes.c_void_p), ("win", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("dst", ctypes.c_void_p), ("matrix", ctypes.c_void_p), ("norm", ctypes.c_void_p), ("in_", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("frames", ctypes.c_int32), ("memory", ctypes.c_int32),
                ("in_frame_stride", ctypes.c_size_t), ("out_frame_stride", ctypes.c_size_t), ("stream", ctypes.c_void_p),
                ("reserved", ctypes.c_int32 * 4)]


class Ycc16InfoC(ctypes.Structure):   # include/lanczos_hip.h: lanczos_ycc16_info
    _fields_ = [(n, ctypes.c_int32) for n in ("luma_kernel", "chroma_kernel", "split", "join", "merge", "launches")] + [
        ("reserved", ctypes.c_int32 * 2)]


class Ycc16Info(collections.namedtuple("Ycc16Info", "luma_kernel chroma_kernel split join merge launches")):
    """lanczos_last_ycc16_info: KERNEL_* of the luma and of the chroma resize of the last resize_ycc16* call (KERNEL_NONE: a
    copy), whether k_rs_ycc_split16, k_rs_ycc_join16 and k_rs_ycc16_merge ran, and the number of launches of the call."""


FLIP_H, FLIP_V = 1, 2   # the bits of lanczos_tensor_view.flip and of a d_flip byte
_FLIP_NAMES = {None: 0, "": 0, "h": FLIP_H, "v": FLIP_V, "hv": FLIP_H | FLIP_V, "vh": FLIP_H | FLIP_V}


class Xfer(ctypes.Structure):
    """lanczos_xfer -- one message of the root exchange (lanczos_multi_exchange_plan)."""
    _fields_ = [("src", ctypes.c_int), ("dst", ctypes.c_int), ("src_off", ctypes.c_size_t), ("dst_off", ctypes.c_size_t),
                ("bytes", ctypes.c_size_t)]


# -- the signatures of include/lanczos_hip.h: _lib() sets them on the symbols the loaded library has
_I, _P, _Z, _F = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
_PI, _PF, _PP = ctypes.POINTER(_I), ctypes.POINTER(_F), ctypes.POINTER(_P)
_PD, _PRD, _PRO, _PRW, _PRC, _PRS, _PRT, _PYS = (ctypes.POINTER(t) for t in (Desc, ResizeDesc, ResizeOpts, ResizeWindow, ResizeCrops,
                                                                           ResizeSource, ResizeDest, YccSource))
_PYD = ctypes.POINTER(YccDest)
_PTO, _PTO16, _PTV, _PTN = (ctypes.POINTER(t) for t in (TensorOut, TensorOut16, TensorView, TensorNorm))
_PLAN, _PLANX = ctypes.POINTER(ResizePlan), ctypes.POINTER(ResizePlanEx)

# every entry that comes as a pair (ctx, <head>, in, out, frames[, in_frame_stride, out_frame_stride, stream]):
# (the device entry, the host entry, <head>)
_ENTRY_PAIRS = [
    ("lanczos_resample_device", "lanczos_resample_host", [_PD]),
    ("lanczos_resize_device", "lanczos_resize_host", [_PRD]),
    ("lanczos_resize_device_ex", "lanczos_resize_host_ex", [_PRD, _PRO]),
    ("lanczos_reduce_device", "lanczos_reduce_host", [_I] * 5 + [_P]),
    ("lanczos_resize_tensor_device", "lanczos_resize_tensor_host", [_PRD, _PRO, _PTO]),
    ("lanczos_resize_tensor16_device", "lanczos_resize_tensor16_host", [_PRD, _PRO, _PTO16]),
    ("lanczos_resize_window_device", "lanczos_resize_window_host", [_PRD, _PRO, _PRW]),
    ("lanczos_resize_tensor_window_device", "lanczos_resize_tensor_window_host", [_PRD, _PRO, _PRW, _PTO]),
    ("lanczos_resize_tensor16_window_device", "lanczos_resize_tensor16_window_host", [_PRD, _PRO, _PRW, _PTO16]),
    ("lanczos_resize_tensor_view_device", "lanczos_resize_tensor_view_host", [_PRD, _PRO, _PRW, _PTV]),
    ("lanczos_resize_tensor_crops_device", "lanczos_resize_tensor_crops_host", [_PRD, _PRO, _PRC, _PTV]),
    ("lanczos_resize_source_device", "lanczos_resize_source_host", [_PRD, _PRO, _PRW, _PRS]),
    ("lanczos_resize_tensor_source_device", "lanczos_resize_tensor_source_host", [_PRD, _PRO, _PRW, _PRC, _PRS, _PTV]),
    ("lanczos_resize_dest_device", "lanczos_resize_dest_host", [_PRD, _PRO, _PRW, _PRS, _PRT]),
    ("lanczos_resize_tensor_norm_device", "lanczos_resize_tensor_norm_host", [_PRD, _PRO, _PRW, _PRS, _PTN]),
    ("lanczos_resize_ycc_device", "lanczos_resize_ycc_host", [_PRD, _PRO, _PRW, _PYS, _P]),
    ("lanczos_resize_ycc_tensor_device", "lanczos_resize_ycc_tensor_host", [_PRD, _PRO, _PRW, _PYS, _P, _PTV]),
]
# name -> (argtypes, restype; None = int)
_SIGNATURES = {
    "lanczos_desc_init": ([_PD] + [_I] * 7, None),
    "lanczos_validate": ([_PD], None),
    "lanczos_inplace_rows": ([_PD], None),
    "lanczos_strip_input_rows": ([_PD, _I, _I, _PI, _PI], None),
    "lanczos_in_frame_bytes": ([_PD], _Z),
    "lanczos_out_frame_bytes": ([_PD], _Z),
    "lanczos_kernel": ([_F, _I], _F),
    "lanczos_kernel_idx": ([_I] * 5, _F),
    "lanczos_taps_host": ([_PD, _I, _P, _P], None),
    "lanczos_create": ([_PP, _I], None),
    "lanczos_destroy": ([_P], None),
    "lanczos_host_alloc": ([_PP, _Z], None),
    "lanczos_host_free": ([_P], None),
    "lanczos_planar_to_interleaved_device": ([_P, _P, _P] + [_I] * 5 + [_P], None),
    "lanczos_interleaved_to_planar_device": ([_P, _P, _P] + [_I] * 5 + [_P], None),
    "lanczos_resample_planar_device": ([_P, _PD, _P, _P, _I, _P], None),
    "lanczos_u8": ([_P, _P, _I, _I, _I, _P, _I, _I, _I], None),
    "lanczos_timing_enable": ([_P, _I], None),
    "lanczos_timing_read": ([_P, _PI, _PF, _PF], None),
    "lanczos_last_kernel": ([_P], None),
    "lanczos_last_hip_error": ([_P], None),
    "lanczos_last_route": ([_P], None),
    "lanczos_last_march_table": ([_P, ctypes.POINTER(MarchTableInfoC), ctypes.POINTER(ctypes.c_int32), _I], None),
    "lanczos_force_kernel": ([_P, _I], None),
    "lanczos_strerror": ([_I], ctypes.c_char_p),
    "lanczos_version": ([], ctypes.c_char_p),
    "lanczos_partition_frames": ([_I, _I, _I, _PI, _PI], None),
    "lanczos_partition_rows": ([_PD, _I, _I, _PI, _PI, _PI, _PI], None),
    "lanczos_multi_create": ([_PP, _PI, _I], None),
    "lanczos_multi_destroy": ([_P], None),
    "lanczos_multi_devices": ([_P], None),
    "lanczos_resample_multi_host": ([_P, _PD, _P, _P, _I, _I], None),
    "lanczos_resample_multi_root": ([_P, _PD, _P, _P, _I, _I, _PF, _PF], None),
    "lanczos_multi_exchange_plan": ([_PD, _I, _I, _I, _I, ctypes.POINTER(Xfer), _I], None),
    "lanczos_multi_exchange_selftest": ([_P, _I, _Z, _I], None),
    "lanczos_resize_desc_init": ([_PRD] + [_I] * 6, None),
    "lanczos_resize_desc_init_ex": ([_PRD] + [_I] * 7, None),
    "lanczos_resize_desc_init_filter": ([_PRD] + [_I] * 7, None),
    "lanczos_resize_validate": ([_PRD], None),
    "lanczos_resize_taps_host": ([_PRD, _I, _P, _P, _P, _PI], None),
    "lanczos_resize_taps_f64_host": ([_PRD, _I, _P, _P, _P, _PI], None),
    "lanczos_resize_force": ([_P, _I], None),
    "lanczos_resize_plan_host": ([_PRD, _I, _PLAN], None),
    "lanczos_resize_opts_init": ([_PRO, _PRD], None),
    "lanczos_resize_taps_host_ex": ([_PRD, _PRO, _I, _P, _P, _P, _PI], None),
    "lanczos_resize_taps_f64_host_ex": ([_PRD, _PRO, _I, _P, _P, _P, _PI], None),
    "lanczos_resize_plan_host_ex": ([_PRD, _PRO, _I, _PLANX], None),
    "lanczos_reduce_size": ([_I] * 4 + [_P, _PI, _PI], None),
    "lanczos_resize_tensor_validate": ([_PRD, _PTO], None),
    "lanczos_tensor_lut_normalize": ([_I, _P, _P, _P], None),
    "lanczos_last_tensor_route": ([_P], None),
    "lanczos_resize_tensor16_validate": ([_PRD, _PTO16], None),
    "lanczos_tensor_lut_convert16": ([_P, _I, _I, _P], None),
    "lanczos_tensor16_lut_normalize": ([_I, _P, _P, _I, _P], None),
    "lanczos_resize_window_init": ([_PRW, _PRD], None),
    "lanczos_resize_window_validate": ([_PRD, _PRW], None),
    "lanczos_resize_window_source": ([_PRD, _PRO, _PRW, _P], None),
    "lanczos_resize_window_plan_host": ([_PRD, _PRO, _PRW, _I, _PLANX], None),
    "lanczos_resize_tensor_window_validate": ([_PRD, _PRW, _PTO], None),
    "lanczos_resize_tensor16_window_validate": ([_PRD, _PRW, _PTO16], None),
    "lanczos_tensor_view_init": ([_PTV, _PRD, _I], None),
    "lanczos_resize_tensor_view_validate": ([_PRD, _PRW, _PTV], None),
    "lanczos_resize_crops_validate": ([_PRD, _PRC], None),
    "lanczos_resize_crops_plan_host": ([_PRD, _PRO, _PRC, _I, _PLANX], None),
    "lanczos_resize_tensor_crops_validate": ([_PRD, _PRC, _PTV], None),
    "lanczos_resize_source_init": ([_PRS, _PRD, _I], None),
    "lanczos_resize_source_validate": ([_PRD, _PRS], None),
    "lanczos_last_source_route": ([_P], None),
    "lanczos_resize_dest_init": ([_PRT, _PRD, _PRW, _I], None),
    "lanczos_resize_dest_validate": ([_PRD, _PRW, _PRT], None),
    "lanczos_last_dest_route": ([_P], None),
    "lanczos_tensor_norm_init": ([_PTN, _PRD, _I, _I], None),
    "lanczos_resize_tensor_norm_validate": ([_PRD, _PRW, _PTN], None),
    "lanczos_ycc_source_init": ([_PYS, _PRD, _I, _I, _I], None),
    "lanczos_ycc_source_validate": ([_PRD, _PYS], None),
    "lanczos_ycc_table": ([_I, _P], None),
    "lanczos_last_ycc_info": ([_P, ctypes.POINTER(YccInfoC)], None),
    "lanczos_ycc_dest_init": ([_PYD, _PRD, _PRW, _I, _I, _I], None),
    "lanczos_ycc_dest_validate": ([_PRD, _PRW, _PYD], None),
    "lanczos_ycc_table_forward": ([_I, _P], None),
    "lanczos_resize_ycc_out": ([_P, ctypes.POINTER(YccOutRequest)], None),
    "lanczos_last_ycc_out_info": ([_P, ctypes.POINTER(YccOutInfoC)], None),
    "lanczos_ycc16_matrix_init": ([ctypes.POINTER(Ycc16Matrix), _I, _I, _I, _I], None),
    "lanczos_ycc16_matrix_validate": ([ctypes.POINTER(Ycc16Matrix)], None),
    "lanczos_ycc16_source_init": ([_PYS, _PRD, _I, _I, _I], None),
    "lanczos_ycc16_source_validate": ([_PRD, _PYS], None),
    "lanczos_ycc16_dest_init": ([_PYD, _PRD, _PRW, _I, _I, _I], None),
    "lanczos_ycc16_dest_validate": ([_PRD, _PRW, _PYD], None),
    "lanczos_ycc16_request_validate": ([ctypes.POINTER(Ycc16Request)], None),
    "lanczos_resize_ycc16": ([_P, ctypes.POINTER(Ycc16Request)], None),
    "lanczos_last_ycc16_info": ([_P, ctypes.POINTER(Ycc16InfoC)], None),
}
for _device, _host, _head in _ENTRY_PAIRS:
    _SIGNATURES[_host] = ([_P] + _head + [_P, _P, _I], None)
    _SIGNATURES[_device] = (_SIGNATURES[_host][0] + [_Z, _Z, _P], None)

_LIB = None


def build(verbose=False):
    """Compile liblanczos_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", _HERE, "--no-print-directory"], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH) and not os.environ.get("LANCZOS_LIB"):
            try:  # a fresh checkout: compile the product (hipcc, ~40 s).  This is a build step, not a fallback.
                build()
            except Exception as e:
                raise RuntimeError(
                    f"{LIB_PATH} is missing and `make -C lanczos-hls_amd` failed ({e}); "
                    "there is no CPU fallback") from e
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C lanczos-hls_amd` "
                "(or __graft_entry__.build()); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(L, name, None)   # an older build of the ABI loaded through LANCZOS_LIB (A/B runs) lacks the later entries
            if fn is not None:
                fn.argtypes = argtypes
                if restype is not None:
                    fn.restype = restype
        _LIB = L
    return _LIB


def _check(rc, what):
    if rc != OK:
        raise LanczosError(rc, what)


def _ref(struct):
    """byref, or NULL for None"""
    return ctypes.byref(struct) if struct is not None else None


def make_desc(in_w, in_h, channels, scale_n, scale_d, a, bytes_per_sample=1, mode=MODE_LSB1,
              out_row0=0, out_rows=0, bit_precision=0):
    """bit_precision: BIT_PRECISION of the HLS mode's fixed-point emulation (lanczos_desc.reserved[0]; 0 = ideal arithmetic)."""
    d = Desc()
    _check(_lib().lanczos_desc_init(ctypes.byref(d), in_w, in_h, channels, bytes_per_sample,
                                    scale_n, scale_d, a), "lanczos_desc_init")
    d.mode = mode
    d.out_row0, d.out_rows = out_row0, out_rows
    d.reserved[0] = bit_precision
    _check(_lib().lanczos_validate(ctypes.byref(d)), "lanczos_validate")
    return d


def lanczos_kernel(x, a):
    """double lanczos_kernel(double x) of full_TB.h:51-53, LANCZOS_A as an argument."""
    return _lib().lanczos_kernel(float(x), int(a))


def lanczos_kernel_idx(in_idx, out_idx, scale_n, scale_d, a):
    """kernel_t lanczos_kernel(input_idx_t, output_idx_t, scale_t) of kernel.h:6 (double result)."""
    return _lib().lanczos_kernel_idx(in_idx, out_idx, scale_n, scale_d, a)


def inplace_rows(desc):
    return _lib().lanczos_inplace_rows(ctypes.byref(desc))


def strip_input_rows(desc, out_row0, out_rows):
    r0, n = ctypes.c_int(), ctypes.c_int()
    _check(_lib().lanczos_strip_input_rows(ctypes.byref(desc), out_row0, out_rows, ctypes.byref(r0),
                                           ctypes.byref(n)), "lanczos_strip_input_rows")
    return r0.value, n.value


def taps_host(desc, axis):
    n = desc.out_w if axis == 0 else desc.out_h
    first = np.empty(n, dtype=np.int32)
    w = np.empty((n, 2 * desc.a), dtype=np.float64)
    _check(_lib().lanczos_taps_host(ctypes.byref(desc), axis, first.ctypes.data, w.ctypes.data),
           "lanczos_taps_host")
    return first, w


def filter_code(filter):
    """FILTER_* of a filter given by name ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest") or as FILTER_*."""
    if isinstance(filter, str):
        if filter.lower() not in FILTER_NAMES:
            raise LanczosError(ERR_BAD_ARG, f"unknown filter {filter!r}: one of {', '.join(FILTER_NAMES)}")
        return FILTER_NAMES.index(filter.lower())
    return int(filter)


def resize_desc(in_w, in_h, out_w, out_h, channels, a=3, alpha=False, bits=8, f32=False, filter=FILTER_LANCZOS):
    """A validated lanczos_resize_desc (Pillow's contract: any output size, downscaling included).  alpha: the fourth of
    four channels is straight alpha, resized as Pillow's mode RGBA (premultiplied inside the kernels).  bits: 8, or 16 for
    uint16 samples resized as Pillow's mode I;16 (double accumulation, Pillow's wrapping store); not with alpha.  f32: float
    samples resized as Pillow's mode F (double accumulation, stored as float, no clamp); not with alpha or bits=16.
    filter: Image.resize's `resample`, a name or FILTER_*; every filter but Lanczos needs a == 3 (ERR_BAD_ARG otherwise), and
    "nearest" gathers whole pixels (no premultiply with alpha; ERR_UNSUPPORTED with bits=16)."""
    if bits not in (8, 16):
        raise LanczosError(ERR_BAD_ARG, "resize_desc: bits must be 8 or 16")
    d = ResizeDesc()
    flags = (RESIZE_ALPHA if alpha else 0) | (RESIZE_U16 if bits == 16 else 0) | (RESIZE_F32 if f32 else 0)
    f = filter_code(filter)
    if f == FILTER_LANCZOS:
        _check(_lib().lanczos_resize_desc_init_ex(ctypes.byref(d), in_w, in_h, out_w, out_h, channels, a, flags),
               "lanczos_resize_desc_init_ex")
        return d
    if a != 3:
        raise LanczosError(ERR_BAD_ARG, "resize_desc: a filter other than Lanczos takes a = 3")
    _check(_lib().lanczos_resize_desc_init_filter(ctypes.byref(d), in_w, in_h, out_w, out_h, channels, f, flags),
           "lanczos_resize_desc_init_filter")
    return d


def resize_opts(desc, box=None, reducing_gap=None):
    """A lanczos_resize_opts for `desc`: box = (x0, y0, x1, y1) in source pixels (None = the whole frame), reducing_gap as
    Pillow's Image.resize takes it (None = none).  Validated where it is used."""
    o = ResizeOpts()
    _check(_lib().lanczos_resize_opts_init(ctypes.byref(o), ctypes.byref(desc)), "lanczos_resize_opts_init")
    if box is not None:
        if len(box) != 4:
            raise LanczosError(ERR_BAD_ARG, "resize_opts: box is (x0, y0, x1, y1)")
        for i in range(4):
            o.box[i] = float(box[i])
    if reducing_gap is not None:
        # 0 means "none" in the C struct; a caller who passes 0 gets what Pillow gives for it, an error
        o.reducing_gap = float(reducing_gap) if float(reducing_gap) != 0.0 else float("nan")
    return o


def _opts_ref(desc, box, reducing_gap, opts):
    if opts is None and (box is not None or reducing_gap is not None):
        opts = resize_opts(desc, box, reducing_gap)
    return _ref(opts)


def _resize_taps(entry, coeff_dtype, desc, axis, box, reducing_gap, opts):
    """the body of resize_taps_host / resize_taps_f64_host: `entry`, or `entry`_ex with options, asked for ksize, then for the tables"""
    ks = ctypes.c_int()
    if box is None and reducing_gap is None and opts is None:
        fn = lambda *a: getattr(_lib(), entry)(ctypes.byref(desc), axis, *a)
    else:
        ref = _opts_ref(desc, box, reducing_gap, opts)
        fn = lambda *a: getattr(_lib(), entry + "_ex")(ctypes.byref(desc), ref, axis, *a)
    _check(fn(None, None, None, ctypes.byref(ks)), entry)
    n = desc.out_w if axis == 0 else desc.out_h
    first = np.empty(n, dtype=np.int32)
    count = np.empty(n, dtype=np.int32)
    coeffs = np.empty((n, ks.value), dtype=coeff_dtype)
    _check(fn(first.ctypes.data, count.ctypes.data, coeffs.ctypes.data, ctypes.byref(ks)), entry)
    return first, count, coeffs


def resize_taps_host(desc, axis, box=None, reducing_gap=None, opts=None):
    """Fixed-point tables of one axis (0 = horizontal, 1 = vertical): (first[out], count[out], coeffs[out][ksize]) int32.
    With a box and / or a gap (or a ready ResizeOpts) the tables of the resize that remains: lanczos_resize_taps_host_ex."""
    return _resize_taps("lanczos_resize_taps_host", np.int32, desc, axis, box, reducing_gap, opts)


def resize_taps_f64_host(desc, axis, box=None, reducing_gap=None, opts=None):
    """Double tables of one axis, what 16-bit and float requests run on: (first[out] int32, count[out] int32, coeffs[out][ksize]
    float64); first and count are those of resize_taps_host.  box / reducing_gap / opts as resize_taps_host."""
    return _resize_taps("lanczos_resize_taps_f64_host", np.float64, desc, axis, box, reducing_gap, opts)


def resize_plan_host(desc, frames=1, box=None, reducing_gap=None, opts=None):
    """The launch plan of a resize under RESIZE_AUTO (no GPU needed): a ResizePlan, fused = 0 for the two-pass path.  With a
    box and / or a gap (or a ready ResizeOpts): a ResizePlanEx -- the reduction (fx, fy, safe_box, reduced_w / reduced_h), the
    box that remains (inner_box), the passes that run, the rows of the two-pass intermediate, and the inner ResizePlan."""
    if box is None and reducing_gap is None and opts is None:
        p = ResizePlan()
        _check(_lib().lanczos_resize_plan_host(ctypes.byref(desc), frames, ctypes.byref(p)), "lanczos_resize_plan_host")
        return p
    p = ResizePlanEx()
    _check(_lib().lanczos_resize_plan_host_ex(ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts), frames,
                                              ctypes.byref(p)), "lanczos_resize_plan_host_ex")
    return p


def resize_window(desc, window=None):
    """A validated ResizeWindow for `desc`: window = (x0, y0, w, h) in output pixels of the full request, inside its output
    (ERR_BAD_ARG otherwise); None = the whole output.  A ready ResizeWindow is validated and returned."""
    if isinstance(window, ResizeWindow):
        win = window
    else:
        win = ResizeWindow()
        _check(_lib().lanczos_resize_window_init(ctypes.byref(win), ctypes.byref(desc)), "lanczos_resize_window_init")
        if window is not None:
            if len(window) != 4:
                raise LanczosError(ERR_BAD_ARG, "resize_window: window is (x0, y0, w, h)")
            win.x0, win.y0, win.w, win.h = (int(v) for v in window)
    _check(_lib().lanczos_resize_window_validate(ctypes.byref(desc), ctypes.byref(win)), "lanczos_resize_window_validate")
    return win


def _window_ref(desc, window):
    return ctypes.byref(resize_window(desc, window)) if window is not None else None


def resize_window_source(desc, window=None, box=None, reducing_gap=None, opts=None):
    """(x0, y0, x1, y1), half open: the source rectangle the windowed request reads (lanczos_resize_window_source).  With a
    reducing_gap that reduces it is the safe box, whatever the window."""
    rect = (ctypes.c_int32 * 4)()
    _check(_lib().lanczos_resize_window_source(ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                               _window_ref(desc, window), rect), "lanczos_resize_window_source")
    return tuple(rect)


def resize_window_plan_host(desc, window=None, frames=1, box=None, reducing_gap=None, opts=None):
    """The ResizePlanEx of the windowed request (no GPU needed): mid_row0 / mid_rows are the rows the window's vertical taps
    read, inner is the fused plan of a w x h output.  The whole output gives resize_plan_host's ResizePlanEx."""
    p = ResizePlanEx()
    _check(_lib().lanczos_resize_window_plan_host(ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                  _window_ref(desc, window), frames, ctypes.byref(p)),
           "lanczos_resize_window_plan_host")
    return p


def resize_crops(w, h, d_origin):
    """A ResizeCrops: every frame stores the w x h window of its resize whose origin is its pair (x0, y0) of the int32 array
    at d_origin (device memory for the device entry, 4-byte aligned), clamped so that the window lies inside the output.
    Validated where it is used (resize_crops_validate)."""
    c = ResizeCrops()
    c.w, c.h, c.d_origin = int(w), int(h), d_origin
    return c


def resize_crops_validate(desc, crops, view=None):
    """lanczos_resize_crops_validate, or with a TensorView lanczos_resize_tensor_crops_validate (the view's strides describe the
    w x h frame): raises LanczosError where the request is refused."""
    cp = _ref(crops)
    if view is None:
        _check(_lib().lanczos_resize_crops_validate(ctypes.byref(desc), cp), "lanczos_resize_crops_validate")
    else:
        _check(_lib().lanczos_resize_tensor_crops_validate(ctypes.byref(desc), cp, ctypes.byref(view)),
               "lanczos_resize_tensor_crops_validate")


def resize_crops_plan_host(desc, crops, frames=1, box=None, reducing_gap=None, opts=None):
    """The ResizePlanEx of a crops request (no GPU needed; d_origin is not read): inner.ring_rows and inner.stage_dw are the
    largest resize_window_plan_host reports for (x0, y0, w, h) over every origin inside the output, and inner.fused is 0 where
    those do not fit.  crops: a ResizeCrops or (w, h)."""
    if not isinstance(crops, ResizeCrops):
        dummy = (ctypes.c_int32 * 2)()
        crops = resize_crops(crops[0], crops[1], ctypes.addressof(dummy))
    p = ResizePlanEx()
    _check(_lib().lanczos_resize_crops_plan_host(ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                 ctypes.byref(crops), frames, ctypes.byref(p)), "lanczos_resize_crops_plan_host")
    return p


def _layout_struct(cls, what, layout, row_stride, chan_stride, init, rows):
    """the body of resize_source / resize_dest: init(struct, code) fills the tight layout, rows() is the height of one plane"""
    if isinstance(layout, cls):
        return layout
    kinds = {"interleaved": SOURCE_INTERLEAVED, "planar": SOURCE_PLANAR}   # DEST_* are the same codes
    if layout not in kinds:
        raise LanczosError(ERR_BAD_ARG, f"{what}: layout is 'planar' or 'interleaved', not {layout!r}")
    s = cls()
    _check(init(ctypes.byref(s), kinds[layout]), f"lanczos_{what}_init")
    if row_stride is not None:
        if chan_stride is None and layout == "planar":   # the planes stay back to back
            chan_stride = int(row_stride) * rows()
        s.row_stride = int(row_stride)
    if chan_stride is not None:
        s.chan_stride = int(chan_stride)
    return s


def resize_source(desc, layout="planar", row_stride=None, chan_stride=None):
    """A ResizeSource for `desc`: layout "planar" (N x C x H x W bytes, what torchvision.io.decode_jpeg(device=) returns) or
    "interleaved"; row_stride / chan_stride in bytes replace the tight layout's (pitched rows, padded planes).  Validated where it
    is used (resize_source_validate); a ready ResizeSource is returned as it is."""
    return _layout_struct(ResizeSource, "resize_source", layout, row_stride, chan_stride,
                          lambda s, kind: _lib().lanczos_resize_source_init(s, ctypes.byref(desc), kind), lambda: desc.in_h)


def resize_source_validate(desc, source):
    """lanczos_resize_source_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the layout is refused."""
    _check(_lib().lanczos_resize_source_validate(ctypes.byref(desc), _ref(source)),
           "lanczos_resize_source_validate")


def resize_dest(desc, layout="planar", row_stride=None, chan_stride=None, window=None):
    """A ResizeDest for the result of `desc` (its window, where one is given): layout "planar" (N x C x H x W bytes, what a torch
    stage takes) or "interleaved"; row_stride / chan_stride in bytes replace the tight layout's (pitched rows, padded planes).
    Validated where it is used (resize_dest_validate); a ready ResizeDest is returned as it is."""
    return _layout_struct(ResizeDest, "resize_dest", layout, row_stride, chan_stride,
                          lambda t, kind: _lib().lanczos_resize_dest_init(t, ctypes.byref(desc), _window_ref(desc, window), kind),
                          lambda: resize_window(desc, window).h)


def resize_dest_validate(desc, dest, window=None):
    """lanczos_resize_dest_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the layout is refused."""
    _check(_lib().lanczos_resize_dest_validate(ctypes.byref(desc), _window_ref(desc, window),
                                               _ref(dest)), "lanczos_resize_dest_validate")


def ycc_source(desc, layout="nv12", sub_x=None, sub_y=None, y_row_stride=None, c_row_stride=None, cb_offset=None, cr_offset=None):
    """A validated YccSource for the frames `desc` resizes (desc: three channels, in_w x in_h the luma size).  layout: a name
    of YCC_LAYOUTS ("nv12", "nv21", "i420", "i422", "i444"), or YCC_PLANAR / YCC_NV12 / YCC_NV21 with sub_x and sub_y given.
    The defaults are the tight layout (Y, then Cb, then Cr or the interleaved plane, rows packed); strides and offsets in
    bytes replace them one by one.  ycc_frame_bytes gives the frame's extent."""
    if isinstance(layout, str):
        if layout.lower() not in YCC_LAYOUTS:
            raise LanczosError(ERR_BAD_ARG, f"ycc_source: layout is one of {', '.join(YCC_LAYOUTS)}, not {layout!r}")
        code, sx, sy = YCC_LAYOUTS[layout.lower()]
        sub_x, sub_y = (sx if sub_x is None else sub_x), (sy if sub_y is None else sub_y)
    else:
        code = int(layout)
        if sub_x is None or sub_y is None:
            raise LanczosError(ERR_BAD_ARG, "ycc_source: a layout given by its code needs sub_x and sub_y")
    s = YccSource()
    _check(_lib().lanczos_ycc_source_init(ctypes.byref(s), ctypes.byref(desc), code, int(sub_x), int(sub_y)), "lanczos_ycc_source_init")
    for name, v in (("y_row_stride", y_row_stride), ("c_row_stride", c_row_stride), ("cb_offset", cb_offset), ("cr_offset", cr_offset)):
        if v is not None:
            setattr(s, name, int(v))
    if code != YCC_PLANAR and cb_offset is not None and cr_offset is None:
        s.cr_offset = s.cb_offset
    _check(_lib().lanczos_ycc_source_validate(ctypes.byref(desc), ctypes.byref(s)), "lanczos_ycc_source_validate")
    return s


def ycc_source_validate(desc, source):
    _check(_lib().lanczos_ycc_source_validate(ctypes.byref(desc), _ref(source)),
           "lanczos_ycc_source_validate")


def ycc_chroma_size(desc, source):
    """(cw, ch): the size of the chroma planes"""
    return (desc.in_w + source.sub_x) >> source.sub_x, (desc.in_h + source.sub_y) >> source.sub_y


def ycc_frame_bytes(desc, source):
    """The extent of one frame in `source`'s layout: the end of its last plane, every plane holding its full pitched rows."""
    cw, ch = ycc_chroma_size(desc, source)
    return max(desc.in_h * source.y_row_stride, source.cb_offset + ch * source.c_row_stride, source.cr_offset + ch * source.c_row_stride)


def ycc_table(standard="jfif"):
    """int32 [3][3][256], t[c][k][v]: out[c] = clip8((t[c][0][y] + t[c][1][cb] + t[c][2][cr]) >> 6).  "jfif" is Pillow's
    convert("RGB") exactly; "bt601" and "bt709" are the limited-range matrices (lanczos_ycc_table).  Any other matrix or
    channel order is an array of this shape built by the caller."""
    code = YCC_STANDARDS.get(standard.lower()) if isinstance(standard, str) else int(standard)
    if code is None:
        raise LanczosError(ERR_BAD_ARG, f"ycc_table: standard is one of {', '.join(YCC_STANDARDS)}, not {standard!r}")
    t = np.empty((3, 3, 256), dtype=np.int32)
    _check(_lib().lanczos_ycc_table(code, t.ctypes.data), "lanczos_ycc_table")
    return t


def _ycc_layout_arg(layout, sub_x, sub_y, what, layouts=YCC_LAYOUTS):
    """(code, sub_x, sub_y) of a layout given by a name of YCC_LAYOUTS or by its code with both subsamplings"""
    if isinstance(layout, str):
        if layout.lower() not in layouts:
            raise LanczosError(ERR_BAD_ARG, f"{what}: layout is one of {', '.join(layouts)}, not {layout!r}")
        code, sx, sy = layouts[layout.lower()]
        return code, (sx if sub_x is None else int(sub_x)), (sy if sub_y is None else int(sub_y))
    if sub_x is None or sub_y is None:
        raise LanczosError(ERR_BAD_ARG, f"{what}: a layout given by its code needs sub_x and sub_y")
    return int(layout), int(sub_x), int(sub_y)


def ycc_dest(desc, layout="nv12", window=None, sub_x=None, sub_y=None, y_row_stride=None, c_row_stride=None, cb_offset=None,
             cr_offset=None, aligned=True):
    """A validated YccDest for the frame a call with `desc` stores: its whole output, or `window` = (x0, y0, w, h) of it.
    layout as ycc_source takes it.  The defaults are the tight layout (Y, then Cb, then Cr or the interleaved plane, rows
    packed); strides and offsets in bytes replace them one by one.  aligned=False: the window origin is not checked against the
    subsampling (RGB frames may be cut anywhere).  ycc_dest_frame_bytes gives the frame's extent."""
    code, sx, sy = _ycc_layout_arg(layout, sub_x, sub_y, "ycc_dest")
    win = resize_window(desc, window)
    t = YccDest()
    _check(_lib().lanczos_ycc_dest_init(ctypes.byref(t), ctypes.byref(desc), ctypes.byref(win), code, sx, sy), "lanczos_ycc_dest_init")
    for name, v in (("y_row_stride", y_row_stride), ("c_row_stride", c_row_stride), ("cb_offset", cb_offset), ("cr_offset", cr_offset)):
        if v is not None:
            setattr(t, name, int(v))
    if code != YCC_PLANAR and cb_offset is not None and cr_offset is None:
        t.cr_offset = t.cb_offset
    if not aligned:   # validated at the window's size: the layout's rules without the origin's
        win = resize_window(desc, (0, 0, win.w, win.h))
    _check(_lib().lanczos_ycc_dest_validate(ctypes.byref(desc), ctypes.byref(win), ctypes.byref(t)), "lanczos_ycc_dest_validate")
    return t


def ycc_dest_validate(desc, dest, window=None):
    """lanczos_ycc_dest_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the layout is refused."""
    _check(_lib().lanczos_ycc_dest_validate(ctypes.byref(desc), _window_ref(desc, window), _ref(dest)), "lanczos_ycc_dest_validate")


def ycc_dest_chroma_size(desc, dest, window=None):
    """(ocw, och): the size of the stored chroma planes"""
    win = resize_window(desc, window)
    return (win.w + dest.sub_x) >> dest.sub_x, (win.h + dest.sub_y) >> dest.sub_y


def ycc_dest_frame_bytes(desc, dest, window=None):
    """The extent of one frame in `dest`'s layout: the end of its last plane, every plane holding its full pitched rows."""
    win = resize_window(desc, window)
    ch = (win.h + dest.sub_y) >> dest.sub_y
    return max(win.h * dest.y_row_stride, dest.cb_offset + ch * dest.c_row_stride, dest.cr_offset + ch * dest.c_row_stride)


def ycc_table_forward(standard="jfif"):
    """int32 [3][3][256], t[c][k][v]: out[c] = clip8((t[c][0][R] + t[c][1][G] + t[c][2][B]) >> 6), c = Y, Cb, Cr.  "jfif" is
    Pillow's convert("YCbCr") exactly; "bt601" and "bt709" are the limited-range matrices (lanczos_ycc_table_forward)."""
    code = YCC_STANDARDS.get(standard.lower()) if isinstance(standard, str) else int(standard)
    if code is None:
        raise LanczosError(ERR_BAD_ARG, f"ycc_table_forward: standard is one of {', '.join(YCC_STANDARDS)}, not {standard!r}")
    t = np.empty((3, 3, 256), dtype=np.int32)
    _check(_lib().lanczos_ycc_table_forward(code, t.ctypes.data), "lanczos_ycc_table_forward")
    return t


def ycc_out_request(desc, dest, in_ptr, out_ptr, frames, source=None, table=None, opts=None, window=None, memory=MEM_DEVICE,
                    in_frame_stride=0, out_frame_stride=0, stream=None):
    """A YccOutRequest over ready structs (None: NULL) and addresses; the structs stay alive with it."""
    rq = YccOutRequest()
    rq._keep = (desc, dest, source, opts, window)
    for name, v in (("d", desc), ("opts", opts), ("win", window), ("src", source), ("dst", dest)):
        setattr(rq, name, ctypes.addressof(v) if v is not None else None)
    rq.table, rq.in_, rq.out, rq.frames, rq.memory = table, in_ptr, out_ptr, int(frames), int(memory)
    rq.in_frame_stride, rq.out_frame_stride, rq.stream = int(in_frame_stride), int(out_frame_stride), stream
    return rq


def ycc16_matrix(standard="bt709", depth=10, msb_aligned=True, full_range=False):
    """A Ycc16Matrix of a standard ("jfif" and "bt601": the BT.601 constants; "bt709"; "bt2020") for words that hold `depth`
    bits (8 .. 16), MSB-aligned as in P010 or LSB-aligned as in yuv420p10le, limited or full range, scaled to RGB words of
    0 .. 65535 (lanczos_ycc16_matrix_init).  Any other matrix is a Ycc16Matrix the caller fills in."""
    code = YCC16_STANDARDS.get(standard.lower()) if isinstance(standard, str) else int(standard)
    if code is None:
        raise LanczosError(ERR_BAD_ARG, f"ycc16_matrix: standard is one of {', '.join(YCC16_STANDARDS)}, not {standard!r}")
    m = Ycc16Matrix()
    _check(_lib().lanczos_ycc16_matrix_init(ctypes.byref(m), code, int(depth), int(bool(msb_aligned)), int(bool(full_range))),
           "lanczos_ycc16_matrix_init")
    return m


def ycc16_matrix_validate(matrix):
    _check(_lib().lanczos_ycc16_matrix_validate(_ref(matrix)), "lanczos_ycc16_matrix_validate")


def _ycc16_fill(s, layout_code, y_row_stride, c_row_stride, cb_offset, cr_offset):
    for name, v in (("y_row_stride", y_row_stride), ("c_row_stride", c_row_stride), ("cb_offset", cb_offset), ("cr_offset", cr_offset)):
        if v is not None:
            setattr(s, name, int(v))
    if layout_code != YCC_PLANAR and cb_offset is not None and cr_offset is None:
        s.cr_offset = s.cb_offset


def ycc16_source(desc, layout="p010", sub_x=None, sub_y=None, y_row_stride=None, c_row_stride=None, cb_offset=None, cr_offset=None):
    """A validated YccSource for frames of 16-bit words (desc: resize_desc(..., 3, bits=16), in_w x in_h the luma size).  layout: a
    name of YCC16_LAYOUTS (those of ycc_source, "p010" / "p016" for the nv12 shape, "p210" / "p216" / "nv16" for 4:2:2 pairs) or a
    code with sub_x and sub_y.  Strides and offsets are BYTES, multiples of 2; the defaults are the tight layout."""
    code, sx, sy = _ycc_layout_arg(layout, sub_x, sub_y, "ycc16_source", YCC16_LAYOUTS)
    s = YccSource()
    _check(_lib().lanczos_ycc16_source_init(ctypes.byref(s), ctypes.byref(desc), code, sx, sy), "lanczos_ycc16_source_init")
    _ycc16_fill(s, code, y_row_stride, c_row_stride, cb_offset, cr_offset)
    _check(_lib().lanczos_ycc16_source_validate(ctypes.byref(desc), ctypes.byref(s)), "lanczos_ycc16_source_validate")
    return s


def ycc16_source_validate(desc, source):
    _check(_lib().lanczos_ycc16_source_validate(ctypes.byref(desc), _ref(source)), "lanczos_ycc16_source_validate")


def ycc16_dest(desc, layout="p010", window=None, sub_x=None, sub_y=None, y_row_stride=None, c_row_stride=None, cb_offset=None,
               cr_offset=None):
    """A validated YccDest for the frame of 16-bit words a call with `desc` stores: its whole output, or `window` = (x0, y0, w, h)
    of it, the origin a multiple of the subsampling.  layout as ycc16_source takes it; strides and offsets in BYTES, multiples of
    2.  ycc_dest_frame_bytes gives the frame's extent."""
    code, sx, sy = _ycc_layout_arg(layout, sub_x, sub_y, "ycc16_dest", YCC16_LAYOUTS)
    win = resize_window(desc, window)
    t = YccDest()
    _check(_lib().lanczos_ycc16_dest_init(ctypes.byref(t), ctypes.byref(desc), ctypes.byref(win), code, sx, sy), "lanczos_ycc16_dest_init")
    _ycc16_fill(t, code, y_row_stride, c_row_stride, cb_offset, cr_offset)
    _check(_lib().lanczos_ycc16_dest_validate(ctypes.byref(desc), ctypes.byref(win), ctypes.byref(t)), "lanczos_ycc16_dest_validate")
    return t


def ycc16_dest_validate(desc, dest, window=None):
    _check(_lib().lanczos_ycc16_dest_validate(ctypes.byref(desc), _window_ref(desc, window), _ref(dest)), "lanczos_ycc16_dest_validate")


def ycc16_request(desc, source, in_ptr, out_ptr, frames, dest=None, matrix=None, norm=None, opts=None, window=None, memory=MEM_DEVICE,
                  in_frame_stride=0, out_frame_stride=0, stream=None):
    """A Ycc16Request over ready structs (None: NULL) and addresses; the structs stay alive with it."""
    rq = Ycc16Request()
    rq._keep = (desc, source, dest, matrix, norm, opts, window)
    for name, v in (("d", desc), ("opts", opts), ("win", window), ("src", source), ("dst", dest), ("matrix", matrix), ("norm", norm)):
        setattr(rq, name, ctypes.addressof(v) if v is not None else None)
    rq.in_, rq.out, rq.frames, rq.memory = in_ptr, out_ptr, int(frames), int(memory)
    rq.in_frame_stride, rq.out_frame_stride, rq.stream = int(in_frame_stride), int(out_frame_stride), stream
    return rq


def ycc16_request_validate(rq):
    """lanczos_ycc16_request_validate: raises LanczosError with the code lanczos_resize_ycc16 would refuse the request with"""
    _check(_lib().lanczos_ycc16_request_validate(_ref(rq)), "lanczos_ycc16_request_validate")


def _ycc_table_arg(standard, table, what, forward=False):
    if table is None:
        return ycc_table_forward(standard) if forward else ycc_table(standard)
    table = np.ascontiguousarray(table)
    if table.dtype != np.int32 or table.shape != (3, 3, 256):
        raise LanczosError(ERR_BAD_ARG, f"{what}: the colour table is int32 [3][3][256]")
    return table


def _frames(img, dtypes, what, planar=False):
    """An image as the host wrappers take it -- [H][W], [H][W][C] or [F][H][W][C], with planar [C][H][W] or [F][C][H][W] -- of
    one of `dtypes`: (the contiguous 4-D array, (f, h, w, c), back), where back(out) gives a 4-D result the axes img had;
    back(out, True) keeps the channel axis of a 2-D image, as the tensor calls do."""
    img = np.ascontiguousarray(img)
    if img.dtype not in dtypes or img.ndim not in ((3, 4) if planar else (2, 3, 4)):
        names = " or ".join(np.dtype(t).name for t in dtypes)
        if planar:
            raise LanczosError(ERR_BAD_ARG, f"{what}: planar=True takes a {names} [C][H][W] or [F][C][H][W] array")
        raise LanczosError(ERR_BAD_ARG, f"{what}: expected a {names} [H][W], [H][W][C] or [F][H][W][C] array")
    ndim = img.ndim
    x = img.reshape(img.shape + (1,)) if ndim == 2 else img
    x = x if x.ndim == 4 else x[None]
    f, h, w, c = (x.shape[0], x.shape[2], x.shape[3], x.shape[1]) if planar else x.shape

    def back(out, keep_channels=False):
        if ndim == 2 and not keep_channels:
            return out[0, :, :, 0]
        return out if ndim == 4 else out[0]
    return x, (f, h, w, c), back


def center_window(out_w, out_h, w, h):
    """The window (x0, y0, w, h) torchvision's CenterCrop((h, w)) takes out of an out_h x out_w image: the origin is
    int(round((out - crop) / 2.0)) per axis with Python's round (a tie goes to the even integer).  A crop larger than the
    output raises ERR_BAD_ARG: CenterCrop would pad there, which is no window."""
    if not (1 <= w <= out_w and 1 <= h <= out_h):
        raise LanczosError(ERR_BAD_ARG, f"center_window: a {w} x {h} crop of a {out_w} x {out_h} output")
    return int(round((out_w - w) / 2.0)), int(round((out_h - h) / 2.0)), int(w), int(h)


def _tensor16_format(dtype, what):
    if dtype not in _TENSOR16_FORMATS:
        raise LanczosError(ERR_BAD_ARG, f"{what}: dtype is 'float32', 'bfloat16' or 'float16', not {dtype!r}")
    return _TENSOR16_FORMATS[dtype]


def _tensor16_array(words, dtype):
    """the words of a 16-bit table or tensor as the caller sees them: np.float16, or the bfloat16 patterns as np.uint16"""
    return words.view(np.float16) if dtype == "float16" else words


def lut_convert16(array, dtype):
    """float32 values -> "bfloat16" (np.uint16 holding the patterns: numpy has no bfloat16) or "float16" (np.float16) of the
    same shape, rounded to nearest-even as torch's .to(torch.bfloat16) / .to(torch.float16) rounds on the CPU."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    out = np.empty(a.shape, dtype=np.uint16)
    _check(_lib().lanczos_tensor_lut_convert16(a.ctypes.data, a.size, _tensor16_format(dtype, "lut_convert16"),
                                               out.ctypes.data), "lanczos_tensor_lut_convert16")
    return _tensor16_array(out, dtype)


def normalize_lut(channels, mean=None, std=None, dtype="float32"):
    """The table of ToTensor() + Normalize(mean, std) as float32 [channels][256]: ((float)v / 255 - mean[c]) / std[c] in IEEE
    float, bit for bit torch's uint8.to(float32).div(255).sub(mean).div(std).  mean=None is 0, std=None is 1.
    dtype="bfloat16" / "float16": that table rounded as lut_convert16 rounds it (np.uint16 patterns / np.float16), bit for bit
    torch's .to(torch.bfloat16) / .to(torch.float16) of the float32 result."""
    def arr(v, what):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float32)
        if a.shape not in ((), (channels,)):
            raise LanczosError(ERR_BAD_ARG, f"normalize_lut: {what} is one value, or one per channel")
        return np.ascontiguousarray(np.broadcast_to(a, (channels,)))
    m, s = arr(mean, "mean"), arr(std, "std")
    if dtype != "float32":
        lut = np.empty((channels, 256), dtype=np.uint16)
        _check(_lib().lanczos_tensor16_lut_normalize(channels, m.ctypes.data if m is not None else None,
                                                     s.ctypes.data if s is not None else None,
                                                     _tensor16_format(dtype, "normalize_lut"), lut.ctypes.data),
               "lanczos_tensor16_lut_normalize")
        return _tensor16_array(lut, dtype)
    lut = np.empty((channels, 256), dtype=np.float32)
    _check(_lib().lanczos_tensor_lut_normalize(channels, m.ctypes.data if m is not None else None,
                                               s.ctypes.data if s is not None else None, lut.ctypes.data),
           "lanczos_tensor_lut_normalize")
    return lut


def tensor_strides(layout, out_w, out_h, channels):
    """(chan_stride, row_stride, pix_stride) in elements of a tightly packed "chw" or "hwc" frame."""
    if layout == "chw":
        return out_h * out_w, out_w, 1
    if layout == "hwc":
        return 1, out_w * channels, channels
    raise LanczosError(ERR_BAD_ARG, f"unknown layout {layout!r}: chw or hwc")


def _flip_arg(flip, frames, what):
    """The flip of a host tensor call, None / "h" / "v" / "hv" or one integer per frame: (the bits for every frame, the uint8
    array of one entry per frame or None)."""
    if flip is not None and not isinstance(flip, str):
        flips = np.ascontiguousarray(flip)
        if flips.shape != (frames,) or flips.dtype.kind not in "iub" or ((flips < 0) | (flips > 3)).any():
            raise LanczosError(ERR_BAD_ARG, f"{what}: flip is 'h', 'v', 'hv' or {frames} integers 0 .. 3, one per frame")
        return 0, flips.astype(np.uint8)
    if flip not in _FLIP_NAMES:
        raise LanczosError(ERR_BAD_ARG, f"{what}: flip is 'h', 'v', 'hv' or one integer per frame, not {flip!r}")
    return _FLIP_NAMES[flip], None


def _lut_arg(lut, mean, std, c, dtype, what):
    """The table of a host tensor call for c output channels, contiguous: the caller's, or normalize_lut(c, mean, std, dtype)."""
    wide = dtype == "float32"
    if lut is None:
        if c == 2:   # lanczos_tensor_lut_normalize builds 1, 3 or 4 channels: two rows of one
            m, s = (None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float32), (2,)) for v in (mean, std))
            lut = np.concatenate([normalize_lut(1, None if m is None else m[k], None if s is None else s[k], dtype)
                                  for k in range(2)])
        else:
            lut = normalize_lut(c, mean, std, dtype)
    elif mean is not None or std is not None:
        raise LanczosError(ERR_BAD_ARG, f"{what}: a table or mean / std, not both")
    lut = np.ascontiguousarray(lut)
    if lut.dtype not in ((np.float32,) if wide else (np.uint16, np.float16)) or lut.size != c * 256:
        raise LanczosError(ERR_BAD_ARG, f"{what}: the table is {'float32' if wide else 'uint16 or float16'} [{c}][256]")
    return lut


def _tensor_out(cls, d_lut, strides):
    t = cls()
    t.d_lut = d_lut
    t.chan_stride, t.row_stride, t.pix_stride = (int(v) for v in strides)
    return t


def _fill_view(s, strides, src, flip, d_flip):
    """what TensorView and TensorNorm share: the strides, the channel map and the flips"""
    s.chan_stride, s.row_stride, s.pix_stride = (int(x) for x in strides)
    s.out_channels = len(src)
    for oc, sc in enumerate(src):
        s.src_channel[oc] = sc
    s.flip = _FLIP_NAMES[flip] if flip in _FLIP_NAMES else int(flip)
    s.d_flip = d_flip
    return s


def tensor_out(d_lut, strides):
    """A TensorOut: d_lut a pointer to channels * 256 floats (device memory for the device entry), strides =
    (chan_stride, row_stride, pix_stride) in floats.  Validated where it is used (resize_tensor_validate)."""
    return _tensor_out(TensorOut, d_lut, strides)


def tensor16_out(d_lut, strides):
    """A TensorOut16: d_lut a pointer to channels * 256 16-bit words (device memory for the device entry), strides =
    (chan_stride, row_stride, pix_stride) in elements.  Validated where it is used (resize_tensor16_validate)."""
    return _tensor_out(TensorOut16, d_lut, strides)


def tensor_view_init(desc, elem_bytes=4):
    """lanczos_tensor_view_init: the identity over every channel, CHW strides of the whole output, no flips, d_lut NULL."""
    v = TensorView()
    _check(_lib().lanczos_tensor_view_init(ctypes.byref(v), ctypes.byref(desc), elem_bytes), "lanczos_tensor_view_init")
    return v


def tensor_view(d_lut, strides, elem_bytes=4, channels_out=(0, 1, 2), flip=0, d_flip=None):
    """A TensorView: d_lut a pointer to len(channels_out) * 256 elements of elem_bytes (4: float32, 2: bfloat16 / float16
    words), indexed by the OUTPUT channel; strides = (chan_stride, row_stride, pix_stride) in elements; channels_out the
    source channel of every output channel, e.g. (2, 1, 0) or (0, 1, 2) of an RGBA frame; flip FLIP_H | FLIP_V bits (or "h",
    "v", "hv") for every frame; d_flip a pointer to one such byte per frame, XORed with flip, or None.  Both pointers are
    device memory for the device entry.  Validated where it is used (resize_tensor_view_validate)."""
    v = TensorView()
    v.d_lut = d_lut
    v.elem_bytes = int(elem_bytes)
    src = [int(c) for c in channels_out]
    if len(src) > 4:
        raise LanczosError(ERR_BAD_ARG, "tensor_view: at most four output channels")
    return _fill_view(v, strides, src, flip, d_flip)


def tensor_norm_init(desc, dtype="float32", layout="chw"):
    """lanczos_tensor_norm_init: the identity over every channel, the tight "chw" or "hwc" strides of the whole output, no
    flips, div = 1, mean = 0, std = 1."""
    n = TensorNorm()
    if dtype not in _TENSOR_NORM_FORMATS or layout not in ("chw", "hwc"):
        raise LanczosError(ERR_BAD_ARG, f"tensor_norm_init: dtype float32 / bfloat16 / float16 and layout chw / hwc, not {dtype!r}, {layout!r}")
    _check(_lib().lanczos_tensor_norm_init(ctypes.byref(n), ctypes.byref(desc), _TENSOR_NORM_FORMATS[dtype],
                                           TENSOR_CHW if layout == "chw" else TENSOR_HWC), "lanczos_tensor_norm_init")
    return n


def tensor_norm(strides, div=1.0, mean=0.0, std=1.0, dtype="float32", channels_out=(0, 1, 2), flip=0, d_flip=None):
    """A TensorNorm: strides = (chan_stride, row_stride, pix_stride) in elements; div / mean / std one value or one per OUTPUT
    channel (float32: they are used as given, torch's .div(div).sub(mean).div(std)); dtype "float32", "bfloat16" or "float16";
    channels_out, flip and d_flip as tensor_view.  Validated where it is used (resize_tensor_norm_validate)."""
    n = TensorNorm()
    if dtype not in _TENSOR_NORM_FORMATS:
        raise LanczosError(ERR_BAD_ARG, f"tensor_norm: dtype is 'float32', 'bfloat16' or 'float16', not {dtype!r}")
    src = [int(c) for c in channels_out]
    if not 1 <= len(src) <= 4:
        raise LanczosError(ERR_BAD_ARG, "tensor_norm: one to four output channels")
    for name, v in (("div", div), ("mean", mean), ("std", std)):
        a = np.asarray(v, dtype=np.float32)
        if a.shape not in ((), (len(src),)):
            raise LanczosError(ERR_BAD_ARG, f"tensor_norm: {name} is one value, or one per output channel")
        a = np.broadcast_to(a, (len(src),))
        for oc in range(len(src)):
            getattr(n, name)[oc] = a[oc]
    n.format = _TENSOR_NORM_FORMATS[dtype]
    return _fill_view(n, strides, src, flip, d_flip)


def resize_tensor_norm_validate(desc, n, window=None):
    """lanczos_resize_tensor_norm_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame."""
    _check(_lib().lanczos_resize_tensor_norm_validate(ctypes.byref(desc), _window_ref(desc, window),
                                                      _ref(n)),
           "lanczos_resize_tensor_norm_validate")


def resize_tensor_view_validate(desc, v, window=None):
    """lanczos_resize_tensor_view_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the view is refused.
    window: the strides describe that window's frame."""
    _check(_lib().lanczos_resize_tensor_view_validate(ctypes.byref(desc), _window_ref(desc, window),
                                                      _ref(v)),
           "lanczos_resize_tensor_view_validate")


def _tensor_validate(kind, desc, t, window):
    """the body of resize_tensor_validate ("tensor") / resize_tensor16_validate ("tensor16")"""
    if window is None:
        name, args = f"lanczos_resize_{kind}_validate", (_ref(t),)
    else:
        name, args = f"lanczos_resize_{kind}_window_validate", (_window_ref(desc, window), _ref(t))
    _check(getattr(_lib(), name)(ctypes.byref(desc), *args), name)


def resize_tensor16_validate(desc, t, window=None):
    """lanczos_resize_tensor16_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame (lanczos_resize_tensor16_window_validate)."""
    _tensor_validate("tensor16", desc, t, window)


def resize_tensor_validate(desc, t, window=None):
    """lanczos_resize_tensor_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame (lanczos_resize_tensor_window_validate)."""
    _tensor_validate("tensor", desc, t, window)


def _factor_pair(factor):
    fx, fy = (factor, factor) if isinstance(factor, (int, np.integer)) else factor
    return int(fx), int(fy)


def reduce_size(in_w, in_h, factor, box=None):
    """(out_w, out_h) of a reduce by `factor` (an int or (fx, fy)) over the integer box (None = the whole frame)."""
    fx, fy = _factor_pair(factor)
    b = (ctypes.c_int32 * 4)(*[int(v) for v in box]) if box is not None else None
    w, h = ctypes.c_int(), ctypes.c_int()
    _check(_lib().lanczos_reduce_size(in_w, in_h, fx, fy, b, ctypes.byref(w), ctypes.byref(h)), "lanczos_reduce_size")
    return w.value, h.value


class PinnedArray:
    """A numpy array over page-locked host memory (lanczos_host_alloc) -- lets lanczos_resample_host overlap
    its PCIe copies.  Keep the object alive while the array is in use."""

    def __init__(self, shape, dtype=np.uint8):
        self.shape = tuple(int(v) for v in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self._p = ctypes.c_void_p()
        _check(_lib().lanczos_host_alloc(ctypes.byref(self._p), self.nbytes), "lanczos_host_alloc")
        buf = (ctypes.c_uint8 * self.nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def close(self):
        if self._p:
            self.array = None
            _lib().lanczos_host_free(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -- which entry a request takes, one function per family.  side is "device" or "host"; has[p] says whether the request has
# argument p ("opts": a box, a gap or ready options; "window"; and the family's own .params); the result is the entry's name and
# its arguments between (ctx, desc) and (in, out, frames).  A request keeps the narrowest entry that can carry it: an older
# build of the library has only those, and LanczosError names the entry.
def _bytes_entry(side, has):
    """bytes out: dest > source > window > opts > plain"""
    if has["dest"]:
        return "lanczos_resize_dest_" + side, ("opts", "window", "source", "dest")
    if has["source"]:
        return "lanczos_resize_source_" + side, ("opts", "window", "source")
    if has["window"]:
        return "lanczos_resize_window_" + side, ("opts", "window")
    if has["opts"]:
        return "lanczos_resize_" + side + "_ex", ("opts",)
    return "lanczos_resize_" + side, ()


def _tensor_entry(side, has):
    """tensor out: source > crops > view > {float32, 16-bit} x {window, none}; has["t"] is the class of the tensor struct, a
    TensorView (which a source and crops need), a TensorOut or a TensorOut16"""
    if has["source"]:
        return "lanczos_resize_tensor_source_" + side, ("opts", "window", "crops", "source", "t")
    if has["crops"]:
        return "lanczos_resize_tensor_crops_" + side, ("opts", "crops", "t")
    if has["t"] is TensorView:
        return "lanczos_resize_tensor_view_" + side, ("opts", "window", "t")
    stem = "lanczos_resize_tensor16_" if has["t"] is TensorOut16 else "lanczos_resize_tensor_"
    if has["window"]:
        return stem + "window_" + side, ("opts", "window", "t")
    return stem + side, ("opts", "t")


def _norm_entry(side, has):
    return "lanczos_resize_tensor_norm_" + side, ("opts", "window", "source", "norm")


def _ycc_entry(side, has):
    """RGB bytes, or with a TensorView tensor elements"""
    if has["view"]:
        return "lanczos_resize_ycc_tensor_" + side, ("opts", "window", "source", "table", "view")
    return "lanczos_resize_ycc_" + side, ("opts", "window", "source", "table")


_bytes_entry.params = ("source", "dest")
_tensor_entry.params = ("crops", "source", "t")
_norm_entry.params = ("source", "norm")
_ycc_entry.params = ("source", "table", "view")


class _Bound(dict):
    """The resize entries of one context, resolved once per request shape so that a call costs no more than the call itself:
    bound[chooser, side, has opts, has window, *(one flag per chooser.params)] is a function
    issue(desc, box, reducing_gap, opts, window, *params, in, out, frames[, in_frame_stride, out_frame_stride, stream]) that
    passes the entry the chooser picked exactly the arguments that shape has -- a struct by reference, a missing one as NULL,
    options and window resolved by _opts_ref / _window_ref, the colour table as it is -- and raises LanczosError(code, entry)
    on any code but OK.  The function is compiled from the chooser's answer the first time the shape is seen."""

    def __init__(self, handle):
        self.handle = handle

    def __missing__(self, key):
        chooser, side, *flags = key
        params = ("opts", "window") + chooser.params
        has = dict(zip(params, flags))
        name, middle = chooser(side, has)
        forms = {"opts": "_opts_ref(desc, box, reducing_gap, opts)", "window": "_window_ref(desc, window)", "table": "table"}
        args = ", ".join(["byref(desc)"] + [forms.get(p, f"byref({p})") if has[p] else "None" for p in middle])
        tail = "d_in, d_out, frames" + (", in_frame_stride, out_frame_stride, stream" if side == "device" else "")
        scope = {"entry": getattr(_lib(), name), "handle": self.handle, "name": name, "byref": ctypes.byref, "_opts_ref": _opts_ref,
                 "_window_ref": _window_ref, "LanczosError": LanczosError}
        exec(f"def issue(desc, box, reducing_gap, {', '.join(params)}, {tail}):\n"
             f"    rc = entry(handle, {args}, {tail})\n"
             f"    if rc:\n"
             f"        raise LanczosError(rc, name)\n", scope)
        self[key] = scope["issue"]
        return scope["issue"]


def _reduce_entry(side, in_w, in_h, channels, factor, box):
    fx, fy = _factor_pair(factor)
    b = (ctypes.c_int32 * 4)(*[int(v) for v in box]) if box is not None else None
    return "lanczos_reduce_" + side, in_w, in_h, channels, fx, fy, b


def _tensor_view_arg(strides, d_lut, dtype, channels_out, channels, flip, d_flip, what):
    """the view of a device tensor call: a ready TensorView, or one of strides, d_lut, dtype and the map (None = the identity
    over `channels` channels)"""
    if isinstance(strides, TensorView):
        return strides
    if dtype != "float32":
        _tensor16_format(dtype, what)
    return tensor_view(d_lut, strides, 4 if dtype == "float32" else 2,
                       channels_out if channels_out is not None else tuple(range(channels)), flip or 0, d_flip)


class Context:
    """One lanczos_ctx: a device, a stream, resident tap tables.  Not shared between threads."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(_lib().lanczos_create(ctypes.byref(self._h), device), "lanczos_create")

    @_cached_property
    def _bound(self):
        return _Bound(self._h)

    def _call(self, name, *args):
        """entry `name` on this context; any code but OK raises LanczosError(code, name)"""
        _check(getattr(_lib(), name)(self._h, *args), name)

    def close(self):
        if self._h:
            _lib().lanczos_destroy(self._h)
            self._h.value = None   # in place: the bound entries hold this object

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host buffers: the drop-in for lanczos(stream_in, stream_out) at full_TB.h:140
    def resample(self, img, scale_n, scale_d, a, mode=MODE_LSB1, out=None, bit_precision=0):
        """img: [H][W][C] (or [F][H][W][C]) uint8/uint16, stb interleaved layout -> scaled image(s).
        `out`: optional preallocated result (e.g. a PinnedArray's .array).  bit_precision: MODE_HLS only (make_desc)."""
        img = np.ascontiguousarray(img)
        batched = img.ndim == 4
        x = img if batched else img[None]
        if x.ndim != 4 or x.dtype not in (np.uint8, np.uint16):
            raise LanczosError(ERR_BAD_ARG, "resample: expected [H][W][C] uint8/uint16")
        f, h, w, c = x.shape
        d = make_desc(w, h, c, scale_n, scale_d, a, x.dtype.itemsize, mode, bit_precision=bit_precision)
        if out is None:
            out = np.empty((f, d.out_h, d.out_w, c), dtype=x.dtype)
        else:
            if out.dtype != x.dtype or out.size != f * d.out_h * d.out_w * c or not out.flags["C_CONTIGUOUS"]:
                raise LanczosError(ERR_BAD_ARG, "resample: `out` has the wrong size/dtype/layout")
            out = out.reshape((f, d.out_h, d.out_w, c))
        self._call("lanczos_resample_host", ctypes.byref(d), x.ctypes.data, out.ctypes.data, f)
        return out if batched else out[0]

    def resample_strip(self, strip_in, desc):
        """One row strip (desc.out_row0/out_rows set); strip_in holds the rows strip_input_rows() names."""
        strip_in = np.ascontiguousarray(strip_in)
        _, need = strip_input_rows(desc, desc.out_row0, desc.out_rows)
        if (strip_in.ndim != 3 or strip_in.shape[0] != need or strip_in.shape[1] != desc.in_w
                or strip_in.shape[2] != desc.channels or strip_in.dtype.itemsize != desc.bytes_per_sample):
            raise LanczosError(ERR_BAD_ARG, f"resample_strip: expected [{need}][{desc.in_w}][{desc.channels}] samples of "
                                            f"{desc.bytes_per_sample} byte(s), got {strip_in.shape} {strip_in.dtype}")
        out = np.empty((desc.out_rows, desc.out_w, desc.channels), dtype=strip_in.dtype)
        self._call("lanczos_resample_host", ctypes.byref(desc), strip_in.ctypes.data, out.ctypes.data, 1)
        return out

    def u8(self, img, out_w, out_h, a):
        """lanczos_u8: the reference's call shape (sizes as ints, scale = out_w/in_w reduced)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, c = img.shape
        out = np.empty((out_h, out_w, c), dtype=np.uint8)
        self._call("lanczos_u8", img.ctypes.data, w, h, c, out.ctypes.data, out_w, out_h, a)
        return out

    # -- device buffers (raw pointers, e.g. torch tensors' data_ptr()), asynchronous
    def resample_device(self, desc, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None):
        self._call("lanczos_resample_device", ctypes.byref(desc), d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    # -- planar frames [C][H][W] (the reference's img_in / img_out_ex arrays, full_TB.h:20-21), device pointers
    def planar_to_interleaved_device(self, d_planar, d_inter, w, h, channels, bytes_per_sample, frames, stream=None):
        self._call("lanczos_planar_to_interleaved_device", d_planar, d_inter, w, h, channels, bytes_per_sample, frames, stream)

    def interleaved_to_planar_device(self, d_inter, d_planar, w, h, channels, bytes_per_sample, frames, stream=None):
        self._call("lanczos_interleaved_to_planar_device", d_inter, d_planar, w, h, channels, bytes_per_sample, frames, stream)

    def resample_planar_device(self, desc, d_in_planar, d_out_planar, frames, stream=None):
        self._call("lanczos_resample_planar_device", ctypes.byref(desc), d_in_planar, d_out_planar, frames, stream)

    # -- resize to any size (Pillow's contract, lanczos_resize_*)
    def resize(self, img, out_w, out_h, a=3, alpha=False, box=None, reducing_gap=None, filter=FILTER_LANCZOS, window=None,
               planar=False, planar_out=False):
        """planar_out=True (uint8, 3 or 4 channels): the result is planes, [C][h][w] or [F][C][h][w], stored that way by the
        library (lanczos_resize_dest_host) -- the bytes of the same call without it moved to [C][h][w].  Combines with planar=True:
        N x C x H x W in, N x C x h x w out.
        planar=True: img is uint8 [C][H][W] or [F][C][H][W] (planes, as a decoder or a torch stage leaves them) and is read
        as it lies (lanczos_resize_source_host); the result is interleaved as ever, [h][w][C] or [F][h][w][C], the bytes of the
        same call on img moved to [H][W][C].
        window = (x0, y0, w, h) in output pixels: compute and return only that window of the out_h x out_w result, [h][w]
        instead of [out_h][out_w] -- exactly Image.resize(...).crop((x0, y0, x0 + w, y0 + h)), without computing the rest
        (center_window gives torchvision's CenterCrop).
        filter: Image.resize's `resample` as a name ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest") or
        FILTER_*; bytes identical to Pillow's for that filter.  Every filter but Lanczos needs a == 3; "nearest" takes no
        reducing_gap and no uint16 frames, and copies RGBA pixels whole.
        box = (x0, y0, x1, y1): resize that (sub-pixel) region of the source, as Image.resize(..., box=box); pixels
        outside it still contribute near its edges.  reducing_gap = g >= 1: first reduce by whole factors (an exact box
        average), then resize what is left, as Image.resize(..., reducing_gap=g) -- Pillow's bytes for the same arguments, not
        those of the resize without a gap; 8-bit without alpha only (ERR_BAD_ARG otherwise, as there is no oracle).
        img: uint8 or uint16 [H][W], [H][W][C] or [F][H][W][C] -> the same layout and dtype at out_h x out_w, bytes
        identical to Pillow's Image.resize((out_w, out_h), Image.LANCZOS) for a = 3.  Four channels: mode RGBX (independent
        channels) by default, mode RGBA (straight alpha in the last channel, premultiplied inside the kernels) with
        alpha=True; alpha=True with any other channel count raises LanczosError(ERR_BAD_ARG).  uint16: every channel as
        Pillow resizes an I;16 plane (a sum above 65535 stores 0xFF00 | low byte, as Pillow does); not with alpha."""
        if planar_out and not planar:
            img = np.asarray(img)
            if img.dtype != np.uint8 or img.ndim not in (3, 4) or img.shape[-1] not in (3, 4):
                raise LanczosError(ERR_BAD_ARG, "resize: planar_out=True takes uint8 frames of 3 or 4 channels")
        return self._resize_host("resize", img, (np.uint8,) if planar or planar_out else (np.uint8, np.uint16), out_w, out_h, a,
                                 alpha, box, reducing_gap, filter, window, planar, planar_out)

    def _resize_host(self, what, img, dtypes, out_w, out_h, a, alpha, box, reducing_gap, filter, window, planar=False,
                     planar_out=False):
        """the body of resize and resize_f32: frames of one of `dtypes` in, the same dtype out"""
        x, (f, h, w, c), back = _frames(img, dtypes, what, planar)
        d = resize_desc(w, h, out_w, out_h, c, a, alpha, 16 if x.dtype == np.uint16 else 8, x.dtype == np.float32, filter)
        win = resize_window(d, window)
        source = resize_source(d, "planar") if planar else None
        dest = resize_dest(d, "planar", window=window) if planar_out else None
        out = np.empty((f, c, win.h, win.w) if planar_out else (f, win.h, win.w, c), dtype=x.dtype)
        self._bound[_bytes_entry, "host", box is not None or reducing_gap is not None, window is not None, bool(planar), bool(planar_out)](
            d, box, reducing_gap, None, win if window is not None else None, source, dest, x.ctypes.data, out.ctypes.data, f)
        return back(out)

    def resize_f32(self, img, out_w, out_h, a=3, box=None, filter=FILTER_LANCZOS, window=None):
        """filter and window as Context.resize.
        img: float32 [H][W], [H][W][C] or [F][H][W][C] (C = 1, 3 or 4) -> the same layout at out_h x out_w, every channel
        bit for bit what Pillow's Image.resize((out_w, out_h), Image.LANCZOS, box) gives for it as a mode F plane (a = 3):
        double accumulation over exactly the window's taps, stored as float -- no clamp, inf on overflow, denormals kept, NaN
        where Pillow has NaN.  box as Context.resize.  No alpha and no reducing_gap for floats."""
        return self._resize_host("resize_f32", img, (np.float32,), out_w, out_h, a, False, box, None, filter, window)

    def resize_device(self, desc, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None, box=None,
                      reducing_gap=None, opts=None, filter=None, window=None, source=None, dest=None):
        """dest: a ResizeDest (resize_dest) saying where the samples of the frames at d_out go -- planar, or interleaved with
        pitched rows; out_frame_stride 0 is then that layout's extent, and every byte the layout does not name keeps its contents
        (lanczos_resize_dest_device).
        source: a ResizeSource (resize_source) saying where the samples of the frames at d_in lie -- planar, or interleaved
        with pitched rows; in_frame_stride 0 is then that layout's extent (lanczos_resize_source_device).
        Device pointers, asynchronous on `stream` (None = the default stream).  box / reducing_gap / opts as
        resize_taps_host.  The filter is the descriptor's (resize_desc(..., filter=)); filter= (a name or FILTER_*) runs
        the same request with that filter instead.  window = (x0, y0, w, h) or a ResizeWindow: the frames at d_out are that
        window of the output, w x h pixels tightly packed (out_frame_stride 0 = one such frame)."""
        if filter is not None:
            d = ResizeDesc.from_buffer_copy(desc)
            d.reserved[0] = (d.reserved[0] & ~(15 << 8)) | (filter_code(filter) << 8)
            desc = d
        self._bound[_bytes_entry, "device", box is not None or reducing_gap is not None or opts is not None, window is not None,
                    source is not None, dest is not None](
            desc, box, reducing_gap, opts, window, source, dest, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    # -- resize straight into a float tensor (PIL.Image.resize -> ToTensor() -> Normalize(), lanczos_resize_tensor_*)
    def resize_tensor(self, img, out_w, out_h, mean=None, std=None, lut=None, layout="chw", a=3, alpha=False, box=None,
                      reducing_gap=None, filter=FILTER_LANCZOS, dtype="float32", window=None, channels_out=None, flip=None,
                      crop=None, origins=None, planar=False):
        """planar=True: img is uint8 [C][H][W] or [F][C][H][W] and is read as it lies (lanczos_resize_tensor_source_host); the
        result is that of the same call on img moved to [H][W][C].
        crop=(w, h) with origins=[(x0, y0), ...], one pair per frame: frame f of the result is the w x h window of its
        resize at origins[f] (Resize -> RandomCrop; lanczos_resize_tensor_crops_host, which refuses an origin outside the
        output).  channels_out and flip apply as below; not together with window.
        channels_out: a tuple of source channel indices, one per channel of the result -- (2, 1, 0) turns BGR into RGB,
        (0, 1, 2) on an RGBA frame drops alpha (with alpha=True the colours are un-premultiplied first, Pillow's resize in mode
        RGBA then .convert("RGB")); distinct indices, no replication.  The result then has len(channels_out) channels, and the
        table (lut, or mean / std) is [len(channels_out)][256] in OUTPUT order.  flip: None, "h", "v", "hv", or an integer
        array with one entry per frame (bit 0 mirrors x, bit 1 mirrors y: torch's .flip(-1) / .flip(-2) of that frame).  With
        neither keyword the call is what it was (lanczos_resize_tensor_*); with either it is lanczos_resize_tensor_view_host.
        window = (x0, y0, w, h): only that window of the output, [F][C][h][w] or [F][h][w][C] (as Context.resize).
        img: uint8 [H][W], [H][W][C] or [F][H][W][C] as Context.resize takes it -> float32 [F][C][H][W] (layout="chw") or
        [F][H][W][C] ("hwc"), the frame axis dropped as resize drops it: lut[c][byte] of the bytes Context.resize returns for
        the same arguments.  lut: float32 [C][256], moved bit for bit; None = normalize_lut(C, mean, std), with which the
        result is bit for bit torch.from_numpy(bytes).permute(2, 0, 1).float().div(255).sub(mean).div(std).
        dtype="float16" returns np.float16 and dtype="bfloat16" np.uint16 holding the bfloat16 patterns (numpy has no
        bfloat16; torch.from_numpy(a.view(np.int16)).view(torch.bfloat16) is the tensor), with normalize_lut(..., dtype=)
        bit for bit the float32 pipeline followed by .to(torch.float16) / .to(torch.bfloat16).  lut is then uint16 or float16
        [C][256], moved bit for bit."""
        wide = dtype == "float32"
        if not wide:
            _tensor16_format(dtype, "resize_tensor")
        x, (f, h, w, c), back = _frames(img, (np.uint8,), "resize_tensor", planar)
        d = resize_desc(w, h, out_w, out_h, c, a, alpha, filter=filter)
        view = planar or channels_out is not None or flip is not None or crop is not None
        if channels_out is not None:
            channels_out = tuple(int(v) for v in channels_out)
            if not 1 <= len(channels_out) <= c:
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor: channels_out names 1 to {c} source channels")
            c = len(channels_out)
        lut = _lut_arg(lut, mean, std, c, dtype, "resize_tensor")
        if (crop is None) != (origins is None) or (crop is not None and window is not None):
            raise LanczosError(ERR_BAD_ARG, "resize_tensor: crop= and origins= come together, and not with window=")
        if crop is not None:
            org = np.ascontiguousarray(origins)
            if len(crop) != 2 or org.shape != (f, 2) or org.dtype.kind not in "iu":
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor: crop is (w, h) and origins {f} integer pairs (x0, y0)")
            org = org.astype(np.int32)
            window = (0, 0, int(crop[0]), int(crop[1]))   # the frame the strides describe
        win = resize_window(d, window)
        strides = tensor_strides(layout, win.w, win.h, c)
        shape = (f, c, win.h, win.w) if layout == "chw" else (f, win.h, win.w, c)
        cr = resize_crops(win.w, win.h, org.ctypes.data) if crop is not None else None   # (the window is then no argument)
        if view:
            bits, flips = _flip_arg(flip, f, "resize_tensor")
            t = tensor_view(lut.ctypes.data, strides, 4 if wide else 2, channels_out if channels_out is not None else tuple(range(c)),
                            bits, flips.ctypes.data if flips is not None else None)
        else:
            t = (tensor_out if wide else tensor16_out)(lut.ctypes.data, strides)
        source = resize_source(d, "planar") if planar else None
        out = np.empty(shape, dtype=np.float32 if wide else np.uint16)
        win = win if window is not None and cr is None else None
        self._bound[_tensor_entry, "host", box is not None or reducing_gap is not None, win is not None, cr is not None, bool(planar),
                    t.__class__](d, box, reducing_gap, None, win, cr, source, t, x.ctypes.data, out.ctypes.data, f)
        return back(out if wide else _tensor16_array(out, dtype), True)

    def resize_tensor_device(self, desc, d_in, d_out, frames, d_lut, strides, in_frame_stride=0, out_frame_stride=0,
                             stream=None, box=None, reducing_gap=None, opts=None, dtype="float32", window=None,
                             channels_out=None, flip=None, d_flip=None, crop=None, d_origin=None, source=None):
        """source: a ResizeSource (resize_source) for the frames at d_in, as Context.resize_device; the request then runs as a
        view (lanczos_resize_tensor_source_device), a ready TensorOut / TensorOut16 as `strides` included.
        crop=(w, h) with d_origin, a device pointer to `frames` int32 pairs (x0, y0) (or crop a ready ResizeCrops): every
        frame stores the w x h window of its resize at its own origin, read and clamped into the output when the kernels run
        (lanczos_resize_tensor_crops_device).  The strides describe the C x h x w frame; not together with window.
        channels_out / flip as Context.resize_tensor (flip: None, "h", "v", "hv" or FLIP_* bits, for every frame); d_flip: a
        device pointer to one byte per frame, XORed with flip and read when the kernels run.  With any of the three, or a ready
        TensorView as `strides`, the call is lanczos_resize_tensor_view_device: the table at d_lut is [len(channels_out)][256]
        in output order and the strides describe a frame of that many channels.
        Device pointers, asynchronous on `stream`: uint8 frames at d_in -> float frames at d_out, out_frame_stride in BYTES
        (0 = one frame's extent).  d_lut: device pointer to channels * 256 floats, read when the kernels run (a replayed
        graph sees its contents of that moment).  strides = (chan_stride, row_stride, pix_stride) in floats, e.g.
        tensor_strides("chw", ...), or a ready TensorOut (d_lut then unused).  box / reducing_gap / opts as resize_device.
        dtype="bfloat16" / "float16" (or a ready TensorOut16): 16-bit elements at d_out and in the table, strides in
        elements, d_out and out_frame_stride multiples of 2.  window = (x0, y0, w, h) or a ResizeWindow: the element frames
        are that window of the output, and the strides describe its C x h x w frame (tensor_strides(layout, w, h, C))."""
        if crop is not None and window is not None:
            raise LanczosError(ERR_BAD_ARG, "resize_tensor_device: crop= or window=, not both")
        if (crop is None or not isinstance(crop, ResizeCrops)) and (crop is None) != (d_origin is None):
            raise LanczosError(ERR_BAD_ARG, "resize_tensor_device: crop=(w, h) and d_origin= come together")
        t = strides
        if source is not None and isinstance(t, (TensorOut, TensorOut16)):   # the same request as a view
            t = tensor_view(t.d_lut, (t.chan_stride, t.row_stride, t.pix_stride), 2 if isinstance(t, TensorOut16) else 4,
                            tuple(range(desc.channels)))
        if isinstance(t, TensorView):
            pass
        elif source is not None or crop is not None or channels_out is not None or flip is not None or d_flip is not None:
            t = _tensor_view_arg(t, d_lut, dtype, channels_out, desc.channels, flip, d_flip, "resize_tensor_device")
        elif isinstance(t, TensorOut16) or dtype != "float32":
            if not isinstance(t, TensorOut16):
                _tensor16_format(dtype, "resize_tensor_device")
                t = tensor16_out(d_lut, t)
        elif not isinstance(t, TensorOut):
            t = tensor_out(d_lut, t)
        cr = crop if crop is None or isinstance(crop, ResizeCrops) else resize_crops(crop[0], crop[1], d_origin)
        self._bound[_tensor_entry, "device", box is not None or reducing_gap is not None or opts is not None, window is not None,
                    cr is not None, source is not None, t.__class__](
            desc, box, reducing_gap, opts, window, cr, source, t, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    # -- 16-bit and float frames straight into normalised tensors (lanczos_resize_tensor_norm_*)
    def resize_tensor_norm(self, img, out_w, out_h, div=None, mean=None, std=None, dtype="float32", layout="chw", a=3, box=None,
                           filter=FILTER_LANCZOS, window=None, channels_out=None, flip=None):
        """img: uint16 or float32 [H][W], [H][W][C] or [F][H][W][C] as Context.resize / Context.resize_f32 take it -> elements
        [F][C][H][W] (layout="chw") or [F][H][W][C] ("hwc"), the frame axis dropped as resize drops it:
        ((float(P) / div - mean) / std) of the samples P those calls return for the same arguments, three IEEE float operations
        -- bit for bit torch.from_numpy(P).permute(2, 0, 1).float().div(div).sub(mean).div(std) on the CPU, followed by
        .to(dtype) for dtype "bfloat16" (returned as np.uint16 patterns) or "float16" (np.float16).  div=None is 65535 for
        uint16 and 1 for float32; mean=None is 0, std=None is 1; each one value or one per channel of the result.  box, filter,
        window, channels_out and flip as Context.resize_tensor.  No reducing_gap, no alpha, no crop origins."""
        x, (f, h, w, c), back = _frames(img, (np.uint16, np.float32), "resize_tensor_norm")
        if dtype not in _TENSOR_NORM_FORMATS:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: dtype is 'float32', 'bfloat16' or 'float16', not {dtype!r}")
        u16 = x.dtype == np.uint16
        d = resize_desc(w, h, out_w, out_h, c, a, bits=16 if u16 else 8, f32=not u16, filter=filter)
        src = tuple(int(v) for v in channels_out) if channels_out is not None else tuple(range(c))
        if not 1 <= len(src) <= c:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: channels_out names 1 to {c} source channels")
        c = len(src)
        bits, flips = _flip_arg(flip, f, "resize_tensor_norm")
        win = resize_window(d, window)
        n = tensor_norm(tensor_strides(layout, win.w, win.h, c), (65535.0 if u16 else 1.0) if div is None else div,
                        0.0 if mean is None else mean, 1.0 if std is None else std, dtype, src,
                        bits, flips.ctypes.data if flips is not None else None)
        out = np.empty((f, c, win.h, win.w) if layout == "chw" else (f, win.h, win.w, c),
                       dtype=np.float32 if dtype == "float32" else np.uint16)
        self._bound[_norm_entry, "host", box is not None, window is not None, False, True](
            d, box, None, None, win if window is not None else None, None, n, x.ctypes.data, out.ctypes.data, f)
        return back(out if dtype == "float32" else _tensor16_array(out, dtype), True)

    def resize_tensor_norm_device(self, desc, d_in, d_out, frames, norm, in_frame_stride=0, out_frame_stride=0, stream=None,
                                  box=None, opts=None, window=None, source=None):
        """Device pointers, asynchronous on `stream`: uint16 (resize_desc(..., bits=16)) or float32 (f32=True) frames at d_in
        -> element frames at d_out as `norm`, a TensorNorm (tensor_norm / tensor_norm_init), describes them; its div / mean /
        std travel by value.  out_frame_stride in BYTES (0 = one frame's extent).  box / opts as resize_device; window =
        (x0, y0, w, h) or a ResizeWindow: the strides describe that window's frame; source: a ResizeSource of pitched
        interleaved rows for the frames at d_in."""
        self._bound[_norm_entry, "device", box is not None or opts is not None, window is not None, source is not None, True](
            desc, box, None, opts, window, source, norm, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    def _ycc_host_args(self, frames, in_w, in_h, out_w, out_h, layout, filter, a, source, what):
        d = resize_desc(in_w, in_h, out_w, out_h, 3, a, filter=filter)
        src = source if source is not None else ycc_source(d, layout)
        ycc_source_validate(d, src)
        x = np.ascontiguousarray(frames)
        n = ycc_frame_bytes(d, src)
        if x.dtype != np.uint8 or x.ndim not in (1, 2) or x.shape[-1] != n:
            raise LanczosError(ERR_BAD_ARG, f"{what}: expected uint8 [{n}] or [N][{n}], the frames as they lie in memory")
        return d, src, x, (x if x.ndim == 2 else x[None])

    def resize_ycc(self, frames, in_w, in_h, out_w, out_h, layout="nv12", standard="jfif", filter=FILTER_LANCZOS, a=3, box=None,
                   reducing_gap=None, window=None, table=None, source=None):
        """YCbCr frames -> uint8 [N][h][w][3] (RGB under the standard tables), byte for byte Pillow's three "L" resizes (chroma
        with the box scaled to its plane), Image.merge("YCbCr", ...) and convert("RGB") under standard="jfif".
        frames: uint8 [N][B] or [B], each frame its B bytes as they lie in memory: the tight layout of `layout` ("nv12", "nv21",
        "i420", "i422", "i444": Y, then Cb and Cr planes or the interleaved plane), or whatever `source` (ycc_source)
        describes.  in_w x in_h: the luma size; chroma planes are ceil(in_w / 2) x ceil(in_h / 2) under 4:2:0, centre-sited.
        box in luma pixels, reducing_gap, filter, a and window = (x0, y0, w, h) as Context.resize.  table: an int32 [3][3][256]
        of the caller's instead of ycc_table(standard)."""
        d, src, x0, x = self._ycc_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc")
        t = _ycc_table_arg(standard, table, "resize_ycc")
        win = resize_window(d, window)
        out = np.empty((x.shape[0], win.h, win.w, 3), dtype=np.uint8)
        self._bound[_ycc_entry, "host", box is not None or reducing_gap is not None, window is not None, True, True, False](
            d, box, reducing_gap, None, win if window is not None else None, src, t.ctypes.data, None, x.ctypes.data, out.ctypes.data,
            x.shape[0])
        return out if x0.ndim == 2 else out[0]

    def resize_ycc_tensor(self, frames, in_w, in_h, out_w, out_h, layout="nv12", standard="jfif", mean=None, std=None, lut=None,
                          dtype="float32", tensor_layout="chw", channels_out=None, flip=None, filter=FILTER_LANCZOS, a=3, box=None,
                          reducing_gap=None, window=None, table=None, source=None):
        """As resize_ycc, into a normalised tensor: lut[oc][byte] of the RGB bytes resize_ycc returns, float32 [N][C][h][w]
        (tensor_layout="chw") or [N][h][w][C] ("hwc"); dtype, mean / std or lut, channels_out and flip as Context.resize_tensor
        takes them (bfloat16 comes back as uint16 patterns)."""
        d, src, x0, x = self._ycc_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc_tensor")
        t = _ycc_table_arg(standard, table, "resize_ycc_tensor")
        wide = dtype == "float32"
        if not wide:
            _tensor16_format(dtype, "resize_ycc_tensor")
        f = x.shape[0]
        channels_out = tuple(int(v) for v in channels_out) if channels_out is not None else (0, 1, 2)
        c = len(channels_out)
        if not 1 <= c <= 3:
            raise LanczosError(ERR_BAD_ARG, "resize_ycc_tensor: channels_out names 1 to 3 source channels")
        lut = _lut_arg(lut, mean, std, c, dtype, "resize_ycc_tensor")
        bits, flips = _flip_arg(flip, f, "resize_ycc_tensor")
        win = resize_window(d, window)
        v = tensor_view(lut.ctypes.data, tensor_strides(tensor_layout, win.w, win.h, c), 4 if wide else 2, channels_out,
                        bits, flips.ctypes.data if flips is not None else None)
        shape = (f, c, win.h, win.w) if tensor_layout == "chw" else (f, win.h, win.w, c)
        out = np.empty(shape, dtype=np.float32 if wide else np.uint16)
        self._bound[_ycc_entry, "host", box is not None or reducing_gap is not None, window is not None, True, True, True](
            d, box, reducing_gap, None, win if window is not None else None, src, t.ctypes.data, v, x.ctypes.data, out.ctypes.data, f)
        out = out if wide else _tensor16_array(out, dtype)
        return out if x0.ndim == 2 else out[0]

    def resize_ycc_device(self, desc, source, d_table, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                          box=None, reducing_gap=None, opts=None, window=None):
        """Device pointers, asynchronous on `stream`: YCbCr frames at d_in in `source`'s layout (any byte address, frames
        in_frame_stride bytes apart, 0 = the layout's extent) -> tightly packed RGB bytes of the window at d_out.  d_out and
        out_frame_stride (0 = w * h * 3 rounded up to a multiple of 4) are multiples of 4.  d_table: device, int32 [3][3][256]
        (ycc_table), read when the kernels run."""
        self._bound[_ycc_entry, "device", box is not None or reducing_gap is not None or opts is not None, window is not None,
                    source is not None, True, False](
            desc, box, reducing_gap, opts, window, source, d_table, None, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    def resize_ycc_tensor_device(self, desc, source, d_table, d_in, d_out, frames, d_lut, strides, in_frame_stride=0,
                                 out_frame_stride=0, stream=None, box=None, reducing_gap=None, opts=None, dtype="float32",
                                 window=None, channels_out=None, flip=None, d_flip=None):
        """... -> tensor elements at d_out: strides (or a ready TensorView), d_lut, dtype, channels_out, flip and d_flip as
        Context.resize_tensor_device takes them, over the RGB bytes resize_ycc_device stores as source channels 0, 1, 2."""
        v = _tensor_view_arg(strides, d_lut, dtype, channels_out, 3, flip, d_flip, "resize_ycc_tensor_device")
        self._bound[_ycc_entry, "device", box is not None or reducing_gap is not None or opts is not None, window is not None,
                    source is not None, True, True](
            desc, box, reducing_gap, opts, window, source, d_table, v, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    def _ycc_out(self, d, dest, in_ptr, out_ptr, frames, source, table, box, reducing_gap, opts, window, memory, in_fs=0, out_fs=0,
                 stream=None):
        if opts is None and (box is not None or reducing_gap is not None):
            opts = resize_opts(d, box, reducing_gap)
        if window is not None and not isinstance(window, ResizeWindow):
            window = resize_window(d, window)
        rq = ycc_out_request(d, dest, in_ptr, out_ptr, frames, source, table, opts, window, memory, in_fs, out_fs, stream)
        self._call("lanczos_resize_ycc_out", ctypes.byref(rq))

    def _ycc_out_host(self, d, x, dest, out_layout, source, table, box, reducing_gap, window, rgb, out):
        """the host side of resize_ycc_to_ycc / resize_rgb_to_ycc: x is [N][bytes of a frame]; out: a caller's buffer [N][extent]"""
        t = dest if dest is not None else ycc_dest(d, out_layout, window, aligned=not rgb)
        n = ycc_dest_frame_bytes(d, t, window)
        if out is None:
            out = np.zeros((x.shape[0], n), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (x.shape[0], n):
            raise LanczosError(ERR_BAD_ARG, f"out: expected a contiguous uint8 [{x.shape[0]}][{n}]")
        self._ycc_out(d, t, x.ctypes.data, out.ctypes.data, x.shape[0], source, table.ctypes.data if table is not None else None,
                      box, reducing_gap, None, window, MEM_HOST)
        return out

    def resize_ycc_to_ycc(self, frames, in_w, in_h, out_w, out_h, layout="nv12", out_layout="nv12", filter=FILTER_LANCZOS, a=3,
                          box=None, reducing_gap=None, window=None, source=None, dest=None, out=None):
        """YCbCr frames -> YCbCr frames, uint8 [N][B'] (or [B'] for one frame [B]), each frame its bytes as `out_layout`
        ("nv12", "nv21", "i420", "i422", "i444": tight) or `dest` (ycc_dest) lays them out: byte for byte Pillow's "L" resize
        of every plane, luma to out_w x out_h and chroma to the destination's chroma size with the box scaled to its plane, no
        colour conversion.  frames, layout / source, box, reducing_gap, filter and a as Context.resize_ycc; window =
        (x0, y0, w, h) in luma output pixels, the origin a multiple of the destination's subsampling.  Bytes of the result
        that the layout does not name are zero, or keep what the caller's `out` ([N][extent]) held."""
        d, src, x0, x = self._ycc_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc_to_ycc")
        res = self._ycc_out_host(d, x, dest, out_layout, src, None, box, reducing_gap, window, False, out)
        return res if x0.ndim == 2 else res[0]

    def resize_rgb_to_ycc(self, img, out_w, out_h, out_layout="nv12", standard="jfif", table=None, filter=FILTER_LANCZOS, a=3,
                          box=None, reducing_gap=None, window=None, dest=None, out=None):
        """RGB images, uint8 [H][W][3] or [N][H][W][3] -> YCbCr frames as resize_ycc_to_ycc returns them: Pillow's resize of the
        RGB image (cut to `window`, any origin), convert("YCbCr") under standard="jfif" and Image.reduce of the chroma planes
        where the layout subsamples them.  table: an int32 [3][3][256] of the caller's instead of ycc_table_forward(standard)."""
        x = np.ascontiguousarray(img)
        if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
            raise LanczosError(ERR_BAD_ARG, "resize_rgb_to_ycc: expected uint8 [H][W][3] or [N][H][W][3]")
        x4 = x if x.ndim == 4 else x[None]
        d = resize_desc(x4.shape[2], x4.shape[1], out_w, out_h, 3, a, filter=filter)
        t = _ycc_table_arg(standard, table, "resize_rgb_to_ycc", forward=True)
        res = self._ycc_out_host(d, x4.reshape(x4.shape[0], -1), dest, out_layout, None, t, box, reducing_gap, window, True, out)
        return res if x.ndim == 4 else res[0]

    def resize_ycc_to_ycc_device(self, desc, source, dest, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                                 box=None, reducing_gap=None, opts=None, window=None):
        """Device pointers, asynchronous on `stream`: YCbCr frames at d_in in `source`'s layout -> YCbCr frames at d_out in
        `dest`'s (ycc_dest, of `window` where one is given), any byte addresses, frames in_frame_stride / out_frame_stride bytes
        apart (0 = the layouts' extents).  Bytes the destination does not name keep their contents."""
        self._ycc_out(desc, dest, d_in, d_out, frames, source, None, box, reducing_gap, opts, window, MEM_DEVICE, in_frame_stride,
                      out_frame_stride, stream)

    def resize_rgb_to_ycc_device(self, desc, dest, d_table, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                                 box=None, reducing_gap=None, opts=None, window=None):
        """... tightly packed RGB frames at d_in (in_frame_stride 0 = in_w * in_h * 3) -> YCbCr frames at d_out.  d_table:
        device, int32 [3][3][256] (ycc_table_forward), read when the kernels run."""
        self._ycc_out(desc, dest, d_in, d_out, frames, None, d_table, box, reducing_gap, opts, window, MEM_DEVICE, in_frame_stride,
                      out_frame_stride, stream)

    def last_ycc_out_info(self):
        """YccOutInfo of the last successful resize_*_to_ycc* call on the context (all zero before any)."""
        info = YccOutInfoC()
        self._call("lanczos_last_ycc_out_info", ctypes.byref(info))
        return YccOutInfo(info.luma_kernel, info.chroma_kernel, bool(info.split), bool(info.join), bool(info.encode), info.launches)

    def _ycc16(self, d, source, in_ptr, out_ptr, frames, dest, matrix, norm, box, opts, window, memory, in_fs=0, out_fs=0, stream=None):
        if opts is None and box is not None:
            opts = resize_opts(d, box, None)
        if window is not None and not isinstance(window, ResizeWindow):
            window = resize_window(d, window)
        rq = ycc16_request(d, source, in_ptr, out_ptr, frames, dest, matrix, norm, opts, window, memory, in_fs, out_fs, stream)
        self._call("lanczos_resize_ycc16", ctypes.byref(rq))

    def _ycc16_host_args(self, frames, in_w, in_h, out_w, out_h, layout, filter, a, source, what):
        d = resize_desc(in_w, in_h, out_w, out_h, 3, a, bits=16, filter=filter)
        src = source if source is not None else ycc16_source(d, layout)
        ycc16_source_validate(d, src)
        x = np.ascontiguousarray(frames)
        n = ycc_frame_bytes(d, src) // 2
        if x.dtype != np.uint16 or x.ndim not in (1, 2) or x.shape[-1] != n:
            raise LanczosError(ERR_BAD_ARG, f"{what}: expected uint16 [{n}] or [N][{n}], the words of the frames as they lie in memory")
        return d, src, x, (x if x.ndim == 2 else x[None])

    def resize_ycc16_to_ycc(self, frames, in_w, in_h, out_w, out_h, layout="p010", out_layout="p010", filter=FILTER_LANCZOS, a=3,
                            box=None, window=None, source=None, dest=None, out=None):
        """YCbCr frames of 16-bit words -> YCbCr frames of 16-bit words, uint16 [N][W'] (or [W'] for one frame [W]): word for word
        Pillow's "I;16" resize of every plane on the raw words, luma to out_w x out_h and chroma to the destination's chroma size
        with the box scaled to its plane; no colour conversion.  frames: uint16 [N][W] or [W], each frame its words as they lie
        in memory in the tight layout of `layout` (a name of YCC16_LAYOUTS: "p010", "p016", "p210", "p216", "nv12", "nv21",
        "nv16", "i420", "i422", "i444") or as `source` (ycc16_source) describes.  The words may hold any depth, LSB- or
        MSB-aligned: sums above 65535 store 0xFF00 | low byte, as Pillow's do.  box in luma pixels, filter (not "nearest") and
        a as Context.resize; no reducing_gap.  window = (x0, y0, w, h) in luma output pixels, the origin a multiple of the
        destination's subsampling.  Words of the result the layout does not name are zero, or keep what `out` held."""
        d, src, x0, x = self._ycc16_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc16_to_ycc")
        t = dest if dest is not None else ycc16_dest(d, out_layout, window)
        n = ycc_dest_frame_bytes(d, t, window) // 2
        if out is None:
            out = np.zeros((x.shape[0], n), dtype=np.uint16)
        elif out.dtype != np.uint16 or not out.flags.c_contiguous or out.shape != (x.shape[0], n):
            raise LanczosError(ERR_BAD_ARG, f"out: expected a contiguous uint16 [{x.shape[0]}][{n}]")
        self._ycc16(d, src, x.ctypes.data, out.ctypes.data, x.shape[0], t, None, None, box, None, window, MEM_HOST)
        return out if x0.ndim == 2 else out[0]

    def resize_ycc16_rgb(self, frames, in_w, in_h, out_w, out_h, layout="p010", matrix=None, filter=FILTER_LANCZOS, a=3, box=None,
                         window=None, source=None):
        """YCbCr frames of 16-bit words -> uint16 [N][h][w][3]: the planes resized as resize_ycc16_to_ycc resizes them (chroma to
        the luma size) and converted through `matrix`, a Ycc16Matrix (None: ycc16_matrix(), BT.709 for limited-range 10-bit
        words, MSB-aligned, to RGB words of 0 .. 65535)."""
        d, src, x0, x = self._ycc16_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc16_rgb")
        m = matrix if matrix is not None else ycc16_matrix()
        win = resize_window(d, window)
        out = np.empty((x.shape[0], win.h, win.w, 3), dtype=np.uint16)
        self._ycc16(d, src, x.ctypes.data, out.ctypes.data, x.shape[0], None, m, None, box, None, window, MEM_HOST)
        return out if x0.ndim == 2 else out[0]

    def resize_ycc16_tensor(self, frames, in_w, in_h, out_w, out_h, layout="p010", matrix=None, mean=None, std=None, div=65535.0,
                            dtype="float32", tensor_layout="chw", channels_out=None, flip=None, filter=FILTER_LANCZOS, a=3, box=None,
                            window=None, source=None):
        """As resize_ycc16_rgb, into a normalised tensor: ((float(P) / div - mean) / std) of the RGB words P that call returns,
        three IEEE float operations as Context.resize_tensor_norm computes them, float32 [N][C][h][w] (tensor_layout="chw") or
        [N][h][w][C] ("hwc"); dtype "bfloat16" comes back as uint16 patterns, "float16" as np.float16.  div, mean and std one
        value or one per channel of the result; channels_out and flip as Context.resize_tensor."""
        d, src, x0, x = self._ycc16_host_args(frames, in_w, in_h, out_w, out_h, layout, filter, a, source, "resize_ycc16_tensor")
        if dtype not in _TENSOR_NORM_FORMATS:
            raise LanczosError(ERR_BAD_ARG, f"resize_ycc16_tensor: dtype is 'float32', 'bfloat16' or 'float16', not {dtype!r}")
        m = matrix if matrix is not None else ycc16_matrix()
        f = x.shape[0]
        ch = tuple(int(v) for v in channels_out) if channels_out is not None else (0, 1, 2)
        c = len(ch)
        if not 1 <= c <= 3:
            raise LanczosError(ERR_BAD_ARG, "resize_ycc16_tensor: channels_out names 1 to 3 source channels")
        bits, flips = _flip_arg(flip, f, "resize_ycc16_tensor")
        win = resize_window(d, window)
        n = tensor_norm(tensor_strides(tensor_layout, win.w, win.h, c), div, 0.0 if mean is None else mean, 1.0 if std is None else std,
                        dtype, ch, bits, flips.ctypes.data if flips is not None else None)
        out = np.empty((f, c, win.h, win.w) if tensor_layout == "chw" else (f, win.h, win.w, c),
                       dtype=np.float32 if dtype == "float32" else np.uint16)
        self._ycc16(d, src, x.ctypes.data, out.ctypes.data, f, None, m, n, box, None, window, MEM_HOST)
        out = out if dtype == "float32" else _tensor16_array(out, dtype)
        return out if x0.ndim == 2 else out[0]

    def resize_ycc16_to_ycc_device(self, desc, source, dest, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                                   box=None, opts=None, window=None):
        """Device pointers, asynchronous on `stream`: frames of 16-bit words at d_in in `source`'s layout (ycc16_source) -> frames
        at d_out in `dest`'s (ycc16_dest, of `window` where one is given).  Addresses and frame strides (bytes; 0 = the layouts'
        extents) are multiples of 2.  Bytes the destination does not name keep their contents."""
        self._ycc16(desc, source, d_in, d_out, frames, dest, None, None, box, opts, window, MEM_DEVICE, in_frame_stride, out_frame_stride,
                    stream)

    def resize_ycc16_rgb_device(self, desc, source, matrix, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                                box=None, opts=None, window=None):
        """... -> tightly packed RGB words of the window at d_out, w * h * 3 per frame; d_out and out_frame_stride (0 = w * h * 6
        rounded up to a multiple of 4) are multiples of 4.  matrix: a Ycc16Matrix, passed by value."""
        self._ycc16(desc, source, d_in, d_out, frames, None, matrix, None, box, opts, window, MEM_DEVICE, in_frame_stride,
                    out_frame_stride, stream)

    def resize_ycc16_tensor_device(self, desc, source, matrix, norm, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0,
                                   stream=None, box=None, opts=None, window=None):
        """... -> tensor elements at d_out as `norm`, a TensorNorm (tensor_norm), describes them over the RGB words as source
        channels 0, 1, 2; its div / mean / std travel by value, its d_flip is a device array read when the kernels run."""
        self._ycc16(desc, source, d_in, d_out, frames, None, matrix, norm, box, opts, window, MEM_DEVICE, in_frame_stride,
                    out_frame_stride, stream)

    def last_ycc16_info(self):
        """Ycc16Info of the last successful resize_ycc16* call on the context (all zero before any)."""
        info = Ycc16InfoC()
        self._call("lanczos_last_ycc16_info", ctypes.byref(info))
        return Ycc16Info(info.luma_kernel, info.chroma_kernel, bool(info.split), bool(info.join), bool(info.merge), info.launches)

    def last_ycc_info(self):
        """YccInfo of the last successful resize_ycc* call on the context (all zero before any)."""
        info = YccInfoC()
        self._call("lanczos_last_ycc_info", ctypes.byref(info))
        return YccInfo(info.luma_kernel, info.chroma_kernel, bool(info.split), info.launches)

    def last_tensor_route(self):
        """TENSOR_FUSED (the resize kernel stored the floats), TENSOR_CONVERTED (bytes to scratch, then a conversion launch),
        or 0 if the last call on the context was no tensor call."""
        return _lib().lanczos_last_tensor_route(self._h)

    def last_dest_route(self):
        """DEST_DIRECT (the resize kernel stored into the destination itself), DEST_UNPACKED (the packed result went to context
        scratch and one launch scattered it), of the last call on the context that had a destination layout; 0 before any."""
        return _lib().lanczos_last_dest_route(self._h)

    def last_source_route(self):
        """SOURCE_DIRECT (the resize kernel read the source as it lies), SOURCE_PACKED (one launch gathered it tightly packed
        into context scratch first), of the last call on the context that had a source layout; 0 before any."""
        return _lib().lanczos_last_source_route(self._h)

    # -- reduce by whole factors (Pillow's Image.reduce, lanczos_reduce_*)
    def reduce(self, img, factor, box=None):
        """img: uint8 [H][W], [H][W][C] or [F][H][W][C] -> the same layout reduced by `factor` (an int or (fx, fy)) over the
        integer box (x0, y0, x1, y1) (None = the whole frame): bytes identical to Pillow's Image.reduce(factor, box)."""
        if np.asarray(img).dtype == np.uint16:
            raise LanczosError(ERR_BAD_ARG, "reduce: 8-bit samples only (Pillow refuses I;16 as well)")
        x, (f, h, w, c), back = _frames(img, (np.uint8,), "reduce")
        ow, oh = reduce_size(w, h, factor, box)
        entry = _reduce_entry("host", w, h, c, factor, box)
        out = np.empty((f, oh, ow, c), dtype=np.uint8)
        self._call(*entry, x.ctypes.data, out.ctypes.data, f)
        return back(out)

    def reduce_device(self, in_w, in_h, channels, factor, d_in, d_out, frames, box=None, in_frame_stride=0,
                      out_frame_stride=0, stream=None):
        """Device pointers, asynchronous on `stream`; the output is reduce_size(in_w, in_h, factor, box) pixels per frame."""
        entry = _reduce_entry("device", in_w, in_h, channels, factor, box)
        self._call(*entry, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream)

    def resize_force(self, path):
        """RESIZE_AUTO / RESIZE_FUSED / RESIZE_TWO_PASS (tests and A/B runs); RESIZE_CONVERT: as AUTO, but a tensor request takes
        the converted route."""
        self._call("lanczos_resize_force", path)

    def timing_enable(self, on=True):
        self._call("lanczos_timing_enable", 1 if on else 0)

    def timing_read(self):
        n, a, b = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        self._call("lanczos_timing_read", ctypes.byref(n), ctypes.byref(a), ctypes.byref(b))
        return n.value, a.value, b.value

    def last_kernel(self):
        return _lib().lanczos_last_kernel(self._h)

    def last_route(self):
        """How the last upscale call was launched: a Route (main kernel, prefix route, launches, prefix routes seen)."""
        r = _lib().lanczos_last_route(self._h)
        seen = (r >> 8) & 0xff
        return Route(r & 0xf, (r >> 4) & 0xf, (r >> 16) & 0x7fff, frozenset(i for i in range(8) if seen >> i & 1))

    def last_march_table(self):
        """The workgroup table of the last k_march launch of the last upscale call: (MarchTableInfo, int32 array
        [workgroups][segs][4] of (frame, strip, m_b, m_e); m_b >= m_e: an empty segment).  All zero, and an empty array, where
        that call launched no k_march."""
        info = MarchTableInfoC()
        n = _lib().lanczos_last_march_table(self._h, ctypes.byref(info), None, 0)
        if n < 0:
            raise LanczosError(-n, "lanczos_last_march_table")
        tab = np.zeros((info.workgroups, info.segs, 4), np.int32)
        if n:
            assert n == info.workgroups * info.segs
            _lib().lanczos_last_march_table(self._h, ctypes.byref(info), tab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n)
        return MarchTableInfo(*(getattr(info, f) for f in MarchTableInfo._fields)), tab

    def force_kernel(self, family):
        self._call("lanczos_force_kernel", family)


def partition_frames(frames, parts, part):
    f0, cnt = ctypes.c_int(), ctypes.c_int()
    _check(_lib().lanczos_partition_frames(frames, parts, part, ctypes.byref(f0), ctypes.byref(cnt)), "lanczos_partition_frames")
    return f0.value, cnt.value


def partition_rows(desc, parts, part):
    v = [ctypes.c_int() for _ in range(4)]
    _check(_lib().lanczos_partition_rows(ctypes.byref(desc), parts, part, *[ctypes.byref(x) for x in v]), "lanczos_partition_rows")
    return tuple(x.value for x in v)   # out_row0, out_rows, in_row0, in_rows


def exchange_plan(desc, frames, split, n_devices, phase):
    """The scatter (phase 0) / gather (phase 1) of lanczos_resample_multi_root as a list of (src, dst, src_off, dst_off, bytes).
    Host only: no GPU, no RCCL."""
    fn = _lib().lanczos_multi_exchange_plan
    n = fn(ctypes.byref(desc), frames, split, n_devices, phase, None, 0)
    if n < 0:
        raise LanczosError(-n, "lanczos_multi_exchange_plan")
    arr = (Xfer * max(n, 1))()
    n2 = fn(ctypes.byref(desc), frames, split, n_devices, phase, arr, n)
    assert n2 == n
    return [(x.src, x.dst, x.src_off, x.dst_off, x.bytes) for x in arr[:n]]


class MultiContext:
    """lanczos_multi: one context per device of one node (frames or row strips split over them, no data-path collective)."""

    def __init__(self, devices):
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices)
        _check(_lib().lanczos_multi_create(ctypes.byref(self._h), arr, len(devices)), "lanczos_multi_create")

    def close(self):
        if self._h:
            _lib().lanczos_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resample(self, frames_hwc, scale_n, scale_d, a, mode=MODE_LSB1, split=SPLIT_FRAMES):
        x = np.ascontiguousarray(frames_hwc)
        f, h, w, c = x.shape
        d = make_desc(w, h, c, scale_n, scale_d, a, x.dtype.itemsize, mode)
        out = np.empty((f, d.out_h, d.out_w, c), dtype=x.dtype)
        _check(_lib().lanczos_resample_multi_host(self._h, ctypes.byref(d), x.ctypes.data, out.ctypes.data, f, split),
               "lanczos_resample_multi_host")
        return out

    def resample_root(self, desc, d_in_root, d_out_root, frames, split=SPLIT_FRAMES):
        """Device pointers on devices[0]; returns (compute_ms, total_ms)."""
        cm, tm = ctypes.c_double(), ctypes.c_double()
        _check(_lib().lanczos_resample_multi_root(self._h, ctypes.byref(desc), d_in_root, d_out_root, frames, split,
                                                  ctypes.byref(cm), ctypes.byref(tm)), "lanczos_resample_multi_root")
        return cm.value, tm.value


    def exchange_selftest(self, messages=4, nbytes=1 << 20, fail_at=-1):
        """The RCCL exchange machinery on one rank (lanczos_multi_exchange_selftest): returns the C status code and, for
        ERR_RCCL, (rccl_error, message index) from lanczos_multi_last_error."""
        lib = _lib()
        rc = lib.lanczos_multi_exchange_selftest(self._h, messages, nbytes, fail_at)
        he, re_, at = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.lanczos_multi_last_error(self._h, ctypes.byref(he), ctypes.byref(re_), ctypes.byref(at))
        return rc, re_.value, at.value


_default_ctx = None


def lanczos(img, scale_n, scale_d=1, a=3, mode=MODE_LSB1):
    """Module-level convenience mirroring the reference entry point: whole frame in, whole frame out."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx.resample(img, scale_n, scale_d, a, mode)
