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
]
SPLIT_FRAMES, SPLIT_ROWS = 0, 1
YCC_PLANAR, YCC_NV12, YCC_NV21 = 0, 1, 2   # lanczos_ycc_source.layout
YCC_JFIF, YCC_BT601, YCC_BT709 = 0, 1, 2   # the standards of lanczos_ycc_table
YCC_STANDARDS = {"jfif": YCC_JFIF, "bt601": YCC_BT601, "bt709": YCC_BT709}
# the frame layouts Context.resize_ycc knows by name: (layout, sub_x, sub_y)
YCC_LAYOUTS = {"nv12": (YCC_NV12, 1, 1), "nv21": (YCC_NV21, 1, 1), "i420": (YCC_PLANAR, 1, 1), "i422": (YCC_PLANAR, 1, 0),
               "i444": (YCC_PLANAR, 0, 0)}


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


FLIP_H, FLIP_V = 1, 2   # the bits of lanczos_tensor_view.flip and of a d_flip byte
_FLIP_NAMES = {None: 0, "": 0, "h": FLIP_H, "v": FLIP_V, "hv": FLIP_H | FLIP_V, "vh": FLIP_H | FLIP_V}

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
        PD = ctypes.POINTER(Desc)
        c_int, c_void_p, c_size_t, c_double = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double
        PI = ctypes.POINTER(c_int)
        L.lanczos_desc_init.argtypes = [PD] + [c_int] * 7
        L.lanczos_validate.argtypes = [PD]
        L.lanczos_inplace_rows.argtypes = [PD]
        L.lanczos_strip_input_rows.argtypes = [PD, c_int, c_int, PI, PI]
        L.lanczos_in_frame_bytes.argtypes = [PD]
        L.lanczos_in_frame_bytes.restype = c_size_t
        L.lanczos_out_frame_bytes.argtypes = [PD]
        L.lanczos_out_frame_bytes.restype = c_size_t
        L.lanczos_kernel.argtypes = [c_double, c_int]
        L.lanczos_kernel.restype = c_double
        L.lanczos_kernel_idx.argtypes = [c_int] * 5
        L.lanczos_kernel_idx.restype = c_double
        L.lanczos_taps_host.argtypes = [PD, c_int, c_void_p, c_void_p]
        L.lanczos_create.argtypes = [ctypes.POINTER(c_void_p), c_int]
        L.lanczos_destroy.argtypes = [c_void_p]
        L.lanczos_host_alloc.argtypes = [ctypes.POINTER(c_void_p), c_size_t]
        L.lanczos_host_free.argtypes = [c_void_p]
        L.lanczos_resample_host.argtypes = [c_void_p, PD, c_void_p, c_void_p, c_int]
        L.lanczos_resample_device.argtypes = [c_void_p, PD, c_void_p, c_void_p, c_int, c_size_t, c_size_t,
                                              c_void_p]
        L.lanczos_planar_to_interleaved_device.argtypes = [c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]
        L.lanczos_interleaved_to_planar_device.argtypes = [c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]
        L.lanczos_resample_planar_device.argtypes = [c_void_p, PD, c_void_p, c_void_p, c_int, c_void_p]
        L.lanczos_u8.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int]
        L.lanczos_timing_enable.argtypes = [c_void_p, c_int]
        L.lanczos_timing_read.argtypes = [c_void_p, PI, ctypes.POINTER(c_double), ctypes.POINTER(c_double)]
        L.lanczos_last_kernel.argtypes = [c_void_p]
        L.lanczos_last_hip_error.argtypes = [c_void_p]
        if hasattr(L, "lanczos_last_route"):   # (an older build loaded through LANCZOS_LIB has none)
            L.lanczos_last_route.argtypes = [c_void_p]
        if hasattr(L, "lanczos_last_march_table"):
            L.lanczos_last_march_table.argtypes = [c_void_p, ctypes.POINTER(MarchTableInfoC), ctypes.POINTER(ctypes.c_int32), c_int]
        L.lanczos_force_kernel.argtypes = [c_void_p, c_int]
        L.lanczos_strerror.argtypes = [c_int]
        L.lanczos_partition_frames.argtypes = [c_int, c_int, c_int, PI, PI]
        L.lanczos_partition_rows.argtypes = [PD, c_int, c_int, PI, PI, PI, PI]
        L.lanczos_multi_create.argtypes = [ctypes.POINTER(c_void_p), PI, c_int]
        L.lanczos_multi_destroy.argtypes = [c_void_p]
        L.lanczos_multi_devices.argtypes = [c_void_p]
        L.lanczos_resample_multi_host.argtypes = [c_void_p, PD, c_void_p, c_void_p, c_int, c_int]
        L.lanczos_resample_multi_root.argtypes = [c_void_p, PD, c_void_p, c_void_p, c_int, c_int,
                                                  ctypes.POINTER(c_double), ctypes.POINTER(c_double)]
        PRD = ctypes.POINTER(ResizeDesc)
        L.lanczos_resize_desc_init.argtypes = [PRD] + [c_int] * 6
        L.lanczos_resize_desc_init_ex.argtypes = [PRD] + [c_int] * 7
        L.lanczos_resize_validate.argtypes = [PRD]
        L.lanczos_resize_taps_host.argtypes = [PRD, c_int, c_void_p, c_void_p, c_void_p, PI]
        L.lanczos_resize_taps_f64_host.argtypes = [PRD, c_int, c_void_p, c_void_p, c_void_p, PI]
        L.lanczos_resize_device.argtypes = [c_void_p, PRD, c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]
        L.lanczos_resize_host.argtypes = [c_void_p, PRD, c_void_p, c_void_p, c_int]
        L.lanczos_resize_force.argtypes = [c_void_p, c_int]
        L.lanczos_resize_plan_host.argtypes = [PRD, c_int, ctypes.POINTER(ResizePlan)]
        PRO = ctypes.POINTER(ResizeOpts)
        L.lanczos_strerror.restype = ctypes.c_char_p
        L.lanczos_version.argtypes = []
        L.lanczos_version.restype = ctypes.c_char_p
        if os.environ.get("LANCZOS_LIB") and not hasattr(L, "lanczos_resize_opts_init"):
            _LIB = L   # an older build of the ABI (A/B runs): everything up to here is there, box / gap / reduce are not
            return _LIB
        L.lanczos_resize_opts_init.argtypes = [PRO, PRD]
        L.lanczos_resize_taps_host_ex.argtypes = [PRD, PRO, c_int, c_void_p, c_void_p, c_void_p, PI]
        L.lanczos_resize_taps_f64_host_ex.argtypes = [PRD, PRO, c_int, c_void_p, c_void_p, c_void_p, PI]
        L.lanczos_resize_plan_host_ex.argtypes = [PRD, PRO, c_int, ctypes.POINTER(ResizePlanEx)]
        L.lanczos_resize_device_ex.argtypes = [c_void_p, PRD, PRO, c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_void_p]
        L.lanczos_resize_host_ex.argtypes = [c_void_p, PRD, PRO, c_void_p, c_void_p, c_int]
        L.lanczos_reduce_size.argtypes = [c_int] * 4 + [c_void_p, PI, PI]
        L.lanczos_reduce_device.argtypes = [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p, c_int, c_size_t,
                                                                      c_size_t, c_void_p]
        L.lanczos_reduce_host.argtypes = [c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_desc_init_filter"):   # (an older build loaded through LANCZOS_LIB has only Lanczos)
            L.lanczos_resize_desc_init_filter.argtypes = [PRD] + [c_int] * 7
        if hasattr(L, "lanczos_resize_tensor_device"):   # (nor has it the tensor entry)
            PTO = ctypes.POINTER(TensorOut)
            L.lanczos_resize_tensor_validate.argtypes = [PRD, PTO]
            L.lanczos_tensor_lut_normalize.argtypes = [c_int, c_void_p, c_void_p, c_void_p]
            L.lanczos_resize_tensor_device.argtypes = [c_void_p, PRD, PRO, PTO, c_void_p, c_void_p, c_int, c_size_t, c_size_t,
                                                       c_void_p]
            L.lanczos_resize_tensor_host.argtypes = [c_void_p, PRD, PRO, PTO, c_void_p, c_void_p, c_int]
            L.lanczos_last_tensor_route.argtypes = [c_void_p]
        if hasattr(L, "lanczos_resize_tensor16_device"):   # (nor the 16-bit one)
            PTO16 = ctypes.POINTER(TensorOut16)
            L.lanczos_resize_tensor16_validate.argtypes = [PRD, PTO16]
            L.lanczos_tensor_lut_convert16.argtypes = [c_void_p, c_int, c_int, c_void_p]
            L.lanczos_tensor16_lut_normalize.argtypes = [c_int, c_void_p, c_void_p, c_int, c_void_p]
            L.lanczos_resize_tensor16_device.argtypes = [c_void_p, PRD, PRO, PTO16, c_void_p, c_void_p, c_int, c_size_t,
                                                         c_size_t, c_void_p]
            L.lanczos_resize_tensor16_host.argtypes = [c_void_p, PRD, PRO, PTO16, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_window_device"):   # (nor the window of the output)
            PRW = ctypes.POINTER(ResizeWindow)
            L.lanczos_resize_window_init.argtypes = [PRW, PRD]
            L.lanczos_resize_window_validate.argtypes = [PRD, PRW]
            L.lanczos_resize_window_source.argtypes = [PRD, PRO, PRW, c_void_p]
            L.lanczos_resize_window_plan_host.argtypes = [PRD, PRO, PRW, c_int, ctypes.POINTER(ResizePlanEx)]
            L.lanczos_resize_window_device.argtypes = [c_void_p, PRD, PRO, PRW, c_void_p, c_void_p, c_int, c_size_t, c_size_t,
                                                       c_void_p]
            L.lanczos_resize_window_host.argtypes = [c_void_p, PRD, PRO, PRW, c_void_p, c_void_p, c_int]
            L.lanczos_resize_tensor_window_validate.argtypes = [PRD, PRW, PTO]
            L.lanczos_resize_tensor16_window_validate.argtypes = [PRD, PRW, PTO16]
            L.lanczos_resize_tensor_window_device.argtypes = [c_void_p, PRD, PRO, PRW, PTO, c_void_p, c_void_p, c_int, c_size_t,
                                                              c_size_t, c_void_p]
            L.lanczos_resize_tensor_window_host.argtypes = [c_void_p, PRD, PRO, PRW, PTO, c_void_p, c_void_p, c_int]
            L.lanczos_resize_tensor16_window_device.argtypes = [c_void_p, PRD, PRO, PRW, PTO16, c_void_p, c_void_p, c_int,
                                                                c_size_t, c_size_t, c_void_p]
            L.lanczos_resize_tensor16_window_host.argtypes = [c_void_p, PRD, PRO, PRW, PTO16, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_tensor_view_device"):   # (nor the view)
            PTV = ctypes.POINTER(TensorView)
            L.lanczos_tensor_view_init.argtypes = [PTV, PRD, c_int]
            L.lanczos_resize_tensor_view_validate.argtypes = [PRD, PRW, PTV]
            L.lanczos_resize_tensor_view_device.argtypes = [c_void_p, PRD, PRO, PRW, PTV, c_void_p, c_void_p, c_int, c_size_t,
                                                            c_size_t, c_void_p]
            L.lanczos_resize_tensor_view_host.argtypes = [c_void_p, PRD, PRO, PRW, PTV, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_tensor_crops_device"):   # (nor a crop origin per frame)
            PRC = ctypes.POINTER(ResizeCrops)
            L.lanczos_resize_crops_validate.argtypes = [PRD, PRC]
            L.lanczos_resize_crops_plan_host.argtypes = [PRD, PRO, PRC, c_int, ctypes.POINTER(ResizePlanEx)]
            L.lanczos_resize_tensor_crops_validate.argtypes = [PRD, PRC, PTV]
            L.lanczos_resize_tensor_crops_device.argtypes = [c_void_p, PRD, PRO, PRC, PTV, c_void_p, c_void_p, c_int, c_size_t,
                                                             c_size_t, c_void_p]
            L.lanczos_resize_tensor_crops_host.argtypes = [c_void_p, PRD, PRO, PRC, PTV, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_source_device"):   # (nor a source layout)
            PRS = ctypes.POINTER(ResizeSource)
            L.lanczos_resize_source_init.argtypes = [PRS, PRD, c_int]
            L.lanczos_resize_source_validate.argtypes = [PRD, PRS]
            L.lanczos_resize_source_device.argtypes = [c_void_p, PRD, PRO, PRW, PRS, c_void_p, c_void_p, c_int, c_size_t, c_size_t,
                                                       c_void_p]
            L.lanczos_resize_tensor_source_device.argtypes = [c_void_p, PRD, PRO, PRW, PRC, PRS, PTV, c_void_p, c_void_p, c_int,
                                                              c_size_t, c_size_t, c_void_p]
            L.lanczos_resize_source_host.argtypes = [c_void_p, PRD, PRO, PRW, PRS, c_void_p, c_void_p, c_int]
            L.lanczos_resize_tensor_source_host.argtypes = [c_void_p, PRD, PRO, PRW, PRC, PRS, PTV, c_void_p, c_void_p, c_int]
            L.lanczos_last_source_route.argtypes = [c_void_p]
        if hasattr(L, "lanczos_resize_dest_device"):   # (nor a destination layout)
            PRT = ctypes.POINTER(ResizeDest)
            L.lanczos_resize_dest_init.argtypes = [PRT, PRD, PRW, c_int]
            L.lanczos_resize_dest_validate.argtypes = [PRD, PRW, PRT]
            L.lanczos_resize_dest_device.argtypes = [c_void_p, PRD, PRO, PRW, PRS, PRT, c_void_p, c_void_p, c_int, c_size_t,
                                                     c_size_t, c_void_p]
            L.lanczos_resize_dest_host.argtypes = [c_void_p, PRD, PRO, PRW, PRS, PRT, c_void_p, c_void_p, c_int]
            L.lanczos_last_dest_route.argtypes = [c_void_p]
        if hasattr(L, "lanczos_resize_tensor_norm_device"):   # (nor 16-bit and float samples into tensors)
            PTN = ctypes.POINTER(TensorNorm)
            L.lanczos_tensor_norm_init.argtypes = [PTN, PRD, c_int, c_int]
            L.lanczos_resize_tensor_norm_validate.argtypes = [PRD, PRW, PTN]
            L.lanczos_resize_tensor_norm_device.argtypes = [c_void_p, PRD, PRO, PRW, PRS, PTN, c_void_p, c_void_p, c_int, c_size_t,
                                                            c_size_t, c_void_p]
            L.lanczos_resize_tensor_norm_host.argtypes = [c_void_p, PRD, PRO, PRW, PRS, PTN, c_void_p, c_void_p, c_int]
        if hasattr(L, "lanczos_resize_ycc_device"):   # (nor YCbCr frames)
            PYS = ctypes.POINTER(YccSource)
            L.lanczos_ycc_source_init.argtypes = [PYS, PRD, c_int, c_int, c_int]
            L.lanczos_ycc_source_validate.argtypes = [PRD, PYS]
            L.lanczos_ycc_table.argtypes = [c_int, c_void_p]
            L.lanczos_resize_ycc_device.argtypes = [c_void_p, PRD, PRO, PRW, PYS, c_void_p, c_void_p, c_void_p, c_int, c_size_t,
                                                    c_size_t, c_void_p]
            L.lanczos_resize_ycc_tensor_device.argtypes = [c_void_p, PRD, PRO, PRW, PYS, c_void_p, PTV, c_void_p, c_void_p, c_int,
                                                           c_size_t, c_size_t, c_void_p]
            L.lanczos_resize_ycc_host.argtypes = [c_void_p, PRD, PRO, PRW, PYS, c_void_p, c_void_p, c_void_p, c_int]
            L.lanczos_resize_ycc_tensor_host.argtypes = [c_void_p, PRD, PRO, PRW, PYS, c_void_p, PTV, c_void_p, c_void_p, c_int]
            L.lanczos_last_ycc_info.argtypes = [c_void_p, ctypes.POINTER(YccInfoC)]
        L.lanczos_strerror.restype = ctypes.c_char_p
        L.lanczos_version.argtypes = []
        L.lanczos_version.restype = ctypes.c_char_p
        _LIB = L
    return _LIB


def _check(rc, what):
    if rc != OK:
        raise LanczosError(rc, what)


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
    return ctypes.byref(opts) if opts is not None else None


def resize_taps_host(desc, axis, box=None, reducing_gap=None, opts=None):
    """Fixed-point tables of one axis (0 = horizontal, 1 = vertical): (first[out], count[out], coeffs[out][ksize]) int32.
    With a box and / or a gap (or a ready ResizeOpts) the tables of the resize that remains: lanczos_resize_taps_host_ex."""
    ks = ctypes.c_int()
    if box is None and reducing_gap is None and opts is None:
        fn = lambda *a: _lib().lanczos_resize_taps_host(ctypes.byref(desc), axis, *a)
    else:
        ref = _opts_ref(desc, box, reducing_gap, opts)
        fn = lambda *a: _lib().lanczos_resize_taps_host_ex(ctypes.byref(desc), ref, axis, *a)
    _check(fn(None, None, None, ctypes.byref(ks)), "lanczos_resize_taps_host")
    n = desc.out_w if axis == 0 else desc.out_h
    first = np.empty(n, dtype=np.int32)
    count = np.empty(n, dtype=np.int32)
    coeffs = np.empty((n, ks.value), dtype=np.int32)
    _check(fn(first.ctypes.data, count.ctypes.data, coeffs.ctypes.data, ctypes.byref(ks)), "lanczos_resize_taps_host")
    return first, count, coeffs


def resize_taps_f64_host(desc, axis, box=None, reducing_gap=None, opts=None):
    """Double tables of one axis, what 16-bit and float requests run on: (first[out] int32, count[out] int32, coeffs[out][ksize]
    float64); first and count are those of resize_taps_host.  box / reducing_gap / opts as resize_taps_host."""
    ks = ctypes.c_int()
    if box is None and reducing_gap is None and opts is None:
        fn = lambda *a: _lib().lanczos_resize_taps_f64_host(ctypes.byref(desc), axis, *a)
    else:
        ref = _opts_ref(desc, box, reducing_gap, opts)
        fn = lambda *a: _lib().lanczos_resize_taps_f64_host_ex(ctypes.byref(desc), ref, axis, *a)
    _check(fn(None, None, None, ctypes.byref(ks)), "lanczos_resize_taps_f64_host")
    n = desc.out_w if axis == 0 else desc.out_h
    first = np.empty(n, dtype=np.int32)
    count = np.empty(n, dtype=np.int32)
    coeffs = np.empty((n, ks.value), dtype=np.float64)
    _check(fn(first.ctypes.data, count.ctypes.data, coeffs.ctypes.data, ctypes.byref(ks)), "lanczos_resize_taps_f64_host")
    return first, count, coeffs


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
    cp = ctypes.byref(crops) if crops is not None else None
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


def resize_source(desc, layout="planar", row_stride=None, chan_stride=None):
    """A ResizeSource for `desc`: layout "planar" (N x C x H x W bytes, what torchvision.io.decode_jpeg(device=) returns) or
    "interleaved"; row_stride / chan_stride in bytes replace the tight layout's (pitched rows, padded planes).  Validated where it
    is used (resize_source_validate); a ready ResizeSource is returned as it is."""
    if isinstance(layout, ResizeSource):
        return layout
    kinds = {"interleaved": SOURCE_INTERLEAVED, "planar": SOURCE_PLANAR}
    if layout not in kinds:
        raise LanczosError(ERR_BAD_ARG, f"resize_source: layout is 'planar' or 'interleaved', not {layout!r}")
    s = ResizeSource()
    _check(_lib().lanczos_resize_source_init(ctypes.byref(s), ctypes.byref(desc), kinds[layout]), "lanczos_resize_source_init")
    if row_stride is not None:
        if chan_stride is None and layout == "planar":   # the planes stay back to back
            chan_stride = int(row_stride) * desc.in_h
        s.row_stride = int(row_stride)
    if chan_stride is not None:
        s.chan_stride = int(chan_stride)
    return s


def resize_source_validate(desc, source):
    """lanczos_resize_source_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the layout is refused."""
    _check(_lib().lanczos_resize_source_validate(ctypes.byref(desc), ctypes.byref(source) if source is not None else None),
           "lanczos_resize_source_validate")


def resize_dest(desc, layout="planar", row_stride=None, chan_stride=None, window=None):
    """A ResizeDest for the result of `desc` (its window, where one is given): layout "planar" (N x C x H x W bytes, what a torch
    stage takes) or "interleaved"; row_stride / chan_stride in bytes replace the tight layout's (pitched rows, padded planes).
    Validated where it is used (resize_dest_validate); a ready ResizeDest is returned as it is."""
    if isinstance(layout, ResizeDest):
        return layout
    kinds = {"interleaved": DEST_INTERLEAVED, "planar": DEST_PLANAR}
    if layout not in kinds:
        raise LanczosError(ERR_BAD_ARG, f"resize_dest: layout is 'planar' or 'interleaved', not {layout!r}")
    t = ResizeDest()
    _check(_lib().lanczos_resize_dest_init(ctypes.byref(t), ctypes.byref(desc), _window_ref(desc, window), kinds[layout]),
           "lanczos_resize_dest_init")
    if row_stride is not None:
        if chan_stride is None and layout == "planar":   # the planes stay back to back
            chan_stride = int(row_stride) * resize_window(desc, window).h
        t.row_stride = int(row_stride)
    if chan_stride is not None:
        t.chan_stride = int(chan_stride)
    return t


def resize_dest_validate(desc, dest, window=None):
    """lanczos_resize_dest_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the layout is refused."""
    _check(_lib().lanczos_resize_dest_validate(ctypes.byref(desc), _window_ref(desc, window),
                                               ctypes.byref(dest) if dest is not None else None), "lanczos_resize_dest_validate")


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
    _check(_lib().lanczos_ycc_source_validate(ctypes.byref(desc), ctypes.byref(source) if source is not None else None),
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


def _ycc_table_arg(standard, table, what):
    if table is None:
        return ycc_table(standard)
    table = np.ascontiguousarray(table)
    if table.dtype != np.int32 or table.shape != (3, 3, 256):
        raise LanczosError(ERR_BAD_ARG, f"{what}: the colour table is int32 [3][3][256]")
    return table


def _planar_frames(img, what):
    """uint8 (C, H, W) or (N, C, H, W) -> a contiguous (N, C, H, W) array"""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim not in (3, 4):
        raise LanczosError(ERR_BAD_ARG, f"{what}: planar=True takes a uint8 [C][H][W] or [F][C][H][W] array")
    return img if img.ndim == 4 else img[None]


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


def tensor_out(d_lut, strides):
    """A TensorOut: d_lut a pointer to channels * 256 floats (device memory for the device entry), strides =
    (chan_stride, row_stride, pix_stride) in floats.  Validated where it is used (resize_tensor_validate)."""
    t = TensorOut()
    t.d_lut = d_lut
    t.chan_stride, t.row_stride, t.pix_stride = (int(v) for v in strides)
    return t


def tensor16_out(d_lut, strides):
    """A TensorOut16: d_lut a pointer to channels * 256 16-bit words (device memory for the device entry), strides =
    (chan_stride, row_stride, pix_stride) in elements.  Validated where it is used (resize_tensor16_validate)."""
    t = TensorOut16()
    t.d_lut = d_lut
    t.chan_stride, t.row_stride, t.pix_stride = (int(v) for v in strides)
    return t


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
    v.chan_stride, v.row_stride, v.pix_stride = (int(x) for x in strides)
    v.elem_bytes = int(elem_bytes)
    src = [int(c) for c in channels_out]
    if len(src) > 4:
        raise LanczosError(ERR_BAD_ARG, "tensor_view: at most four output channels")
    v.out_channels = len(src)
    for oc, sc in enumerate(src):
        v.src_channel[oc] = sc
    v.flip = _FLIP_NAMES[flip] if flip in _FLIP_NAMES else int(flip)
    v.d_flip = d_flip
    return v


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
    n.chan_stride, n.row_stride, n.pix_stride = (int(x) for x in strides)
    n.format = _TENSOR_NORM_FORMATS[dtype]
    n.out_channels = len(src)
    for oc, sc in enumerate(src):
        n.src_channel[oc] = sc
    n.flip = _FLIP_NAMES[flip] if flip in _FLIP_NAMES else int(flip)
    n.d_flip = d_flip
    return n


def resize_tensor_norm_validate(desc, n, window=None):
    """lanczos_resize_tensor_norm_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame."""
    _check(_lib().lanczos_resize_tensor_norm_validate(ctypes.byref(desc), _window_ref(desc, window),
                                                      ctypes.byref(n) if n is not None else None),
           "lanczos_resize_tensor_norm_validate")


def resize_tensor_view_validate(desc, v, window=None):
    """lanczos_resize_tensor_view_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the view is refused.
    window: the strides describe that window's frame."""
    _check(_lib().lanczos_resize_tensor_view_validate(ctypes.byref(desc), _window_ref(desc, window),
                                                      ctypes.byref(v) if v is not None else None),
           "lanczos_resize_tensor_view_validate")


def resize_tensor16_validate(desc, t, window=None):
    """lanczos_resize_tensor16_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame (lanczos_resize_tensor16_window_validate)."""
    tp = ctypes.byref(t) if t is not None else None
    if window is None:
        _check(_lib().lanczos_resize_tensor16_validate(ctypes.byref(desc), tp), "lanczos_resize_tensor16_validate")
    else:
        _check(_lib().lanczos_resize_tensor16_window_validate(ctypes.byref(desc), _window_ref(desc, window), tp),
               "lanczos_resize_tensor16_window_validate")


def resize_tensor_validate(desc, t, window=None):
    """lanczos_resize_tensor_validate: raises LanczosError (ERR_BAD_ARG / ERR_UNSUPPORTED) where the request is refused.
    window: the strides describe that window's frame (lanczos_resize_tensor_window_validate)."""
    tp = ctypes.byref(t) if t is not None else None
    if window is None:
        _check(_lib().lanczos_resize_tensor_validate(ctypes.byref(desc), tp), "lanczos_resize_tensor_validate")
    else:
        _check(_lib().lanczos_resize_tensor_window_validate(ctypes.byref(desc), _window_ref(desc, window), tp),
               "lanczos_resize_tensor_window_validate")


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


class Context:
    """One lanczos_ctx: a device, a stream, resident tap tables.  Not shared between threads."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(_lib().lanczos_create(ctypes.byref(self._h), device), "lanczos_create")

    def close(self):
        if self._h:
            _lib().lanczos_destroy(self._h)
            self._h = ctypes.c_void_p()

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
        _check(_lib().lanczos_resample_host(self._h, ctypes.byref(d), x.ctypes.data, out.ctypes.data, f),
               "lanczos_resample_host")
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
        _check(_lib().lanczos_resample_host(self._h, ctypes.byref(desc), strip_in.ctypes.data,
                                            out.ctypes.data, 1), "lanczos_resample_host")
        return out

    def u8(self, img, out_w, out_h, a):
        """lanczos_u8: the reference's call shape (sizes as ints, scale = out_w/in_w reduced)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, c = img.shape
        out = np.empty((out_h, out_w, c), dtype=np.uint8)
        _check(_lib().lanczos_u8(self._h, img.ctypes.data, w, h, c, out.ctypes.data, out_w, out_h, a),
               "lanczos_u8")
        return out

    # -- device buffers (raw pointers, e.g. torch tensors' data_ptr()), asynchronous
    def resample_device(self, desc, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None):
        _check(_lib().lanczos_resample_device(self._h, ctypes.byref(desc), d_in, d_out, frames,
                                              in_frame_stride, out_frame_stride, stream),
               "lanczos_resample_device")

    # -- planar frames [C][H][W] (the reference's img_in / img_out_ex arrays, full_TB.h:20-21), device pointers
    def planar_to_interleaved_device(self, d_planar, d_inter, w, h, channels, bytes_per_sample, frames, stream=None):
        _check(_lib().lanczos_planar_to_interleaved_device(self._h, d_planar, d_inter, w, h, channels,
                                                           bytes_per_sample, frames, stream),
               "lanczos_planar_to_interleaved_device")

    def interleaved_to_planar_device(self, d_inter, d_planar, w, h, channels, bytes_per_sample, frames, stream=None):
        _check(_lib().lanczos_interleaved_to_planar_device(self._h, d_inter, d_planar, w, h, channels,
                                                           bytes_per_sample, frames, stream),
               "lanczos_interleaved_to_planar_device")

    def resample_planar_device(self, desc, d_in_planar, d_out_planar, frames, stream=None):
        _check(_lib().lanczos_resample_planar_device(self._h, ctypes.byref(desc), d_in_planar, d_out_planar, frames,
                                                     stream), "lanczos_resample_planar_device")

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
        if planar_out:
            if planar:
                x = _planar_frames(img, "resize")
                f, c, h, w = x.shape
            else:
                x = np.ascontiguousarray(img)
                if x.dtype != np.uint8 or x.ndim not in (3, 4) or x.shape[-1] not in (3, 4):
                    raise LanczosError(ERR_BAD_ARG, "resize: planar_out=True takes uint8 frames of 3 or 4 channels")
                x = x if x.ndim == 4 else x[None]
                f, h, w, c = x.shape
            d = resize_desc(w, h, out_w, out_h, c, a, alpha, filter=filter)
            win = resize_window(d, window)
            wref = ctypes.byref(win) if window is not None else None
            out = np.empty((f, c, win.h, win.w), dtype=np.uint8)
            _check(_lib().lanczos_resize_dest_host(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None), wref,
                                                   ctypes.byref(resize_source(d, "planar")) if planar else None,
                                                   ctypes.byref(resize_dest(d, "planar", window=window)), x.ctypes.data,
                                                   out.ctypes.data, f), "lanczos_resize_dest_host")
            return out if np.ndim(img) == 4 else out[0]
        if planar:
            x = _planar_frames(img, "resize")
            f, c, h, w = x.shape
            d = resize_desc(w, h, out_w, out_h, c, a, alpha, filter=filter)
            win = resize_window(d, window)
            out = np.empty((f, win.h, win.w, c), dtype=np.uint8)
            _check(_lib().lanczos_resize_source_host(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None),
                                                     ctypes.byref(win) if window is not None else None,
                                                     ctypes.byref(resize_source(d, "planar")), x.ctypes.data, out.ctypes.data, f),
                   "lanczos_resize_source_host")
            return out if np.ndim(img) == 4 else out[0]
        img = np.ascontiguousarray(img)
        if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3, 4):
            raise LanczosError(ERR_BAD_ARG, "resize: expected a uint8 or uint16 [H][W], [H][W][C] or [F][H][W][C] array")
        x = img.reshape(img.shape + (1,)) if img.ndim == 2 else img
        x = x if x.ndim == 4 else x[None]
        f, h, w, c = x.shape
        d = resize_desc(w, h, out_w, out_h, c, a, alpha, 8 * img.dtype.itemsize, filter=filter)
        win = resize_window(d, window)
        out = np.empty((f, win.h, win.w, c), dtype=img.dtype)
        if window is not None:
            _check(_lib().lanczos_resize_window_host(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None),
                                                     ctypes.byref(win), x.ctypes.data, out.ctypes.data, f),
                   "lanczos_resize_window_host")
        elif box is None and reducing_gap is None:
            _check(_lib().lanczos_resize_host(self._h, ctypes.byref(d), x.ctypes.data, out.ctypes.data, f),
                   "lanczos_resize_host")
        else:
            _check(_lib().lanczos_resize_host_ex(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None),
                                                 x.ctypes.data, out.ctypes.data, f), "lanczos_resize_host_ex")
        if img.ndim == 2:
            return out[0, :, :, 0]
        return out if img.ndim == 4 else out[0]

    def resize_f32(self, img, out_w, out_h, a=3, box=None, filter=FILTER_LANCZOS, window=None):
        """filter and window as Context.resize.
        img: float32 [H][W], [H][W][C] or [F][H][W][C] (C = 1, 3 or 4) -> the same layout at out_h x out_w, every channel
        bit for bit what Pillow's Image.resize((out_w, out_h), Image.LANCZOS, box) gives for it as a mode F plane (a = 3):
        double accumulation over exactly the window's taps, stored as float -- no clamp, inf on overflow, denormals kept, NaN
        where Pillow has NaN.  box as Context.resize.  No alpha and no reducing_gap for floats."""
        img = np.ascontiguousarray(img)
        if img.dtype != np.float32 or img.ndim not in (2, 3, 4):
            raise LanczosError(ERR_BAD_ARG, "resize_f32: expected a float32 [H][W], [H][W][C] or [F][H][W][C] array")
        x = img.reshape(img.shape + (1,)) if img.ndim == 2 else img
        x = x if x.ndim == 4 else x[None]
        f, h, w, c = x.shape
        d = resize_desc(w, h, out_w, out_h, c, a, f32=True, filter=filter)
        win = resize_window(d, window)
        out = np.empty((f, win.h, win.w, c), dtype=np.float32)
        if window is not None:
            _check(_lib().lanczos_resize_window_host(self._h, ctypes.byref(d), _opts_ref(d, box, None, None),
                                                     ctypes.byref(win), x.ctypes.data, out.ctypes.data, f),
                   "lanczos_resize_window_host")
        elif box is None:
            _check(_lib().lanczos_resize_host(self._h, ctypes.byref(d), x.ctypes.data, out.ctypes.data, f),
                   "lanczos_resize_host")
        else:
            _check(_lib().lanczos_resize_host_ex(self._h, ctypes.byref(d), _opts_ref(d, box, None, None),
                                                 x.ctypes.data, out.ctypes.data, f), "lanczos_resize_host_ex")
        if img.ndim == 2:
            return out[0, :, :, 0]
        return out if img.ndim == 4 else out[0]

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
        if dest is not None:
            _check(_lib().lanczos_resize_dest_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                     _window_ref(desc, window), ctypes.byref(source) if source is not None else None,
                                                     ctypes.byref(dest), d_in, d_out, frames, in_frame_stride, out_frame_stride,
                                                     stream), "lanczos_resize_dest_device")
        elif source is not None:
            _check(_lib().lanczos_resize_source_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                       _window_ref(desc, window), ctypes.byref(source), d_in, d_out, frames,
                                                       in_frame_stride, out_frame_stride, stream), "lanczos_resize_source_device")
        elif window is not None:
            _check(_lib().lanczos_resize_window_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                       _window_ref(desc, window), d_in, d_out, frames, in_frame_stride,
                                                       out_frame_stride, stream), "lanczos_resize_window_device")
        elif box is None and reducing_gap is None and opts is None:
            _check(_lib().lanczos_resize_device(self._h, ctypes.byref(desc), d_in, d_out, frames, in_frame_stride,
                                                out_frame_stride, stream), "lanczos_resize_device")
        else:
            _check(_lib().lanczos_resize_device_ex(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                   d_in, d_out, frames, in_frame_stride, out_frame_stride, stream),
                   "lanczos_resize_device_ex")

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
        if planar:
            x = _planar_frames(img, "resize_tensor")
            f, c, h, w = x.shape
            img = x if np.ndim(img) == 4 else x[0]
        else:
            img = np.ascontiguousarray(img)
            if img.dtype != np.uint8 or img.ndim not in (2, 3, 4):
                raise LanczosError(ERR_BAD_ARG, "resize_tensor: expected a uint8 [H][W], [H][W][C] or [F][H][W][C] array")
            x = img.reshape(img.shape + (1,)) if img.ndim == 2 else img
            x = x if x.ndim == 4 else x[None]
            f, h, w, c = x.shape
        d = resize_desc(w, h, out_w, out_h, c, a, alpha, filter=filter)
        view = planar or channels_out is not None or flip is not None
        if channels_out is not None:
            channels_out = tuple(int(v) for v in channels_out)
            if not 1 <= len(channels_out) <= c:
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor: channels_out names 1 to {c} source channels")
            c = len(channels_out)
        if lut is None:
            if c == 2:   # lanczos_tensor_lut_normalize builds 1, 3 or 4 channels: two rows of one
                m, s = (None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float32), (2,)) for v in (mean, std))
                lut = np.concatenate([normalize_lut(1, None if m is None else m[k], None if s is None else s[k], dtype)
                                      for k in range(2)])
            else:
                lut = normalize_lut(c, mean, std, dtype)
        elif mean is not None or std is not None:
            raise LanczosError(ERR_BAD_ARG, "resize_tensor: a table or mean / std, not both")
        lut = np.ascontiguousarray(lut)
        if lut.dtype not in ((np.float32,) if wide else (np.uint16, np.float16)) or lut.size != c * 256:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor: the table is {'float32' if wide else 'uint16 or float16'} [{c}][256]")
        if (crop is None) != (origins is None) or (crop is not None and window is not None):
            raise LanczosError(ERR_BAD_ARG, "resize_tensor: crop= and origins= come together, and not with window=")
        org = None
        if crop is not None:
            org = np.ascontiguousarray(origins)
            if len(crop) != 2 or org.shape != (f, 2) or org.dtype.kind not in "iu":
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor: crop is (w, h) and origins {f} integer pairs (x0, y0)")
            org = org.astype(np.int32)
            window = (0, 0, int(crop[0]), int(crop[1]))   # the frame the strides describe
            view = True
        win = resize_window(d, window)
        strides = tensor_strides(layout, win.w, win.h, c)
        shape = (f, c, win.h, win.w) if layout == "chw" else (f, win.h, win.w, c)
        opts = _opts_ref(d, box, reducing_gap, None)
        wref = ctypes.byref(win) if window is not None else None
        if view:
            flips = None
            if flip is not None and not isinstance(flip, str):
                flips = np.ascontiguousarray(flip)
                if flips.shape != (f,) or flips.dtype.kind not in "iub" or ((flips < 0) | (flips > 3)).any():
                    raise LanczosError(ERR_BAD_ARG, f"resize_tensor: flip is 'h', 'v', 'hv' or {f} integers 0 .. 3, one per frame")
                flips = flips.astype(np.uint8)
            elif flip not in _FLIP_NAMES:
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor: flip is 'h', 'v', 'hv' or one integer per frame, not {flip!r}")
            v = tensor_view(lut.ctypes.data, strides, 4 if wide else 2,
                            channels_out if channels_out is not None else tuple(range(c)),
                            0 if flips is not None else flip, flips.ctypes.data if flips is not None else None)
            out = np.empty(shape, dtype=np.float32 if wide else np.uint16)
            if planar:
                cr = resize_crops(win.w, win.h, org.ctypes.data) if org is not None else None
                _check(_lib().lanczos_resize_tensor_source_host(self._h, ctypes.byref(d), opts, None if cr is not None else wref,
                                                                ctypes.byref(cr) if cr is not None else None,
                                                                ctypes.byref(resize_source(d, "planar")), ctypes.byref(v),
                                                                x.ctypes.data, out.ctypes.data, f),
                       "lanczos_resize_tensor_source_host")
            elif org is not None:
                cr = resize_crops(win.w, win.h, org.ctypes.data)
                _check(_lib().lanczos_resize_tensor_crops_host(self._h, ctypes.byref(d), opts, ctypes.byref(cr), ctypes.byref(v),
                                                               x.ctypes.data, out.ctypes.data, f),
                       "lanczos_resize_tensor_crops_host")
            else:
                _check(_lib().lanczos_resize_tensor_view_host(self._h, ctypes.byref(d), opts, wref, ctypes.byref(v), x.ctypes.data,
                                                              out.ctypes.data, f), "lanczos_resize_tensor_view_host")
            out = out if wide else _tensor16_array(out, dtype)
        elif wide:
            t = tensor_out(lut.ctypes.data, strides)
            out = np.empty(shape, dtype=np.float32)
            if wref is None:
                _check(_lib().lanczos_resize_tensor_host(self._h, ctypes.byref(d), opts, ctypes.byref(t), x.ctypes.data,
                                                         out.ctypes.data, f), "lanczos_resize_tensor_host")
            else:
                _check(_lib().lanczos_resize_tensor_window_host(self._h, ctypes.byref(d), opts, wref, ctypes.byref(t),
                                                                x.ctypes.data, out.ctypes.data, f),
                       "lanczos_resize_tensor_window_host")
        else:
            t = tensor16_out(lut.ctypes.data, strides)
            out = np.empty(shape, dtype=np.uint16)
            if wref is None:
                _check(_lib().lanczos_resize_tensor16_host(self._h, ctypes.byref(d), opts, ctypes.byref(t), x.ctypes.data,
                                                           out.ctypes.data, f), "lanczos_resize_tensor16_host")
            else:
                _check(_lib().lanczos_resize_tensor16_window_host(self._h, ctypes.byref(d), opts, wref, ctypes.byref(t),
                                                                  x.ctypes.data, out.ctypes.data, f),
                       "lanczos_resize_tensor16_window_host")
            out = _tensor16_array(out, dtype)
        return out if img.ndim == 4 else out[0]

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
        oref = _opts_ref(desc, box, reducing_gap, opts)
        if crop is not None and window is not None:
            raise LanczosError(ERR_BAD_ARG, "resize_tensor_device: crop= or window=, not both")
        if (crop is None or not isinstance(crop, ResizeCrops)) and (crop is None) != (d_origin is None):
            raise LanczosError(ERR_BAD_ARG, "resize_tensor_device: crop=(w, h) and d_origin= come together")
        wref = _window_ref(desc, window)
        if source is not None and isinstance(strides, (TensorOut, TensorOut16)):   # the same request as a view
            t = strides
            strides = tensor_view(t.d_lut, (t.chan_stride, t.row_stride, t.pix_stride), 2 if isinstance(t, TensorOut16) else 4,
                                  tuple(range(desc.channels)))
        if source is not None or crop is not None or isinstance(strides, TensorView) or channels_out is not None or flip is not None or d_flip is not None:
            if isinstance(strides, TensorView):
                v = strides
            else:
                if dtype != "float32":
                    _tensor16_format(dtype, "resize_tensor_device")
                v = tensor_view(d_lut, strides, 4 if dtype == "float32" else 2,
                                channels_out if channels_out is not None else tuple(range(desc.channels)), flip or 0, d_flip)
            if source is not None:
                cr = None if crop is None else crop if isinstance(crop, ResizeCrops) else resize_crops(crop[0], crop[1], d_origin)
                _check(_lib().lanczos_resize_tensor_source_device(self._h, ctypes.byref(desc), oref, wref,
                                                                  ctypes.byref(cr) if cr is not None else None, ctypes.byref(source),
                                                                  ctypes.byref(v), d_in, d_out, frames, in_frame_stride,
                                                                  out_frame_stride, stream), "lanczos_resize_tensor_source_device")
                return
            if crop is not None:
                cr = crop if isinstance(crop, ResizeCrops) else resize_crops(crop[0], crop[1], d_origin)
                _check(_lib().lanczos_resize_tensor_crops_device(self._h, ctypes.byref(desc), oref, ctypes.byref(cr), ctypes.byref(v),
                                                                 d_in, d_out, frames, in_frame_stride, out_frame_stride, stream),
                       "lanczos_resize_tensor_crops_device")
                return
            _check(_lib().lanczos_resize_tensor_view_device(self._h, ctypes.byref(desc), oref, wref, ctypes.byref(v), d_in,
                                                            d_out, frames, in_frame_stride, out_frame_stride, stream),
                   "lanczos_resize_tensor_view_device")
            return
        if isinstance(strides, TensorOut16) or dtype != "float32":
            if not isinstance(strides, TensorOut16):
                _tensor16_format(dtype, "resize_tensor_device")
            t = strides if isinstance(strides, TensorOut16) else tensor16_out(d_lut, strides)
            if wref is None:
                _check(_lib().lanczos_resize_tensor16_device(self._h, ctypes.byref(desc), oref, ctypes.byref(t), d_in, d_out,
                                                             frames, in_frame_stride, out_frame_stride, stream),
                       "lanczos_resize_tensor16_device")
            else:
                _check(_lib().lanczos_resize_tensor16_window_device(self._h, ctypes.byref(desc), oref, wref, ctypes.byref(t),
                                                                    d_in, d_out, frames, in_frame_stride, out_frame_stride,
                                                                    stream), "lanczos_resize_tensor16_window_device")
            return
        t = strides if isinstance(strides, TensorOut) else tensor_out(d_lut, strides)
        if wref is None:
            _check(_lib().lanczos_resize_tensor_device(self._h, ctypes.byref(desc), oref, ctypes.byref(t), d_in, d_out, frames,
                                                       in_frame_stride, out_frame_stride, stream),
                   "lanczos_resize_tensor_device")
        else:
            _check(_lib().lanczos_resize_tensor_window_device(self._h, ctypes.byref(desc), oref, wref, ctypes.byref(t), d_in,
                                                              d_out, frames, in_frame_stride, out_frame_stride, stream),
                   "lanczos_resize_tensor_window_device")

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
        img = np.ascontiguousarray(img)
        if img.dtype not in (np.uint16, np.float32) or img.ndim not in (2, 3, 4):
            raise LanczosError(ERR_BAD_ARG, "resize_tensor_norm: expected a uint16 or float32 [H][W], [H][W][C] or [F][H][W][C] array")
        if dtype not in _TENSOR_NORM_FORMATS:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: dtype is 'float32', 'bfloat16' or 'float16', not {dtype!r}")
        x = img.reshape(img.shape + (1,)) if img.ndim == 2 else img
        x = x if x.ndim == 4 else x[None]
        f, h, w, c = x.shape
        u16 = img.dtype == np.uint16
        d = resize_desc(w, h, out_w, out_h, c, a, bits=16 if u16 else 8, f32=not u16, filter=filter)
        src = tuple(int(v) for v in channels_out) if channels_out is not None else tuple(range(c))
        if not 1 <= len(src) <= c:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: channels_out names 1 to {c} source channels")
        c = len(src)
        flips = None
        if flip is not None and not isinstance(flip, str):
            flips = np.ascontiguousarray(flip)
            if flips.shape != (f,) or flips.dtype.kind not in "iub" or ((flips < 0) | (flips > 3)).any():
                raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: flip is 'h', 'v', 'hv' or {f} integers 0 .. 3, one per frame")
            flips = flips.astype(np.uint8)
        elif flip not in _FLIP_NAMES:
            raise LanczosError(ERR_BAD_ARG, f"resize_tensor_norm: flip is 'h', 'v', 'hv' or one integer per frame, not {flip!r}")
        win = resize_window(d, window)
        n = tensor_norm(tensor_strides(layout, win.w, win.h, c), (65535.0 if u16 else 1.0) if div is None else div,
                        0.0 if mean is None else mean, 1.0 if std is None else std, dtype, src,
                        0 if flips is not None else flip, flips.ctypes.data if flips is not None else None)
        out = np.empty((f, c, win.h, win.w) if layout == "chw" else (f, win.h, win.w, c),
                       dtype=np.float32 if dtype == "float32" else np.uint16)
        _check(_lib().lanczos_resize_tensor_norm_host(self._h, ctypes.byref(d), _opts_ref(d, box, None, None),
                                                      ctypes.byref(win) if window is not None else None, None, ctypes.byref(n),
                                                      x.ctypes.data, out.ctypes.data, f), "lanczos_resize_tensor_norm_host")
        out = out if dtype == "float32" else _tensor16_array(out, dtype)
        return out if img.ndim == 4 else out[0]

    def resize_tensor_norm_device(self, desc, d_in, d_out, frames, norm, in_frame_stride=0, out_frame_stride=0, stream=None,
                                  box=None, opts=None, window=None, source=None):
        """Device pointers, asynchronous on `stream`: uint16 (resize_desc(..., bits=16)) or float32 (f32=True) frames at d_in
        -> element frames at d_out as `norm`, a TensorNorm (tensor_norm / tensor_norm_init), describes them; its div / mean /
        std travel by value.  out_frame_stride in BYTES (0 = one frame's extent).  box / opts as resize_device; window =
        (x0, y0, w, h) or a ResizeWindow: the strides describe that window's frame; source: a ResizeSource of pitched
        interleaved rows for the frames at d_in."""
        _check(_lib().lanczos_resize_tensor_norm_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, None, opts),
                                                        _window_ref(desc, window),
                                                        ctypes.byref(source) if source is not None else None, ctypes.byref(norm),
                                                        d_in, d_out, frames, in_frame_stride, out_frame_stride, stream),
               "lanczos_resize_tensor_norm_device")

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
        _check(_lib().lanczos_resize_ycc_host(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None),
                                              ctypes.byref(win) if window is not None else None, ctypes.byref(src), t.ctypes.data,
                                              x.ctypes.data, out.ctypes.data, x.shape[0]), "lanczos_resize_ycc_host")
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
        if lut is None:
            if c == 2:
                m, s = (None if v is None else np.broadcast_to(np.asarray(v, dtype=np.float32), (2,)) for v in (mean, std))
                lut = np.concatenate([normalize_lut(1, None if m is None else m[k], None if s is None else s[k], dtype)
                                      for k in range(2)])
            else:
                lut = normalize_lut(c, mean, std, dtype)
        elif mean is not None or std is not None:
            raise LanczosError(ERR_BAD_ARG, "resize_ycc_tensor: a table or mean / std, not both")
        lut = np.ascontiguousarray(lut)
        if lut.dtype not in ((np.float32,) if wide else (np.uint16, np.float16)) or lut.size != c * 256:
            raise LanczosError(ERR_BAD_ARG, f"resize_ycc_tensor: the table is {'float32' if wide else 'uint16 or float16'} [{c}][256]")
        flips = None
        if flip is not None and not isinstance(flip, str):
            flips = np.ascontiguousarray(flip)
            if flips.shape != (f,) or flips.dtype.kind not in "iub" or ((flips < 0) | (flips > 3)).any():
                raise LanczosError(ERR_BAD_ARG, f"resize_ycc_tensor: flip is 'h', 'v', 'hv' or {f} integers 0 .. 3, one per frame")
            flips = flips.astype(np.uint8)
        elif flip not in _FLIP_NAMES:
            raise LanczosError(ERR_BAD_ARG, f"resize_ycc_tensor: flip is 'h', 'v', 'hv' or one integer per frame, not {flip!r}")
        win = resize_window(d, window)
        v = tensor_view(lut.ctypes.data, tensor_strides(tensor_layout, win.w, win.h, c), 4 if wide else 2, channels_out,
                        0 if flips is not None else flip, flips.ctypes.data if flips is not None else None)
        shape = (f, c, win.h, win.w) if tensor_layout == "chw" else (f, win.h, win.w, c)
        out = np.empty(shape, dtype=np.float32 if wide else np.uint16)
        _check(_lib().lanczos_resize_ycc_tensor_host(self._h, ctypes.byref(d), _opts_ref(d, box, reducing_gap, None),
                                                     ctypes.byref(win) if window is not None else None, ctypes.byref(src),
                                                     t.ctypes.data, ctypes.byref(v), x.ctypes.data, out.ctypes.data, f),
               "lanczos_resize_ycc_tensor_host")
        out = out if wide else _tensor16_array(out, dtype)
        return out if x0.ndim == 2 else out[0]

    def resize_ycc_device(self, desc, source, d_table, d_in, d_out, frames, in_frame_stride=0, out_frame_stride=0, stream=None,
                          box=None, reducing_gap=None, opts=None, window=None):
        """Device pointers, asynchronous on `stream`: YCbCr frames at d_in in `source`'s layout (any byte address, frames
        in_frame_stride bytes apart, 0 = the layout's extent) -> tightly packed RGB bytes of the window at d_out.  d_out and
        out_frame_stride (0 = w * h * 3 rounded up to a multiple of 4) are multiples of 4.  d_table: device, int32 [3][3][256]
        (ycc_table), read when the kernels run."""
        _check(_lib().lanczos_resize_ycc_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                _window_ref(desc, window), ctypes.byref(source) if source is not None else None,
                                                d_table, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream),
               "lanczos_resize_ycc_device")

    def resize_ycc_tensor_device(self, desc, source, d_table, d_in, d_out, frames, d_lut, strides, in_frame_stride=0,
                                 out_frame_stride=0, stream=None, box=None, reducing_gap=None, opts=None, dtype="float32",
                                 window=None, channels_out=None, flip=None, d_flip=None):
        """... -> tensor elements at d_out: strides (or a ready TensorView), d_lut, dtype, channels_out, flip and d_flip as
        Context.resize_tensor_device takes them, over the RGB bytes resize_ycc_device stores as source channels 0, 1, 2."""
        if isinstance(strides, TensorView):
            v = strides
        else:
            if dtype != "float32":
                _tensor16_format(dtype, "resize_ycc_tensor_device")
            v = tensor_view(d_lut, strides, 4 if dtype == "float32" else 2, channels_out if channels_out is not None else (0, 1, 2),
                            flip or 0, d_flip)
        _check(_lib().lanczos_resize_ycc_tensor_device(self._h, ctypes.byref(desc), _opts_ref(desc, box, reducing_gap, opts),
                                                       _window_ref(desc, window), ctypes.byref(source) if source is not None else None,
                                                       d_table, ctypes.byref(v), d_in, d_out, frames, in_frame_stride,
                                                       out_frame_stride, stream), "lanczos_resize_ycc_tensor_device")

    def last_ycc_info(self):
        """YccInfo of the last successful resize_ycc* call on the context (all zero before any)."""
        info = YccInfoC()
        _check(_lib().lanczos_last_ycc_info(self._h, ctypes.byref(info)), "lanczos_last_ycc_info")
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
        img = np.ascontiguousarray(img)
        if img.dtype == np.uint16:
            raise LanczosError(ERR_BAD_ARG, "reduce: 8-bit samples only (Pillow refuses I;16 as well)")
        if img.dtype != np.uint8 or img.ndim not in (2, 3, 4):
            raise LanczosError(ERR_BAD_ARG, "reduce: expected a uint8 [H][W], [H][W][C] or [F][H][W][C] array")
        x = img.reshape(img.shape + (1,)) if img.ndim == 2 else img
        x = x if x.ndim == 4 else x[None]
        f, h, w, c = x.shape
        fx, fy = _factor_pair(factor)
        ow, oh = reduce_size(w, h, (fx, fy), box)
        b = (ctypes.c_int32 * 4)(*[int(v) for v in box]) if box is not None else None
        out = np.empty((f, oh, ow, c), dtype=np.uint8)
        _check(_lib().lanczos_reduce_host(self._h, w, h, c, fx, fy, b, x.ctypes.data, out.ctypes.data, f),
               "lanczos_reduce_host")
        if img.ndim == 2:
            return out[0, :, :, 0]
        return out if img.ndim == 4 else out[0]

    def reduce_device(self, in_w, in_h, channels, factor, d_in, d_out, frames, box=None, in_frame_stride=0,
                      out_frame_stride=0, stream=None):
        """Device pointers, asynchronous on `stream`; the output is reduce_size(in_w, in_h, factor, box) pixels per frame."""
        fx, fy = _factor_pair(factor)
        b = (ctypes.c_int32 * 4)(*[int(v) for v in box]) if box is not None else None
        _check(_lib().lanczos_reduce_device(self._h, in_w, in_h, channels, fx, fy, b, d_in, d_out, frames, in_frame_stride,
                                            out_frame_stride, stream), "lanczos_reduce_device")

    def resize_force(self, path):
        """RESIZE_AUTO / RESIZE_FUSED / RESIZE_TWO_PASS (tests and A/B runs); RESIZE_CONVERT: as AUTO, but a tensor request takes
        the converted route."""
        _check(_lib().lanczos_resize_force(self._h, path), "lanczos_resize_force")

    def timing_enable(self, on=True):
        _check(_lib().lanczos_timing_enable(self._h, 1 if on else 0), "lanczos_timing_enable")

    def timing_read(self):
        n, a, b = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _check(_lib().lanczos_timing_read(self._h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b)),
               "lanczos_timing_read")
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
        _check(_lib().lanczos_force_kernel(self._h, family), "lanczos_force_kernel")


def partition_frames(frames, parts, part):
    f0, cnt = ctypes.c_int(), ctypes.c_int()
    _check(_lib().lanczos_partition_frames(frames, parts, part, ctypes.byref(f0), ctypes.byref(cnt)), "lanczos_partition_frames")
    return f0.value, cnt.value


def partition_rows(desc, parts, part):
    v = [ctypes.c_int() for _ in range(4)]
    _check(_lib().lanczos_partition_rows(ctypes.byref(desc), parts, part, *[ctypes.byref(x) for x in v]), "lanczos_partition_rows")
    return tuple(x.value for x in v)   # out_row0, out_rows, in_row0, in_rows


class Xfer(ctypes.Structure):
    """lanczos_xfer -- one message of the root exchange (lanczos_multi_exchange_plan)."""
    _fields_ = [("src", ctypes.c_int), ("dst", ctypes.c_int), ("src_off", ctypes.c_size_t), ("dst_off", ctypes.c_size_t),
                ("bytes", ctypes.c_size_t)]


def exchange_plan(desc, frames, split, n_devices, phase):
    """The scatter (phase 0) / gather (phase 1) of lanczos_resample_multi_root as a list of (src, dst, src_off, dst_off, bytes).
    Host only: no GPU, no RCCL."""
    fn = _lib().lanczos_multi_exchange_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(Desc), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Xfer), ctypes.c_int]
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
        lib.lanczos_multi_exchange_selftest.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
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
