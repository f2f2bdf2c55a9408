"""The call trace of the Python binding: a list of calls of the public surface (CASES), and a recorder that stands in for the
loaded library, so that what a call hands to the C ABI -- which entry, which scalars, which struct contents, which memory -- can
be written down without a GPU and compared between two versions of lanczos-hls_amd/__init__.py.

    tests/golden/make_binding_calls_golden.py   writes tests/golden/binding_calls.json from a tree's module
    tests/test_binding_calls.py                 replays CASES on this tree's module and compares
    scripts/binding_host_time.py --fake         times the wrappers over Recorder(..., keep=False)

The recorder forwards every symbol that needs no device (init, validate, plan, taps, lut, table, strerror, ...) to the real
library, answers lanczos_create with a fake handle, and for every launching entry (launching(L)) records the call and returns
OK without calling the library.  Device pointers are the small integers the cases pass (D_IN, D_OUT, ...), recorded as given;
a host pointer to memory of known length is recorded as a digest of that memory; the output array, filled by nobody, as "out".

The handle is not real, so a case may call nothing that reads a context and is no launching entry (last_kernel, timing_read,
resize_force, ...).
"""
import ctypes
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_calls.json")
FAKE_HANDLE = 0x1000
D_IN, D_OUT, D_LUT, D_FLIP, D_ORIGIN, D_TABLE, STREAM = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
W, H, OW, OH = 7, 5, 4, 3   # every resize of the cases: 7 x 5 -> 4 x 3


def load_module(root=ROOT, name="lanczos_hls_amd_under_trace"):
    """lanczos-hls_amd/__init__.py of the tree at `root` as a module of its own (LANCZOS_LIB names the library for another tree)."""
    pkg = os.path.join(root, "lanczos-hls_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def is_launching(name):
    """the entries that need a device: every *_host / *_device resize, ycc, reduce and resample entry, the layout conversions,
    and lanczos_u8 -- not the host-side tables and plans, not the allocators, and not MultiContext's"""
    if name == "lanczos_u8":
        return True
    if any(k in name for k in ("_taps_", "_plan_host", "_multi_", "_alloc", "_free", "_copy")):
        return False
    return name.endswith(("_host", "_device", "_host_ex", "_device_ex"))


def launching(L):
    return sorted(n for n in L.ABI_SYMBOLS if is_launching(n))


def _digest(ptr, nbytes):
    if not ptr:
        return None
    return f"sha1:{nbytes}:" + hashlib.sha1(ctypes.string_at(ptr, nbytes)).hexdigest()[:16]


def _plain(v):
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, ctypes.Array):
        return [_plain(x) for x in v]
    if isinstance(v, ctypes.Structure):
        return _struct(v, {})
    if isinstance(v, ctypes.c_void_p):
        return v.value
    return v


def _struct(s, mem):
    """field -> value; a pointer field named in `mem` (host memory of known length) as the digest of what it points to"""
    out = {"_type": type(s).__name__}
    for field in s._fields_:
        v = getattr(s, field[0])
        out[field[0]] = _digest(v, mem[field[0]]) if field[0] in mem else _plain(v)
    return out


def _host_mem(real, name, args):
    """for a host entry: {argument index: bytes} of the pointers to digest, the index of `out`, and the lengths of the host
    memory the structs point to"""
    if name == "lanczos_u8":
        return {1: args[2] * args[3] * args[4]}, 5, {}
    frames, i_in = args[-1], len(args) - 3
    desc = args[1]._obj if hasattr(args[1], "_obj") else None
    mem = {"d_flip": frames, "d_origin": frames * 8}
    ptrs = {}
    if name == "lanczos_reduce_host":
        ptrs[i_in] = args[1] * args[2] * args[3] * frames
    elif name == "lanczos_resample_host":
        rows = desc.in_h
        if desc.out_rows:   # a strip: the rows lanczos_strip_input_rows names
            r0, n = ctypes.c_int(), ctypes.c_int()
            real.lanczos_strip_input_rows(args[1], desc.out_row0, desc.out_rows, ctypes.byref(r0), ctypes.byref(n))
            rows = n.value
        ptrs[i_in] = rows * desc.in_w * desc.channels * desc.bytes_per_sample * frames
    elif "ycc" in name:
        i_src = 4
        src = args[i_src]._obj
        ch = (desc.in_h + src.sub_y) >> src.sub_y
        ptrs[i_in] = frames * max(desc.in_h * src.y_row_stride, src.cb_offset + ch * src.c_row_stride,
                                  src.cr_offset + ch * src.c_row_stride)
        ptrs[5] = 9216   # the colour table
    else:
        flags = desc.reserved[0]
        elem = 2 if flags & 4 else 4 if flags & 16 else 1
        ptrs[i_in] = desc.in_w * desc.in_h * desc.channels * elem * frames
    for a in args:
        s = getattr(a, "_obj", None)
        if type(s).__name__ in ("TensorOut", "TensorOut16"):
            mem["d_lut"] = desc.channels * 256 * (2 if type(s).__name__ == "TensorOut16" else 4)
        elif type(s).__name__ == "TensorView":
            mem["d_lut"] = s.out_channels * 256 * s.elem_bytes
    return ptrs, i_in + 1, mem


class Recorder:
    """Stands in for the module's _LIB.  keep=False: launching entries only return OK (scripts/binding_host_time.py --fake)."""

    def __init__(self, real, names, keep=True):
        self._real, self._names, self._keep = real, frozenset(names), keep
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name == "lanczos_create":
            def fn(handle_ref, device):
                handle_ref._obj.value = FAKE_HANDLE
                return 0
        elif name == "lanczos_destroy":
            fn = lambda handle: 0
        elif name in self._names:
            fn = (lambda *args: self._record(name, args)) if self._keep else (lambda *args: 0)
        else:
            fn = getattr(self._real, name)   # AttributeError where the library lacks it, as ctypes raises
        setattr(self, name, fn)
        return fn

    def _record(self, name, args):
        host = name == "lanczos_u8" or name.endswith(("_host", "_host_ex"))
        ptrs, i_out, mem = _host_mem(self._real, name, args) if host else ({}, -1, {})
        rec = []
        for i, a in enumerate(args):
            if hasattr(a, "_obj"):
                rec.append(_struct(a._obj, mem))
            elif i in ptrs:
                rec.append(_digest(a, ptrs[i]))
            elif i == i_out:
                rec.append("out" if a else None)
            else:
                rec.append(_plain(a))
        self.calls.append({"entry": name, "args": rec})
        return 0


def img(shape, dtype=np.uint8, seed=1):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def ycc_frames(L, layout, frames=None):
    n = L.ycc_frame_bytes(_d(L), L.ycc_source(_d(L), layout))
    return img((n,) if frames is None else (frames, n))


def _d(L, c=3, **kw):
    return L.resize_desc(W, H, OW, OH, c, **kw)


def _dev(d):
    return (d, D_IN, D_OUT, 2)


def _lut(L, c=3, dtype="float32"):
    return L.normalize_lut(c, 0.5, 0.25, dtype)


def _strip(L, ctx):
    d = L.make_desc(8, 8, 3, 2, 1, 3, out_row0=4, out_rows=8)
    _, need = L.strip_input_rows(d, 4, 8)
    return ctx.resample_strip(img((need, 8, 3)), d)


def _ycc_src(L, **kw):
    return L.ycc_source(_d(L), "i420", **kw)


RGB, RGBA, PLANES = (H, W, 3), (H, W, 4), (3, H, W)
S = ctypes.c_void_p(STREAM)
WIN = (1, 1, 2, 2)
CHW = (OW * OH, OW, 1)       # strides of the whole 4 x 3 output
CHW_WIN = (4, 2, 1)          # ... and of the 2 x 2 window

# (name, call(L, ctx)) -- a call returns what the wrapper returned
CASES = [
    # -- Context.resize
    ("resize_2d", lambda L, c: c.resize(img((H, W)), OW, OH)),
    ("resize_3d", lambda L, c: c.resize(img(RGB), OW, OH)),
    ("resize_4d", lambda L, c: c.resize(img((2,) + RGB), OW, OH)),
    ("resize_u16", lambda L, c: c.resize(img(RGB, np.uint16), OW, OH)),
    ("resize_u16_2d_window", lambda L, c: c.resize(img((H, W), np.uint16), OW, OH, window=WIN)),
    ("resize_box", lambda L, c: c.resize(img(RGB), OW, OH, box=(1, 0.5, 6, 4.5))),
    ("resize_gap", lambda L, c: c.resize(img(RGB), OW, OH, reducing_gap=2.0)),
    ("resize_box_gap", lambda L, c: c.resize(img(RGB), OW, OH, box=(0, 0, 6, 4), reducing_gap=1.5)),
    ("resize_window", lambda L, c: c.resize(img(RGB), OW, OH, window=WIN)),
    ("resize_window_box", lambda L, c: c.resize(img((2,) + RGB), OW, OH, window=WIN, box=(1, 1, 6, 4))),
    ("resize_filter_name", lambda L, c: c.resize(img(RGB), OW, OH, filter="bicubic")),
    ("resize_filter_code", lambda L, c: c.resize(img(RGB), OW, OH, filter=L.FILTER_NEAREST)),
    ("resize_a2", lambda L, c: c.resize(img(RGB), OW, OH, a=2)),
    ("resize_alpha", lambda L, c: c.resize(img(RGBA), OW, OH, alpha=True)),
    ("resize_planar", lambda L, c: c.resize(img(PLANES), OW, OH, planar=True)),
    ("resize_planar_4d_window_box", lambda L, c: c.resize(img((2,) + PLANES), OW, OH, planar=True, window=WIN, box=(1, 1, 6, 4))),
    ("resize_planar_out", lambda L, c: c.resize(img(RGB), OW, OH, planar_out=True)),
    ("resize_planar_out_4d_alpha", lambda L, c: c.resize(img((2,) + RGBA), OW, OH, alpha=True, planar_out=True, reducing_gap=2.0)),
    ("resize_planar_both", lambda L, c: c.resize(img((2,) + PLANES), OW, OH, planar=True, planar_out=True)),
    ("resize_planar_both_3d", lambda L, c: c.resize(img(PLANES), OW, OH, planar=True, planar_out=True, filter="box")),
    ("resize_planar_out_window", lambda L, c: c.resize(img(RGB), OW, OH, planar_out=True, window=WIN)),
    # -- Context.resize_f32
    ("f32_plain", lambda L, c: c.resize_f32(img(RGB, np.float32), OW, OH)),
    ("f32_2d", lambda L, c: c.resize_f32(img((H, W), np.float32), OW, OH)),
    ("f32_4d_filter", lambda L, c: c.resize_f32(img((2,) + RGB, np.float32), OW, OH, filter="hamming")),
    ("f32_box", lambda L, c: c.resize_f32(img(RGB, np.float32), OW, OH, box=(1, 0.5, 6, 4.5))),
    ("f32_window", lambda L, c: c.resize_f32(img(RGB, np.float32), OW, OH, window=WIN)),
    ("f32_window_box", lambda L, c: c.resize_f32(img(RGB, np.float32), OW, OH, a=2, window=WIN, box=(1, 1, 6, 4))),
    # -- Context.resize_device
    ("dev_plain", lambda L, c: c.resize_device(*_dev(_d(L)))),
    ("dev_strides_stream", lambda L, c: c.resize_device(*_dev(_d(L)), 128, 64, S)),
    ("dev_box", lambda L, c: c.resize_device(*_dev(_d(L)), box=(1, 0.5, 6, 4.5))),
    ("dev_gap", lambda L, c: c.resize_device(*_dev(_d(L)), reducing_gap=3)),
    ("dev_opts", lambda L, c: c.resize_device(*_dev(_d(L)), opts=L.resize_opts(_d(L), (0, 0, 6, 4), 2.0))),
    ("dev_window", lambda L, c: c.resize_device(*_dev(_d(L)), window=WIN)),
    ("dev_window_ready", lambda L, c: c.resize_device(*_dev(_d(L)), stream=S, window=L.resize_window(_d(L), WIN), box=(1, 1, 6, 4))),
    ("dev_source", lambda L, c: c.resize_device(*_dev(_d(L)), source=L.resize_source(_d(L), "planar"))),
    ("dev_source_window", lambda L, c: c.resize_device(*_dev(_d(L)), source=L.resize_source(_d(L), "interleaved", row_stride=32), window=WIN)),
    ("dev_dest", lambda L, c: c.resize_device(*_dev(_d(L)), dest=L.resize_dest(_d(L), "planar"))),
    ("dev_dest_window", lambda L, c: c.resize_device(*_dev(_d(L)), dest=L.resize_dest(_d(L), "planar", row_stride=16, window=WIN), window=WIN)),
    ("dev_source_dest", lambda L, c: c.resize_device(*_dev(_d(L)), 0, 0, S, source=L.resize_source(_d(L), "planar", row_stride=16),
                                                     dest=L.resize_dest(_d(L), "interleaved", row_stride=16), reducing_gap=2.0)),
    ("dev_filter", lambda L, c: c.resize_device(*_dev(_d(L)), filter="bilinear")),
    ("dev_filter_window", lambda L, c: c.resize_device(*_dev(_d(L, filter="box")), filter=L.FILTER_HAMMING, window=WIN)),
    ("dev_u16", lambda L, c: c.resize_device(*_dev(_d(L, bits=16)))),
    # -- Context.resize_tensor
    ("tensor_f32", lambda L, c: c.resize_tensor(img(RGB), OW, OH)),
    ("tensor_bf16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, dtype="bfloat16")),
    ("tensor_f16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, dtype="float16")),
    ("tensor_f32_window", lambda L, c: c.resize_tensor(img(RGB), OW, OH, window=WIN)),
    ("tensor_bf16_window", lambda L, c: c.resize_tensor(img(RGB), OW, OH, dtype="bfloat16", window=WIN)),
    ("tensor_f16_window", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, dtype="float16", window=WIN, box=(1, 1, 6, 4))),
    ("tensor_2d", lambda L, c: c.resize_tensor(img((H, W)), OW, OH, mean=0.5, std=0.25)),
    ("tensor_4d_mean_std", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, mean=(0.1, 0.2, 0.3), std=(0.5, 0.6, 0.7), reducing_gap=2.0)),
    ("tensor_hwc", lambda L, c: c.resize_tensor(img(RGB), OW, OH, layout="hwc")),
    ("tensor_hwc_window_f16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, layout="hwc", window=WIN, dtype="float16")),
    ("tensor_lut", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L))),
    ("tensor_lut_bf16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L, 3, "bfloat16"), dtype="bfloat16")),
    ("tensor_lut_f16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L, 3, "float16"), dtype="float16", filter="bicubic")),
    ("tensor_alpha", lambda L, c: c.resize_tensor(img(RGBA), OW, OH, alpha=True)),
    ("tensor_channels3", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(2, 1, 0), mean=(0.1, 0.2, 0.3))),
    ("tensor_channels3_of_rgba", lambda L, c: c.resize_tensor(img(RGBA), OW, OH, alpha=True, channels_out=(0, 1, 2))),
    ("tensor_channels2", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(0, 2), mean=(0.1, 0.2), std=0.5)),
    ("tensor_channels2_f16_no_mean", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(2, 0), dtype="float16")),
    ("tensor_channels1", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(1,), layout="hwc")),
    ("tensor_channels_lut", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(2, 1), lut=_lut(L)[:2])),
    ("tensor_flip_h", lambda L, c: c.resize_tensor(img(RGB), OW, OH, flip="h")),
    ("tensor_flip_hv_window", lambda L, c: c.resize_tensor(img(RGB), OW, OH, flip="hv", window=WIN, dtype="bfloat16")),
    ("tensor_flip_array", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, flip=[1, 2])),
    ("tensor_flip_array_bool", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, flip=np.array([True, False]), channels_out=(2, 1, 0))),
    ("tensor_crop", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, crop=(2, 2), origins=[(0, 1), (2, 0)])),
    ("tensor_crop_flip_f16", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, crop=(3, 2), origins=np.array([[1, 1], [0, 0]], np.int64),
                                                          flip=[3, 0], dtype="float16", layout="hwc")),
    ("tensor_planar", lambda L, c: c.resize_tensor(img(PLANES), OW, OH, planar=True)),
    ("tensor_planar_4d_window", lambda L, c: c.resize_tensor(img((2,) + PLANES), OW, OH, planar=True, window=WIN, dtype="bfloat16")),
    ("tensor_planar_crop", lambda L, c: c.resize_tensor(img((2,) + PLANES), OW, OH, planar=True, crop=(2, 2), origins=[(0, 1), (2, 0)])),
    ("tensor_planar_channels_flip", lambda L, c: c.resize_tensor(img(PLANES), OW, OH, planar=True, channels_out=(2, 0), flip="v")),
    # -- Context.resize_tensor_device
    ("tdev_strides", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW)),
    ("tdev_strides_frame_strides", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, 128, 256, S, box=(1, 1, 6, 4))),
    ("tdev_tensor_out", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_out(D_LUT, CHW))),
    ("tdev_tensor_out16", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor16_out(D_LUT, CHW))),
    ("tdev_tensor_out_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_out(D_LUT, CHW_WIN), window=WIN)),
    ("tdev_tensor_out16_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor16_out(D_LUT, CHW_WIN), window=L.resize_window(_d(L), WIN))),
    ("tdev_view", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_view(D_LUT, CHW, 2, (2, 1, 0), "h", D_FLIP))),
    ("tdev_view_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, L.tensor_view(D_LUT, CHW_WIN), window=WIN, dtype="float16")),
    ("tdev_bf16", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, dtype="bfloat16")),
    ("tdev_f16_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, dtype="float16", window=WIN, reducing_gap=2.0)),
    ("tdev_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, window=WIN)),
    ("tdev_opts", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, opts=L.resize_opts(_d(L), (0, 0, 6, 4)))),
    ("tdev_channels", lambda L, c: c.resize_tensor_device(*_dev(_d(L, 4, alpha=True)), D_LUT, CHW, channels_out=(0, 1, 2))),
    ("tdev_channels_f16", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, channels_out=(1,), dtype="float16")),
    ("tdev_flip", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, flip="v")),
    ("tdev_flip_bits", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, flip=L.FLIP_H | L.FLIP_V, window=WIN)),
    ("tdev_d_flip", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, d_flip=D_FLIP)),
    ("tdev_crop", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, crop=(2, 2), d_origin=D_ORIGIN)),
    ("tdev_crop_ready", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, crop=L.resize_crops(2, 2, D_ORIGIN), dtype="bfloat16",
                                                            flip="h", stream=S)),
    ("tdev_crop_ready_view", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_view(D_LUT, CHW_WIN), crop=L.resize_crops(2, 2, D_ORIGIN))),
    ("tdev_source", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, source=L.resize_source(_d(L), "planar"))),
    ("tdev_source_window_f16", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, source=L.resize_source(_d(L), "planar"),
                                                                   window=WIN, dtype="float16", channels_out=(2, 1, 0))),
    ("tdev_source_tensor_out", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_out(D_LUT, CHW), source=L.resize_source(_d(L), "planar"))),
    ("tdev_source_tensor_out16", lambda L, c: c.resize_tensor_device(*_dev(_d(L, 4)), None, L.tensor16_out(D_LUT, CHW),
                                                                     source=L.resize_source(_d(L, 4), "planar"))),
    ("tdev_source_view", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), None, L.tensor_view(D_LUT, CHW, 4, (0, 1)),
                                                             source=L.resize_source(_d(L), "interleaved", row_stride=32))),
    ("tdev_source_crop", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, source=L.resize_source(_d(L), "planar"),
                                                             crop=(2, 2), d_origin=D_ORIGIN)),
    ("tdev_source_crop_ready", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, source=L.resize_source(_d(L), "planar"),
                                                                   crop=L.resize_crops(2, 2, D_ORIGIN), d_flip=D_FLIP)),
    # -- Context.resize_tensor_norm / _device
    ("norm_u16_f32", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH)),
    ("norm_u16_bf16", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, dtype="bfloat16")),
    ("norm_u16_f16", lambda L, c: c.resize_tensor_norm(img((2,) + RGB, np.uint16), OW, OH, dtype="float16", mean=0.5, std=(0.1, 0.2, 0.3))),
    ("norm_f32_f32", lambda L, c: c.resize_tensor_norm(img(RGB, np.float32), OW, OH, div=2.0)),
    ("norm_f32_bf16", lambda L, c: c.resize_tensor_norm(img((H, W), np.float32), OW, OH, dtype="bfloat16")),
    ("norm_f32_f16_hwc", lambda L, c: c.resize_tensor_norm(img(RGB, np.float32), OW, OH, dtype="float16", layout="hwc", filter="bilinear")),
    ("norm_channels", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, channels_out=(2, 0), mean=(0.1, 0.2))),
    ("norm_flip_name", lambda L, c: c.resize_tensor_norm(img(RGB, np.float32), OW, OH, flip="hv")),
    ("norm_flip_array", lambda L, c: c.resize_tensor_norm(img((2,) + RGB, np.uint16), OW, OH, flip=[2, 1])),
    ("norm_window_box", lambda L, c: c.resize_tensor_norm(img(RGB, np.float32), OW, OH, window=WIN, box=(1, 1, 6, 4))),
    ("normdev_plain", lambda L, c: c.resize_tensor_norm_device(*_dev(_d(L, bits=16)), L.tensor_norm_init(_d(L, bits=16), "bfloat16", "hwc"))),
    ("normdev_window_opts", lambda L, c: c.resize_tensor_norm_device(*_dev(_d(L, f32=True)), L.tensor_norm(CHW_WIN, 2.0, 0.5, (1, 2, 3), "float16",
                                                                     (2, 1, 0), "h", D_FLIP), 64, 128, S, opts=L.resize_opts(_d(L, f32=True), (1, 1, 6, 4)), window=WIN)),
    ("normdev_source_box", lambda L, c: c.resize_tensor_norm_device(*_dev(_d(L, bits=16)), L.tensor_norm(CHW), box=(1, 1, 6, 4),
                                                                    source=L.resize_source(_d(L, bits=16), "interleaved", row_stride=64))),
    # -- YCbCr
    ("ycc_nv12", lambda L, c: c.resize_ycc(ycc_frames(L, "nv12"), W, H, OW, OH)),
    ("ycc_nv21", lambda L, c: c.resize_ycc(ycc_frames(L, "nv21", 2), W, H, OW, OH, layout="nv21")),
    ("ycc_i420", lambda L, c: c.resize_ycc(ycc_frames(L, "i420"), W, H, OW, OH, layout="i420", standard="bt601")),
    ("ycc_i422", lambda L, c: c.resize_ycc(ycc_frames(L, "i422"), W, H, OW, OH, layout="i422", standard="bt709")),
    ("ycc_i444", lambda L, c: c.resize_ycc(ycc_frames(L, "i444", 2), W, H, OW, OH, layout="i444", filter="bicubic")),
    ("ycc_table", lambda L, c: c.resize_ycc(ycc_frames(L, "nv12"), W, H, OW, OH, table=L.ycc_table("bt709")[::-1])),
    ("ycc_source", lambda L, c: c.resize_ycc(img((2, 92)), W, H, OW, OH, source=_ycc_src(L, y_row_stride=8, c_row_stride=8, cb_offset=40, cr_offset=68))),
    ("ycc_window_box_gap", lambda L, c: c.resize_ycc(ycc_frames(L, "nv12"), W, H, OW, OH, window=WIN, box=(0, 0, 6, 4), reducing_gap=2.0)),
    ("ycct_nv12", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH)),
    ("ycct_i420_hwc", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "i420", 2), W, H, OW, OH, layout="i420", tensor_layout="hwc", mean=(0.1, 0.2, 0.3))),
    ("ycct_channels2", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv21"), W, H, OW, OH, layout="nv21", channels_out=(2, 0), mean=0.5, std=(0.1, 0.2))),
    ("ycct_channels1_lut", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, channels_out=(1,), lut=_lut(L, 1))),
    ("ycct_flip_name", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "i444"), W, H, OW, OH, layout="i444", flip="v")),
    ("ycct_flip_array", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "i422", 2), W, H, OW, OH, layout="i422", flip=np.array([3, 1], np.uint8))),
    ("ycct_bf16", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, dtype="bfloat16")),
    ("ycct_f16_window_table", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, dtype="float16", window=WIN,
                                                               table=L.ycc_table("bt601"), lut=_lut(L, 3, "float16"), box=(0, 0, 6, 4))),
    ("ycct_source", lambda L, c: c.resize_ycc_tensor(img((92,)), W, H, OW, OH, source=_ycc_src(L, y_row_stride=8, c_row_stride=8, cb_offset=40, cr_offset=68))),
    ("yccdev_plain", lambda L, c: c.resize_ycc_device(_d(L), L.ycc_source(_d(L), "nv12"), D_TABLE, D_IN, D_OUT, 2)),
    ("yccdev_window_opts", lambda L, c: c.resize_ycc_device(_d(L), L.ycc_source(_d(L), "i420"), D_TABLE, D_IN, D_OUT, 2, 128, 64, S,
                                                            opts=L.resize_opts(_d(L), (0, 0, 6, 4), 2.0), window=WIN)),
    ("yccdev_box", lambda L, c: c.resize_ycc_device(_d(L), L.ycc_source(_d(L), "nv21"), D_TABLE, D_IN, D_OUT, 1, box=(0, 0, 6, 4))),
    ("ycctdev_strides", lambda L, c: c.resize_ycc_tensor_device(_d(L), L.ycc_source(_d(L), "nv12"), D_TABLE, D_IN, D_OUT, 2, D_LUT, CHW)),
    ("ycctdev_f16_channels_flip", lambda L, c: c.resize_ycc_tensor_device(_d(L), L.ycc_source(_d(L), "i444"), D_TABLE, D_IN, D_OUT, 2, D_LUT, CHW_WIN, 0, 64, S,
                                                                          dtype="float16", window=WIN, channels_out=(2, 1), flip="hv", d_flip=D_FLIP, reducing_gap=2.0)),
    ("ycctdev_view", lambda L, c: c.resize_ycc_tensor_device(_d(L), L.ycc_source(_d(L), "nv12"), D_TABLE, D_IN, D_OUT, 2, None,
                                                             L.tensor_view(D_LUT, CHW, 2, (0, 1, 2)), dtype="float16")),
    # -- reduce
    ("reduce_2d", lambda L, c: c.reduce(img((H, W)), 2)),
    ("reduce_3d_pair", lambda L, c: c.reduce(img(RGB), (2, 1))),
    ("reduce_4d_box", lambda L, c: c.reduce(img((2,) + RGB), 2, box=(1, 1, 7, 5))),
    ("reducedev_plain", lambda L, c: c.reduce_device(W, H, 3, 2, D_IN, D_OUT, 2)),
    ("reducedev_box_strides", lambda L, c: c.reduce_device(W, H, 3, (2, 3), D_IN, D_OUT, 2, (1, 1, 7, 5), 128, 64, S)),
    # -- the upscale entries
    ("resample_3d", lambda L, c: c.resample(img((8, 8, 3)), 2, 1, 3)),
    ("resample_4d_u16_exact", lambda L, c: c.resample(img((2, 8, 8, 3), np.uint16), 3, 2, 2, L.MODE_EXACT)),
    ("resample_out", lambda L, c: c.resample(img((8, 8, 3)), 2, 1, 3, out=np.empty(16 * 16 * 3, np.uint8))),
    ("resample_strip", _strip),
    ("u8", lambda L, c: c.u8(img((8, 8, 3)), 16, 16, 3)),
    ("resample_device", lambda L, c: c.resample_device(L.make_desc(8, 8, 3, 2, 1, 3), D_IN, D_OUT, 2, 256, 1024, S)),
    ("resample_device_defaults", lambda L, c: c.resample_device(L.make_desc(8, 8, 3, 2, 1, 3), D_IN, D_OUT, 1)),
    ("resample_planar_device", lambda L, c: c.resample_planar_device(L.make_desc(8, 8, 3, 2, 1, 3), D_IN, D_OUT, 2, S)),
    ("planar_to_interleaved", lambda L, c: c.planar_to_interleaved_device(D_IN, D_OUT, 8, 6, 3, 1, 2)),
    ("interleaved_to_planar", lambda L, c: c.interleaved_to_planar_device(D_IN, D_OUT, 8, 6, 3, 2, 2, S)),
    ("module_lanczos", lambda L, c: L.lanczos(img((8, 8, 3)), 2)),
    # -- refusals the module itself raises: code and message
    ("no_filter", lambda L, c: L.filter_code("sinc")),
    ("no_desc_bits", lambda L, c: L.resize_desc(W, H, OW, OH, 3, bits=12)),
    ("no_desc_filter_a", lambda L, c: L.resize_desc(W, H, OW, OH, 3, a=2, filter="box")),
    ("no_opts_box", lambda L, c: L.resize_opts(_d(L), box=(0, 0, 4))),
    ("no_window_len", lambda L, c: L.resize_window(_d(L), (0, 0, 2))),
    ("no_window_outside", lambda L, c: L.resize_window(_d(L), (3, 2, 2, 2))),
    ("no_source_layout", lambda L, c: L.resize_source(_d(L), "tiled")),
    ("no_dest_layout", lambda L, c: L.resize_dest(_d(L), "tiled")),
    ("no_ycc_layout", lambda L, c: L.ycc_source(_d(L), "yuy2")),
    ("no_ycc_layout_code", lambda L, c: L.ycc_source(_d(L), L.YCC_NV12)),
    ("no_ycc_standard", lambda L, c: L.ycc_table("bt2020")),
    ("no_center_window", lambda L, c: L.center_window(4, 3, 5, 3)),
    ("no_lut_convert16_dtype", lambda L, c: L.lut_convert16(np.zeros(4, np.float32), "float64")),
    ("no_normalize_lut_dtype", lambda L, c: L.normalize_lut(3, dtype="float64")),
    ("no_normalize_lut_mean", lambda L, c: L.normalize_lut(3, mean=(1, 2))),
    ("no_normalize_lut_std", lambda L, c: L.normalize_lut(3, std=(1, 2))),
    ("no_tensor_strides", lambda L, c: L.tensor_strides("cwh", 4, 3, 3)),
    ("no_tensor_view_channels", lambda L, c: L.tensor_view(D_LUT, CHW, 4, (0, 1, 2, 3, 0))),
    ("no_tensor_norm_init", lambda L, c: L.tensor_norm_init(_d(L, bits=16), "float64")),
    ("no_tensor_norm_init_layout", lambda L, c: L.tensor_norm_init(_d(L, bits=16), "float32", "cwh")),
    ("no_tensor_norm_dtype", lambda L, c: L.tensor_norm(CHW, dtype="int8")),
    ("no_tensor_norm_channels", lambda L, c: L.tensor_norm(CHW, channels_out=())),
    ("no_tensor_norm_div", lambda L, c: L.tensor_norm(CHW, div=(1, 2))),
    ("no_tensor_norm_std", lambda L, c: L.tensor_norm(CHW, std=(1, 2, 3, 4))),
    ("no_resample_dtype", lambda L, c: c.resample(img((8, 8, 3), np.float32), 2, 1, 3)),
    ("no_resample_ndim", lambda L, c: c.resample(img((8, 8)), 2, 1, 3)),
    ("no_resample_out", lambda L, c: c.resample(img((8, 8, 3)), 2, 1, 3, out=np.empty(5, np.uint8))),
    ("no_resample_strip", lambda L, c: c.resample_strip(img((3, 8, 3)), L.make_desc(8, 8, 3, 2, 1, 3, out_row0=4, out_rows=8))),
    ("no_resize_dtype", lambda L, c: c.resize(img(RGB, np.float32), OW, OH)),
    ("no_resize_ndim", lambda L, c: c.resize(img((W,)), OW, OH)),
    ("no_resize_planar", lambda L, c: c.resize(img(PLANES, np.uint16), OW, OH, planar=True)),
    ("no_resize_planar_ndim", lambda L, c: c.resize(img((H, W)), OW, OH, planar=True, planar_out=True)),
    ("no_resize_planar_out_dtype", lambda L, c: c.resize(img(RGB, np.uint16), OW, OH, planar_out=True)),
    ("no_resize_planar_out_channels", lambda L, c: c.resize(img((H, W, 1)), OW, OH, planar_out=True)),
    ("no_resize_planar_out_2d", lambda L, c: c.resize(img((H, W)), OW, OH, planar_out=True)),
    ("no_resize_alpha_rgb", lambda L, c: c.resize(img(RGB), OW, OH, alpha=True)),
    ("no_f32_dtype", lambda L, c: c.resize_f32(img(RGB), OW, OH)),
    ("no_f32_ndim", lambda L, c: c.resize_f32(img((W,), np.float32), OW, OH)),
    ("no_tensor_dtype", lambda L, c: c.resize_tensor(img(RGB), OW, OH, dtype="float64")),
    ("no_tensor_img", lambda L, c: c.resize_tensor(img(RGB, np.uint16), OW, OH)),
    ("no_tensor_planar", lambda L, c: c.resize_tensor(img((H, W)), OW, OH, planar=True)),
    ("no_tensor_channels", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=(0, 1, 2, 0))),
    ("no_tensor_channels_none", lambda L, c: c.resize_tensor(img(RGB), OW, OH, channels_out=())),
    ("no_tensor_lut_and_mean", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L), mean=0.5)),
    ("no_tensor_lut_dtype", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L).astype(np.float64))),
    ("no_tensor_lut_dtype16", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L), dtype="float16")),
    ("no_tensor_lut_size", lambda L, c: c.resize_tensor(img(RGB), OW, OH, lut=_lut(L), channels_out=(0, 1))),
    ("no_tensor_crop_alone", lambda L, c: c.resize_tensor(img(RGB), OW, OH, crop=(2, 2))),
    ("no_tensor_crop_window", lambda L, c: c.resize_tensor(img(RGB), OW, OH, crop=(2, 2), origins=[(0, 0)], window=WIN)),
    ("no_tensor_crop_shape", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, crop=(2, 2), origins=[(0, 0)])),
    ("no_tensor_crop_kind", lambda L, c: c.resize_tensor(img(RGB), OW, OH, crop=(2, 2), origins=[(0.5, 0.0)])),
    ("no_tensor_flip_array", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, flip=[1, 4])),
    ("no_tensor_flip_shape", lambda L, c: c.resize_tensor(img((2,) + RGB), OW, OH, flip=[1])),
    ("no_tensor_flip_name", lambda L, c: c.resize_tensor(img(RGB), OW, OH, flip="x")),
    ("no_tensor_layout", lambda L, c: c.resize_tensor(img(RGB), OW, OH, layout="cwh")),
    ("no_tdev_crop_window", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, crop=(2, 2), d_origin=D_ORIGIN, window=WIN)),
    ("no_tdev_crop_alone", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, crop=(2, 2))),
    ("no_tdev_origin_alone", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW_WIN, d_origin=D_ORIGIN)),
    ("no_tdev_dtype", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, dtype="float64")),
    ("no_tdev_dtype_view", lambda L, c: c.resize_tensor_device(*_dev(_d(L)), D_LUT, CHW, dtype="int8", flip="h")),
    ("no_norm_img", lambda L, c: c.resize_tensor_norm(img(RGB), OW, OH)),
    ("no_norm_dtype", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, dtype="float64")),
    ("no_norm_channels", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, channels_out=(0, 1, 2, 0))),
    ("no_norm_flip_array", lambda L, c: c.resize_tensor_norm(img((2,) + RGB, np.uint16), OW, OH, flip=[0, 7])),
    ("no_norm_flip_name", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, flip="d")),
    ("no_norm_mean", lambda L, c: c.resize_tensor_norm(img(RGB, np.uint16), OW, OH, mean=(1, 2))),
    ("no_ycc_frames", lambda L, c: c.resize_ycc(img((10,)), W, H, OW, OH)),
    ("no_ycc_table", lambda L, c: c.resize_ycc(ycc_frames(L, "nv12"), W, H, OW, OH, table=np.zeros((3, 256), np.int32))),
    ("no_ycct_frames", lambda L, c: c.resize_ycc_tensor(img((2, 3, 10)), W, H, OW, OH)),
    ("no_ycct_table", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, table=np.zeros((3, 3, 256), np.int64))),
    ("no_ycct_dtype", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, dtype="float64")),
    ("no_ycct_channels", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, channels_out=(0, 1, 2, 0))),
    ("no_ycct_lut_and_std", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, lut=_lut(L), std=0.5)),
    ("no_ycct_lut_size", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, lut=_lut(L, 1))),
    ("no_ycct_flip_array", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12", 2), W, H, OW, OH, flip=[0.5, 1.0])),
    ("no_ycct_flip_name", lambda L, c: c.resize_ycc_tensor(ycc_frames(L, "nv12"), W, H, OW, OH, flip="hh")),
    ("no_ycctdev_dtype", lambda L, c: c.resize_ycc_tensor_device(_d(L), L.ycc_source(_d(L), "nv12"), D_TABLE, D_IN, D_OUT, 2, D_LUT, CHW, dtype="float64")),
    ("no_reduce_u16", lambda L, c: c.reduce(img(RGB, np.uint16), 2)),
    ("no_reduce_dtype", lambda L, c: c.reduce(img(RGB, np.float32), 2)),
    ("no_reduce_factor", lambda L, c: c.reduce(img(RGB), 0)),
]
NAMES = [name for name, _ in CASES]
assert len(set(NAMES)) == len(NAMES)


def _returned(ret):
    if ret is None:
        return None
    if isinstance(ret, np.ndarray):
        return {"shape": list(ret.shape), "dtype": str(ret.dtype), "contiguous": bool(ret.flags["C_CONTIGUOUS"])}
    return repr(ret)


def run_case(L, real, call):
    """One case on module L over a fresh recorder: {"calls": [...], "returned": ...} or {"calls": [...], "error": ...}.
    `real` is L's loaded library (L._lib() before any recorder was put in)."""
    rec = Recorder(real, launching(L))
    saved_ctx = L._default_ctx
    L._LIB, L._default_ctx = rec, None
    ctx = L.Context()
    try:
        try:
            out = {"calls": rec.calls, "returned": _returned(call(L, ctx))}
        except L.LanczosError as e:
            out = {"calls": rec.calls, "error": {"code": e.code, "message": str(e)}}
    finally:
        for c in (ctx, L._default_ctx):   # closed while the recorder answers: the handles are not real
            if c is not None:
                c.close()
        L._LIB, L._default_ctx = real, saved_ctx
    return out


def run_all(L):
    real = L._lib()
    return {name: run_case(L, real, call) for name, call in CASES}
