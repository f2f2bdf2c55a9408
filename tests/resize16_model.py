"""Numpy restatement of the 16-bit resize contract (Pillow's Image.resize with LANCZOS on mode I;16, any a in {2, 3, 4}).

Written from the recipe in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code.  Per axis the tap geometry
is that of the 8-bit contract (tests/resize_model.py); the coefficients stay double, one pass is
    ss = 0.0; for i ascending: ss = ss + (double)sample[first + i] * k[i]       (a multiply and an add, two roundings)
    v  = (int)(ss < 0 ? ss - 0.5 : ss + 0.5)                                    (truncating)
    stored = clip8(v % 256) | clip8(v >> 8) << 8                                (C's %, the sign of v)
so a negative v stores 0 and a v above 65535 stores 0xFF00 | (v & 255): Pillow's store, the wrap of the low byte included.
numpy's float64 array arithmetic does not contract a multiply and an add into an FMA.
"""
import math

import numpy as np

import resize_model as M


def _filter(x, a):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    if -a <= x < a:
        return sinc(x) * sinc(x / a)
    return 0.0


def ksize(in_n, out_n, a):
    scale = in_n / out_n
    fs = max(scale, 1.0)
    return int(math.ceil(a * fs)) * 2 + 1


def axis_tables(in_n, out_n, a):
    """(first[out] int32, count[out] int32, coeffs[out][ksize] float64, zero beyond count)."""
    scale = in_n / out_n
    fs = max(scale, 1.0)
    support = a * fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_n, np.int32)
    count = np.zeros(out_n, np.int32)
    k = np.zeros((out_n, ks), np.float64)
    for o in range(out_n):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_n)
        n = xmax - xmin
        w = [_filter(((i + xmin) - center + 0.5) * ss, a) for i in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            k[o, i] = v / ww if ww != 0.0 else v
        first[o], count[o] = xmin, n
    return first, count, k


def store(v, saturate=False):
    """int64 rounded sums -> stored samples (int64 0..65535).  saturate=True: the variant Pillow does NOT implement
    (clamp to 65535), kept so that a fixture can prove it tells the two apart."""
    if saturate:
        return np.clip(v, 0, 65535)
    lo = np.clip(np.where(v < 0, -((-v) % 256), v % 256), 0, 255)   # C's %: the sign of the dividend
    hi = np.clip(v >> 8, 0, 255)
    return lo | (hi << 8)


def pass_sums(x, axis, first, count, k):
    """x: float64 along `axis`; the rounded integer sums v (int64) of one pass along that axis, before the store."""
    out_n, ks = k.shape
    n_in = x.shape[axis]
    xm = np.moveaxis(x, axis, 0)                       # [n_in, ...]
    out = np.empty((out_n,) + xm.shape[1:], np.int64)
    for o in range(out_n):
        ss = np.zeros(xm.shape[1:], np.float64)
        f = int(first[o])
        for i in range(int(count[o])):
            ss = ss + xm[f + i] * k[o, i]
        out[o] = np.where(ss < 0, ss - 0.5, ss + 0.5).astype(np.int64)   # astype truncates toward zero
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, a=3, saturate=False, stats=None, order=None):
    """img: uint16 [H][W], [H][W][C] or [F][H][W][C] -> the resized image(s), same layout.  stats: an optional dict that
    receives the smallest and largest pre-store value met ("vmin", "vmax")."""
    img = np.asarray(img)
    assert img.dtype == np.uint16
    x = img
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim == 3:
        x = x[None]
    in_h, in_w = x.shape[1], x.shape[2]
    y = x.astype(np.int64)
    sizes = {2: (in_w, out_w), 1: (in_h, out_h)}
    for axis in M.pass_order(in_w, in_h, out_h, order):
        in_n, out_n = sizes[axis]
        if in_n == out_n:
            continue
        f, c, k = axis_tables(in_n, out_n, a)
        v = pass_sums(y.astype(np.float64), axis, f, c, k)
        if stats is not None:
            stats["vmin"] = min(stats.get("vmin", 0), int(v.min()))
            stats["vmax"] = max(stats.get("vmax", 0), int(v.max()))
        y = store(v, saturate)
    y = y.astype(np.uint16)
    if img.ndim == 2:
        return y[0, :, :, 0]
    if img.ndim == 3:
        return y[0]
    return y
