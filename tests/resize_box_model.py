"""Numpy restatement of the box / reduce / reducing_gap contract (Pillow's Image.resize(size, LANCZOS, box, reducing_gap)
and Image.reduce(factor, box)), on top of resize_model, resize16_model and resize_alpha_model, which it extends.

Written from the contract in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code and not from Pillow's:

  box     per axis (b0, b1): both rounded to float32, their difference taken in float32, scale = that / out in double,
          centre = b0f + (o + 0.5) * scale; first / count clipped to the whole source axis; the rest is resize_model's recipe.
          A pass runs iff out != in or b0f != 0 or b1f != in.  Their order is resize_model.pass_order's, on the sizes of the
          frame the resize reads (the reduced one under a gap).
  reduce  out = ((sum + d // 2) * (2^24 // d)) >> 24 in uint32, d = the source pixels the block really covers.
  gap     fx = int((x1 - x0) / out_w / g) or 1 (fy likewise) in double; safe box with s = a - 0.5; reduce over it; resize the
          reduced frame with the box shifted and divided (in double, float32 after).

`float_box=False` and `own_divisor=False` are the near misses the fixture has to tell from the contract.
"""
import math

import numpy as np

import resize16_model as M16
import resize_alpha_model as MA
import resize_model as M

PRECISION_BITS = M.PRECISION_BITS


def f32(v):
    return float(np.float32(v))


def axis_scale(out_n, b0, b1, float_box=True):
    if float_box:
        return float(np.float32(np.float32(b1) - np.float32(b0))) / out_n, f32(b0)
    return (b1 - b0) / out_n, float(b0)


def axis_runs(in_n, out_n, b0, b1):
    return out_n != in_n or f32(b0) != 0.0 or f32(b1) != float(in_n)


def ksize(out_n, a, b0, b1):
    scale, _ = axis_scale(out_n, b0, b1)
    return int(math.ceil(a * max(scale, 1.0))) * 2 + 1


def axis_tables(in_n, out_n, a, b0, b1, f64=False, float_box=True):
    """(first[out] int32, count[out] int32, coeffs[out][ksize]): int32 22-bit fixed point, or float64 with f64."""
    scale, c0 = axis_scale(out_n, b0, b1, float_box)
    fs = max(scale, 1.0)
    support = a * fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_n, np.int32)
    count = np.zeros(out_n, np.int32)
    k = np.zeros((out_n, ks), np.float64 if f64 else np.int32)
    for o in range(out_n):
        center = c0 + (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_n)
        n = xmax - xmin
        w = [M._filter(((i + xmin) - center + 0.5) * ss, a) for i in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for i, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            if f64:
                k[o, i] = v
            else:
                k[o, i] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        first[o], count[o] = xmin, n
    return first, count, k


def _as4(img):
    x = np.asarray(img)
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim == 3:
        x = x[None]
    return x


def _like(img, y):
    if np.asarray(img).ndim == 2:
        return y[0, :, :, 0]
    if np.asarray(img).ndim == 3:
        return y[0]
    return y


def resize_box(img, out_w, out_h, box=None, a=3, alpha=False, float_box=True, order=None):
    """img: uint8 or uint16 [H][W], [H][W][C] or [F][H][W][C] -> the box resized to out_h x out_w, same layout.  alpha: the
    last of four channels is straight alpha (mode RGBA)."""
    x = _as4(img)
    in_h, in_w = x.shape[1], x.shape[2]
    if box is None:
        box = (0, 0, in_w, in_h)
    x0, y0, x1, y1 = box
    run_h, run_v = axis_runs(in_w, out_w, x0, x1), axis_runs(in_h, out_h, y0, y1)
    if not run_h and not run_v:
        return np.asarray(img).copy()
    u16 = x.dtype == np.uint16
    assert u16 or x.dtype == np.uint8
    if alpha:
        assert not u16 and x.shape[-1] == 4
        x = MA.premultiply(x)
    y = x.astype(np.int64)
    spans = {2: (run_h, in_w, out_w, x0, x1), 1: (run_v, in_h, out_h, y0, y1)}
    for axis in M.pass_order(in_w, in_h, out_h, order):
        run, in_n, out_n, b0, b1 = spans[axis]
        if not run:
            continue
        f, c, k = axis_tables(in_n, out_n, a, b0, b1, f64=u16, float_box=float_box)
        if u16:
            y = M16.store(M16.pass_sums(y.astype(np.float64), axis, f, c, k))
        else:
            y = M._pass(y, axis, f, k)
    y = y.astype(x.dtype)
    if alpha:
        y = MA.unpremultiply(y)
    return _like(img, y)


def reduce_size(in_w, in_h, factor, box=None):
    fx, fy = (factor, factor) if isinstance(factor, int) else factor
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    return -(-(x1 - x0) // fx), -(-(y1 - y0) // fy)


def reduce(img, factor, box=None, own_divisor=True):
    """img: uint8 [H][W], [H][W][C] or [F][H][W][C] -> reduced by factor (int or (fx, fy)) over the integer box."""
    x = _as4(img)
    assert x.dtype == np.uint8
    fx, fy = (factor, factor) if isinstance(factor, int) else factor
    in_h, in_w = x.shape[1], x.shape[2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    assert 0 <= x0 < x1 <= in_w and 0 <= y0 < y1 <= in_h and fx * fy < 65536
    ow, oh = -(-(x1 - x0) // fx), -(-(y1 - y0) // fy)
    crop = x[:, y0:y1, x0:x1].astype(np.int64)
    pad = np.zeros((x.shape[0], oh * fy, ow * fx, x.shape[3]), np.int64)
    pad[:, :y1 - y0, :x1 - x0] = crop
    sums = pad.reshape(x.shape[0], oh, fy, ow, fx, x.shape[3]).sum(axis=(2, 4))
    wcol = np.full(ow, fx, np.int64)
    wcol[-1] = (x1 - x0) - (ow - 1) * fx
    hrow = np.full(oh, fy, np.int64)
    hrow[-1] = (y1 - y0) - (oh - 1) * fy
    d = (hrow[:, None] * wcol[None, :]) if own_divisor else np.full((oh, ow), fx * fy, np.int64)
    d = d[None, :, :, None]
    out = (((sums + d // 2) * ((1 << 24) // d)) & 0xFFFFFFFF) >> 24
    return _like(img, out.astype(np.uint8))


def gap_plan(in_w, in_h, out_w, out_h, box=None, gap=None, a=3):
    """(fx, fy, safe_box, (reduced_w, reduced_h), inner_box): how a request with reducing_gap resolves; fx = fy = 1 when
    nothing is reduced (safe box = the whole frame, inner box = the caller's)."""
    x0, y0, x1, y1 = [float(v) for v in (box if box is not None else (0, 0, in_w, in_h))]
    if gap is None:
        return 1, 1, (0, 0, in_w, in_h), (in_w, in_h), (x0, y0, x1, y1)
    assert gap >= 1.0
    fx = int((x1 - x0) / out_w / gap) or 1
    fy = int((y1 - y0) / out_h / gap) or 1
    if fx == 1 and fy == 1:
        return 1, 1, (0, 0, in_w, in_h), (in_w, in_h), (x0, y0, x1, y1)
    s = a - 0.5
    sx = s * ((x1 - x0) / out_w)
    sy = s * ((y1 - y0) / out_h)
    rb = (max(0, int(x0 - sx)), max(0, int(y0 - sy)), min(in_w, math.ceil(x1 + sx)), min(in_h, math.ceil(y1 + sy)))
    rw, rh = -(-(rb[2] - rb[0]) // fx), -(-(rb[3] - rb[1]) // fy)
    inner = ((x0 - rb[0]) / fx, (y0 - rb[1]) / fy, (x1 - rb[0]) / fx, (y1 - rb[1]) / fy)
    return fx, fy, rb, (rw, rh), inner


def resize(img, out_w, out_h, box=None, reducing_gap=None, a=3, alpha=False, order=None):
    """The whole call: Image.resize((out_w, out_h), LANCZOS, box, reducing_gap) on uint8 / uint16 frames."""
    x = _as4(img)
    in_h, in_w = x.shape[1], x.shape[2]
    fx, fy, rb, _, inner = gap_plan(in_w, in_h, out_w, out_h, box, reducing_gap, a)
    if fx == 1 and fy == 1:
        return resize_box(img, out_w, out_h, box, a, alpha, order=order)
    assert not alpha and x.dtype == np.uint8
    return _like(img, resize_box(reduce(x, (fx, fy), rb), out_w, out_h, inner, a, order=order))
