"""Numpy restatement of the float resize contract (Pillow's Image.resize(size, LANCZOS, box) on mode F, a in {2, 3, 4}).

Written from the recipe in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code.  Per axis the tap geometry
and the double coefficients are those of the 16-bit contract (resize16_model.axis_tables; with a box resize_box_model's);
one pass is, per output sample,
    ss = 0.0; for i = 0 .. count - 1 ascending: ss = ss + (double)sample[first + i] * k[i]    (a multiply and an add)
    stored = (float)ss                                                                         (nearest even)
with no clamp: a sum beyond FLT_MAX stores inf, a denormal stays a denormal, a tiny negative sum stores -0.0.  Exactly count
taps are multiplied -- one whose weight is 0.0 too (inf * 0.0 = NaN), none outside the window.  The first pass (the
horizontal one, unless resize_model.pillow_vertical_first) stores a float32 intermediate; a pass whose axis keeps its size with an idle box is skipped; no pass is a copy.
numpy's float64 array arithmetic does not contract a multiply and an add, and does not flush denormals.

The keyword switches of resize() are the near misses a fixture has to tell from the contract:
    acc32        accumulate in float32 instead of double
    mid64        keep the intermediate between the passes in double
    flush        flush float32 denormals to zero where samples are read and where they are stored
    pad_to       multiply taps up to max(count, pad_to(ksize)) with the table's +0.0 behind count, by the neighbouring sample
                 (0.0 beyond the axis), as a kernel that pads its loop to an instance's tap count would
    skip_zero_k  skip taps whose weight is 0.0 (a guard on the coefficient instead of on count)
"""
import numpy as np

import resize16_model as M16
import resize_box_model as MB
import resize_model as M

FUSED_K = (7, 9, 11, 13, 17, 25)
FLT_MIN = np.float32(1.17549435e-38)


def bucket(ks):
    """the tap count of the smallest fused instance that holds ks (ks itself beyond the widest)"""
    return next((k for k in FUSED_K if k >= ks), ks)


def tables(in_n, out_n, a, b0=None, b1=None):
    if b0 is None:
        return M16.axis_tables(in_n, out_n, a)
    return MB.axis_tables(in_n, out_n, a, b0, b1, f64=True)


def _flush(x):
    return np.where(np.abs(x) < FLT_MIN, np.copysign(np.float32(0), x), x).astype(np.float32)


def one_pass(x, axis, first, count, k, acc32=False, flush=False, pad_to=None, skip_zero_k=False):
    """x: float32 -> float64 sums of one pass along `axis` (float32-valued with acc32)."""
    out_n, ks = k.shape
    xm = np.moveaxis(x, axis, 0)
    n_in = xm.shape[0]
    if flush:
        xm = _flush(xm)
    acc_t = np.float32 if acc32 else np.float64
    out = np.empty((out_n,) + xm.shape[1:], acc_t)
    zero = np.zeros(xm.shape[1:], acc_t)
    with np.errstate(all="ignore"):
        for o in range(out_n):
            ss = zero.copy()
            f, n = int(first[o]), int(count[o])
            taps = n if pad_to is None else max(n, pad_to(ks))
            for i in range(taps):
                ki = k[o, i] if i < ks else 0.0
                if skip_zero_k and ki == 0.0:
                    continue
                s = xm[f + i].astype(acc_t) if f + i < n_in else zero
                ss = ss + s * acc_t(ki)
            out[o] = ss
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, a=3, box=None, acc32=False, mid64=False, flush=False, pad_to=None, skip_zero_k=False,
           order=None):
    """img: float32 [H][W], [H][W][C] or [F][H][W][C] -> the box (None = the whole frame) resized to out_h x out_w, same
    layout, every channel an independent plane."""
    img = np.asarray(img)
    assert img.dtype == np.float32
    x = img
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim == 3:
        x = x[None]
    in_h, in_w = x.shape[1], x.shape[2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    y = x
    ran = False
    with np.errstate(all="ignore"):
        spans = {2: (in_w, out_w, x0, x1), 1: (in_h, out_h, y0, y1)}
        for axis in M.pass_order(in_w, in_h, out_h, order):
            in_n, out_n, b0, b1 = spans[axis]
            if not MB.axis_runs(in_n, out_n, b0, b1):
                continue
            f, c, k = tables(in_n, out_n, a, b0, b1)
            src = y if (mid64 and ran) else y.astype(np.float32)
            ss = one_pass(src, axis, f, c, k, acc32, flush, pad_to, skip_zero_k)
            y = ss if mid64 else ss.astype(np.float32)
            ran = True
        y = y.astype(np.float32)
    if flush and ran:
        y = _flush(y)
    if not ran:
        y = x.copy()
    if img.ndim == 2:
        return y[0, :, :, 0]
    if img.ndim == 3:
        return y[0]
    return y


def same(got, want):
    """The comparison rule: NaN positions coincide, every other sample equal as a 32-bit pattern (inf, -0.0, denormals)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    return not differs(got, want).any()


def differs(got, want):
    """per sample: True where the comparison rule fails"""
    gn, wn = np.isnan(got), np.isnan(want)
    return (gn != wn) | (~gn & ~wn & (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)))
