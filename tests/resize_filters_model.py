"""Numpy restatement of the resize contract for Pillow's other filters (Image.resize(size, resample, box, reducing_gap) with
resample in BOX, BILINEAR, HAMMING, BICUBIC, NEAREST; LANCZOS is here too, as filter 0, so that one function serves all).

Written from the contract in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code and not from Pillow's.  It
stands on the models of the Lanczos paths (resize_model, resize16_model, resize32_model, resize_alpha_model,
resize_box_model) and changes what the contract says a filter changes:

  weighted  the support S that stands where Lanczos has a, and the weight function w(x); tap geometry, normalisation, 22-bit
            rounding, double tables, passes, premultiplied alpha, the I;16 store and the float rule are the other models'.
  nearest   per axis idx[o] = int(xo), xo = b0f + step / 2 advanced by xo += step (a running sum in double), step =
            float32(b1f - b0f) / out; out[y][x] = in[idx_v[y]][idx_h[x]], whole pixels, no premultiply.

The keyword switches are the near misses a fixture has to tell from the contract:
    hamming_double   0.54 and 0.46 as double literals (Pillow's are float literals widened to double)
    box_symmetric    BOX weighs |x| <= 0.5 (Pillow's interval is -0.5 < x <= 0.5)
    bicubic_a        another a of the bicubic (-0.75 is the other common one; Pillow's is -0.5)
    nearest_direct   idx[o] = int(b0f + (o + 0.5) * step) instead of the running sum
    nearest_premul   NEAREST on RGBA with the premultiply round trip of the weighted filters
    order="h_first"  the horizontal pass first whatever the shape (Pillow runs a tall frame that shrinks vertical first:
                     resize_model.pillow_vertical_first)
"""
import math

import numpy as np

import resize16_model as M16
import resize32_model as M32
import resize_alpha_model as MA
import resize_box_model as MB
import resize_model as M

LANCZOS, BOX, BILINEAR, HAMMING, BICUBIC, NEAREST = range(6)
NAMES = ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest")
WEIGHTED = (LANCZOS, BOX, BILINEAR, HAMMING, BICUBIC)
PRECISION_BITS = M.PRECISION_BITS
F054, F046 = float(np.float32(0.54)), float(np.float32(0.46))


def support(filt, a=3):
    return {LANCZOS: float(a), BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0}[filt]


def weight(filt, x, a=3, hamming_double=False, box_symmetric=False, bicubic_a=-0.5):
    if filt == LANCZOS:
        return M._filter(x, a)
    if filt == BOX:
        if box_symmetric:
            return 1.0 if abs(x) <= 0.5 else 0.0
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    x = abs(x)
    if filt == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if filt == HAMMING:
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        c54, c46 = (0.54, 0.46) if hamming_double else (F054, F046)
        return math.sin(x) / x * (c54 + c46 * math.cos(x))
    if filt == BICUBIC:
        ca = bicubic_a
        if x < 1.0:
            return ((ca + 2.0) * x - (ca + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * ca
        return 0.0
    raise ValueError(filt)


def ksize(filt, out_n, b0, b1, a=3):
    if filt == NEAREST:
        return 1
    scale, _ = MB.axis_scale(out_n, b0, b1)
    return int(math.ceil(support(filt, a) * max(scale, 1.0))) * 2 + 1


def nearest_index(in_n, out_n, b0, b1, direct=False):
    step, c0 = MB.axis_scale(out_n, b0, b1)
    if direct:
        return np.array([int(c0 + (o + 0.5) * step) for o in range(out_n)], np.int32)
    idx = np.zeros(out_n, np.int32)
    xo = c0 + step * 0.5
    for o in range(out_n):
        idx[o] = int(xo)
        xo += step
    return idx


def axis_tables(filt, in_n, out_n, b0=None, b1=None, a=3, f64=False, **variant):
    """(first[out] int32, count[out] int32, coeffs[out][ksize]): int32 22-bit fixed point, or float64 with f64.  NEAREST:
    first = the source index, count = 1, one coefficient 2^22 or 1.0."""
    if b0 is None:
        b0, b1 = 0, in_n
    if filt == NEAREST:
        first = nearest_index(in_n, out_n, b0, b1, variant.get("nearest_direct", False))
        one = np.ones((out_n, 1), np.float64) if f64 else np.full((out_n, 1), 1 << PRECISION_BITS, np.int32)
        return first, np.ones(out_n, np.int32), one
    wv = {k: v for k, v in variant.items() if k in ("hamming_double", "box_symmetric", "bicubic_a")}
    scale, c0 = MB.axis_scale(out_n, b0, b1)
    fs = max(scale, 1.0)
    sup = support(filt, a) * fs
    ss = 1.0 / fs
    ks = int(math.ceil(sup)) * 2 + 1
    first = np.zeros(out_n, np.int32)
    count = np.zeros(out_n, np.int32)
    k = np.zeros((out_n, ks), np.float64 if f64 else np.int32)
    for o in range(out_n):
        center = c0 + (o + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), in_n)
        n = xmax - xmin
        w = [weight(filt, ((i + xmin) - center + 0.5) * ss, a, **wv) for i in range(n)]
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


def gap_plan(filt, in_w, in_h, out_w, out_h, box=None, gap=None, a=3):
    """resize_box_model.gap_plan with the filter's support in the safe box (S - 0.5 where Lanczos has a - 0.5)."""
    return MB.gap_plan(in_w, in_h, out_w, out_h, box, gap, a=support(filt, a))


def _resize_plain(x, filt, out_w, out_h, box, a, alpha, variant):
    """x: [F][H][W][C] uint8 / uint16 / float32, no gap"""
    in_h, in_w = x.shape[1], x.shape[2]
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    run_h, run_v = MB.axis_runs(in_w, out_w, x0, x1), MB.axis_runs(in_h, out_h, y0, y1)
    if not run_h and not run_v:
        return x.copy()
    if filt == NEAREST:
        direct = variant.get("nearest_direct", False)
        ih = nearest_index(in_w, out_w, x0, x1, direct)
        iv = nearest_index(in_h, out_h, y0, y1, direct)
        premul = alpha and variant.get("nearest_premul", False)
        src = MA.premultiply(x) if premul else x
        y = src[:, iv][:, :, ih]
        return (MA.unpremultiply(y) if premul else y).astype(x.dtype)
    f32, u16 = x.dtype == np.float32, x.dtype == np.uint16
    spans = {2: (2, run_h, in_w, out_w, x0, x1), 1: (1, run_v, in_h, out_h, y0, y1)}
    axes = [spans[axis] for axis in M.pass_order(in_w, in_h, out_h, variant.get("order"))]
    if f32:
        y = x
        with np.errstate(all="ignore"):
            for axis, run, in_n, out_n, b0, b1 in axes:
                if run:
                    f, c, k = axis_tables(filt, in_n, out_n, b0, b1, a, f64=True, **variant)
                    y = M32.one_pass(y, axis, f, c, k).astype(np.float32)
        return y
    if alpha:
        assert not u16 and x.shape[-1] == 4
        x = MA.premultiply(x)
    y = x.astype(np.int64)
    for axis, run, in_n, out_n, b0, b1 in axes:
        if not run:
            continue
        f, c, k = axis_tables(filt, in_n, out_n, b0, b1, a, f64=u16, **variant)
        if u16:
            y = M16.store(M16.pass_sums(y.astype(np.float64), axis, f, c, k))
        else:
            y = M._pass(y, axis, f, k)
    y = y.astype(x.dtype)
    return MA.unpremultiply(y) if alpha else y


def resize(img, filt, out_w, out_h, box=None, reducing_gap=None, a=3, alpha=False, **variant):
    """The whole call: Image.resize((out_w, out_h), filt, box, reducing_gap) on uint8 / uint16 / float32 frames [H][W],
    [H][W][C] or [F][H][W][C]; alpha: the last of four 8-bit channels is straight alpha (mode RGBA)."""
    x = MB._as4(img)
    in_h, in_w = x.shape[1], x.shape[2]
    if reducing_gap is not None:
        assert filt != NEAREST and x.dtype == np.uint8 and not alpha
        fx, fy, rb, _, inner = gap_plan(filt, in_w, in_h, out_w, out_h, box, reducing_gap, a)
        if fx > 1 or fy > 1:
            return MB._like(img, _resize_plain(MB.reduce(x, (fx, fy), rb), filt, out_w, out_h, inner, a, False, variant))
    return MB._like(img, _resize_plain(x, filt, out_w, out_h, box, a, alpha, variant))


def same(got, want):
    """bytes equal; for float32 NaN positions coincide and every other sample is equal as a 32-bit pattern"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        return M32.same(got, want)
    return np.array_equal(got, want)
