"""Numpy restatement of the resize contract (Pillow's Image.resize with LANCZOS, 8-bit, any a in {2, 3, 4}).

Written from the recipe in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code.  Tables are built per
axis in double with math.sin (libm, like Pillow); the passes are vectorised int64 sums, which equal Pillow's int32 sums
because the accumulator provably stays below 2^31 (tests/test_resize_host.py checks the bound).
"""
import math

import numpy as np

PRECISION_BITS = 22


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
    """(first[out], count[out], coeffs[out][ksize]) as int32 arrays."""
    scale = in_n / out_n
    fs = max(scale, 1.0)
    support = a * fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_n, np.int32)
    count = np.zeros(out_n, np.int32)
    k = np.zeros((out_n, ks), np.int32)
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
            if ww != 0.0:
                v = v / ww
            k[o, i] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        first[o], count[o] = xmin, n
    return first, count, k


def _pass(x, axis, first, k):
    """x: int64 [..., n_in, ...] along `axis`; returns the clipped pass along that axis (int64 values 0..255).
    Works through the outputs in chunks so that a full-size frame stays within a few hundred MB."""
    out_n, ks = k.shape
    n_in = x.shape[axis]
    other = x.size // n_in
    step = max(1, (1 << 23) // max(1, other * ks))
    parts = []
    for o0 in range(0, out_n, step):
        kc = k[o0:o0 + step].astype(np.int64)
        m = kc.shape[0]
        idx = first[o0:o0 + step, None].astype(np.int64) + np.arange(ks)[None, :]
        idx = np.where(idx < n_in, idx, 0)                    # taps past the count carry a zero coefficient
        g = np.take(x, idx.reshape(-1), axis=axis)            # [..., m * ks, ...]
        shape = list(x.shape)
        shape[axis:axis + 1] = [m, ks]
        g = g.reshape(shape)
        kshape = [1] * len(shape)
        kshape[axis], kshape[axis + 1] = m, ks
        acc = (g * kc.reshape(kshape)).sum(axis=axis + 1) + (1 << (PRECISION_BITS - 1))
        parts.append(np.clip(acc >> PRECISION_BITS, 0, 255))
    return np.concatenate(parts, axis=axis)


def pillow_vertical_first(in_w, in_h, out_h):
    """Pillow 12.2.0's Image.resize runs the vertical pass first, over the full width, when the frame it resizes (the
    reduced one under a reducing_gap) is more than 100 times as tall as wide and shrinks in height.  The sizes are those
    after any gap reduction.  It only matters where both passes run; the intermediate is stored in the image's mode."""
    return in_h > 100 * in_w and out_h < in_h


def pass_order(in_w, in_h, out_h, order=None):
    """The axes of [F][H][W][C] in the order every model runs its passes: (2, 1) is horizontal first.  order="h_first" is
    the near miss a fixture has to tell from the contract: horizontal first whatever the shape."""
    assert order in (None, "h_first"), order
    return (1, 2) if order is None and pillow_vertical_first(in_w, in_h, out_h) else (2, 1)


def resize(img, out_w, out_h, a=3, order=None):
    """img: uint8 [H][W], [H][W][C] or [F][H][W][C] -> the resized image(s), same layout."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    x = img
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim == 3:
        x = x[None]
    in_h, in_w = x.shape[1], x.shape[2]
    y = x.astype(np.int64)
    sizes = {2: (in_w, out_w), 1: (in_h, out_h)}
    for axis in pass_order(in_w, in_h, out_h, order):
        in_n, out_n = sizes[axis]
        if out_n != in_n:
            f, _, k = axis_tables(in_n, out_n, a)
            y = _pass(y, axis, f, k)
    y = y.astype(np.uint8)
    if img.ndim == 2:
        return y[0, :, :, 0]
    if img.ndim == 3:
        return y[0]
    return y
