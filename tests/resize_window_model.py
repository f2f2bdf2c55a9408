"""The resize contract on a window of the source: the numpy models' tables and passes applied to just the rectangle that a
chosen set of output rows and columns reads, so that a frame of gigabytes can be checked in milliseconds.

Nothing of the contract is restated here.  The two axis tables are the models' (resize_box_model.axis_tables for Lanczos,
resize_filters_model.axis_tables for the other weighted filters, with f64 for 16-bit and float samples; NEAREST:
resize_filters_model.nearest_index), built for the whole axis.  The passes are the models' too (resize_model._pass,
resize16_model.pass_sums + store, resize32_model.one_pass, resize_alpha_model.premultiply / unpremultiply), called with
`first` shifted by the window's origin: int64 sums for 8-bit, one IEEE multiply and one IEEE add per tap in ascending order
for the wide samples.  Horizontal first, into the intermediate Pillow stores, for the rows the chosen output rows read; then
vertical -- or vertical first over the columns the chosen output columns read, where resize_model.pass_order says so.  An axis that keeps its size with an idle box is skipped (its chosen rows / columns are taken as they are), and a
request that changes neither axis is a copy.

    fetch(y0, y1, x0, x1) -> ndarray [y1 - y0][x1 - x0][C] of the request's dtype: that rectangle of the source

is called once, with rows [min first_v, max(first_v + count_v)) and columns [min first_h, max(first_h + count_h)) over the
chosen outputs.  tests/test_resize_window_model.py pins this module to the whole-frame models bit for bit.
"""
import functools

import numpy as np

import resize16_model as M16
import resize32_model as M32
import resize_alpha_model as MA
import resize_box_model as MB
import resize_filters_model as F
import resize_model as M


@functools.lru_cache(maxsize=64)
def axis_tables(filt, in_n, out_n, b0, b1, a, f64):
    """The whole axis' (first, count, coeffs) from the models; cached, a table of 65535 outputs takes a second."""
    if filt == F.LANCZOS:
        return MB.axis_tables(in_n, out_n, a, b0, b1, f64=f64)
    return F.axis_tables(filt, in_n, out_n, b0, b1, a, f64=f64)


class Axis:
    """One axis of a request for a chosen set of outputs `sel`: whether its pass runs, the source interval [lo, hi) those
    outputs read, and (a running, weighted axis) their first / count / coeffs."""

    def __init__(self, filt, in_n, out_n, b0, b1, a, f64, sel):
        self.sel = np.asarray(sel, np.int64)
        assert self.sel.ndim == 1 and self.sel.size and 0 <= self.sel.min() and self.sel.max() < out_n
        self.runs = MB.axis_runs(in_n, out_n, b0, b1)
        self.first = self.count = self.k = None
        if filt == F.NEAREST:
            self.index = F.nearest_index(in_n, out_n, b0, b1).astype(np.int64)[self.sel]
            self.lo, self.hi = int(self.index.min()), int(self.index.max()) + 1
        elif self.runs:
            f, c, k = axis_tables(filt, in_n, out_n, b0, b1, a, f64)
            self.first, self.count, self.k = f[self.sel].astype(np.int64), c[self.sel].astype(np.int64), k[self.sel]
            self.lo, self.hi = int(self.first.min()), int((self.first + self.count).max())
        else:
            self.index = self.sel
            self.lo, self.hi = int(self.sel.min()), int(self.sel.max()) + 1
        assert 0 <= self.lo < self.hi <= in_n


def axes(in_w, in_h, out_w, out_h, dtype, rows, cols, a=3, filt=F.LANCZOS, box=None):
    """(horizontal Axis over `cols`, vertical Axis over `rows`) of a request: what the reference will fetch."""
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    f64 = np.dtype(dtype) != np.uint8
    return (Axis(filt, in_w, out_w, x0, x1, a, f64, cols), Axis(filt, in_h, out_h, y0, y1, a, f64, rows))


def _pass(y, axis, ax, origin, dtype):
    """one pass of the models along `axis` of y [1][h][w][C] for the outputs of `ax`, the window starting at `origin`"""
    first = (ax.first - origin).astype(np.int32)
    if dtype == np.uint8:
        return M._pass(y, axis, first, ax.k)
    if dtype == np.uint16:
        return M16.store(M16.pass_sums(y.astype(np.float64), axis, first, ax.count, ax.k))
    return M32.one_pass(y, axis, first, ax.count, ax.k).astype(np.float32)


def resize(fetch, in_w, in_h, out_w, out_h, channels, dtype, rows, cols, a=3, filt=F.LANCZOS, alpha=False, box=None):
    """Output rows `rows` x output columns `cols` (index arrays, any order) of the request, [len(rows)][len(cols)][C] of
    `dtype` (uint8, uint16 or float32).  alpha: the last of four 8-bit channels is straight alpha."""
    dtype = np.dtype(dtype)
    assert dtype in (np.uint8, np.uint16, np.float32) and (not alpha or (dtype == np.uint8 and channels == 4))
    H, V = axes(in_w, in_h, out_w, out_h, dtype, rows, cols, a, filt, box)
    src = np.asarray(fetch(V.lo, V.hi, H.lo, H.hi))
    assert src.shape == (V.hi - V.lo, H.hi - H.lo, channels) and src.dtype == dtype, (src.shape, src.dtype)
    gather_h = lambda y: y[:, :, H.index - H.lo]
    gather_v = lambda y: y[:, V.index - V.lo]
    x = src[None]
    if filt == F.NEAREST or not (H.runs or V.runs):     # whole pixels (NEAREST: no premultiply), or the copy
        return gather_h(gather_v(x))[0].copy()
    if alpha:
        x = MA.premultiply(x)
    with np.errstate(all="ignore"):
        y = x if dtype == np.float32 else x.astype(np.int64)
        for axis in M.pass_order(in_w, in_h, out_h):
            if axis == 2:
                y = _pass(y, 2, H, H.lo, dtype) if H.runs else gather_h(y)
            else:
                y = _pass(y, 1, V, V.lo, dtype) if V.runs else gather_v(y)
    y = y.astype(dtype)
    if alpha:
        y = MA.unpremultiply(y)
    return y[0]
