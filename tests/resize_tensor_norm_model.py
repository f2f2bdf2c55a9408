"""numpy model of the normalised-tensor contract for 16-bit and float samples (include/lanczos_hip.h, lanczos_tensor_norm):

    out[f][oc * chan_stride + Y * row_stride + X * pix_stride] = cvt(((float32)P[f][y][x][src[oc]] / div[oc] - mean[oc]) / std[oc])

three float32 operations, each rounded on its own (numpy's float32 `/` and `-` are IEEE operations and keep denormals), then
L.lut_convert16 for bfloat16 / float16 elements.  X, Y mirror x, y per frame by bits 0 and 1 of the frame's flip.  The samples P
are whatever the sample request gives (Context.resize / Context.resize_f32, a Pillow fixture): this file only applies the
arithmetic, the map, the flips and the strides.  Results are bit patterns: uint32 for float32, uint16 for the 16-bit formats."""
import numpy as np

import lanczos_hls_amd as L


def _per_channel(v, n):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (n,)))


def elements(samples, div, mean, std, dtype="float32"):
    """samples [..., C] (uint16 or float32), div / mean / std one value or C of them -> the elements' bit patterns, same shape"""
    p = np.asarray(samples)
    assert p.dtype in (np.uint16, np.float32), p.dtype
    c = p.shape[-1]
    d, m, s = (_per_channel(v, c) for v in (div, mean, std))
    with np.errstate(all="ignore"):
        e = ((p.astype(np.float32) / d) - m) / s
    assert e.dtype == np.float32
    if dtype == "float32":
        return np.ascontiguousarray(e).view(np.uint32)
    return np.ascontiguousarray(L.lut_convert16(e, dtype)).view(np.uint16)


def folded(samples, div, mean, std):
    """the form the contract forbids: one multiply by a folded scale and one add, as float32 patterns"""
    p = np.asarray(samples)
    c = p.shape[-1]
    d, m, s = (_per_channel(v, c) for v in (div, mean, std))
    with np.errstate(all="ignore"):
        scale = np.float32(1.0) / (d * s)
        bias = -m / s
        e = p.astype(np.float32) * scale + bias
    return np.ascontiguousarray(e.astype(np.float32)).view(np.uint32)


def default_div(samples):
    return 65535.0 if np.asarray(samples).dtype == np.uint16 else 1.0


def strides(layout, w, h, c):
    return {"chw": (h * w, w, 1), "hwc": (1, w * c, c)}[layout]


def extent(w, h, c, st):
    """elements from the first to the last of one frame"""
    return (c - 1) * st[0] + (h - 1) * st[1] + (w - 1) * st[2] + 1


def _flips(flips, f):
    return [int(flips) & 3] * f if np.ndim(flips) == 0 else [int(m) & 3 for m in flips]


def scatter(out, base, samples_fhwc, div, mean, std, dtype, src, flips, st, frame_stride):
    """Writes the patterns the contract names into `out` (1-D, uint32 or uint16) in place: frame f starts at element base + f *
    frame_stride.  div / mean / std are in OUTPUT order.  Returns the number written (every address once: asserted)."""
    f, h, w, _ = samples_fhwc.shape
    oc = len(src)
    el = elements(np.asarray(samples_fhwc)[..., list(src)], div, mean, std, dtype)   # [F][h][w][OC]
    assert el.dtype == out.dtype
    ci, yi, xi = np.meshgrid(np.arange(oc), np.arange(h), np.arange(w), indexing="ij")
    for k, m in enumerate(_flips(flips, f)):
        X = w - 1 - xi if m & 1 else xi
        Y = h - 1 - yi if m & 2 else yi
        at = (ci * st[0] + Y * st[1] + X * st[2]).reshape(-1)
        assert len(np.unique(at)) == at.size, "strides overlap"
        out[base + k * frame_stride + at] = el[k][yi, xi, ci].reshape(-1)
    return f * oc * h * w


def norm(samples, div=None, mean=0.0, std=1.0, dtype="float32", src=None, flips=0, layout="chw"):
    """The patterns of a tightly packed result for [H][W], [H][W][C] or [F][H][W][C] samples, shaped as
    Context.resize_tensor_norm shapes it: [F][OC][H][W] or [F][H][W][OC], the frame axis dropped with the input's."""
    b = np.asarray(samples)
    x = b.reshape(b.shape + (1,)) if b.ndim == 2 else b
    x = x if x.ndim == 4 else x[None]
    f, h, w, c = x.shape
    src = tuple(range(c)) if src is None else tuple(src)
    oc = len(src)
    st = strides(layout, w, h, oc)
    n = extent(w, h, oc, st)
    out = np.zeros(f * n, dtype=np.uint32 if dtype == "float32" else np.uint16)
    assert scatter(out, 0, x, default_div(b) if div is None else div, mean, std, dtype, src, flips, st, n) == out.size
    out = out.reshape((f, oc, h, w) if layout == "chw" else (f, h, w, oc))
    return out if b.ndim == 4 else out[0]


def patterns(a):
    """what Context.resize_tensor_norm returns -> its bit patterns"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def nan_mask(words, dtype):
    w = patterns(words)
    if dtype == "float32":
        return np.isnan(w.view(np.float32))
    if dtype == "float16":
        return np.isnan(w.view(np.float16))
    return ((w & 0x7F80) == 0x7F80) & ((w & 0x007F) != 0)


def same_bits(got, want, dtype):
    """NaN positions coincide and everything else is equal as patterns (the contract sends a NaN to some NaN)"""
    g, w = patterns(got), patterns(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    gn, wn = nan_mask(g, dtype), nan_mask(w, dtype)
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))
