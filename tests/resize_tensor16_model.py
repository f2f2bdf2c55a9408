"""numpy model of the 16-bit tensor contract (include/lanczos_hip.h, lanczos_tensor16_out):

    out[f][c * chan_stride + y * row_stride + x * pix_stride] = lut[c * 256 + bytes[f][y][x][c]]

on 16-bit words (bfloat16 or float16 patterns), strides in elements.  The bytes are whatever the byte request gives
(Context.resize, a Pillow fixture): this file only applies the table and the strides."""
import numpy as np


def words(a):
    """a uint16 or float16 array -> its 16-bit patterns"""
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.uint16, np.float16), a.dtype
    return a.view(np.uint16)


def identity_lut16(channels):
    """lut[c][v] = the word c << 8 | v: it names channel and byte, so a result names what was looked up.  Read as bfloat16 or
    as float16 the entries are zeros and subnormals (channel 0) and small normals; `special_lut16` has the rest."""
    c, v = np.mgrid[0:channels, 0:256]
    return (c << 8 | v).astype(np.uint16)


def special_lut16(channels):
    """identity_lut16 moved into the top of both formats: 0x7C00 | c << 8 | v and, for odd bytes, its negative.  In float16
    these are inf (v = 0, c = 0) and NaNs of every payload; in bfloat16 large normals, inf (0x7F80) and NaNs.  Distinct words,
    so they still name channel and byte."""
    c, v = np.mgrid[0:channels, 0:256]
    return (0x7C00 | (v & 1) << 15 | c << 8 | v).astype(np.uint16)


def strides(layout, w, h, c):
    return {"chw": (h * w, w, 1), "hwc": (1, w * c, c)}[layout]


def extent(w, h, c, st):
    """elements from the first to the last of one frame"""
    return (c - 1) * st[0] + (h - 1) * st[1] + (w - 1) * st[2] + 1


def scatter(out, base, bytes_fhwc, lut, st, frame_stride):
    """Writes the words the contract names into `out` (uint16, 1-D) in place: frame f starts at element base + f *
    frame_stride.  Returns the number of words written (every address once: asserted)."""
    f, h, w, c = bytes_fhwc.shape
    lb = words(lut).reshape(c, 256)
    ci, yi, xi = np.meshgrid(np.arange(c), np.arange(h), np.arange(w), indexing="ij")
    at = (ci * st[0] + yi * st[1] + xi * st[2]).reshape(-1)
    assert len(np.unique(at)) == at.size, "strides overlap"
    for k in range(f):
        out[base + k * frame_stride + at] = lb[ci, bytes_fhwc[k][yi, xi, ci]].reshape(-1)
    return f * at.size


def tensor16(ref_bytes, lut, layout="chw"):
    """The words of a tightly packed result for [H][W], [H][W][C] or [F][H][W][C] bytes, shaped as Context.resize_tensor
    shapes it: uint16 [F][C][H][W] or [F][H][W][C], the frame axis dropped with the input's."""
    b = np.asarray(ref_bytes)
    x = b.reshape(b.shape + (1,)) if b.ndim == 2 else b
    x = x if x.ndim == 4 else x[None]
    f, h, w, c = x.shape
    st = strides(layout, w, h, c)
    n = extent(w, h, c, st)
    assert n == c * h * w
    out = np.zeros(f * n, dtype=np.uint16)
    assert scatter(out, 0, x, lut, st, n) == out.size
    out = out.reshape((f, c, h, w) if layout == "chw" else (f, h, w, c))
    return out if b.ndim == 4 else out[0]
