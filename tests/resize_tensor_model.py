"""numpy model of the tensor contract (include/lanczos_hip.h, lanczos_tensor_out):

    out[f][c * chan_stride + y * row_stride + x * pix_stride] = lut[c * 256 + bytes[f][y][x][c]]

on 32-bit words, so that table entries move as bit patterns (NaN payloads included).  The bytes are whatever the byte request
gives (Context.resize, a Pillow fixture, a model): this file only applies the table and the strides."""
import numpy as np


def bits(a):
    """float32 array -> its 32-bit patterns"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def identity_lut(channels):
    """lut[c][v] = the float whose bits are 0x7FC00000 | c << 8 | v: a quiet NaN whose payload names channel and byte, so a
    result names what was looked up, and anything computed on an entry would lose it."""
    c, v = np.mgrid[0:channels, 0:256]
    return (0x7FC00000 | c << 8 | v).astype(np.uint32).view(np.float32)


def strides(layout, w, h, c):
    return {"chw": (h * w, w, 1), "hwc": (1, w * c, c)}[layout]


def extent(w, h, c, st):
    """floats from the first to the last of one frame"""
    return (c - 1) * st[0] + (h - 1) * st[1] + (w - 1) * st[2] + 1


def scatter(words, base, bytes_fhwc, lut, st, frame_stride):
    """Writes the words the contract names into `words` (uint32, 1-D) in place: frame f starts at word base + f *
    frame_stride.  Returns the number of words written (every address once: asserted)."""
    f, h, w, c = bytes_fhwc.shape
    lb = bits(lut).reshape(c, 256)
    ci, yi, xi = np.meshgrid(np.arange(c), np.arange(h), np.arange(w), indexing="ij")
    at = (ci * st[0] + yi * st[1] + xi * st[2]).reshape(-1)
    assert len(np.unique(at)) == at.size, "strides overlap"
    for k in range(f):
        words[base + k * frame_stride + at] = lb[ci, bytes_fhwc[k][yi, xi, ci]].reshape(-1)
    return f * at.size


def tensor(bytes_img, lut, layout="chw"):
    """The words of a tightly packed result for [H][W], [H][W][C] or [F][H][W][C] bytes, shaped as Context.resize_tensor
    shapes it: uint32 [F][C][H][W] or [F][H][W][C], the frame axis dropped with the input's."""
    b = np.asarray(bytes_img)
    x = b.reshape(b.shape + (1,)) if b.ndim == 2 else b
    x = x if x.ndim == 4 else x[None]
    f, h, w, c = x.shape
    st = strides(layout, w, h, c)
    n = extent(w, h, c, st)
    assert n == c * h * w
    words = np.zeros(f * n, dtype=np.uint32)
    assert scatter(words, 0, x, lut, st, n) == words.size
    out = words.reshape((f, c, h, w) if layout == "chw" else (f, h, w, c))
    return out if b.ndim == 4 else out[0]
