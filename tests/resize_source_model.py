"""numpy model of a source layout (lanczos_resize_source): sample (y, x, c) of frame f lies at byte
    at + f * frame_stride + c * chan_stride + y * row_stride + x * pix_stride
of a buffer.  build() lays an (N, H, W, C) array out that way and fills EVERY byte the layout does not name -- row padding, plane
gaps, the gap between frames, the margins in front and behind -- with noise from another seed, never with zeros, so that padding
which leaks into a tap shows in the result.  unpack() is the inverse."""
import collections

import numpy as np

Source = collections.namedtuple("Source", "buf at layout row_stride chan_stride pix_stride frame_stride extent")
MARGIN = 64   # bytes in front of frame 0 (a multiple of 4: `base` alone sets the residue of the first byte) and behind the last


def strides(shape, itemsize, layout, row_stride=None, chan_stride=None):
    """(row_stride, chan_stride, pix_stride, extent) in bytes; None = the tight layout of that kind"""
    _, h, w, c = shape
    if layout == "planar":
        rs = w * itemsize if row_stride is None else row_stride
        cs = h * rs if chan_stride is None else chan_stride
        return rs, cs, itemsize, c * cs
    assert layout == "interleaved", layout
    rs = w * c * itemsize if row_stride is None else row_stride
    return rs, itemsize, c * itemsize, h * rs


def _offsets(shape, itemsize, rs, cs, ps, fs):
    """the byte offset of the first byte of every sample, [N][H][W][C]"""
    n, h, w, c = shape
    f, y, x, ch = np.ix_(np.arange(n, dtype=np.int64), np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64),
                         np.arange(c, dtype=np.int64))
    return f * fs + ch * cs + y * rs + x * ps


def build(frames, layout, row_stride=None, chan_stride=None, base=0, frame_stride=None, seed=1, fill_seed=None):
    """frames: (N, H, W, C) of uint8, uint16 or float32.  base: 0..3, the residue of frame 0's first byte where the buffer itself
    starts on a dword.  fill_seed: the seed of the noise in the unnamed bytes (two buffers that differ only there)."""
    frames = np.ascontiguousarray(frames)
    assert frames.ndim == 4 and 0 <= base < 4
    b = frames.dtype.itemsize
    rs, cs, ps, extent = strides(frames.shape, b, layout, row_stride, chan_stride)
    fs = extent if frame_stride is None else frame_stride
    assert fs >= extent
    n = frames.shape[0]
    total = MARGIN + base + (n - 1) * fs + extent + MARGIN
    buf = np.random.default_rng(10007 + (seed if fill_seed is None else fill_seed)).integers(1, 256, total, dtype=np.uint8)
    at = MARGIN + base
    off = _offsets(frames.shape, b, rs, cs, ps, fs) + at
    raw = frames.reshape(frames.shape + (1,)).view(np.uint8)          # [N][H][W][C][b]
    named = np.zeros(total, dtype=bool)
    for k in range(b):
        assert not named[off + k].any(), "the layout names a byte twice"
        named[off + k] = True
        buf[off + k] = raw[..., k]
    return Source(buf, at, layout, rs, cs, ps, fs, extent)


def unpack(src, shape, dtype=np.uint8):
    """the (N, H, W, C) array a Source holds"""
    b = np.dtype(dtype).itemsize
    off = _offsets(shape, b, src.row_stride, src.chan_stride, src.pix_stride, src.frame_stride) + src.at
    raw = np.stack([src.buf[off + k] for k in range(b)], axis=-1)
    return np.ascontiguousarray(raw).view(dtype)[..., 0]


def named_mask(src, shape, itemsize=1):
    """True at every byte of the buffer the layout names"""
    off = _offsets(shape, itemsize, src.row_stride, src.chan_stride, src.pix_stride, src.frame_stride) + src.at
    m = np.zeros(src.buf.size, dtype=bool)
    for k in range(itemsize):
        m[off + k] = True
    return m
