"""numpy model of a destination layout (lanczos_resize_dest): sample (y, x, c) of frame f goes to byte
    at + f * frame_stride + c * chan_stride + y * row_stride + x * pix_stride
of a buffer.  build() makes the buffer a call stores into and fills the WHOLE of it with noise, never zeros -- the bytes the layout
names, row padding, plane gaps, the gaps between frames and the margins in front and behind -- so that a store which is one byte
too wide shows: either in a neighbour's sample (row_stride == w) or in the noise.  The buffer ends MARGIN bytes behind the last
byte the layout names: the padding behind the last row of the last frame is not part of it.  unpack() reads the frames back,
named_mask() says which bytes a call may change.  A destination read back as a source (tests/resize_source_model.py) gives the
frames: the two layouts are one formula."""
import collections

import numpy as np

import resize_source_model as SM

Dest = collections.namedtuple("Dest", "buf at layout row_stride chan_stride pix_stride frame_stride extent named")
MARGIN = SM.MARGIN   # bytes in front of frame 0 (a multiple of 4: `base` alone sets the residue of the first byte) and behind


def strides(shape, itemsize, layout, row_stride=None, chan_stride=None):
    """(row_stride, chan_stride, pix_stride, extent, named) in bytes; None = the tight layout of that kind.  extent is the default
    frame stride, named the last named byte of a frame + 1"""
    _, h, w, c = shape
    rs, cs, ps, extent = SM.strides(shape, itemsize, layout, row_stride, chan_stride)
    if layout == "planar":
        return rs, cs, ps, extent, (c - 1) * cs + (h - 1) * rs + w * itemsize
    return rs, cs, ps, extent, (h - 1) * rs + w * c * itemsize


def build(shape, layout, row_stride=None, chan_stride=None, base=0, frame_stride=None, seed=1, itemsize=1):
    """shape: (N, H, W, C) of the frames the call stores.  base: 0..3, the residue of frame 0's first byte where the buffer itself
    starts on a dword.  Every byte is noise in 1..255"""
    assert len(shape) == 4 and 0 <= base < 4
    rs, cs, ps, extent, named = strides(shape, itemsize, layout, row_stride, chan_stride)
    fs = extent if frame_stride is None else frame_stride
    assert fs >= named
    total = MARGIN + base + (shape[0] - 1) * fs + named + MARGIN
    buf = np.random.default_rng(20011 + seed).integers(1, 256, total, dtype=np.uint8)
    t = Dest(buf, MARGIN + base, layout, rs, cs, ps, fs, extent, named)
    m = named_mask(t, shape, itemsize)
    assert int(m.sum()) == int(np.prod(shape)) * itemsize, "the layout names a byte twice"
    return t


def _offsets(t, shape, itemsize):
    return SM._offsets(shape, itemsize, t.row_stride, t.chan_stride, t.pix_stride, t.frame_stride) + t.at


def named_mask(t, shape, itemsize=1):
    """True at every byte of the buffer the layout names"""
    off = _offsets(t, shape, itemsize)
    m = np.zeros(t.buf.size, dtype=bool)
    for k in range(itemsize):
        m[off + k] = True
    return m


def unpack(t, shape, dtype=np.uint8, buf=None):
    """the (N, H, W, C) array the buffer (t.buf, or `buf` of the same layout) holds"""
    buf = t.buf if buf is None else buf
    b = np.dtype(dtype).itemsize
    off = _offsets(t, shape, b)
    raw = np.stack([buf[off + k] for k in range(b)], axis=-1)
    return np.ascontiguousarray(raw).view(dtype)[..., 0]


def pack(t, frames):
    """a copy of t.buf with `frames` (N, H, W, C) stored by the formula: what a call has to leave behind"""
    frames = np.ascontiguousarray(frames)
    b = frames.dtype.itemsize
    off = _offsets(t, frames.shape, b)
    raw = frames.reshape(frames.shape + (1,)).view(np.uint8)
    out = t.buf.copy()
    for k in range(b):
        out[off + k] = raw[..., k]
    return out


def as_source(t):
    """the same layout as a Source of tests/resize_source_model.py (over the same buffer)"""
    return SM.Source(t.buf, t.at, t.layout, t.row_stride, t.chan_stride, t.pix_stride, t.frame_stride, t.extent)
