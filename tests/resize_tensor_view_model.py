"""numpy model of the tensor view contract (include/lanczos_hip.h, lanczos_tensor_view):

    out[f][oc * chan_stride + Y * row_stride + X * pix_stride] = lut[oc * 256 + bytes[f][y][x][src[oc]]]
    X = w - 1 - x where bit 0 of flips[f] is set, Y = h - 1 - y where bit 1 is

on 32-bit or 16-bit words, strides in elements.  The bytes [F][h][w][C] are whatever the byte request gives for the same
window (Context.resize, a Pillow fixture): this file only applies the map, the table, the flips and the strides."""
import numpy as np

WORD = {4: np.uint32, 2: np.uint16}


def words(a):
    """a float32 / uint32 or float16 / uint16 array -> its bit patterns"""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize in WORD and a.dtype.kind in "fu", a.dtype
    return a.view(WORD[a.dtype.itemsize])


def strides(layout, w, h, oc):
    return {"chw": (h * w, w, 1), "hwc": (1, w * oc, oc)}[layout]


def extent(w, h, oc, st):
    """elements from the first to the last of one frame of oc output channels"""
    return (oc - 1) * st[0] + (h - 1) * st[1] + (w - 1) * st[2] + 1


def frame_flips(flips, frames):
    """None, an int for every frame, or one per frame -> one int per frame; bits 2..7 are ignored, as the kernels ignore them"""
    f = np.zeros(frames, dtype=np.int64) if flips is None else np.broadcast_to(np.asarray(flips, dtype=np.int64), (frames,))
    return f & 3


def scatter(out, base, bytes_fhwc, lut, src, flips, st, frame_stride):
    """Writes the words the contract names into `out` (1-D, uint32 or uint16) in place: frame f starts at element base + f *
    frame_stride.  Returns the number of words written (every address once: asserted)."""
    f, h, w, c = bytes_fhwc.shape
    src = np.asarray(src, dtype=np.int64)
    assert len(set(src.tolist())) == src.size and src.min() >= 0 and src.max() < c, "the map is injective and inside the source"
    lb = words(lut).reshape(src.size, 256)
    assert lb.dtype == out.dtype
    oi, yi, xi = np.meshgrid(np.arange(src.size), np.arange(h), np.arange(w), indexing="ij")
    for k, m in enumerate(frame_flips(flips, f)):
        X = w - 1 - xi if m & 1 else xi
        Y = h - 1 - yi if m & 2 else yi
        at = (oi * st[0] + Y * st[1] + X * st[2]).reshape(-1)
        assert len(np.unique(at)) == at.size, "strides overlap"
        out[base + k * frame_stride + at] = lb[oi, bytes_fhwc[k][yi, xi, src[oi]]].reshape(-1)
    return f * src.size * h * w


def view(bytes_img, lut, src=None, flips=None, layout="chw"):
    """The words of a tightly packed result for [H][W], [H][W][C] or [F][H][W][C] bytes, shaped as Context.resize_tensor shapes
    it: [F][OC][H][W] or [F][H][W][OC] of the table's word, the frame axis dropped with the input's.  src None: the identity."""
    b = np.asarray(bytes_img)
    x = b.reshape(b.shape + (1,)) if b.ndim == 2 else b
    x = x if x.ndim == 4 else x[None]
    f, h, w, c = x.shape
    src = tuple(range(c)) if src is None else tuple(src)
    oc = len(src)
    st = strides(layout, w, h, oc)
    n = extent(w, h, oc, st)
    assert n == oc * h * w
    out = np.zeros(f * n, dtype=words(lut).dtype)
    assert scatter(out, 0, x, lut, src, flips, st, n) == out.size
    out = out.reshape((f, oc, h, w) if layout == "chw" else (f, h, w, oc))
    return out if b.ndim == 4 else out[0]
