"""Numpy restatement of the resize contract for four channels with straight alpha (LANCZOS_RESIZE_ALPHA: Pillow's
Image.resize with LANCZOS in mode RGBA), on top of resize_model.resize.

Written from the contract in include/lanczos_hip.h / DESIGN.md 4.5, not from the library's C code:
  1. premultiply every input pixel: t = c * A + 128, c' = ((t >> 8) + t) >> 8; alpha unchanged;
  2. the plain resize of the premultiplied four channels (alpha filtered like any other channel);
  3. un-premultiply every output pixel with its resized alpha A: A == 0 or A == 255 keeps the colour samples, otherwise
     c = min(255, 255 * c' // A);
  4. a resize that changes neither axis is a copy of the input (no round trip through 1 and 3).
"""
import numpy as np

import resize_model as M


def premultiply(x):
    """uint8 [..., 4] straight alpha -> premultiplied."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.shape[-1] == 4
    v = x.astype(np.int64)
    t = v[..., :3] * v[..., 3:4] + 128
    out = x.copy()
    out[..., :3] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(x):
    """uint8 [..., 4] premultiplied -> straight alpha."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.shape[-1] == 4
    v = x.astype(np.int64)
    a = v[..., 3:4]
    q = np.minimum(255, (255 * v[..., :3]) // np.maximum(a, 1))
    keep = (a == 0) | (a == 255)
    out = x.copy()
    out[..., :3] = np.where(keep, v[..., :3], q).astype(np.uint8)
    return out


def clamp_hits(img, out_w, out_h, a=3):
    """How many colour samples of the output have c' > A with 0 < A < 255 (the min() of step 3 decides them)."""
    img = np.asarray(img)
    if (img.shape[-2], img.shape[-3]) == (out_w, out_h):
        return 0
    y = M.resize(premultiply(img), out_w, out_h, a).astype(np.int64)
    al = y[..., 3:4]
    return int(((y[..., :3] > al) & (al > 0) & (al < 255)).sum())


def resize(img, out_w, out_h, a=3):
    """img: uint8 [H][W][4] or [F][H][W][4], alpha last -> the resized image(s), same layout."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (3, 4) and img.shape[-1] == 4
    if (img.shape[-2], img.shape[-3]) == (out_w, out_h):
        return img.copy()
    return unpremultiply(M.resize(premultiply(img), out_w, out_h, a))
