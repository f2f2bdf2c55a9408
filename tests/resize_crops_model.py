"""numpy model of a tensor view with a crop origin per frame (include/lanczos_hip.h, lanczos_resize_crops):

    out[f][oc * chan_stride + Y * row_stride + X * pix_stride] = lut[oc * 256 + full[f][y0_f + y][x0_f + x][src[oc]]]
    x0_f = min(max(origin[f][0], 0), out_w - w)        y0_f = min(max(origin[f][1], 0), out_h - h)

`full` [F][out_h][out_w][C] are the bytes of the request WITHOUT a window (Context.resize, a Pillow fixture, the numpy models):
this file clamps the origins and slices; the map, the table, the flips and the strides are resize_tensor_view_model's."""
import numpy as np

import resize_tensor_view_model as V


def clamp(origins, out_w, out_h, w, h):
    """[F][2] origins as the kernels clamp them: the w x h window lies inside the out_w x out_h output"""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    assert 1 <= w <= out_w and 1 <= h <= out_h
    return np.stack([np.clip(o[:, 0], 0, out_w - w), np.clip(o[:, 1], 0, out_h - h)], axis=1)


def slices(full, w, h, origins):
    """[F][h][w][C]: frame f's window of full[f] at its clamped origin"""
    full = np.asarray(full)
    assert full.ndim == 4
    f, oh, ow, _ = full.shape
    o = clamp(origins, ow, oh, w, h)
    assert len(o) == f, "one origin per frame"
    return np.stack([full[k, y0:y0 + h, x0:x0 + w] for k, (x0, y0) in enumerate(o)])


def crops(full, lut, w, h, origins, src=None, flips=None, layout="chw"):
    """the words of a tightly packed result, shaped as Context.resize_tensor(..., crop=(w, h), origins=) shapes it"""
    return V.view(slices(full, w, h, origins), lut, src, flips, layout)


def scatter(out, base, full, lut, w, h, origins, src, flips, st, frame_stride):
    """V.scatter over the frames' windows: writes the words the contract names into `out` in place"""
    return V.scatter(out, base, slices(full, w, h, origins), lut, src, flips, st, frame_stride)
