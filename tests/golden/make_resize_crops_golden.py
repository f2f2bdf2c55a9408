"""Writes tests/golden/resize_pillow_crops.npz: Image.resize(size, resample, box, reducing_gap).crop(window).transpose(flip) as
Pillow makes it, for five small seeded frames per case, each with a window origin and a flip of its own, in the 8-bit modes L,
RGB, RGBX and RGBA -- what a tensor view with a crop origin per frame (lanczos_resize_crops) has to name byte for byte.

The file holds the cropped and mirrored outputs only (`out_<case>`, [5][h][w] or [5][h][w][C]) and the CRC-32 of every case's
inputs (`in_crc`); inputs, origins and flips are rebuilt from their seeds by make_case().  The generator refuses to write a
fixture
  - that the numpy models (tests/resize_filters_model.py for the full resize, tests/resize_crops_model.py for the slices, numpy's
    own flips) do not reproduce byte for byte;
  - in which a case does not have five pairwise distinct origins, among them (0, 0) and the far corner, and every flip 0 .. 3.
    python tests/golden/make_resize_crops_golden.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_crops.npz")
FRAMES = 5

CHANNELS = {"L": 1, "RGB": 3, "RGBX": 4, "RGBA": 4}
# (name, mode, filter, in_w, in_h, out_w, out_h, box, reducing_gap, crop = (w, h))
CASES = [
    ("L_lanczos", "L", "lanczos", 120, 90, 67, 50, None, None, (40, 30)),
    ("RGB_lanczos", "RGB", "lanczos", 100, 75, 68, 51, None, None, (44, 44)),
    ("RGB_up", "RGB", "lanczos", 40, 31, 90, 61, None, None, (33, 27)),
    ("RGBX_bicubic", "RGBX", "bicubic", 70, 50, 41, 77, None, None, (20, 21)),
    ("RGBA_lanczos", "RGBA", "lanczos", 64, 48, 90, 31, None, None, (30, 17)),
    ("RGBA_bicubic", "RGBA", "bicubic", 50, 61, 37, 43, None, None, (21, 30)),
    ("RGB_fractional_box", "RGB", "lanczos", 110, 80, 56, 43, (7.3, 5.6, 101.2, 77.75), None, (27, 21)),
    ("RGB_gap", "RGB", "lanczos", 400, 300, 50, 38, None, 2.0, (24, 20)),               # reduces by (4, 3)
    ("L_h_only", "L", "lanczos", 97, 41, 55, 41, None, None, (30, 25)),                 # the vertical axis is idle
    ("RGB_v_only", "RGB", "bicubic", 45, 80, 45, 37, None, None, (31, 22)),             # the horizontal axis is idle
    ("RGB_idle", "RGB", "lanczos", 43, 30, 43, 30, None, None, (23, 19)),               # both idle: rows of 129 bytes
    ("RGBA_idle", "RGBA", "lanczos", 40, 30, 40, 30, None, None, (23, 19)),             # both idle: no premultiply round trip
]
FILTERS = ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest")   # resize_filters_model.NAMES


def make_case(index):
    """(inputs [5][ih][iw] or [5][ih][iw][C], origins [5][2] int32, flips [5] uint8) of case `index`"""
    name, mode, _, iw, ih, ow, oh, _, _, (w, h) = CASES[index]
    rng = np.random.default_rng(9700 + index)
    x = rng.integers(0, 256, (FRAMES, ih, iw, CHANNELS[mode])).astype(np.uint8)
    if mode == "RGBA":   # every kind of alpha: 0, 255 and partial
        a = x[..., 3]
        a[rng.random(a.shape) < 0.25] = 0
        a[rng.random(a.shape) < 0.25] = 255
    mx, my = ow - w, oh - h
    origins = np.array([(0, 0), (mx, my), (int(rng.integers(1, mx)), int(rng.integers(1, my))), (mx, 0),
                        (int(rng.integers(1, mx)) | 1, int(rng.integers(1, my)) | 1)], dtype=np.int32)
    flips = np.array([0, 1, 2, 3, 1], dtype=np.uint8)
    return (x[..., 0] if mode == "L" else x), origins, flips


def _to_pillow(img, mode):
    from PIL import Image
    if mode == "L":
        im = Image.fromarray(img)
    elif mode == "RGBX":
        im = Image.frombuffer("RGBX", (img.shape[1], img.shape[0]), img.tobytes(), "raw", "RGBX", 0, 1)
    else:
        im = Image.fromarray(img, mode)
    assert im.mode == mode, (im.mode, mode)
    return im


def _from_pillow(r, mode):
    w, h = r.size
    if mode == "RGBX":
        return np.frombuffer(r.tobytes(), np.uint8).reshape(h, w, 4).copy()
    return np.asarray(r).copy()


def pillow_crops(imgs, origins, flips, case):
    """Image.resize(...).crop(frame's window).transpose(frame's flip), frame by frame"""
    from PIL import Image
    T = Image.Transpose
    how = {0: None, 1: T.FLIP_LEFT_RIGHT, 2: T.FLIP_TOP_BOTTOM, 3: T.ROTATE_180}
    _, mode, filt, _, _, ow, oh, box, gap, (w, h) = case
    out = []
    for img, (x0, y0), m in zip(imgs, origins, flips):
        r = _to_pillow(img, mode).resize((ow, oh), getattr(Image, filt.upper()), box=box, reducing_gap=gap)
        assert r.mode == mode
        r = r.crop((int(x0), int(y0), int(x0) + w, int(y0) + h))
        if how[int(m)] is not None:
            r = r.transpose(how[int(m)])
        out.append(_from_pillow(r, mode))
    return np.stack(out)


def model_full(imgs, case):
    """the numpy models' resize of every frame WITHOUT a window: [5][oh][ow][C]"""
    sys.path.insert(0, os.path.dirname(HERE))
    import resize_filters_model as FM
    _, mode, filt, _, _, ow, oh, box, gap, _ = case
    full = np.stack([FM.resize(img, FILTERS.index(filt), ow, oh, box, gap, alpha=mode == "RGBA") for img in imgs])
    return full[..., None] if full.ndim == 3 else full


def model_crops(imgs, origins, flips, case):
    """the models' full resize, sliced per frame (resize_crops_model) and mirrored with numpy"""
    sys.path.insert(0, os.path.dirname(HERE))
    import resize_crops_model as RC
    w, h = case[9]
    cut = RC.slices(model_full(imgs, case), w, h, origins)
    out = np.stack([fr[::-1 if m & 2 else 1, ::-1 if m & 1 else 1] for fr, m in zip(cut, flips)])
    return out[..., 0] if imgs.ndim == 3 else out


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def load(path=OUT):
    """{case name: (case, inputs, origins, flips, Pillow's cropped and mirrored outputs)}"""
    z = np.load(path)
    crc = z["in_crc"]
    out = {}
    for i, case in enumerate(CASES):
        imgs, origins, flips = make_case(i)
        assert zlib.crc32(imgs.tobytes() + origins.tobytes() + flips.tobytes()) == int(crc[i]), f"{case[0]}: the seeded case changed"
        out[case[0]] = (case, imgs, origins, flips, z[f"out_{case[0]}"])
    assert len(z.files) == len(CASES) + 1
    return out


def main():
    arrays, crcs = {}, []
    for i, case in enumerate(CASES):
        imgs, origins, flips = make_case(i)
        (w, h), (ow, oh) = case[9], case[5:7]
        assert len({tuple(o) for o in origins.tolist()}) == FRAMES, case[0]
        assert [0, 0] in origins.tolist() and [ow - w, oh - h] in origins.tolist() and set(flips.tolist()) == {0, 1, 2, 3}
        want = pillow_crops(imgs, origins, flips, case)
        assert want.shape[:3] == (FRAMES, h, w), case[0]
        assert same(model_crops(imgs, origins, flips, case), want), f"{case[0]}: the models do not reproduce this Pillow build"
        crcs.append(zlib.crc32(imgs.tobytes() + origins.tobytes() + flips.tobytes()))
        arrays[f"out_{case[0]}"] = want
    np.savez_compressed(OUT, in_crc=np.array(crcs, np.uint32), **arrays)
    back = load()
    assert all(same(back[c[0]][4], arrays[f"out_{c[0]}"]) for c in CASES)
    print(OUT, os.path.getsize(OUT), "bytes,", len(back), "cases")


if __name__ == "__main__":
    main()
