"""Writes tests/golden/resize_pillow_window.npz: Image.resize(size, resample, box, reducing_gap).crop(window) as Pillow makes
it, for small seeded frames in modes L, RGB, RGBX, RGBA, I;16 and F -- what a resize with a window of the output
(lanczos_resize_window) has to reproduce byte for byte.

The file holds the cropped outputs only (`out_<case>`) and the CRC-32 of every input (`in_crc`); the inputs are rebuilt from
their seeds by make_input().  The generator refuses to write a fixture
  - that the numpy models (tests/resize_filters_model.py and the models it stands on), sliced to the window, do not
    reproduce -- byte for byte, mode F bit for bit;
  - none of whose cases tells the window from the source box over "the same region" (Image.resize(window's size, box = the
    window scaled back to the source)): the two differ, which is why the window exists.

The recipe lives beside its siblings (tests/golden/make_resize_*_golden.py); tests/resize_window_model.py is the model of a
window of the SOURCE and has no part in it.
    python tests/golden/make_resize_window_golden.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_window.npz")

CHANNELS = {"L": 1, "RGB": 3, "RGBX": 4, "RGBA": 4, "I;16": 1, "F": 1}
# (name, mode, filter, in_w, in_h, out_w, out_h, box, reducing_gap, window = (x0, y0, w, h))
CASES = [
    ("L_down", "L", "lanczos", 120, 90, 67, 50, None, None, (10, 7, 40, 30)),
    ("RGB_up", "RGB", "lanczos", 60, 45, 150, 100, None, None, (37, 21, 25, 19)),
    ("RGB_center", "RGB", "lanczos", 100, 75, 68, 51, None, None, (12, 4, 44, 44)),          # CenterCrop(44): the tie 3.5 rounds to 4
    ("RGBX_bicubic", "RGBX", "bicubic", 70, 50, 41, 77, None, None, (5, 30, 20, 21)),
    ("RGBA_lanczos", "RGBA", "lanczos", 64, 48, 90, 31, None, None, (33, 3, 30, 17)),
    ("I16_lanczos", "I;16", "lanczos", 80, 60, 47, 95, None, None, (9, 40, 31, 33)),
    ("F_lanczos", "F", "lanczos", 75, 55, 120, 33, None, None, (60, 6, 35, 20)),
    ("RGB_box_edges", "RGB", "box", 90, 70, 37, 29, None, None, (20, 12, 17, 17)),            # the right and bottom edges
    ("RGB_nearest", "RGB", "nearest", 83, 61, 131, 40, None, None, (0, 11, 31, 23)),           # the left edge
    ("F_nearest", "F", "nearest", 50, 40, 23, 67, None, None, (7, 0, 16, 40)),                 # the top edge
    ("RGB_fractional_box", "RGB", "lanczos", 110, 80, 56, 43, (7.3, 5.6, 101.2, 77.75), None, (19, 11, 27, 21)),
    ("RGB_gap", "RGB", "lanczos", 400, 300, 50, 38, None, 2.0, (13, 9, 24, 20)),               # reduces by (4, 3)
    ("L_h_only", "L", "lanczos", 97, 41, 55, 41, None, None, (20, 10, 30, 25)),               # the vertical axis is idle
    ("RGBA_idle", "RGBA", "lanczos", 40, 30, 40, 30, None, None, (11, 5, 23, 19)),            # both idle: the crop copy
    ("L_one", "L", "hamming", 33, 27, 71, 19, None, None, (35, 9, 1, 1)),
]
FILTERS = ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest")   # resize_filters_model.NAMES


def make_input(index):
    name, mode, _, iw, ih = CASES[index][:5]
    rng = np.random.default_rng(9300 + index)
    if mode == "I;16":   # full range with hard edges: the filter overshoots past 65535 and below 0
        x = rng.integers(0, 65536, (ih, iw)).astype(np.uint16)
        x[rng.random((ih, iw)) < 0.2] = 65535
        x[rng.random((ih, iw)) < 0.2] = 0
        return x
    if mode == "F":
        return (rng.random((ih, iw), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
    x = rng.integers(0, 256, (ih, iw, CHANNELS[mode])).astype(np.uint8)
    if mode == "RGBA":   # every kind of alpha: 0, 255 and partial
        a = x[:, :, 3]
        a[rng.random((ih, iw)) < 0.25] = 0
        a[rng.random((ih, iw)) < 0.25] = 255
    return x[:, :, 0] if mode == "L" else x


def _to_pillow(img, mode):
    from PIL import Image
    if mode in ("L", "F"):
        im = Image.fromarray(img)
    elif mode == "I;16":
        im = Image.frombytes("I;16", (img.shape[1], img.shape[0]), img.astype("<u2").tobytes())
    elif mode == "RGBX":
        im = Image.frombuffer("RGBX", (img.shape[1], img.shape[0]), img.tobytes(), "raw", "RGBX", 0, 1)
    else:
        im = Image.fromarray(img, mode)
    assert im.mode == mode, (im.mode, mode)
    return im


def _from_pillow(r, mode):
    w, h = r.size
    if mode == "I;16":
        return np.frombuffer(r.tobytes(), "<u2").astype(np.uint16).reshape(h, w)
    if mode == "RGBX":
        return np.frombuffer(r.tobytes(), np.uint8).reshape(h, w, 4).copy()
    return np.asarray(r).copy()


def pillow_resize_crop(img, case):
    """Image.resize(...).crop(window) of one case"""
    from PIL import Image
    _, mode, filt, _, _, ow, oh, box, gap, (x0, y0, w, h) = case
    r = _to_pillow(img, mode).resize((ow, oh), getattr(Image, filt.upper()), box=box, reducing_gap=gap)
    assert r.mode == mode
    return _from_pillow(r.crop((x0, y0, x0 + w, y0 + h)), mode)


def pillow_box_instead(img, case):
    """the near miss: the window given as a source box of a resize to the window's size"""
    from PIL import Image
    _, mode, filt, iw, ih, ow, oh, box, gap, (x0, y0, w, h) = case
    bx0, by0, bx1, by1 = box if box is not None else (0, 0, iw, ih)
    sx, sy = (bx1 - bx0) / ow, (by1 - by0) / oh
    sub = (bx0 + x0 * sx, by0 + y0 * sy, bx0 + (x0 + w) * sx, by0 + (y0 + h) * sy)
    return _from_pillow(_to_pillow(img, mode).resize((w, h), getattr(Image, filt.upper()), box=sub), mode)


def model_resize_crop(img, case):
    """the numpy models' full resize, sliced to the window"""
    sys.path.insert(0, os.path.dirname(HERE))
    import resize_filters_model as FM
    _, mode, filt, _, _, ow, oh, box, gap, (x0, y0, w, h) = case
    full = FM.resize(img, FILTERS.index(filt), ow, oh, box, gap, alpha=mode == "RGBA")
    return full[y0:y0 + h, x0:x0 + w]


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    return np.array_equal(np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8))


def load(path=OUT):
    """{case name: (case, input, Pillow's cropped output)}"""
    z = np.load(path)
    crc = z["in_crc"]
    out = {}
    for i, case in enumerate(CASES):
        img = make_input(i)
        assert zlib.crc32(img.tobytes()) == int(crc[i]), f"{case[0]}: the seeded input changed"
        out[case[0]] = (case, img, z[f"out_{case[0]}"])
    assert len(z.files) == len(CASES) + 1
    return out


def main():
    arrays, crcs, told = {}, [], []
    for i, case in enumerate(CASES):
        img = make_input(i)
        want = pillow_resize_crop(img, case)
        x0, y0, w, h = case[9]
        assert want.shape[:2] == (h, w), case[0]
        assert same(model_resize_crop(img, case), want), f"{case[0]}: the sliced model does not reproduce this Pillow build"
        if case[8] is None and case[2] != "nearest" and case[5:7] != case[3:5]:
            if not same(pillow_box_instead(img, case), want):
                told.append(case[0])
        crcs.append(zlib.crc32(img.tobytes()))
        arrays[f"out_{case[0]}"] = want
    print("a source box over the same region differs from the crop in", len(told), "cases:", " ".join(told))
    assert told, "the fixture does not tell the window from a source box"
    np.savez_compressed(OUT, in_crc=np.array(crcs, np.uint32), **arrays)
    back = load()
    assert all(same(back[c[0]][2], arrays[f"out_{c[0]}"]) for c in CASES)
    print(OUT, os.path.getsize(OUT), "bytes,", len(back), "cases")


if __name__ == "__main__":
    main()
