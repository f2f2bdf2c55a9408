"""Writes tests/golden/resize_pillow.npz: seeded inputs and what Pillow's Image.resize(size, Image.LANCZOS) makes of them.

The GPU tests read this file (Pillow need not be installed where they run); tests/test_resize_host.py checks that the
numpy model (tests/resize_model.py) reproduces it and, where Pillow imports, that Pillow still does.
    python tests/golden/make_resize_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow.npz")

# (name, in_w, in_h, out_w, out_h, mode)
CASES = [
    ("down_L", 97, 61, 40, 23, "L"),
    ("down_RGB", 96, 64, 48, 32, "RGB"),
    ("up_RGBX", 40, 30, 97, 71, "RGBX"),
    ("mixed_RGB", 60, 40, 23, 90, "RGB"),
    ("h_only_L", 33, 77, 20, 77, "L"),
    ("v_only_RGB", 77, 33, 77, 20, "RGB"),
    ("identity_RGB", 31, 17, 31, 17, "RGB"),
    ("to_1x1_RGB", 101, 71, 1, 1, "RGB"),
    ("one_wide_L", 1, 5, 9, 17, "L"),
    ("large_reduction_L", 160, 120, 7, 5, "L"),
    ("down_RGBX", 90, 70, 33, 21, "RGBX"),
    ("up_nonint_RGB", 25, 19, 61, 40, "RGB"),
]
CHANNELS = {"L": 1, "RGB": 3, "RGBX": 4}


def make_input(i, w, h, c):
    rng = np.random.default_rng(1000 + i)
    if i % 3 == 2:   # a smooth gradient with a little noise next to plain noise
        y, x = np.mgrid[0:h, 0:w]
        base = (x * 255 // max(w - 1, 1) + y * 97 // max(h - 1, 1)) % 256
        img = np.clip(base[..., None] + rng.integers(-20, 21, (h, w, c)), 0, 255)
        return img.astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def pillow_resize(img, out_w, out_h, mode):
    from PIL import Image
    h, w, c = img.shape
    im = Image.frombytes(mode, (w, h), img.tobytes())
    r = im.resize((out_w, out_h), Image.LANCZOS)
    return np.frombuffer(r.tobytes(), np.uint8).reshape(out_h, out_w, c)


def main():
    arrays = {}
    for i, (name, iw, ih, ow, oh, mode) in enumerate(CASES):
        img = make_input(i, iw, ih, CHANNELS[mode])
        arrays[f"{name}_in"] = img
        arrays[f"{name}_out"] = pillow_resize(img, ow, oh, mode)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
