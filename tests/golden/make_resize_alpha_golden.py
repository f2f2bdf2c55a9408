"""Writes tests/golden/resize_pillow_alpha.npz: seeded RGBA inputs (straight alpha in the last channel) and what Pillow's
Image.resize(size, Image.LANCZOS) makes of them in mode RGBA.

The GPU tests read this file (Pillow need not be installed where they run); tests/test_resize_alpha_host.py checks that the
numpy model (tests/resize_alpha_model.py) reproduces it and, where Pillow imports, that Pillow still does.
    python tests/golden/make_resize_alpha_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_alpha.npz")

# (name, in_w, in_h, out_w, out_h, alpha kind)
CASES = [
    ("down_noise", 57, 41, 24, 17, "noise"),
    ("down_disc", 64, 48, 32, 24, "disc"),
    ("up_noise", 30, 22, 71, 53, "noise"),
    ("up_disc", 25, 19, 61, 40, "disc"),
    ("mixed_low", 50, 30, 23, 70, "low"),
    ("mixed_extremes", 30, 44, 67, 19, "extremes"),
    ("h_only_noise", 33, 47, 20, 47, "noise"),
    ("v_only_extremes", 47, 33, 47, 20, "extremes"),
    ("identity_noise", 31, 17, 31, 17, "noise"),
    ("to_1x1_noise", 51, 37, 1, 1, "noise"),
    ("large_reduction_low", 120, 90, 5, 4, "low"),
    ("large_reduction_disc", 100, 80, 5, 4, "disc"),
    ("down_opaque", 60, 46, 33, 21, "opaque"),
    ("up_low", 21, 33, 50, 61, "low"),
    ("down_extremes", 64, 50, 43, 33, "extremes"),
    ("one_wide_noise", 1, 5, 9, 17, "noise"),
]


def make_alpha(kind, rng, w, h):
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "low":                       # alpha in 0..3 only
        return rng.integers(0, 4, (h, w), dtype=np.uint8)
    if kind == "extremes":                  # alpha from {0, 1, 254, 255} only
        return np.array([0, 1, 254, 255], np.uint8)[rng.integers(0, 4, (h, w))]
    if kind == "opaque":
        return np.full((h, w), 255, np.uint8)
    if kind == "disc":                      # a soft-edged disc: 255 inside, 0 outside, a ramp a few pixels wide between
        y, x = np.mgrid[0:h, 0:w]
        r = np.hypot(x - (w - 1) / 2, y - (h - 1) / 2)
        edge = 0.35 * min(w, h)
        return np.clip((edge + 2.0 - r) * (255.0 / 4.0), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def make_input(i, w, h, kind):
    """Noise colour (also where alpha is 0: what must not bleed) under the alpha of `kind`."""
    rng = np.random.default_rng(3000 + i)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = make_alpha(kind, rng, w, h)
    return img


def pillow_resize(img, out_w, out_h):
    from PIL import Image
    h, w, _ = img.shape
    im = Image.frombytes("RGBA", (w, h), img.tobytes())
    r = im.resize((out_w, out_h), Image.LANCZOS)
    assert r.mode == "RGBA"
    return np.frombuffer(r.tobytes(), np.uint8).reshape(out_h, out_w, 4)


def main():
    arrays = {}
    for i, (name, iw, ih, ow, oh, kind) in enumerate(CASES):
        img = make_input(i, iw, ih, kind)
        arrays[f"{name}_in"] = img
        arrays[f"{name}_out"] = pillow_resize(img, ow, oh)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
