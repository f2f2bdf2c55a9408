"""Writes tests/golden/resize_pillow_box.npz: seeded inputs and what Pillow makes of them with a source box, with
Image.reduce, and with reducing_gap:

    Image.resize(size, Image.LANCZOS, box=box)                    L / RGB / RGBX / RGBA (straight alpha) / I;16
    Image.reduce((fx, fy), box=box)                               L / RGB / RGBX
    Image.resize(size, Image.LANCZOS, box=box, reducing_gap=g)    L / RGB / RGBX

The GPU tests read this file (Pillow need not be installed where they run); tests/test_resize_box_host.py checks that the
numpy model (tests/resize_box_model.py) reproduces it and, where Pillow imports, that Pillow still does.  The inputs are
regenerated from their seeds by make_input and not stored (a test checks one stored input against it).

The generator refuses to write a fixture that cannot tell the contract from its near misses (check_discrimination).
    python tests/golden/make_resize_box_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_box.npz")
sys.path.insert(0, os.path.dirname(HERE))

CHANNELS = {"L": 1, "RGB": 3, "RGBX": 4, "RGBA": 4, "I;16": 1}

# (name, in_w, in_h, out_w, out_h, mode, box)
BOX_CASES = [
    ("int_down_RGB", 97, 61, 20, 13, "RGB", (10, 5, 80, 50)),
    ("frac_up_RGB", 60, 40, 120, 90, "RGB", (10.3, 5.7, 40.1, 25.9)),      # the float32 box is live here
    ("frac_up_RGBX", 60, 40, 120, 90, "RGBX", (10.3, 5.7, 40.1, 25.9)),
    ("frac_down_L", 97, 61, 17, 11, "L", (3.25, 2.5, 90.75, 58.125)),
    ("mixed_RGBX", 60, 40, 11, 70, "RGBX", (5.5, 10.25, 55.5, 30.75)),
    ("h_only_L", 64, 33, 20, 33, "L", (7.5, 0, 50.25, 33)),
    ("v_only_RGB", 33, 64, 33, 20, "RGB", (0, 7.5, 33, 50.25)),
    ("shift_equal_size_RGB", 40, 30, 40, 30, "RGB", (0.5, 0.25, 40, 30)),
    ("shift_h_only_L", 40, 30, 40, 30, "L", (0.3, 0, 40, 30)),
    ("touch_left_top_RGB", 50, 40, 25, 30, "RGB", (0, 0, 30.5, 20.5)),
    ("touch_right_bottom_L", 50, 40, 25, 30, "L", (20.5, 10.5, 50, 40)),
    ("full_box_RGB", 50, 40, 20, 15, "RGB", (0, 0, 50, 40)),
    ("tiny_box_up_L", 50, 40, 31, 29, "L", (20.2, 20.4, 23.7, 22.9)),
    ("large_reduction_RGB", 160, 120, 5, 4, "RGB", (8.5, 4.5, 150.5, 115.5)),
    ("alpha_frac_down", 64, 48, 20, 15, "RGBA", (4.25, 3.5, 60.75, 44.5)),
    ("alpha_frac_up", 30, 20, 50, 40, "RGBA", (5.3, 2.7, 20.1, 15.9)),
    ("alpha_shift", 30, 20, 30, 20, "RGBA", (0.5, 0.5, 30, 20)),
    ("alpha_v_only", 30, 40, 30, 13, "RGBA", (0, 3.5, 30, 33.25)),
    ("u16_frac_down", 64, 48, 20, 15, "I;16", (4.25, 3.5, 60.75, 44.5)),
    ("u16_frac_up", 30, 20, 50, 40, "I;16", (5.3, 2.7, 20.1, 15.9)),
    ("u16_shift", 30, 20, 30, 20, "I;16", (0.5, 0.5, 30, 20)),
    ("u16_h_only", 40, 20, 17, 20, "I;16", (3.5, 0, 33.25, 20)),
]

# (name, in_w, in_h, mode, (fx, fy), box or None)
REDUCE_CASES = [
    ("sq2_RGB", 64, 48, "RGB", (2, 2), None),
    ("sq3_ragged_L", 65, 49, "L", (3, 3), None),
    ("sq5_ragged_RGBX", 63, 47, "RGBX", (5, 5), None),
    ("7x5_ragged_RGB", 100, 73, "RGB", (7, 5), None),
    ("12x12_RGB", 130, 121, "RGB", (12, 12), None),
    ("1x4_L", 40, 50, "L", (1, 4), None),
    ("3x1_RGB", 50, 40, "RGB", (3, 1), None),
    ("1x7_ragged_RGBX", 20, 45, "RGBX", (1, 7), None),
    ("6x1_ragged_L", 45, 20, "L", (6, 1), None),
    ("box_4x3_RGB", 90, 70, "RGB", (4, 3), (5, 7, 86, 66)),
    ("box_ragged_both_L", 90, 70, "L", (8, 6), (3, 2, 88, 69)),
    ("box_16x9_RGBX", 200, 100, "RGBX", (16, 9), (11, 5, 197, 98)),
    ("bigger_than_box_RGB", 40, 30, "RGB", (50, 40), (2, 3, 39, 28)),
    ("1x1_box_L", 40, 30, "L", (1, 1), (5, 6, 30, 20)),
    ("30x20_L", 200, 150, "L", (30, 20), None),
    ("bilevel_3x3_RGB", 64, 50, "RGB", (3, 3), None),
    ("bilevel_7x2_L", 64, 50, "L", (7, 2), (1, 1, 63, 50)),
]

# (name, in_w, in_h, out_w, out_h, mode, box or None, gap)
GAP_CASES = [
    ("g1.0_RGB", 200, 150, 20, 15, "RGB", None, 1.0),
    ("g1.1_L", 200, 150, 21, 16, "L", None, 1.1),
    ("g2.0_RGB", 200, 150, 20, 15, "RGB", None, 2.0),
    ("g3.0_RGBX", 200, 150, 13, 11, "RGBX", None, 3.0),
    ("g2.0_nondividing_L", 211, 157, 17, 9, "L", None, 2.0),
    ("g1.0_box_RGB", 200, 150, 12, 10, "RGB", (20.5, 10.25, 180.75, 140.5), 1.0),
    ("g2.0_box_RGBX", 200, 150, 12, 10, "RGBX", (20.5, 10.25, 180.75, 140.5), 2.0),
    ("g3.0_box_L", 240, 200, 9, 8, "L", (3.3, 7.7, 230.1, 190.9), 3.0),
    ("g1.1_box_int_RGB", 200, 150, 16, 12, "RGB", (8, 6, 190, 140), 1.1),
    ("g2.0_fx_only_L", 240, 60, 20, 25, "L", None, 2.0),            # fx = 6, fy = 1
    ("g2.0_fy_only_RGB", 60, 240, 25, 20, "RGB", None, 2.0),        # fx = 1, fy = 6
    ("g1.0_fx_only_box_RGB", 240, 60, 20, 40, "RGB", (2.5, 1.5, 236.5, 58.5), 1.0),
]


def make_input(kind, i, w, h, mode):
    """Seeded input of case i of list `kind` (0 box, 1 reduce, 2 gap): [h][w][c] uint8, or [h][w] uint16 for I;16."""
    rng = np.random.default_rng(7000 + 100 * kind + i)
    c = CHANNELS[mode]
    if mode == "I;16":
        return rng.integers(0, 65536, (h, w), dtype=np.uint16)
    if kind == 1 and "bilevel" in REDUCE_CASES[i][0]:   # 0 / 255 in runs: every rounding at its extreme
        return (rng.integers(0, 2, (h, w, c), dtype=np.uint8) * 255).astype(np.uint8)
    if i % 3 == 2:   # a smooth gradient with a little noise next to plain noise
        y, x = np.mgrid[0:h, 0:w]
        base = (x * 255 // max(w - 1, 1) + y * 97 // max(h - 1, 1)) % 256
        return np.clip(base[..., None] + rng.integers(-20, 21, (h, w, c)), 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def _image(img, mode):
    from PIL import Image
    if mode == "I;16":
        h, w = img.shape
        return Image.frombytes("I;16", (w, h), img.astype("<u2").tobytes())
    h, w, _ = img.shape
    return Image.frombytes(mode, (w, h), img.tobytes())


def _array(r, mode):
    w, h = r.size
    if mode == "I;16":
        return np.frombuffer(r.tobytes(), "<u2").reshape(h, w).astype(np.uint16)
    return np.frombuffer(r.tobytes(), np.uint8).reshape(h, w, CHANNELS[mode])


def pillow_resize(img, out_w, out_h, mode, box=None, gap=None):
    from PIL import Image
    return _array(_image(img, mode).resize((out_w, out_h), Image.LANCZOS, box=box, reducing_gap=gap), mode)


def pillow_reduce(img, mode, factor, box=None):
    return _array(_image(img, mode).reduce(factor, box=box), mode)


def check_discrimination(arrays):
    """The near misses must be visible in the fixture: a double box, a ragged edge divided by fx * fy, a dropped gap."""
    import resize_box_model as BM
    double_box = 0
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(BOX_CASES):
        if mode in ("RGBA", "I;16"):
            continue
        img = make_input(0, i, iw, ih, mode)
        double_box += not np.array_equal(BM.resize_box(img, ow, oh, box, float_box=False), arrays[f"box_{name}"])
    if not double_box:
        raise SystemExit("refusing to write: no box case tells float32 boxes from double ones")
    ragged = 0
    for i, (name, iw, ih, mode, factor, box) in enumerate(REDUCE_CASES):
        img = make_input(1, i, iw, ih, mode)
        ragged += not np.array_equal(BM.reduce(img, factor, box, own_divisor=False), arrays[f"reduce_{name}"])
    if not ragged:
        raise SystemExit("refusing to write: no reduce case tells a ragged edge's own divisor from fx * fy")
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(GAP_CASES):
        img = make_input(2, i, iw, ih, mode)
        if np.array_equal(pillow_resize(img, ow, oh, mode, box, None), arrays[f"gap_{name}"]):
            raise SystemExit(f"refusing to write: gapped case {name} equals its ungapped resize")
    return double_box, ragged


def main():
    arrays = {}
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(BOX_CASES):
        arrays[f"box_{name}"] = pillow_resize(make_input(0, i, iw, ih, mode), ow, oh, mode, box)
    for i, (name, iw, ih, mode, factor, box) in enumerate(REDUCE_CASES):
        arrays[f"reduce_{name}"] = pillow_reduce(make_input(1, i, iw, ih, mode), mode, factor, box)
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(GAP_CASES):
        arrays[f"gap_{name}"] = pillow_resize(make_input(2, i, iw, ih, mode), ow, oh, mode, box, gap)
    arrays["input_check"] = make_input(0, 0, *BOX_CASES[0][1:3], BOX_CASES[0][5])   # pins the seeded generator
    n_box, n_ragged = check_discrimination(arrays)
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", n_box, "box case(s) tell float32 from double boxes,", n_ragged,
          "reduce case(s) tell own divisors from fx * fy")


if __name__ == "__main__":
    main()
