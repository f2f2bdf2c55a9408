"""Writes tests/golden/resize_pillow_u16.npz: seeded 16-bit planes and what Pillow's Image.resize(size, Image.LANCZOS)
makes of them in mode I;16 (Image.fromarray of a 2-D uint16 array).

To stay no larger than resize_pillow.npz the file holds the outputs only, all high bytes and all low bytes as two
arrays in an LZMA-compressed zip (numpy.load reads it like any .npz).  The inputs are not stored: make_input() rebuilds
them from their seeds and load() checks each against the CRC-32 the file carries.

Pillow has single-channel I;16 only; the tests build 3- and 4-channel frames by stacking these planes, every channel
being resized as an independent I;16 plane.  The fixture has to exercise Pillow's store (a sum above 65535 keeps its low
byte under a high byte of 255, a negative sum stores 0): the generator refuses to write a fixture on which a saturating
store would give nearly the same bytes.
    python tests/golden/make_resize16_golden.py
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_u16.npz")

# (in_w, in_h, out_w, out_h)
SHAPES = [
    (64, 48, 31, 17),
    (64, 48, 128, 96),
    (97, 53, 33, 200),
    (50, 40, 50, 13),
    (50, 40, 7, 40),
    (200, 120, 9, 5),
    (33, 21, 100, 77),
]
PATTERNS = ["noise", "bilevel", "blocks", "gradient"]


def case_name(si, pattern):
    return f"s{si}_{pattern}"


def make_input(si, pattern, w, h):
    rng = np.random.default_rng(7000 + 10 * si + PATTERNS.index(pattern))
    if pattern == "noise":
        return rng.integers(0, 65536, (h, w), dtype=np.uint16)
    if pattern == "bilevel":
        return (rng.integers(0, 2, (h, w)) * 65535).astype(np.uint16)
    if pattern == "blocks":   # 0 / 65535 blocks, 5 wide and 3 high
        by, bx = (h + 2) // 3, (w + 4) // 5
        b = rng.integers(0, 2, (by, bx))
        return (np.repeat(np.repeat(b, 3, axis=0), 5, axis=1)[:h, :w] * 65535).astype(np.uint16)
    y, x = np.mgrid[0:h, 0:w]   # a gradient that wraps several times over the frame
    return ((x * 4099 + y * 2053) % 65536).astype(np.uint16)


def pillow_resize(plane, out_w, out_h):
    from PIL import Image
    im = Image.fromarray(plane)
    assert im.mode == "I;16", im.mode
    r = im.resize((out_w, out_h), Image.LANCZOS)
    return np.asarray(r).astype(np.uint16).reshape(out_h, out_w)


def load(path=OUT):
    """{case name: (input plane, Pillow's output plane)}, both uint16."""
    z = np.load(path)
    flat = z["out_lo"].astype(np.uint16) | (z["out_hi"].astype(np.uint16) << 8)   # every case's output, in case order
    crc = z["in_crc"]
    cases = {}
    at = 0
    for si, (iw, ih, ow, oh) in enumerate(SHAPES):
        for pattern in PATTERNS:
            name = case_name(si, pattern)
            img = make_input(si, pattern, iw, ih)
            assert zlib.crc32(img.tobytes()) == int(crc[len(cases)]), f"{name}: the seeded input changed"
            cases[name] = (img, flat[at:at + ow * oh].reshape(oh, ow))
            at += ow * oh
    assert at == flat.size
    return cases


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import resize16_model as M
    crcs, outs = [], []
    total = diff_model = diff_sat = 0
    stats = {}
    for si, (iw, ih, ow, oh) in enumerate(SHAPES):
        for pattern in PATTERNS:
            img = make_input(si, pattern, iw, ih)
            want = pillow_resize(img, ow, oh)
            crcs.append(zlib.crc32(img.tobytes()))
            outs.append(want.reshape(-1))
            total += want.size
            diff_model += int((M.resize(img, ow, oh, 3, stats=stats) != want).sum())
            diff_sat += int((M.resize(img, ow, oh, 3, saturate=True) != want).sum())
    print(f"samples {total}: model differs in {diff_model}, saturating variant in {diff_sat} "
          f"({100.0 * diff_sat / total:.1f} %), pre-store range {stats['vmin']} .. {stats['vmax']}")
    assert diff_model == 0, "the model does not reproduce this Pillow build"
    assert diff_sat >= total // 10, "the fixture does not exercise the wrap of the store"
    assert stats["vmin"] < 0 and stats["vmax"] > 65535, "no negative / no overflowing pre-store value in the fixture"
    flat = np.concatenate(outs)
    arrays = {"in_crc": np.array(crcs, np.uint32), "out_hi": (flat >> 8).astype(np.uint8),
              "out_lo": (flat & 255).astype(np.uint8)}
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_LZMA) as zf:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.save(buf, arr)
            zf.writestr(key + ".npy", buf.getvalue())
    assert all(np.array_equal(c[1].reshape(-1), o) for c, o in zip(load().values(), outs))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
