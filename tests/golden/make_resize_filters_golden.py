"""Writes tests/golden/resize_pillow_filters.npz: what Pillow's Image.resize(size, resample, box, reducing_gap) makes of small
seeded planes with resample in BOX, BILINEAR, HAMMING, BICUBIC and NEAREST, in modes L, RGB, RGBX, RGBA, I;16 and F.

The file holds the outputs only, as one byte stream in an LZMA-compressed zip (numpy.load reads it like any .npz).  The
inputs are rebuilt from their seeds by make_input(); load() checks each against the CRC-32 the file carries.

The generator refuses to write a fixture
  - that the model (tests/resize_filters_model.py) does not reproduce, byte for byte (mode F: bit for bit, NaN positions
    coinciding);
  - on which one of these near misses reproduces Pillow in every case (each must differ in at least one sample of one case):
      double Hamming literals, a symmetric BOX interval, NEAREST by direct multiplication, NEAREST with a premultiply round
      trip on RGBA, a bicubic with a = -0.75.
NEAREST on I;16 is NOT in the fixture: Pillow sends that mode through its generic transform, whose source indices are computed
by direct multiplication.  The generator checks that this is so (Pillow's I;16 output differs from the running-sum gather on
the one-row case "acc" and equals the direct-multiplication gather); the library refuses the combination.
    python tests/golden/make_resize_filters_golden.py
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_filters.npz")

FILTERS = ("box", "bilinear", "hamming", "bicubic", "nearest")
MODES = ("L", "RGB", "RGBX", "RGBA", "I;16", "F")
# name -> (in_w, in_h, out_w, out_h, box, reducing_gap)
SHAPES = {
    "up": (23, 17, 50, 37, None, None),
    "down": (61, 47, 26, 11, None, None),
    "mixed": (19, 41, 47, 13, None, None),                    # up across, down down
    "idle": (30, 26, 30, 9, None, None),                      # the horizontal axis keeps its size
    "box": (40, 32, 17, 19, (5.3, 4.7, 36.1, 28.2), None),    # a sub-pixel box
    "shift": (24, 18, 24, 18, (1.5, 0.75, 24, 18), None),     # equal size, shifted box: both passes run
    "edge": (101, 9, 6, 4, (0.5, 0, 94.5, 9), None),          # a pixel centre on the left edge of a BOX window (x = -0.5)
    "gap": (101, 97, 12, 11, None, 1.5),                      # reducing_gap: weighted filters, 8-bit without alpha
    "row": (2999, 1, 1777, 1, None, None),                    # NEAREST: a long running sum
    "one": (1, 1, 57, 1, None, None),                         # NEAREST: 1 -> N
    "acc": (8, 1, 204, 1, None, None),                        # NEAREST: the running sum and (o + 0.5) * step part ways here
}


def cases():
    """[(filter, mode, shape name)] in file order"""
    out = []
    for f in FILTERS:
        for m in MODES:
            if f == "nearest" and m == "I;16":
                continue
            for s in ("up", "down", "mixed", "idle", "box", "shift", "edge"):
                out.append((f, m, s))
            if f != "nearest" and m in ("L", "RGB"):
                out.append((f, m, "gap"))
            if f == "nearest" and m in ("L", "RGB", "F"):
                out += [(f, m, "row"), (f, m, "one"), (f, m, "acc")]
    return out


def case_name(f, m, s):
    return f"{f}_{m.replace(';', '')}_{s}"


def channels(mode):
    return {"L": 1, "RGB": 3, "RGBX": 4, "RGBA": 4, "I;16": 1, "F": 1}[mode]


def make_input(f, m, s):
    iw, ih = SHAPES[s][:2]
    rng = np.random.default_rng(7100 + 100 * FILTERS.index(f) + 10 * MODES.index(m) + list(SHAPES).index(s))
    if m == "I;16":   # full range: the weighted filters overshoot past 65535 and below 0 at hard edges
        x = rng.integers(0, 65536, (ih, iw)).astype(np.uint16)
        x[rng.random((ih, iw)) < 0.2] = 65535
        x[rng.random((ih, iw)) < 0.2] = 0
        return x
    if m == "F":
        return (rng.random((ih, iw), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
    x = rng.integers(0, 256, (ih, iw, channels(m))).astype(np.uint8)
    if m == "RGBA":   # every kind of alpha: 0, 255 and partial
        a = x[:, :, 3]
        a[rng.random((ih, iw)) < 0.25] = 0
        a[rng.random((ih, iw)) < 0.25] = 255
    return x[:, :, 0] if m == "L" else x


def pillow_resize(img, f, m, s):
    from PIL import Image
    _, _, ow, oh, box, gap = SHAPES[s]
    if m in ("L", "F"):
        im = Image.fromarray(img)
    elif m == "I;16":
        im = Image.frombytes("I;16", (img.shape[1], img.shape[0]), img.astype("<u2").tobytes())
    elif m == "RGBX":
        im = Image.frombuffer("RGBX", (img.shape[1], img.shape[0]), img.tobytes(), "raw", "RGBX", 0, 1)
    else:
        im = Image.fromarray(img, m)
    assert im.mode == m, (im.mode, m)
    r = im.resize((ow, oh), getattr(Image, f.upper()), box=box, reducing_gap=gap)
    assert r.mode == m
    if m == "I;16":
        return np.frombuffer(r.tobytes(), "<u2").astype(np.uint16).reshape(oh, ow)
    if m == "RGBX":
        return np.frombuffer(r.tobytes(), np.uint8).reshape(oh, ow, 4).copy()
    return np.asarray(r).copy()


def load(path=OUT):
    """{case name: (filter, mode, shape name, input, Pillow's output)}"""
    z = np.load(path)
    stream, crc = z["bytes"], z["in_crc"]
    out = {}
    at = 0
    for n, (f, m, s) in enumerate(cases()):
        img = make_input(f, m, s)
        assert zlib.crc32(img.tobytes()) == int(crc[n]), f"{case_name(f, m, s)}: the seeded input changed"
        ow, oh = SHAPES[s][2:4]
        shape = (oh, ow) if img.ndim == 2 else (oh, ow, img.shape[2])
        nbytes = int(np.prod(shape)) * img.dtype.itemsize
        out[case_name(f, m, s)] = (f, m, s, img, stream[at:at + nbytes].view(img.dtype).reshape(shape))
        at += nbytes
    assert at == stream.size
    return out


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import resize_filters_model as FM
    variants = {"hamming_double": dict(hamming_double=True), "box_symmetric": dict(box_symmetric=True),
                "nearest_direct": dict(nearest_direct=True), "nearest_premul": dict(nearest_premul=True),
                "bicubic_a": dict(bicubic_a=-0.75)}
    applies = {"hamming_double": "hamming", "box_symmetric": "box", "nearest_direct": "nearest", "nearest_premul": "nearest",
               "bicubic_a": "bicubic"}
    told = {v: [] for v in variants}
    crcs, outs = [], []
    for f, m, s in cases():
        _, _, ow, oh, box, gap = SHAPES[s]
        img = make_input(f, m, s)
        want = pillow_resize(img, f, m, s)
        crcs.append(zlib.crc32(img.tobytes()))
        outs.append(np.frombuffer(want.tobytes(), np.uint8))
        filt = FM.NAMES.index(f)
        got = FM.resize(img, filt, ow, oh, box, gap, alpha=m == "RGBA")
        assert FM.same(got, want), f"{case_name(f, m, s)}: the model does not reproduce this Pillow build"
        for v, kw in variants.items():
            if applies[v] == f and (v != "nearest_premul" or m == "RGBA"):
                if not FM.same(FM.resize(img, filt, ow, oh, box, gap, alpha=m == "RGBA", **kw), want):
                    told[v].append(case_name(f, m, s))
    for v, names in told.items():
        print(f"{v:16s} differs from Pillow in {len(names)} cases: {' '.join(names[:6])}")
        assert names, f"the fixture does not tell {v} from the contract"
    # NEAREST on I;16: Pillow's generic transform, indices by direct multiplication -- refused by the library, not stored
    img = make_input("nearest", "I;16", "acc")
    want = pillow_resize(img, "nearest", "I;16", "acc")
    assert not FM.same(FM.resize(img, FM.NEAREST, 204, 1), want), "Pillow's I;16 NEAREST is the running-sum gather after all"
    assert FM.same(FM.resize(img, FM.NEAREST, 204, 1, nearest_direct=True), want)
    print("nearest on I;16: Pillow gathers by direct multiplication (differs from the running sum): not in the fixture")
    arrays = {"in_crc": np.array(crcs, np.uint32), "bytes": np.concatenate(outs)}
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_LZMA) as zf:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.save(buf, arr)
            zf.writestr(key + ".npy", buf.getvalue())
    back = load()
    assert all(np.array_equal(np.frombuffer(c[4].tobytes(), np.uint8), o) for c, o in zip(back.values(), outs))
    print(OUT, os.path.getsize(OUT), "bytes,", len(back), "cases")


if __name__ == "__main__":
    main()
