"""Writes tests/golden/resize_pillow_tall.npz: what Pillow's Image.resize(size, resample, box, reducing_gap) makes of frames
on either side of its order rule.  Image.resize runs the vertical pass first, over the full width, and the horizontal pass
second when the frame it resizes (the reduced one under a reducing_gap) has height > 100 * width and shrinks in height; the
intermediate is stored in the image's mode.  Every other frame runs horizontal first.

  ordinary tall   widths 2..6, heights up to 700; every mode with the five weighted filters, NEAREST on L, RGBA and F; each
                  with no box, a fractional box and a whole-pixel box.  (A frame one pixel wide has an exact horizontal pass:
                  its order cannot be observed, so it is among the one-axis cases below.)
  boundaries      pairs on either side of an edge of the rule: height == 100 * width and + 1; out_h == in_h - 1, in_h (with
                  a shifted box, so that the pass runs) and in_h + 1; tall frames whose width stays (one pass: order is moot);
                  reducing_gap on L and RGB that moves the frame into the rule, out of it, keeps it inside, and reduces nothing.

The file holds the outputs only, as one byte stream in an LZMA-compressed zip (numpy.load reads it like any .npz).  The
inputs are rebuilt from their seeds by make_input(); load() checks each against the CRC-32 the file carries.

The generator refuses to write a fixture
  - that the model (tests/resize_filters_model.py) does not reproduce, byte for byte (mode F: bit for bit);
  - in which a tall case with a weighted filter whose two passes both run is also reproduced by the model with
    order="h_first": every such case has to tell the two orders apart.
    python tests/golden/make_resize_tall_golden.py
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_tall.npz")
PILLOW = "12.2.0"

FILTERS = ("lanczos", "box", "bilinear", "hamming", "bicubic", "nearest")
MODES = ("L", "RGB", "RGBX", "RGBA", "I;16", "F")


def channels(mode):
    return {"L": 1, "RGB": 3, "RGBX": 4, "RGBA": 4, "I;16": 1, "F": 1}[mode]


def vertical_first(in_w, in_h, out_h):
    return in_h > 100 * in_w and out_h < in_h


def _ordinary():
    """{name: (filter, mode, in_w, in_h, out_w, out_h, box, gap)}"""
    out = {}
    n = 0
    for f in FILTERS:
        for m in MODES:
            if f == "nearest" and m not in ("L", "RGBA", "F"):
                continue
            iw = 2 + n % 5
            ih = 100 * iw + 1 + (n * 37) % 90
            if f == "box":   # a BOX upscale copies single pixels, exactly: only a downscale across mixes samples
                iw, ih = 5 + n % 2, 100 * (5 + n % 2) + 1 + (n * 37) % 90
            ow = iw - 2 if (f == "box" or (iw >= 4 and n % 2)) else iw + 3 + n % 7
            oh = 23 + (n * 11) % 50
            boxes = {"full": None, "frac": (0.25, 3.5, iw - 0.5, ih - 7.25), "whole": (1 if iw >= 3 else 0, 5, iw, ih - 9)}
            for b, box in boxes.items():
                out[f"{f}_{m.replace(';', '')}_{b}"] = (f, m, iw, ih, ow, oh, box, None)
            n += 1
    return out


# name -> (in_w, in_h, out_w, out_h, box, gap); the first word of a name says which edge, the rest which side
EDGES = {
    "h100_at": (3, 300, 7, 40, None, None),              # in_h == 100 * in_w: horizontal first
    "h100_over": (3, 301, 7, 40, None, None),            # one more row: vertical first
    "shrink_by1": (3, 400, 7, 399, None, None),          # out_h == in_h - 1: vertical first
    "shrink_by0": (3, 400, 7, 400, (0, 0.5, 3, 400), None),   # out_h == in_h (a shifted box runs the pass): horizontal first
    "shrink_grow": (3, 400, 7, 401, None, None),         # out_h > in_h: horizontal first
    "onepass_w4": (4, 500, 4, 60, None, None),           # tall, the width stays: the vertical pass alone
    "onepass_w1": (1, 300, 1, 50, (0, 2.25, 1, 290.5), None),
}
GAPS = {
    "gap_into": (13, 700, 2, 500, None, 1.0),            # 13 x 700 is not tall; reduced by (6, 1) to 3 x 700 it is
    "gap_outof": (5, 700, 7, 9, None, 1.0),              # 5 x 700 is tall; reduced by (1, 77) to 5 x 10 it is not
    "gap_stays": (2, 690, 3, 100, None, 2.0),            # reduced by (1, 3) to 2 x 230: still tall
    "gap_unit": (3, 400, 5, 300, (0.5, 1.5, 3, 397.25), 3.0),   # fx = fy = 1: nothing is reduced, tall
}


def all_cases():
    """{name: (filter, mode, in_w, in_h, out_w, out_h, box, gap)} in file order"""
    out = _ordinary()
    for s, shape in EDGES.items():
        for f in ("lanczos", "bilinear"):
            for m in ("L", "RGBA", "I;16", "F"):
                out[f"{s}_{f}_{m.replace(';', '')}"] = (f, m) + shape
    for s, shape in GAPS.items():
        for f in ("lanczos", "bicubic"):
            for m in ("L", "RGB"):
                out[f"{s}_{f}_{m}"] = (f, m) + shape
    return out


def make_plane(rng, mode, w, h):
    """a seeded frame as the filter fixture's generator builds them: full-range I;16 with forced 0 and 65535, every kind of
    alpha, F in [-1, 3)"""
    if mode == "I;16":
        x = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        x[rng.random((h, w)) < 0.2] = 65535
        x[rng.random((h, w)) < 0.2] = 0
        return x
    if mode == "F":
        return (rng.random((h, w), dtype=np.float32) * np.float32(4.0) - np.float32(1.0)).astype(np.float32)
    x = rng.integers(0, 256, (h, w, channels(mode))).astype(np.uint8)
    if mode == "RGBA":
        a = x[:, :, 3]
        a[rng.random((h, w)) < 0.25] = 0
        a[rng.random((h, w)) < 0.25] = 255
    return x[:, :, 0] if mode == "L" else x


def make_input(name):
    _, m, iw, ih = all_cases()[name][:4]
    return make_plane(np.random.default_rng(zlib.crc32(name.encode())), m, iw, ih)


def pillow_resize(img, mode, filt, ow, oh, box=None, gap=None):
    from PIL import Image
    if mode in ("L", "F"):
        im = Image.fromarray(img)
    elif mode == "I;16":
        im = Image.frombytes("I;16", (img.shape[1], img.shape[0]), img.astype("<u2").tobytes())
    elif mode == "RGBX":
        im = Image.frombuffer("RGBX", (img.shape[1], img.shape[0]), img.tobytes(), "raw", "RGBX", 0, 1)
    else:
        im = Image.frombuffer(mode, (img.shape[1], img.shape[0]), img.tobytes(), "raw", mode, 0, 1)
    assert im.mode == mode, (im.mode, mode)
    r = im.resize((ow, oh), getattr(Image, filt.upper()), box=box, reducing_gap=gap)
    assert r.mode == mode and r.size == (ow, oh)
    if mode == "I;16":
        return np.frombuffer(r.tobytes(), "<u2").astype(np.uint16).reshape(oh, ow)
    if mode == "L":
        return np.frombuffer(r.tobytes(), np.uint8).reshape(oh, ow).copy()
    if mode == "F":
        return np.asarray(r).copy()
    return np.frombuffer(r.tobytes(), np.uint8).reshape(oh, ow, channels(mode)).copy()


def load(path=OUT):
    """{case name: (filter, mode, in_w, in_h, out_w, out_h, box, gap, input, Pillow's output)}"""
    z = np.load(path)
    stream, crc = z["bytes"], z["in_crc"]
    out = {}
    at = 0
    for n, (name, case) in enumerate(all_cases().items()):
        f, m, iw, ih, ow, oh, box, gap = case
        img = make_input(name)
        assert zlib.crc32(img.tobytes()) == int(crc[n]), f"{name}: the seeded input changed"
        shape = (oh, ow) if img.ndim == 2 else (oh, ow, img.shape[2])
        nbytes = int(np.prod(shape)) * img.dtype.itemsize
        out[name] = case + (img, stream[at:at + nbytes].view(img.dtype).reshape(shape))
        at += nbytes
    assert at == stream.size
    return out


def reduced_size(FM, case):
    """the size of the frame the resize reads: the request's, or the reduced one under a gap that reduces"""
    f, m, iw, ih, ow, oh, box, gap = case
    if gap is None:
        return iw, ih
    return FM.gap_plan(FM.NAMES.index(f), iw, ih, ow, oh, box, gap)[3]


def axes_run(MB, FM, case):
    """(the horizontal pass runs, the vertical pass runs) on the frame the resize reads"""
    f, m, iw, ih, ow, oh, box, gap = case
    rw, rh = reduced_size(FM, case)
    b = box if box is not None else (0, 0, iw, ih)
    if (rw, rh) != (iw, ih):
        b = FM.gap_plan(FM.NAMES.index(f), iw, ih, ow, oh, box, gap)[4]
    return MB.axis_runs(rw, ow, b[0], b[2]), MB.axis_runs(rh, oh, b[1], b[3])


def both_run(MB, FM, case):
    return all(axes_run(MB, FM, case))


def tells_the_orders_apart(MB, FM, case):
    """a tall case with a weighted filter whose passes both run: the h_first model must not reproduce it"""
    rw, rh = reduced_size(FM, case)
    return case[0] != "nearest" and vertical_first(rw, rh, case[5]) and both_run(MB, FM, case)


def main():
    import PIL
    assert PIL.__version__ == PILLOW, f"this fixture records Pillow {PILLOW}, not {PIL.__version__}"
    sys.path.insert(0, os.path.dirname(HERE))
    import resize_box_model as MB
    import resize_filters_model as FM
    crcs, outs = [], []
    told = tall = 0
    for name, case in all_cases().items():
        f, m, iw, ih, ow, oh, box, gap = case
        img = make_input(name)
        want = pillow_resize(img, m, f, ow, oh, box, gap)
        crcs.append(zlib.crc32(img.tobytes()))
        outs.append(np.frombuffer(want.tobytes(), np.uint8))
        filt = FM.NAMES.index(f)
        got = FM.resize(img, filt, ow, oh, box, gap, alpha=m == "RGBA")
        assert FM.same(got, want), f"{name}: the model does not reproduce this Pillow build"
        tall += vertical_first(*reduced_size(FM, case), oh)
        if tells_the_orders_apart(MB, FM, case):
            old = FM.resize(img, filt, ow, oh, box, gap, alpha=m == "RGBA", order="h_first")
            assert not FM.same(old, want), f"{name}: horizontal first gives Pillow's bytes too: the case proves nothing"
            told += 1
    print(f"{len(outs)} cases, {tall} of them vertical first, {told} of those tell the two orders apart")
    arrays = {"in_crc": np.array(crcs, np.uint32), "bytes": np.concatenate(outs)}
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_LZMA) as zf:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.save(buf, arr)
            zf.writestr(key + ".npy", buf.getvalue())
    back = load()
    assert all(np.array_equal(np.frombuffer(c[9].tobytes(), np.uint8), o) for c, o in zip(back.values(), outs))
    assert os.path.getsize(OUT) < 1 << 20
    print(OUT, os.path.getsize(OUT), "bytes,", len(back), "cases")


if __name__ == "__main__":
    main()
