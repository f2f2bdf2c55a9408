"""Writes tests/golden/resize_pillow_ycc.npz: what Pillow itself makes of the cases of tests/resize_ycc_model.py (CASES) with

    Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
    Cbo = Image.fromarray(Cb, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
    Cro = Image.fromarray(Cr, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
    rgb = Image.merge("YCbCr", (Yo, Cbo, Cro)).convert("RGB")

Two frames per case.  The GPU tests read this file (Pillow need not be installed where they run); tests/test_resize_ycc_host.py
checks that the numpy model reproduces it.  The inputs are regenerated from their seeds (resize_ycc_model.make_planes) and not
stored, but for one case that pins the generator.  The generator refuses to write a fixture that cannot tell the contract from
its near misses: a chroma box that is not scaled, chroma replicated to luma size and resized with the luma box, a dropped gap.
    python tests/golden/make_resize_ycc_golden.py        (written with Pillow 12.2.0)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_ycc.npz")
sys.path.insert(0, os.path.dirname(HERE))

import resize_ycc_model as Y  # noqa: E402

FRAMES = 2


def _resize(plane, out_w, out_h, filt, box, gap):
    from PIL import Image
    resample = getattr(Image.Resampling, filt.upper())
    return Image.fromarray(plane, "L").resize((out_w, out_h), resample, box=box, reducing_gap=gap)


def pillow_compose(y, cb, cr, case, chroma_box=None, gap="case"):
    from PIL import Image
    bc = Y.chroma_box(case.box, case.in_w, case.in_h, case.sx, case.sy) if chroma_box is None else chroma_box
    g = case.gap if gap == "case" else gap
    planes = (_resize(y, case.out_w, case.out_h, case.filt, case.box, g), _resize(cb, case.out_w, case.out_h, case.filt, bc, g),
              _resize(cr, case.out_w, case.out_h, case.filt, bc, g))
    return np.asarray(Image.merge("YCbCr", planes).convert("RGB"))


def main():
    arrays, told = {}, {"box": 0, "replicate": 0}
    for case in Y.CASES:
        y, cb, cr = Y.make_planes(case, FRAMES)
        out = np.stack([pillow_compose(y[f], cb[f], cr[f], case) for f in range(FRAMES)])
        arrays[f"{case.name}_out"] = out
        cw, ch = Y.chroma_size(case.in_w, case.in_h, case.sx, case.sy)
        if case.sx or case.sy:
            if case.box is not None:   # the luma box handed to the chroma plane, where it fits
                x0, y0, x1, y1 = case.box
                near = pillow_compose(y[0], cb[0], cr[0], case, chroma_box=(x0, y0, min(x1, cw), min(y1, ch)))
                told["box"] += not np.array_equal(near, out[0])
            if (case.in_w & case.sx) or (case.in_h & case.sy):   # odd sizes: replicated chroma has another geometry
                rep = lambda p: np.repeat(np.repeat(p, 1 << case.sy, 0), 1 << case.sx, 1)[:case.in_h, :case.in_w]
                near = pillow_compose(y[0], rep(cb[0]), rep(cr[0]), case, chroma_box=case.box or (0, 0, case.in_w, case.in_h))
                told["replicate"] += not np.array_equal(near, out[0])
        if case.gap is not None and np.array_equal(pillow_compose(y[0], cb[0], cr[0], case, gap=None), out[0]):
            raise SystemExit(f"refusing to write: gapped case {case.name} equals its ungapped composition")
    if not all(told.values()):
        raise SystemExit(f"refusing to write: a near miss is invisible in the fixture: {told}")
    for k, p in zip(("y", "cb", "cr"), Y.make_planes(Y.CASES[0], FRAMES)):
        arrays[f"input_check_{k}"] = p
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", told)


if __name__ == "__main__":
    main()
