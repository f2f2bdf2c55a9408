"""Writes tests/golden/resize_pillow_ycc_out.npz: what Pillow itself makes of the cases of tests/resize_ycc_out_model.py.

CASES (YCbCr planes in, planes out; two frames each), stored as <name>_y, <name>_cb, <name>_cr:

    Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
    Cbo = Image.fromarray(Cb, "L").resize((OCW, OCH), filt, box=bc, reducing_gap=g)          (Cr likewise)

RGB_CASES (RGB frames in; two frames each), stored as <name>_y and, per destination subsampling, <name>_<sub>_cb / _cr:

    rgb = Image.fromarray(x, "RGB").resize((out_w, out_h), filt)
    Y, Cb, Cr = rgb.convert("YCbCr").split();  Cb, Cr = Cb.reduce((1 << dsx, 1 << dsy)), Cr.reduce(...)

The GPU tests read this file (Pillow need not be installed where they run); tests/test_resize_ycc_out_host.py checks that the
numpy model reproduces it.  The inputs are regenerated from their seeds and not stored, but for one case of either list that
pins the generators.  The generator refuses to write a fixture that cannot tell the contract from its near miss: the chroma box
scaled by the destination's subsampling instead of the source's.
    python tests/golden/make_resize_ycc_out_golden.py        (written with Pillow 12.2.0)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_ycc_out.npz")
sys.path.insert(0, os.path.dirname(HERE))

import resize_ycc_model as Y  # noqa: E402
import resize_ycc_out_model as M  # noqa: E402


def _resize(plane, mode, out_w, out_h, filt, box, gap):
    from PIL import Image
    return Image.fromarray(plane, mode).resize((out_w, out_h), getattr(Image.Resampling, filt.upper()), box=box, reducing_gap=gap)


def pillow_planes(y, cb, cr, case, chroma_box=None):
    bc = Y.chroma_box(case.box, case.in_w, case.in_h, case.ssx, case.ssy) if chroma_box is None else chroma_box
    ocw, och = M.out_chroma_size(case.out_w, case.out_h, case.dsx, case.dsy)
    return (np.asarray(_resize(y, "L", case.out_w, case.out_h, case.filt, case.box, case.gap)),
            np.asarray(_resize(cb, "L", ocw, och, case.filt, bc, case.gap)), np.asarray(_resize(cr, "L", ocw, och, case.filt, bc, case.gap)))


def pillow_rgb(x, case, dsx, dsy):
    yy, cb, cr = _resize(x, "RGB", case.out_w, case.out_h, case.filt, None, None).convert("YCbCr").split()
    if dsx or dsy:
        cb, cr = cb.reduce((1 << dsx, 1 << dsy)), cr.reduce((1 << dsx, 1 << dsy))
    return np.asarray(yy), np.asarray(cb), np.asarray(cr)


def main():
    arrays, told = {}, 0
    for case in M.CASES:
        y, cb, cr = M.make_planes(case)
        out = [pillow_planes(y[f], cb[f], cr[f], case) for f in range(M.FRAMES)]
        for k, name in enumerate(("y", "cb", "cr")):
            arrays[f"{case.name}_{name}"] = np.stack([o[k] for o in out])
        if case.box is not None and (case.ssx, case.ssy) != (case.dsx, case.dsy):
            x0, y0, x1, y1 = Y.chroma_box(case.box, case.in_w, case.in_h, case.dsx, case.dsy)
            cw, ch = Y.chroma_size(case.in_w, case.in_h, case.ssx, case.ssy)       # (cut to the plane, where Pillow takes it)
            near = pillow_planes(y[0], cb[0], cr[0], case, chroma_box=(x0, y0, min(x1, cw), min(y1, ch)))
            told += not np.array_equal(near[1], out[0][1])
    if not told:
        raise SystemExit("refusing to write: a chroma box scaled by the destination's subsampling is invisible in the fixture")
    for case in M.RGB_CASES:
        x = M.make_rgb(case)
        for sub, (dsx, dsy) in M.SUBS.items():
            out = [pillow_rgb(x[f], case, dsx, dsy) for f in range(M.FRAMES)]
            arrays[f"{case.name}_y"] = np.stack([o[0] for o in out])
            arrays[f"{case.name}_{sub}_cb"] = np.stack([o[1] for o in out])
            arrays[f"{case.name}_{sub}_cr"] = np.stack([o[2] for o in out])
    for k, p in zip(("y", "cb", "cr"), M.make_planes(M.CASES[0])):
        arrays[f"input_check_{k}"] = p
    arrays["input_check_rgb"] = M.make_rgb(M.RGB_CASES[1])
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
