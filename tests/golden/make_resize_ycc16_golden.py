"""Writes tests/golden/resize_pillow_ycc16.npz: what Pillow itself makes of the cases of tests/resize_ycc16_model.py, every plane
resized as mode I;16 on its raw words (two frames each):

    <name>_y                Image.fromarray(Y,  "I;16").resize((out_w, out_h), filt, box=bl)
    <name>_cb,  <name>_cr   Image.fromarray(Cb, "I;16").resize((out_w, out_h), filt, box=bc)      what the matrix converts
    <name>_dcb, <name>_dcr  Image.fromarray(Cb, "I;16").resize((OCW, OCH), filt, box=bc)          what a YCbCr destination stores

with bc the luma box scaled by the source's subsampling and (OCW, OCH) the full output's chroma size under the case's
destination subsampling.  A case's window is not applied here: the tests cut it out of these planes.  The GPU tests read this
file (Pillow need not be installed where they run); tests/test_resize_ycc16_host.py checks that the numpy model reproduces it.
The inputs are regenerated from their seeds and not stored, but for one case that pins the generator.  The generator refuses to
write a fixture in which one of these near misses would be invisible: an unscaled chroma box, replicated instead of resized
chroma, swapped Cb and Cr, a saturating store in place of 0xFF00 | low byte.
    python tests/golden/make_resize_ycc16_golden.py        (written with Pillow 12.2.0)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_ycc16.npz")
sys.path.insert(0, os.path.dirname(HERE))

import resize_ycc16_model as M  # noqa: E402


def _resize(plane, out_w, out_h, filt, box):
    from PIL import Image
    im = Image.fromarray(plane, "I;16").resize((out_w, out_h), getattr(Image.Resampling, filt.upper()), box=box)
    assert im.mode == "I;16"
    return np.asarray(im).astype(np.uint16)


def pillow_case(y, cb, cr, case, chroma_box=None):
    """(Yo, Cbo, Cro, dCbo, dCro) of one frame"""
    bc = M.chroma_box(case.box, case.in_w, case.in_h, case.ssx, case.ssy) if chroma_box is None else chroma_box
    ocw, och = M.out_chroma_size(case.out_w, case.out_h, case.dsx, case.dsy)
    return (_resize(y, case.out_w, case.out_h, case.filt, case.box),
            _resize(cb, case.out_w, case.out_h, case.filt, bc), _resize(cr, case.out_w, case.out_h, case.filt, bc),
            _resize(cb, ocw, och, case.filt, bc), _resize(cr, ocw, och, case.filt, bc))


def main():
    arrays = {}
    told = dict(box=0, replicated=0, swapped=0, store=0, wrapped_words=0)
    for case in M.CASES:
        y, cb, cr = M.make_planes(case)
        out = [pillow_case(y[f], cb[f], cr[f], case) for f in range(M.FRAMES)]
        for k, name in enumerate(("y", "cb", "cr", "dcb", "dcr")):
            arrays[f"{case.name}_{name}"] = np.stack([o[k] for o in out])
        yo, cbo, cro = (arrays[f"{case.name}_{n}"] for n in ("y", "cb", "cr"))
        if case.box is not None and (case.ssx or case.ssy):    # the luma box on the chroma plane, cut to it where Pillow takes it
            cw, ch = M.chroma_size(case.in_w, case.in_h, case.ssx, case.ssy)
            x0, y0, x1, y1 = case.box
            near = pillow_case(y[0], cb[0], cr[0], case, chroma_box=(x0, y0, min(x1, cw), min(y1, ch)))
            told["box"] += not np.array_equal(near[1], out[0][1])
        if case.ssx and case.ssy and (case.out_w, case.out_h) == (case.in_w, case.in_h):   # chroma repeated 2 x 2 in place of a resize
            rep = np.repeat(np.repeat(cb, 2, axis=1), 2, axis=2)[:, :case.out_h, :case.out_w]
            told["replicated"] += not np.array_equal(rep, cbo)
        told["swapped"] += not np.array_equal(cbo, cro)
        sat = M.resize_plane_saturating(y, case.filt, case.out_w, case.out_h, case.box)
        wrapped = int((sat != yo).sum())
        told["store"] += wrapped > 0
        told["wrapped_words"] += wrapped                        # (either pass may wrap: the words that differ, not where it began)
    for what, n in told.items():
        if not n:
            raise SystemExit(f"refusing to write: the near miss '{what}' is invisible in the fixture")
    for k, p in zip(("y", "cb", "cr"), M.make_planes(M.CASES[0])):
        arrays[f"input_check_{k}"] = p
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", told)


if __name__ == "__main__":
    main()
