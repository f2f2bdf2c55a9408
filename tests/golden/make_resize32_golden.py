"""Writes tests/golden/resize_pillow_f32.npz: seeded float32 planes and what Pillow's Image.resize(size, Image.LANCZOS, box)
makes of them in mode F (Image.fromarray of a 2-D float32 array).

The file holds the outputs only, as their four byte planes in an LZMA-compressed zip (numpy.load reads it like any .npz).
The inputs are not stored: make_input() rebuilds them from their seeds and load() checks each against the CRC-32 the file
carries.  Pillow's mode F has one channel; the tests build 3- and 4-channel frames by stacking these planes.

Comparison rule, here and in every test (resize32_model.same): NaN positions coincide, every other sample is equal as a
32-bit pattern.  The generator refuses to write a fixture
  - that the model (tests/resize32_model.py) does not reproduce;
  - on which one of these near misses gives nearly Pillow's output:
      float32 accumulation            must differ in >= 10 % of the samples of every unit-noise case;
      a double intermediate           the same, on the unit-noise cases in which both passes run (with one pass there is
                                      no intermediate);
      denormals flushed to zero       must differ in every sample of every all-denormal case;
      taps up to the bucket K         (a neighbouring sample times the table's +0.0) must differ in at least one sample of
                                      every non-finite case that has a pass padded that way;
      a k == 0 guard                  (instead of a guard on count) must differ in at least one sample of the non-finite cases.
    The last one rests on a zero weight INSIDE Pillow's window.  The case with the box (3, 0, 43, 40) has them on its
    horizontal axis: a whole-pixel shift at equal width puts the last tap of every window at distance a exactly, where
    the filter is 0.0.  (A box of whole pixels whose width AND height equal the output's is no case: Pillow crops then
    and computes nothing)  Without such a case the condition would have been dropped;
  - in which NaNs exceed 15 % of a case's samples.
    python tests/golden/make_resize32_golden.py
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "resize_pillow_f32.npz")

# (in_w, in_h, out_w, out_h, box)
SHAPES = [
    (64, 48, 31, 17, None),                       # down
    (33, 21, 80, 50, None),                       # up
    (31, 17, 300, 9, None),                       # mixed: up across, down down
    (50, 40, 50, 13, None),                       # vertical pass only
    (50, 40, 7, 40, None),                        # horizontal pass only
    (50, 40, 40, 30, (3, 0, 43, 40)),             # columns cropped by whole pixels (equal width), rows reduced
    (50, 40, 40, 30, (3.5, 2.25, 43.5, 32.25)),   # equal size, shifted by fractions
    (64, 48, 23, 29, (5.3, 4.7, 60.1, 40.2)),     # a fractional box
]
KINDS = ["noise", "decades", "denormal", "overflow", "tinyneg", "nonfinite"]
# kind -> the shapes it runs on.  Shape 5 carries no unit-noise plane: its horizontal pass, a whole-pixel shift at equal
# width, has the weights of the identity up to 1e-17, so a double intermediate is Pillow's float one there; its planes are
# there for the zero weight at the end of every horizontal window
KIND_SHAPES = {"noise": (0, 1, 2, 3, 4, 6, 7), "decades": range(8), "denormal": (0, 1, 2, 6), "overflow": (0, 1, 2, 6),
               "tinyneg": (0, 1, 7), "nonfinite": (0, 1, 2, 3, 4, 5, 7)}
CASES = [(si, kind) for kind in KINDS for si in KIND_SHAPES[kind]]


def case_name(si, kind):
    return f"s{si}_{kind}"


def make_input(si, kind, w, h):
    rng = np.random.default_rng(3200 + 10 * si + KINDS.index(kind))
    if kind == "noise":                  # unit noise
        return rng.random((h, w), dtype=np.float32)
    if kind == "decades":                # magnitudes over 60 decades, both signs
        return (rng.choice([-1.0, 1.0], (h, w)) * 10.0 ** rng.uniform(-30, 30, (h, w))).astype(np.float32)
    if kind == "denormal":               # every sample below FLT_MIN = 1.17e-38
        return (rng.integers(1, 1 << 23, (h, w)).astype(np.uint32)).view(np.float32)
    if kind == "overflow":               # half of the samples 3e38, the others 0: the filter's overshoot passes FLT_MAX
        return (rng.integers(0, 2, (h, w)) * np.float32(3e38)).astype(np.float32)
    if kind == "tinyneg":                # a third of the samples the smallest negative denormal, the others 0
        return np.where(rng.random((h, w)) < 0.33, np.float32(-1e-45), np.float32(0)).astype(np.float32)
    x = rng.random((h, w), dtype=np.float32)   # nonfinite: unit noise with one inf, one -inf, one NaN; denormals, near-FLT_MAX
    pos = rng.choice(h * w, 9, replace=False)
    flat = x.reshape(-1)
    flat[pos[0]], flat[pos[1]], flat[pos[2]] = np.inf, -np.inf, np.nan
    flat[pos[3:6]] = np.float32(1e-41)
    flat[pos[6:9]] = np.float32(3.3e38)
    return x


def pillow_resize(plane, out_w, out_h, box=None):
    from PIL import Image
    im = Image.fromarray(plane)
    assert im.mode == "F", im.mode
    r = im.resize((out_w, out_h), Image.LANCZOS, box=box)
    return np.asarray(r).astype(np.float32).reshape(out_h, out_w)


def load(path=OUT):
    """{case name: (input plane, Pillow's output plane)}, both float32."""
    z = np.load(path)
    flat = (z["b0"].astype(np.uint32) | (z["b1"].astype(np.uint32) << 8) | (z["b2"].astype(np.uint32) << 16)
            | (z["b3"].astype(np.uint32) << 24)).view(np.float32)
    crc = z["in_crc"]
    cases = {}
    at = 0
    for si, kind in CASES:
        iw, ih, ow, oh, _ = SHAPES[si]
        img = make_input(si, kind, iw, ih)
        assert zlib.crc32(img.tobytes()) == int(crc[len(cases)]), f"{case_name(si, kind)}: the seeded input changed"
        cases[case_name(si, kind)] = (img, flat[at:at + ow * oh].reshape(oh, ow))
        at += ow * oh
    assert at == flat.size
    return cases


def zero_weight_taps(si, M):
    """taps inside a window of the case's tables whose weight is exactly 0.0"""
    iw, ih, ow, oh, box = SHAPES[si]
    x0, y0, x1, y1 = box if box is not None else (0, 0, iw, ih)
    n = 0
    for in_n, out_n, b0, b1 in ((iw, ow, x0, x1), (ih, oh, y0, y1)):
        if M.MB.axis_runs(in_n, out_n, b0, b1):
            _, c, k = M.tables(in_n, out_n, 3, b0, b1)
            n += int(((k == 0.0) & (np.arange(k.shape[1])[None, :] < c[:, None])).sum())
    return n


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import resize32_model as M
    crcs, outs = [], []
    zero_k_cases = guard_diff = 0
    for si, kind in CASES:
        iw, ih, ow, oh, box = SHAPES[si]
        name = case_name(si, kind)
        img = make_input(si, kind, iw, ih)
        want = pillow_resize(img, ow, oh, box)
        crcs.append(zlib.crc32(img.tobytes()))
        outs.append(want.reshape(-1))
        assert M.same(M.resize(img, ow, oh, 3, box), want), f"{name}: the model does not reproduce this Pillow build"
        nan = float(np.isnan(want).mean())
        assert nan <= 0.15, f"{name}: {100 * nan:.1f} % NaN"
        line = f"{name:14s} {iw}x{ih}->{ow}x{oh} NaN {100 * nan:4.1f} % inf {100 * float(np.isinf(want).mean()):4.1f} %"

        def share(**kw):
            return float(M.differs(M.resize(img, ow, oh, 3, box, **kw), want).mean())
        if kind == "noise":
            s = share(acc32=True)
            line += f"  float32 accumulation differs {100 * s:.0f} %"
            assert s >= 0.10, name
            x0, y0, x1, y1 = box if box is not None else (0, 0, iw, ih)
            if M.MB.axis_runs(iw, ow, x0, x1) and M.MB.axis_runs(ih, oh, y0, y1):
                s = share(mid64=True)
                line += f", double intermediate {100 * s:.0f} %"
                assert s >= 0.10, name
        if kind == "denormal":
            s = share(flush=True)
            line += f"  flushed differs {100 * s:.0f} %"
            assert s == 1.0, name
        if kind == "tinyneg":
            line += f"  -0.0 in {100 * float((want.view(np.uint32) == 0x80000000).mean()):.0f} %"
            assert (want.view(np.uint32) == 0x80000000).any(), name
        if kind == "overflow":
            assert np.isinf(want).any(), name
        if kind == "nonfinite":
            padded = M.differs(M.resize(img, ow, oh, 3, box, pad_to=M.bucket), M.resize(img, ow, oh, 3, box,
                                                                                      pad_to=lambda ks: 0)).any()
            s = share(pad_to=M.bucket)
            line += f"  padded to K differs in {int(round(s * want.size))}"
            assert s > 0 or not padded, name
            z = zero_weight_taps(si, M)
            if z:
                zero_k_cases += 1
                g = share(skip_zero_k=True)
                guard_diff += g > 0
                line += f", {z} zero weights in windows: k == 0 guard differs in {int(round(g * want.size))}"
        print(line)
    assert zero_k_cases >= 1 and guard_diff >= 1, "no case tells a k == 0 guard from a count guard"
    flat = np.concatenate(outs).view(np.uint32)
    arrays = {"in_crc": np.array(crcs, np.uint32)}
    for b in range(4):
        arrays[f"b{b}"] = ((flat >> (8 * b)) & 255).astype(np.uint8)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_LZMA) as zf:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.save(buf, arr)
            zf.writestr(key + ".npy", buf.getvalue())
    assert all(M.same(c[1].reshape(-1), o) and np.array_equal(c[1].reshape(-1).view(np.uint32), o.view(np.uint32))
               for c, o in zip(load().values(), outs))
    print(OUT, os.path.getsize(OUT), "bytes,", flat.size, "samples")


if __name__ == "__main__":
    main()
