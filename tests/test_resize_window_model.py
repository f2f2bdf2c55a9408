"""tests/resize_window_model.py against the whole-frame numpy models, bit for bit (CPU only): every sample type, every filter,
with and without a fractional box, for all output rows and columns and for a scattered subset of them; and that it fetches
the rectangle it promises and nothing else."""
import numpy as np
import pytest

import resize32_model as M32
import resize_filters_model as F
import resize_window_model as W

# name -> (dtype, channels, alpha)
TYPES = {"u8c1": (np.uint8, 1, False), "u8c3": (np.uint8, 3, False), "u8c4": (np.uint8, 4, False),
         "rgba": (np.uint8, 4, True), "u16c3": (np.uint16, 3, False), "f32c3": (np.float32, 3, False)}
# (in_w, in_h, out_w, out_h): both axes down, both up, mixed, one axis only (each way), neither
SHAPES = [(120, 90, 37, 29), (40, 30, 117, 88), (117, 89, 61, 97), (119, 90, 119, 31), (120, 87, 43, 87), (64, 48, 64, 48),
          (6, 640, 4, 77)]   # the last one runs vertical first (resize_model.pillow_vertical_first)


def _frame(dtype, h, w, c, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        x = (rng.standard_normal((h, w, c)) * 1000).astype(np.float32)
        x[3, 5, 0], x[h - 2, w - 3, c - 1] = np.float32(1e-41), np.float32(-3e38)   # a denormal, a sample near -FLT_MAX
        return x
    return rng.integers(0, np.iinfo(dtype).max + 1, (h, w, c), dtype=dtype)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = M32.differs(got, want) if got.dtype == np.float32 else got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} samples differ, first at {tuple(np.argwhere(bad)[0])}"


class _Fetch:
    """the source as resize_window_model reads it; remembers the rectangles asked for"""

    def __init__(self, img):
        self.img, self.calls = img, []

    def __call__(self, y0, y1, x0, x1):
        self.calls.append((y0, y1, x0, x1))
        return self.img[y0:y1, x0:x1]


def _box(in_w, in_h):
    return (in_w * 0.11 + 0.25, in_h * 0.07 + 0.5, in_w - 3.0, in_h - 1.75)


@pytest.mark.parametrize("filt", range(6), ids=F.NAMES)
@pytest.mark.parametrize("name", list(TYPES))
def test_window_equals_whole_frame(name, filt):
    dtype, c, alpha = TYPES[name]
    rng = np.random.default_rng(filt * 16 + c)
    for k, (iw, ih, ow, oh) in enumerate(SHAPES):
        img = _frame(dtype, ih, iw, c, seed=filt * 100 + k)
        for box in (None, _box(iw, ih)):
            want = F.resize(img, filt, ow, oh, box=box, alpha=alpha)
            assert want.shape == (oh, ow, c)
            what = f"{name} {F.NAMES[filt]} {iw}x{ih}->{ow}x{oh} box {box}"
            fetch = _Fetch(img)
            got = W.resize(fetch, iw, ih, ow, oh, c, dtype, np.arange(oh), np.arange(ow), 3, filt, alpha, box)
            _same(got, want, what + " (all)")
            assert len(fetch.calls) == 1
            rows = rng.permutation(oh)[:max(1, oh // 7)]           # scattered, unsorted
            cols = rng.permutation(ow)[:max(1, ow // 5)]
            fetch = _Fetch(img)
            got = W.resize(fetch, iw, ih, ow, oh, c, dtype, rows, cols, 3, filt, alpha, box)
            _same(got, want[rows][:, cols], what + " (scattered)")
            H, V = W.axes(iw, ih, ow, oh, dtype, rows, cols, 3, filt, box)
            assert fetch.calls == [(V.lo, V.hi, H.lo, H.hi)]


@pytest.mark.parametrize("a", [2, 4])
def test_other_lanczos_supports(a):
    iw, ih, ow, oh = 101, 77, 58, 90
    for name in ("u8c3", "u16c3", "f32c3"):
        dtype, c, alpha = TYPES[name]
        img = _frame(dtype, ih, iw, c, seed=a)
        want = F.resize(img, F.LANCZOS, ow, oh, box=_box(iw, ih), a=a)
        rows, cols = np.array([89, 0, 44, 45]), np.array([57, 3, 0])
        got = W.resize(_Fetch(img), iw, ih, ow, oh, c, dtype, rows, cols, a, F.LANCZOS, alpha, _box(iw, ih))
        _same(got, want[rows][:, cols], f"{name} a={a}")


def test_the_window_is_what_the_tables_say_and_no_more():
    """One output row and column in the middle of a downscale: the rectangle is that output's taps, from the model's tables,
    and a source that is NaN / poison everywhere else gives the same result."""
    iw, ih, ow, oh, c = 120, 90, 37, 29, 3
    fh, ch, _ = F.axis_tables(F.LANCZOS, iw, ow)
    fv, cv, _ = F.axis_tables(F.LANCZOS, ih, oh)
    r, q = 14, 20
    H, V = W.axes(iw, ih, ow, oh, np.float32, [r], [q])
    assert (H.lo, H.hi, V.lo, V.hi) == (fh[q], fh[q] + ch[q], fv[r], fv[r] + cv[r])
    assert H.hi - H.lo < iw // 4 and V.hi - V.lo < ih // 4
    img = _frame(np.float32, ih, iw, c, seed=5)
    want = F.resize(img, F.LANCZOS, ow, oh)[r:r + 1, q:q + 1]
    poisoned = np.full_like(img, np.nan)
    poisoned[V.lo:V.hi, H.lo:H.hi] = img[V.lo:V.hi, H.lo:H.hi]
    _same(W.resize(_Fetch(poisoned), iw, ih, ow, oh, c, np.float32, [r], [q]), want, "poisoned outside the window")


def test_the_wide_address_cases_stay_inside_their_frames():
    """The requests tests/test_resize_wide_addresses_gpu.py runs on frames of 2 GiB: for each, the library's host tables are
    the model's (first and count of both axes), and every source index they name -- so every address the two-pass, nearest
    and tensor kernels form from them with plain global accesses -- lies inside the frame.  No GPU needed."""
    import lanczos_hls_amd as L
    import test_resize_wide_addresses_gpu as G
    from test_resize_plan import FRAMES_2GIB, OUT_EDGE, corner_box, frames_below_2gib

    def check(spec, ow, oh, box, filt=F.LANCZOS):
        name, iw, ih, c, kw, bps = spec
        d = L.resize_desc(iw, ih, ow, oh, c, filter=filt, **kw)
        H, V = W.axes(iw, ih, ow, oh, G.DTYPES[bps], np.arange(oh), np.arange(ow), 3, filt, box)
        for axis, ax, in_n in ((0, H, iw), (1, V, ih)):
            if filt != F.NEAREST and not ax.runs:
                continue                      # no table for an idle axis
            f, n, _ = (L.resize_taps_f64_host if bps > 1 else L.resize_taps_host)(d, axis, box=box)
            if filt == F.NEAREST:
                assert np.array_equal(f, ax.index) and (n == 1).all(), (name, axis, box)
            else:
                assert np.array_equal(f, ax.first) and np.array_equal(n, ax.count), (name, axis, box)
            assert f.min() >= 0 and (f.astype(np.int64) + n).max() <= in_n, (name, axis, box)

    ow, oh = OUT_EDGE
    for spec in FRAMES_2GIB:
        name, iw, ih, c, kw, bps = spec
        for box in G.boxes_2a(iw, ih, iw * c * bps, c * bps).values():
            assert 0 <= box[0] < box[2] <= iw and 0 <= box[1] < box[3] <= ih, (name, box)
            check(spec, ow, oh, box)
        for what, w, h, box, windows in G.one_axis_cases(spec):
            check(spec, w, h, box)
            for rows, cols in windows:
                assert rows.min() >= 0 and rows.max() < h and cols.min() >= 0 and cols.max() < w
        if bps != 2:
            check(spec, ow, oh, corner_box(iw, ih), F.NEAREST)
    for filt in (F.BILINEAR, F.BICUBIC):
        check(FRAMES_2GIB[0], ow, oh, corner_box(65535, 32769), filt)
    for spec in frames_below_2gib():
        for w in (ow, 261):
            check(spec, w, oh, corner_box(spec[1], spec[2]))
            end, size = G.staged_end(spec, w, oh, corner_box(spec[1], spec[2]))
            assert end > size, (spec[0], w, end, size)
    check(("u8c1", 40, 30, 1, {}, 1), 65535, 32769, None)
    check(("u8c1", 328, 32769, 1, {}, 1), 65535, 8, None)
