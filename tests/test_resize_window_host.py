"""CPU-only checks of the window of the output (lanczos_resize_window, lanczos_resize_window_* and lanczos_resize_tensor*_window_*):
every refusal returns its code, the whole-output window is the call without one, the source rectangle is the union of the
window's taps as the host tables give them, the plan follows the window, the tensor validators use the window's extent, and
center_window is torchvision's CenterCrop.  The committed fixture (Pillow's Image.resize(...).crop(window)) equals the numpy
models sliced to the window and, where Pillow imports, Pillow.  No GPU needed.

test_pillow_still_equals_the_fixture needs Pillow and SKIPS where it does not import (as its siblings do); every other test here,
the fixture against the models included, runs without it."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_filters_model as F
import resize_window_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_window.npz")


def _gen():
    spec = importlib.util.spec_from_file_location("make_resize_window_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_window_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


def _code(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except L.LanczosError as e:
        return e.code
    return L.OK


def _raw(x0, y0, w, h, reserved=(0, 0, 0, 0)):
    win = L.ResizeWindow()
    win.x0, win.y0, win.w, win.h = x0, y0, w, h
    for i, v in enumerate(reserved):
        win.reserved[i] = v
    return win


# ---- the struct, the symbols, validation ------------------------------------------------------------------------------

def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.ResizeWindow) == 8 * 4
    for name in ("lanczos_resize_window_init", "lanczos_resize_window_validate", "lanczos_resize_window_source",
                 "lanczos_resize_window_plan_host", "lanczos_resize_window_device", "lanczos_resize_window_host",
                 "lanczos_resize_tensor_window_validate", "lanczos_resize_tensor16_window_validate",
                 "lanczos_resize_tensor_window_device", "lanczos_resize_tensor_window_host",
                 "lanczos_resize_tensor16_window_device", "lanczos_resize_tensor16_window_host"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name), name


def test_window_init_is_the_whole_output():
    d = L.resize_desc(211, 163, 600, 70, 3)
    win = L.ResizeWindow()
    for i in range(4):
        win.reserved[i] = 7                                        # init clears them
    assert L._lib().lanczos_resize_window_init(ctypes.byref(win), ctypes.byref(d)) == L.OK
    assert (win.x0, win.y0, win.w, win.h, list(win.reserved)) == (0, 0, 600, 70, [0, 0, 0, 0])
    w = L.resize_window(d)
    assert (w.x0, w.y0, w.w, w.h) == (0, 0, 600, 70)
    assert L._lib().lanczos_resize_window_init(None, ctypes.byref(d)) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.out_w = 0
    assert L._lib().lanczos_resize_window_init(ctypes.byref(win), ctypes.byref(bad)) == L.ERR_BAD_ARG


def test_validation_codes():
    d = L.resize_desc(211, 163, 600, 70, 3)
    v = lambda win: L._lib().lanczos_resize_window_validate(ctypes.byref(d), ctypes.byref(win) if win is not None else None)
    assert v(None) == L.OK                                         # NULL: the whole output
    for ok in ((0, 0, 600, 70), (0, 0, 1, 1), (599, 69, 1, 1), (250, 5, 300, 37), (583, 61, 17, 9), (0, 69, 600, 1)):
        assert v(_raw(*ok)) == L.OK, ok
    for bad in ((-1, 0, 10, 10), (0, -1, 10, 10), (0, 0, 0, 10), (0, 0, 10, 0), (0, 0, -5, 10), (0, 0, 601, 70),
                (0, 0, 600, 71), (1, 0, 600, 70), (0, 1, 600, 70), (600, 0, 1, 1), (0, 70, 1, 1), (591, 0, 10, 10),
                (2**31 - 1, 0, 2, 2), (5, 5, 2**31 - 1, 2)):
        assert v(_raw(*bad)) == L.ERR_BAD_ARG, bad
    for i in range(4):                                             # each reserved word is refused
        r = [0, 0, 0, 0]
        r[i] = 1
        assert v(_raw(0, 0, 600, 70, r)) == L.ERR_BAD_ARG, i
        r[i] = -(2**31)
        assert v(_raw(10, 10, 20, 20, r)) == L.ERR_BAD_ARG, i
    bad_desc = L.ResizeDesc.from_buffer_copy(d)
    bad_desc.channels = 2
    assert L._lib().lanczos_resize_window_validate(ctypes.byref(bad_desc), None) == L.ERR_BAD_ARG
    # the Python wrappers raise the same codes
    assert _code(L.resize_window, d, (590, 0, 11, 5)) == L.ERR_BAD_ARG
    assert _code(L.resize_window, d, (0, 0, 5)) == L.ERR_BAD_ARG
    assert _code(L.resize_window, d, _raw(0, 0, 5, 5, (0, 0, 0, 3))) == L.ERR_BAD_ARG
    # every host entry refuses a bad window, whatever else it is given
    rect = (ctypes.c_int32 * 4)()
    plan = L.ResizePlanEx()
    for win in (_raw(0, 0, 601, 70), _raw(0, 0, 10, 10, (0, 1, 0, 0))):
        assert L._lib().lanczos_resize_window_source(ctypes.byref(d), None, ctypes.byref(win), rect) == L.ERR_BAD_ARG
        assert L._lib().lanczos_resize_window_plan_host(ctypes.byref(d), None, ctypes.byref(win), 1,
                                                        ctypes.byref(plan)) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_window_source(ctypes.byref(d), None, None, None) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_window_plan_host(ctypes.byref(d), None, None, 0, ctypes.byref(plan)) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_window_plan_host(ctypes.byref(d), None, None, 1, None) == L.ERR_BAD_ARG


def test_center_window_is_torchvisions_center_crop():
    assert L.center_window(341, 256, 224, 224) == (58, 16, 224, 224)      # the tie 58.5 rounds to even
    assert L.center_window(343, 256, 224, 224) == (60, 16, 224, 224)      # the tie 59.5 too
    assert L.center_window(342, 257, 224, 224) == (59, 16, 224, 224)      # 16.5 -> 16
    assert L.center_window(224, 224, 224, 224) == (0, 0, 224, 224)
    assert L.center_window(10, 9, 3, 2) == (4, 4, 3, 2)                   # 3.5 -> 4
    for ow, oh, w, h in ((223, 256, 224, 224), (341, 223, 224, 224), (10, 10, 0, 5), (10, 10, 5, 0)):
        assert _code(L.center_window, ow, oh, w, h) == L.ERR_BAD_ARG      # CenterCrop would pad: no window
    for ow, oh, w, h in ((341, 256, 224, 224), (97, 61, 1, 1), (600, 70, 599, 69)):
        L.resize_window(L.resize_desc(500, 375, ow, oh, 3), L.center_window(ow, oh, w, h))


# ---- the source rectangle ---------------------------------------------------------------------------------------------

def _rect_from_tables(d, window, box=None, gap=None):
    """the rectangle recomputed from the host tables of the request"""
    x0, y0, w, h = window
    p = L.resize_plan_host(d, 1, opts=L.resize_opts(d, box, gap))
    if p.fx > 1 or p.fy > 1:
        return tuple(p.safe_box)
    wide = bool(d.reserved[0] & (L.RESIZE_U16 | L.RESIZE_F32))
    taps = L.resize_taps_f64_host if wide else L.resize_taps_host
    lo_hi = []
    for axis, runs, o0, n in ((0, p.pass_h, x0, w), (1, p.pass_v, y0, h)):
        if not runs:
            lo_hi.append((o0, o0 + n))
            continue
        first, count, _ = taps(d, axis, opts=L.resize_opts(d, box, gap))
        f, c = first[o0:o0 + n].astype(np.int64), count[o0:o0 + n].astype(np.int64)
        lo_hi.append((int(f.min()), int((f + c).max())))
    return lo_hi[0][0], lo_hi[1][0], lo_hi[0][1], lo_hi[1][1]


SOURCE_CASES = [
    # (what, desc arguments, keywords, box, gap, windows)
    ("down", (300, 200, 97, 61, 3), {}, None, None,
     [(30, 20, 40, 21), (0, 0, 17, 9), (80, 52, 17, 9), (0, 30, 97, 5), (48, 30, 1, 1), (0, 0, 97, 61)]),
    ("up", (211, 163, 600, 70, 3), {}, None, None,
     [(250, 5, 300, 37), (0, 0, 17, 9), (583, 61, 17, 9), (299, 33, 1, 1), (0, 0, 600, 70)]),
    ("box", (110, 80, 56, 43, 3), {}, (7.3, 5.6, 101.2, 77.75), None, [(19, 11, 27, 21), (0, 0, 1, 1), (55, 42, 1, 1)]),
    ("gap", (400, 300, 50, 38, 3), {}, None, 2.0, [(13, 9, 24, 20), (0, 0, 50, 38), (49, 37, 1, 1)]),
    ("gap with a box", (400, 300, 50, 38, 1), {}, (40.5, 30.25, 380.0, 290.0), 2.0, [(13, 9, 24, 20)]),
    ("nearest", (83, 61, 131, 40, 3), {"filter": "nearest"}, None, None, [(0, 11, 31, 23), (130, 39, 1, 1), (17, 0, 60, 40)]),
    ("nearest, one axis idle", (83, 61, 131, 61, 1), {"filter": "nearest"}, None, None, [(5, 7, 31, 23)]),
    ("h only", (97, 41, 55, 41, 1), {}, None, None, [(20, 10, 30, 25), (0, 0, 55, 41)]),
    ("v only", (97, 41, 97, 90, 4), {"alpha": True}, None, None, [(20, 10, 30, 25), (96, 89, 1, 1)]),
    ("both idle", (40, 30, 40, 30, 4), {}, None, None, [(11, 5, 23, 19), (0, 0, 40, 30), (39, 29, 1, 1)]),
    ("uint16", (80, 60, 47, 95, 3), {"bits": 16}, None, None, [(9, 40, 31, 33)]),
    ("float, bicubic", (75, 55, 120, 33, 1), {"f32": True, "filter": "bicubic"}, (0.5, 0.0, 75.0, 50.5), None, [(60, 6, 35, 20)]),
]


@pytest.mark.parametrize("case", SOURCE_CASES, ids=[c[0] for c in SOURCE_CASES])
def test_window_source_is_the_union_of_the_windows_taps(case):
    what, dargs, kw, box, gap, windows = case
    d = L.resize_desc(*dargs, **kw)
    iw, ih = dargs[:2]
    for window in windows:
        got = L.resize_window_source(d, window, box=box, reducing_gap=gap)
        assert got == _rect_from_tables(d, window, box, gap), (what, window)
        assert 0 <= got[0] < got[2] <= iw and 0 <= got[1] < got[3] <= ih, (what, window, got)
    # no window is the whole output
    assert L.resize_window_source(d, None, box=box, reducing_gap=gap) == _rect_from_tables(d, (0, 0, d.out_w, d.out_h), box, gap)


def test_window_source_in_numbers():
    """what the rectangle is, spelled out once.  Halving with a = 3: centre = 2 o + 1, support 6, first = int(centre - 5.5), end
    = int(centre + 6.5) -- outputs 40 .. 49 read [75, 105), outputs 20 .. 24 read [35, 55).  An idle axis reads its own range, a
    gap the whole safe box"""
    d = L.resize_desc(200, 100, 100, 50, 3)
    assert L.resize_window_source(d, (40, 20, 10, 5)) == (75, 35, 105, 55)
    assert L.resize_window_source(d, (0, 0, 10, 5)) == (0, 0, 25, 15)
    d = L.resize_desc(200, 100, 100, 100, 3)
    assert L.resize_window_source(d, (40, 20, 10, 5)) == (75, 20, 105, 25)
    d = L.resize_desc(400, 300, 50, 38, 3)
    p = L.resize_plan_host(d, 1, reducing_gap=2.0)
    assert (p.fx, p.fy) == (4, 3) and tuple(p.safe_box) == (0, 0, 400, 300)
    assert L.resize_window_source(d, (20, 20, 2, 2), reducing_gap=2.0) == (0, 0, 400, 300)
    # the numpy model of a window of the source agrees (tests/resize_window_model.py)
    H, V = W.axes(211, 163, 600, 70, np.uint8, np.arange(5, 42), np.arange(250, 550))
    assert L.resize_window_source(L.resize_desc(211, 163, 600, 70, 3), (250, 5, 300, 37)) == (H.lo, V.lo, H.hi, V.hi)


# ---- the plan ---------------------------------------------------------------------------------------------------------

def test_the_whole_window_plans_as_the_call_without_one():
    for dargs, kw, box, gap in (((211, 163, 600, 70, 3), {}, None, None), ((300, 200, 97, 61, 4), {"alpha": True}, None, None),
                                ((500, 375, 341, 256, 3), {}, None, None), ((110, 80, 56, 43, 3), {}, (7.3, 5.6, 101.2, 77.75), None),
                                ((400, 300, 50, 38, 3), {}, None, 2.0), ((97, 41, 55, 41, 1), {}, None, None),
                                ((40, 30, 40, 30, 3), {}, None, None), ((83, 61, 131, 40, 3), {"filter": "nearest"}, None, None),
                                ((80, 60, 47, 95, 3), {"bits": 16}, None, None), ((2000, 1500, 100, 80, 3), {}, None, None)):
        d = L.resize_desc(*dargs, **kw)
        for frames in (1, 5):
            want = L.resize_plan_host(d, frames, opts=L.resize_opts(d, box, gap))
            for window in (None, (0, 0, d.out_w, d.out_h)):
                got = L.resize_window_plan_host(d, window, frames, box=box, reducing_gap=gap)
                assert bytes(got) == bytes(want), (dargs, window, frames)


def test_the_plan_is_made_on_the_window():
    d = L.resize_desc(211, 163, 600, 70, 3)
    full = L.resize_window_plan_host(d, None, 1)
    assert full.inner.fused and full.inner.strips == 3 and full.pass_h and full.pass_v
    assert (full.mid_row0, full.mid_rows) == (0, 163)
    fv, cv, _ = L.resize_taps_host(d, 1)
    for window, strips in (((250, 5, 300, 37), 2), ((0, 0, 17, 9), 1), ((583, 61, 17, 9), 1), ((299, 33, 1, 1), 1)):
        x0, y0, w, h = window
        p = L.resize_window_plan_host(d, window, 1)
        assert p.inner.fused and p.inner.K == full.inner.K and p.inner.strips == strips, window
        assert p.inner.chunks * p.inner.rows_per_chunk >= h and (p.inner.chunks - 1) * p.inner.rows_per_chunk < h
        assert p.inner.ring_rows <= full.inner.ring_rows and p.inner.lds_bytes <= full.inner.lds_bytes
        # the rows the window's vertical taps read: fewer than the full request's
        assert (p.mid_row0, p.mid_rows) == (fv[y0], fv[y0 + h - 1] + cv[y0 + h - 1] - fv[y0]), window
        assert p.mid_rows < full.mid_rows
        assert (p.fx, p.fy, p.pass_h, p.pass_v) == (1, 1, 1, 1)
    # the plan of a window is the plan of a request of the window's size would get from the same tables: same strips and
    # chunks as a 300 x 37 output
    p = L.resize_window_plan_host(d, (250, 5, 300, 37), 1)
    q = L.resize_plan_host(L.resize_desc(211, 163, 300, 37, 3), 1)
    assert (p.inner.strips, p.inner.chunks, p.inner.rows_per_chunk) == (q.strips, q.chunks, q.rows_per_chunk)
    # a downscale whose ring does not fit for the full height... still plans by the window: mid_rows follows
    d = L.resize_desc(300, 200, 97, 61, 3)
    full = L.resize_window_plan_host(d, None, 1)
    p = L.resize_window_plan_host(d, (30, 20, 40, 3), 1)
    assert p.mid_rows < full.mid_rows / 3 and p.mid_row0 > 0
    # one pass or none: nothing to fuse and no intermediate, with a window as without
    for dargs in ((97, 41, 55, 41, 1), (97, 41, 97, 90, 1), (40, 30, 40, 30, 3)):
        d = L.resize_desc(*dargs)
        p = L.resize_window_plan_host(d, (3, 4, 20, 10), 1)
        assert not p.inner.fused and (p.mid_row0, p.mid_rows) == (0, 0)
        assert (p.pass_h, p.pass_v) == (int(dargs[0] != dargs[2]), int(dargs[1] != dargs[3]))


# ---- the tensor validators ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elem", [4, 2])
def test_tensor_validators_use_the_windows_extent(elem):
    d = L.resize_desc(211, 163, 600, 70, 3)
    lut = np.zeros((3, 256), dtype=np.float32 if elem == 4 else np.uint16)
    make = L.tensor_out if elem == 4 else L.tensor16_out
    validate = L.resize_tensor_validate if elem == 4 else L.resize_tensor16_validate
    window = (250, 5, 300, 37)
    for layout in ("chw", "hwc"):
        tight_win = make(lut.ctypes.data, L.tensor_strides(layout, 300, 37, 3))
        tight_full = make(lut.ctypes.data, L.tensor_strides(layout, 600, 70, 3))
        # legal for w x h, overlapping for out_w x out_h: accepted with the window, refused without it and with the whole one
        assert _code(validate, d, tight_win, window=window) == L.OK, layout
        assert _code(validate, d, tight_win) == L.ERR_BAD_ARG, layout
        assert _code(validate, d, tight_win, window=(0, 0, 600, 70)) == L.ERR_BAD_ARG, layout
        # the full frame's strides name a slice of a larger tensor: fine for both
        assert _code(validate, d, tight_full, window=window) == L.OK, layout
        assert _code(validate, d, tight_full) == L.OK, layout
    # overlapping for the window itself
    assert _code(validate, d, make(lut.ctypes.data, (300 * 37, 299, 1)), window=window) == L.ERR_BAD_ARG
    assert _code(validate, d, make(lut.ctypes.data, (300 * 37 - 1, 300, 1)), window=window) == L.ERR_BAD_ARG
    # a window of one row or one column: that axis' stride takes no part
    assert _code(validate, d, make(lut.ctypes.data, (300, 1, 1)), window=(250, 5, 300, 1)) == L.OK
    assert _code(validate, d, make(lut.ctypes.data, (37, 1, 1)), window=(250, 5, 1, 37)) == L.OK
    # a bad window, a null table and reserved words are refused as ever
    assert _code(validate, d, tight_win, window=_raw(250, 5, 400, 37)) == L.ERR_BAD_ARG
    assert _code(validate, d, make(None, (300 * 37, 300, 1)), window=window) == L.ERR_BAD_ARG
    t = make(lut.ctypes.data, (300 * 37, 300, 1))
    t.reserved[2] = 1
    assert _code(validate, d, t, window=window) == L.ERR_BAD_ARG
    assert _code(validate, L.resize_desc(211, 163, 600, 70, 3, bits=16), tight_win, window=window) == L.ERR_UNSUPPORTED


# ---- the fixture ------------------------------------------------------------------------------------------------------

def test_fixture_is_small_and_covers_what_it_has_to():
    assert os.path.getsize(GOLDEN) < 64 * 1024
    cases = G.load()
    assert len(cases) >= 12
    assert {c[1] for c in G.CASES} == {"L", "RGB", "RGBX", "RGBA", "I;16", "F"}
    assert {"lanczos", "bicubic", "box", "nearest"} <= {c[2] for c in G.CASES}
    assert any(c[7] is not None and not all(float(v).is_integer() for v in c[7]) for c in G.CASES)   # a fractional box
    assert any(c[8] == 2.0 for c in G.CASES)
    for name, (case, img, out) in cases.items():
        _, mode, filt, iw, ih, ow, oh, box, gap, (x0, y0, w, h) = case
        assert out.shape[:2] == (h, w) and out.dtype == img.dtype, name
        assert 0 <= x0 and x0 + w <= ow and 0 <= y0 and y0 + h <= oh, name
        assert ow * oh < 20000, name
        if gap is not None:
            fx, fy = F.gap_plan(G.FILTERS.index(filt), iw, ih, ow, oh, box, gap)[:2]
            assert fx > 1 and fy > 1, name


def test_fixture_equals_the_models_sliced_to_the_window():
    for name, (case, img, out) in G.load().items():
        assert G.same(G.model_resize_crop(img, case), out), name


def test_fixture_equals_the_model_of_the_windows_source_rectangle():
    """tests/resize_window_model.py computes chosen output rows and columns from the source rectangle they read: a window is
    such a choice, and the rectangle the library reports is the one that model fetches"""
    for name, (case, img, out) in G.load().items():
        _, mode, filt, iw, ih, ow, oh, box, gap, (x0, y0, w, h) = case
        if gap is not None:
            continue                                               # that model has no reduction
        c = G.CHANNELS[mode]
        x = img.reshape(ih, iw, c)
        fetched = []

        def fetch(r0, r1, c0, c1):
            fetched.append((c0, r0, c1, r1))
            return x[r0:r1, c0:c1]

        got = W.resize(fetch, iw, ih, ow, oh, c, img.dtype, np.arange(y0, y0 + h), np.arange(x0, x0 + w), 3,
                       G.FILTERS.index(filt), mode == "RGBA", box)
        assert G.same(got.reshape(out.shape), out), name
        d = L.resize_desc(iw, ih, ow, oh, c, alpha=mode == "RGBA", bits=16 if mode == "I;16" else 8, f32=mode == "F",
                          filter=filt)
        assert [L.resize_window_source(d, (x0, y0, w, h), box=box)] == fetched, name


def test_pillow_still_equals_the_fixture():
    pytest.importorskip("PIL")
    for name, (case, img, out) in G.load().items():
        assert G.same(G.pillow_resize_crop(img, case), out), name
