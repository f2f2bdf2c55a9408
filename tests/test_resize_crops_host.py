"""Host-side checks of a tensor view with a crop origin per frame (lanczos_resize_crops, lanczos_resize_crops_*,
lanczos_resize_tensor_crops_*; include/lanczos_hip.h): every refusal of the two validators, the plan that holds for every origin
against the window plans at every origin, and the numpy model against Pillow's fixture.  No GPU.  (The host ENTRY's refusal of
an origin outside the output needs a context, and is in tests/test_resize_crops_gpu.py.)"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_crops_model as RC
import resize_tensor_model as T32
import resize_tensor_view_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 9, 7          # the output of the refusal tests
CW, CH = 5, 4        # ... and its crops
MAX_LDS = 80 * 1024

# (in_w, in_h, out_w, out_h, channels, crop w, crop h): the three requests of DESIGN.md 4.5's table, one with four channels and a
# last block of three rows, and K = 25 near the LDS limit
PLAN_SHAPES = [(500, 375, 341, 256, 3, 224, 224), (496, 97, 300, 43, 3, 259, 27), (392, 61, 100, 43, 4, 71, 27),
               (200, 37, 90, 75, 4, 71, 51), (1018, 120, 300, 43, 3, 259, 27)]
# the window at (0, 0) is fused, the crops are not: found with the two plan queries over in_h = 150 .. 700 of the last shape
NOT_FITTING = (1018, 367, 300, 43, 3, 259, 11)


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize_crops_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_crops_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _crops(w=CW, h=CH, d_origin=4):
    return L.resize_crops(w, h, d_origin)


def _code(desc, crops):
    return L._lib().lanczos_resize_crops_validate(ctypes.byref(desc), ctypes.byref(crops) if crops is not None else None)


def _tcode(desc, crops, v):
    return L._lib().lanczos_resize_tensor_crops_validate(ctypes.byref(desc), ctypes.byref(crops) if crops is not None else None,
                                                         ctypes.byref(v) if v is not None else None)


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.ResizeCrops) == 4 + 4 + 8 + 4 * 4
    assert (L.ResizeCrops.w.offset, L.ResizeCrops.h.offset, L.ResizeCrops.d_origin.offset, L.ResizeCrops.reserved.offset) == (0, 4, 8, 16)
    for name in ("lanczos_resize_crops_validate", "lanczos_resize_crops_plan_host", "lanczos_resize_tensor_crops_validate",
                 "lanczos_resize_tensor_crops_device", "lanczos_resize_tensor_crops_host"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name)


def test_crops_refusals():
    d = L.resize_desc(20, 20, W, H, 3)
    assert _code(d, _crops()) == L.OK
    assert _code(d, _crops(W, H)) == L.OK and _code(d, _crops(1, 1)) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG                                   # a null struct
    for w, h in ((0, CH), (-1, CH), (W + 1, CH), (CW, 0), (CW, -3), (CW, H + 1), (1 << 20, 1 << 20)):
        assert _code(d, _crops(w, h)) == L.ERR_BAD_ARG, (w, h)
    assert _code(d, _crops(d_origin=None)) == L.ERR_BAD_ARG                  # no origins
    for off in (1, 2, 3):
        assert _code(d, _crops(d_origin=8 + off)) == L.ERR_BAD_ARG           # int32 pairs lie on a dword
    for i in range(4):
        c = _crops()
        c.reserved[i] = 1
        assert _code(d, c) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert _code(bad, _crops()) == L.ERR_BAD_ARG                             # what lanczos_resize_validate refuses
    with pytest.raises(L.LanczosError) as e:
        L.resize_crops_validate(d, _crops(W + 1, CH))
    assert e.value.code == L.ERR_BAD_ARG
    L.resize_crops_validate(d, _crops())
    # the plan query refuses the same, a frame count below 1 and a null result
    lib = L._lib()
    p = L.ResizePlanEx()
    for crops, frames, out, want in ((_crops(), 1, p, L.OK), (_crops(W + 1, CH), 1, p, L.ERR_BAD_ARG), (_crops(), 0, p, L.ERR_BAD_ARG),
                                     (_crops(), 1, None, L.ERR_BAD_ARG), (_crops(d_origin=None), 1, p, L.ERR_BAD_ARG)):
        got = lib.lanczos_resize_crops_plan_host(ctypes.byref(d), None, ctypes.byref(crops), frames,
                                                 ctypes.byref(out) if out is not None else None)
        assert got == want, (crops.w, frames)
    assert lib.lanczos_resize_crops_plan_host(ctypes.byref(d), None, None, 1, ctypes.byref(p)) == L.ERR_BAD_ARG


def test_tensor_crops_refusals_judge_the_view_on_the_crop():
    """everything the view validator refuses, with (w, h) as the frame the strides describe"""
    d = L.resize_desc(20, 20, W, H, 3)
    chw = L.tensor_strides("chw", CW, CH, 3)
    ident = (0, 1, 2)
    view = lambda st, src=ident, **kw: L.tensor_view(kw.pop("lut", 1), st, kw.pop("elem", 4), src, **kw)
    assert _tcode(d, _crops(), view(chw)) == L.OK
    assert _tcode(d, _crops(), view(L.tensor_strides("hwc", CW, CH, 3))) == L.OK
    assert _tcode(d, None, view(chw)) == L.ERR_BAD_ARG and _tcode(d, _crops(), None) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(W + 1, CH), view(chw)) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(d_origin=None), view(chw)) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(), view(chw, lut=None)) == L.ERR_BAD_ARG
    # strides sized for the crop are accepted; one element less in a row or a plane of the CROP overlaps
    assert _tcode(d, _crops(), view((CH * CW - 1, CW, 1))) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(), view((CH * CW, CW - 1, 1))) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(), view((1, CW * 3 - 1, 3))) == L.ERR_BAD_ARG
    # ... and strides that only fit because the frame is the crop and not the whole output
    assert _tcode(d, _crops(), view(chw)) == L.OK and L._lib().lanczos_resize_tensor_view_validate(
        ctypes.byref(d), None, ctypes.byref(view(chw))) == L.ERR_BAD_ARG
    for i in range(3):
        for bad in (0, -1, (1 << 40) + 1):
            st = list(chw)
            st[i] = bad
            assert _tcode(d, _crops(), view(st)) == L.ERR_BAD_ARG, st
    for elem in (0, 1, 3, 8):
        assert _tcode(d, _crops(), view(chw, elem=elem)) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(), view(chw, elem=2)) == L.OK
    for src in ((0, 1, 3), (0, 0, 1), (1, 1), ()):
        assert _tcode(d, _crops(), view(chw, src)) == L.ERR_BAD_ARG, src
    assert _tcode(d, _crops(), view(chw, (2, 0))) == L.OK
    for flip in (4, -1):
        assert _tcode(d, _crops(), view(chw, flip=flip)) == L.ERR_BAD_ARG
    assert _tcode(d, _crops(), view(chw, (2, 1, 0), flip="hv", d_flip=1)) == L.OK
    v = view(chw)
    v.reserved[2] = 1
    assert _tcode(d, _crops(), v) == L.ERR_BAD_ARG
    # sample widths without a table
    assert _tcode(L.resize_desc(20, 20, W, H, 3, bits=16), _crops(), view(chw)) == L.ERR_UNSUPPORTED
    assert _tcode(L.resize_desc(20, 20, W, H, 3, f32=True), _crops(), view(chw)) == L.ERR_UNSUPPORTED
    assert _tcode(L.resize_desc(20, 20, W, H, 4, alpha=True), _crops(), view(chw)) == L.OK
    with pytest.raises(L.LanczosError) as e:
        L.resize_crops_validate(d, _crops(), view((1, 1, 1)))
    assert e.value.code == L.ERR_BAD_ARG
    L.resize_crops_validate(d, _crops(), view(chw))


def _window_plans(d, w, h, frames):
    """the window plans along each axis: stage_dw depends on x0 alone and ring_rows on y0 alone (checked on a sample below)"""
    xs = [L.resize_window_plan_host(d, (x, 0, w, h), frames) for x in range(d.out_w - w + 1)]
    ys = [L.resize_window_plan_host(d, (0, y, w, h), frames) for y in range(d.out_h - h + 1)]
    return xs, ys


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_the_plan_holds_for_every_origin(shape):
    iw, ih, ow, oh, c, w, h = shape
    frames = 5
    d = L.resize_desc(iw, ih, ow, oh, c)
    got = L.resize_crops_plan_host(d, (w, h), frames)
    xs, ys = _window_plans(d, w, h, frames)
    rng = np.random.default_rng(ow)
    for _ in range(40):                      # the two sizes do not depend on the other axis' origin
        x, y = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
        p = L.resize_window_plan_host(d, (x, y, w, h), frames).inner
        assert (p.stage_dw, p.ring_rows) == (xs[x].inner.stage_dw, ys[y].inner.ring_rows), (x, y)
    assert all(p.inner.fused for p in xs + ys) and got.inner.fused == 1
    stage_dw, ring_rows = max(p.inner.stage_dw for p in xs), max(p.inner.ring_rows for p in ys)
    assert (got.inner.stage_dw, got.inner.ring_rows) == (stage_dw, ring_rows)
    # the list shows something: some origin's plan is strictly smaller than the one that holds for all
    assert min(p.inner.stage_dw for p in xs) < stage_dw or min(p.inner.ring_rows for p in ys) < ring_rows
    for p in xs + ys:                        # what depends on (w, h) and the frame count alone
        for name in ("K", "strips", "rows_per_chunk", "chunks"):
            assert getattr(got.inner, name) == getattr(p.inner, name), name
        for name in ("fx", "fy", "reduced_w", "reduced_h", "pass_h", "pass_v"):
            assert getattr(got, name) == getattr(p, name), name
    # stage_rows and the LDS sum follow from the maxima by the rule of the window plan
    sw = 64 if c == 4 else 256
    assert got.inner.lds_bytes == ring_rows * sw * c + got.inner.stage_rows * stage_dw * 4 <= MAX_LDS
    assert 4 <= got.inner.stage_rows <= min(p.inner.stage_rows for p in xs + ys)
    grow = ring_rows * sw * c + (got.inner.stage_rows + 1) * stage_dw * 4
    assert got.inner.stage_rows == max(p.inner.stage_rows for p in xs + ys) or grow > MAX_LDS
    # the whole output's intermediate: what the converted route computes
    whole = L.resize_window_plan_host(d, None, frames)
    assert (got.mid_row0, got.mid_rows) == (whole.mid_row0, whole.mid_rows)
    # a ResizeCrops works as (w, h) does, and d_origin is not read
    again = L.resize_crops_plan_host(d, L.resize_crops(w, h, 4), frames)
    assert bytes(again) == bytes(got)


def test_the_first_shape_is_the_documented_one():
    """500x375 -> 341x256 RGB, crops of 224x224: stage_dw 253 at (0, 0), 256 at 111 of 118 x origins"""
    d = L.resize_desc(500, 375, 341, 256, 3)
    xs, ys = _window_plans(d, 224, 224, 256)
    assert xs[0].inner.stage_dw == 253 and [p.inner.stage_dw for p in xs].count(256) == 111 and len(xs) == 118
    rr = [p.inner.ring_rows for p in ys]
    assert len(ys) == 33 and rr.count(max(rr)) == 29
    assert L.resize_crops_plan_host(d, (224, 224), 256).inner.stage_dw == 256


def test_maxima_that_do_not_fit_are_not_fused():
    """the window at (0, 0) fits 80 KiB, the largest over every origin does not: the request takes the converted route"""
    iw, ih, ow, oh, c, w, h = NOT_FITTING
    d = L.resize_desc(iw, ih, ow, oh, c)
    assert L.resize_window_plan_host(d, (0, 0, w, h), 5).inner.fused == 1
    xs, ys = _window_plans(d, w, h, 5)
    assert not all(p.inner.fused for p in ys)
    got = L.resize_crops_plan_host(d, (w, h), 5)
    assert got.inner.fused == 0 and got.inner.lds_bytes == 0 and (got.pass_h, got.pass_v) == (1, 1)


def test_requests_without_a_fused_plan():
    """one idle axis, both idle, NEAREST: the crops plan is the window plan's, not fused"""
    for iw, ih, ow, oh, filt in ((97, 41, 55, 41, "lanczos"), (45, 80, 45, 37, "lanczos"), (43, 30, 43, 30, "lanczos"),
                                 (83, 61, 131, 40, "nearest")):
        d = L.resize_desc(iw, ih, ow, oh, 3, filter=filt)
        got = L.resize_crops_plan_host(d, (20, 17), 3)
        want = L.resize_window_plan_host(d, None, 3)
        assert got.inner.fused == 0 and (got.pass_h, got.pass_v) == (want.pass_h, want.pass_v)
    # a gap reduces in front, and the plan is that of the resize that remains
    d = L.resize_desc(400, 300, 50, 38, 3)
    got = L.resize_crops_plan_host(d, (24, 20), 5, reducing_gap=2.0)
    assert (got.fx, got.fy, got.inner.fused) == (4, 3, 1)


def test_the_model_clamps_and_slices():
    full = np.arange(3 * 6 * 8 * 2, dtype=np.uint8).reshape(3, 6, 8, 2)
    o = RC.clamp([(-3, 1), (9, -1), (2, 7)], 8, 6, 5, 4)
    assert o.tolist() == [[0, 1], [3, 0], [2, 2]]
    s = RC.slices(full, 5, 4, [(-3, 1), (9, -1), (2, 7)])
    assert s.shape == (3, 4, 5, 2)
    assert np.array_equal(s[0], full[0, 1:5, 0:5]) and np.array_equal(s[1], full[1, 0:4, 3:8]) and np.array_equal(s[2], full[2, 2:6, 2:7])
    lut = T32.identity_lut(2)
    got = RC.crops(full, lut, 5, 4, o, (1, 0), [0, 1, 2])
    assert np.array_equal(got, V.view(s, lut, (1, 0), [0, 1, 2]))


def test_the_model_reproduces_pillows_fixture():
    """Image.resize(...).crop(frame's window).transpose(frame's flip), five frames a case: the numpy models of the full resize,
    sliced per frame and mirrored, byte for byte -- and the words of the contract name exactly those bytes"""
    G = _golden()
    cases = G.load()
    assert len(cases) == 12 and {c[1] for c, *_ in cases.values()} == {"L", "RGB", "RGBX", "RGBA"}
    for name, (case, imgs, origins, flips, want) in cases.items():
        w, h = case[9]
        assert G.same(G.model_crops(imgs, origins, flips, case), want), name
        full = G.model_full(imgs, case)
        c = full.shape[-1]
        lut = T32.identity_lut(c)
        words = RC.crops(full, lut, w, h, origins, None, flips, "hwc")
        want4 = want[..., None] if want.ndim == 3 else want
        assert np.array_equal(words & 0xff, want4) and np.array_equal((words >> 8) & 0xff, np.broadcast_to(np.arange(c), words.shape))


def test_python_argument_checks():
    c = L.resize_crops(224, 200, 64)
    assert (c.w, c.h, c.d_origin, list(c.reserved)) == (224, 200, 64, [0] * 4)
