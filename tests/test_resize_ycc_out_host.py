"""Host checks of lanczos_resize_ycc_out (no GPU): the ABI, lanczos_ycc_dest_init / _validate and every refusal the entry makes
before it touches a device, the three forward tables -- JFIF against the installed Pillow over all 2^24 (R, G, B) triples, the
limited-range ones against their formula and the float64 matrix -- and the numpy model (tests/resize_ycc_out_model.py) against
Pillow's committed fixture and against the installed Pillow."""
import ctypes
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_ycc_model as Y
import resize_ycc_out_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc_out.npz")
W, H, OW, OH = 37, 23, 22, 14


def _desc(c=3, **kw):
    return L.resize_desc(W, H, OW, OH, c, **kw)


def _code(d, t, win=None):
    return L._lib().lanczos_ycc_dest_validate(ctypes.byref(d) if d is not None else None, ctypes.byref(win) if win is not None else None,
                                              ctypes.byref(t) if t is not None else None)


def _win(d, x0, y0, w, h):
    return L.resize_window(d, (x0, y0, w, h))


def test_abi_structs_match_the_header():
    T = L.YccDest
    assert ctypes.sizeof(T) == ctypes.sizeof(L.YccSource) == 4 * 8 + 3 * 4 + 5 * 4
    assert (T.y_row_stride.offset, T.c_row_stride.offset, T.cb_offset.offset, T.cr_offset.offset) == (0, 8, 16, 24)
    assert (T.layout.offset, T.sub_x.offset, T.sub_y.offset, T.reserved.offset) == (32, 36, 40, 44)
    R = L.YccOutRequest
    assert ctypes.sizeof(R) == 8 * 8 + 2 * 4 + 3 * 8 + 4 * 4
    assert [getattr(R, n).offset for n in ("d", "opts", "win", "src", "dst", "table", "in_", "out")] == list(range(0, 64, 8))
    assert (R.frames.offset, R.memory.offset, R.in_frame_stride.offset, R.out_frame_stride.offset, R.stream.offset,
            R.reserved.offset) == (64, 68, 72, 80, 88, 96)
    assert ctypes.sizeof(L.YccOutInfoC) == 8 * 4 and L.YccOutInfoC.launches.offset == 20
    assert (L.MEM_DEVICE, L.MEM_HOST) == (0, 1)
    with open(os.path.join(ROOT, "include", "lanczos_hip.h")) as f:
        header = f.read()
    assert "#define LANCZOS_MEM_DEVICE 0" in header and "#define LANCZOS_MEM_HOST 1" in header
    for name in ("lanczos_ycc_dest_init", "lanczos_ycc_dest_validate", "lanczos_ycc_table_forward", "lanczos_resize_ycc_out",
                 "lanczos_last_ycc_out_info"):
        assert name in header and name in L.ABI_SYMBOLS and name in L._SIGNATURES and getattr(L._lib(), name).argtypes, name
    # the launching entry keeps out of the suffix pattern tests/test_binding_calls.py pins
    assert not any(n.endswith(s) for n in ("lanczos_resize_ycc_out", "lanczos_last_ycc_out_info")
                   for s in ("_host", "_device", "_host_ex", "_device_ex"))
    assert L._lib().lanczos_last_ycc_out_info(None, None) == L.ERR_BAD_ARG


@pytest.mark.parametrize("win", [None, (0, 0, 22, 14), (2, 4, 7, 5), (20, 12, 1, 1)])
def test_init_is_the_tight_layout_of_the_stored_frame(win):
    d = _desc()
    w, h = (OW, OH) if win is None else win[2:]
    wref = ctypes.byref(_win(d, *win)) if win is not None else None
    for sx in (0, 1):
        for sy in (0, 1):
            cw, ch = M.out_chroma_size(w, h, sx, sy)
            t = L.YccDest()
            for i in range(5):
                t.reserved[i] = 9                                  # init clears them
            assert L._lib().lanczos_ycc_dest_init(ctypes.byref(t), ctypes.byref(d), wref, L.YCC_PLANAR, sx, sy) == L.OK
            assert (t.y_row_stride, t.c_row_stride, t.cb_offset, t.cr_offset) == (w, cw, w * h, w * h + cw * ch)
            assert (t.layout, t.sub_x, t.sub_y, list(t.reserved)) == (L.YCC_PLANAR, sx, sy, [0] * 5)
            assert L.ycc_dest_frame_bytes(d, t, win) == w * h + 2 * cw * ch
            for layout in (L.YCC_NV12, L.YCC_NV21):
                rc = L._lib().lanczos_ycc_dest_init(ctypes.byref(t), ctypes.byref(d), wref, layout, sx, sy)
                if sx != 1:
                    assert rc == L.ERR_BAD_ARG
                    continue
                assert rc == L.OK and (t.y_row_stride, t.c_row_stride, t.cb_offset, t.cr_offset) == (w, 2 * cw, w * h, w * h)
    for name, (layout, sx, sy) in L.YCC_LAYOUTS.items():
        t = L.ycc_dest(d, name, win)
        assert (t.layout, t.sub_x, t.sub_y) == (layout, sx, sy) and L.ycc_dest_chroma_size(d, t, win) == M.out_chroma_size(w, h, sx, sy)


def test_init_refusals():
    d = _desc()
    assert L._lib().lanczos_ycc_dest_init(None, ctypes.byref(d), None, 0, 1, 1) == L.ERR_BAD_ARG
    assert L._lib().lanczos_ycc_dest_init(ctypes.byref(L.YccDest()), None, None, 0, 1, 1) == L.ERR_BAD_ARG
    for layout, sx, sy in ((3, 1, 1), (-1, 1, 1), (0, 2, 0), (0, 0, 2), (0, -1, 0), (0, 1, -1), (1, 0, 1), (2, 0, 0)):
        assert L._lib().lanczos_ycc_dest_init(ctypes.byref(L.YccDest()), ctypes.byref(d), None, layout, sx, sy) == L.ERR_BAD_ARG
    bad = L.ResizeWindow()
    bad.x0, bad.y0, bad.w, bad.h = 20, 0, 3, 3                     # leaves the output
    assert L._lib().lanczos_ycc_dest_init(ctypes.byref(L.YccDest()), ctypes.byref(d), ctypes.byref(bad), 0, 1, 1) == L.ERR_BAD_ARG


def test_validate_refusals_by_code():
    d = _desc()
    cw, ch = M.out_chroma_size(OW, OH, 1, 1)

    def mk(name, **kw):
        t = L.ycc_dest(d, name)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    planar, nv = (lambda **kw: mk("i420", **kw)), (lambda **kw: mk("nv12", **kw))
    assert _code(d, planar()) == L.OK and _code(d, nv()) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG and _code(None, planar()) == L.ERR_BAD_ARG
    # pitched and spaced planes at any residue are fine
    assert _code(d, planar(y_row_stride=29, c_row_stride=13, cb_offset=29 * OH + 3, cr_offset=29 * OH + 3 + 13 * ch + 1)) == L.OK
    assert _code(d, planar(cb_offset=OW * OH + cw * ch, cr_offset=OW * OH)) == L.OK                 # Cr in front of Cb
    assert _code(d, nv(y_row_stride=29, c_row_stride=25, cb_offset=29 * OH + 1, cr_offset=29 * OH + 1)) == L.OK
    bad = [planar(layout=3), planar(layout=-1),                                                     # an unknown layout
           planar(sub_x=2), planar(sub_y=-1),                                                       # a subsampling other than 0 or 1
           nv(sub_x=0), nv(layout=L.YCC_NV21, sub_x=0), nv(cr_offset=OW * OH + 1),                  # NV: sub_x != 1, two offsets
           planar(y_row_stride=OW - 1), planar(c_row_stride=cw - 1), nv(c_row_stride=2 * cw - 1), planar(y_row_stride=0),
           planar(y_row_stride=(1 << 40) + 1), planar(c_row_stride=(1 << 40) + 1),                  # strides
           planar(cb_offset=-1), planar(cr_offset=-1), nv(cb_offset=-1, cr_offset=-1),              # negative offsets
           planar(cb_offset=OW * OH - 1), planar(cr_offset=OW * OH + cw * ch - 1), planar(cr_offset=OW * OH),
           planar(y_row_stride=OW + 1), nv(cb_offset=OW * OH - 1, cr_offset=OW * OH - 1)]           # overlapping planes
    for i, t in enumerate(bad):
        assert _code(d, t) == L.ERR_BAD_ARG, i
    for i in range(5):
        t = planar()
        t.reserved[i] = 1
        assert _code(d, t) == L.ERR_BAD_ARG, i
    # the window's origin against the destination's subsampling; sizes may be odd
    for name, ok, refused in (("i420", [(2, 4), (0, 0), (20, 12)], [(1, 0), (0, 1), (3, 3)]),
                              ("i422", [(2, 1), (0, 3)], [(1, 0), (3, 2)]), ("i444", [(1, 1), (3, 2)], []),
                              ("nv12", [(4, 2)], [(1, 2), (2, 1)])):
        for x0, y0 in ok:
            win = _win(d, x0, y0, 1, 1)
            assert _code(d, L.ycc_dest(d, name, win), win) == L.OK, (name, x0, y0)
        for x0, y0 in refused:
            win = _win(d, x0, y0, 1, 1)
            assert _code(d, L.ycc_dest(d, name, win, aligned=False), win) == L.ERR_BAD_ARG, (name, x0, y0)
            with pytest.raises(L.LanczosError):
                L.ycc_dest(d, name, win)
    # the descriptor: three channels; alpha, 16-bit and float samples are not built
    for c in (1, 4):
        assert _code(_desc(c), planar()) == L.ERR_BAD_ARG
    for kw in ({"bits": 16}, {"f32": True}):
        assert _code(_desc(**kw), planar()) == L.ERR_UNSUPPORTED, kw
    da = _desc()
    da.reserved[0] |= L.RESIZE_ALPHA
    assert _code(da, planar()) == L.ERR_UNSUPPORTED
    for filt in L.FILTER_NAMES:
        assert _code(_desc(filter=filt), planar()) == L.OK, filt


def test_entry_refusals_before_any_device_work():
    """what lanczos_resize_ycc_out refuses from its arguments alone, on a null context first: nothing here needs a device"""
    d = _desc()
    t = L.ycc_dest(d, "nv12")
    buf = np.zeros(4096, np.uint8)
    rq = L.ycc_out_request(d, t, buf.ctypes.data, buf.ctypes.data, 1, L.ycc_source(d, "nv12"))
    assert L._lib().lanczos_resize_ycc_out(None, ctypes.byref(rq)) == L.ERR_BAD_ARG
    assert "lanczos_resize_ycc_out" not in __import__("binding_calls_cfg").launching(L)


def test_forward_table_refusals():
    t = np.zeros((3, 3, 256), np.int32)
    assert L._lib().lanczos_ycc_table_forward(0, None) == L.ERR_BAD_ARG
    for std in (-1, 3, 99):
        assert L._lib().lanczos_ycc_table_forward(std, t.ctypes.data) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.ycc_table_forward("bt2020")


def _all_rgb():
    """a 4096 x 4096 RGB image holding every (R, G, B) once"""
    return np.stack(Y.all_triples(), -1)


def test_jfif_forward_table_is_pillows_convert_over_all_triples():
    from PIL import Image
    rgb = _all_rgb()
    t = L.ycc_table_forward("jfif")
    assert t.dtype == np.int32 and t.shape == (3, 3, 256) and np.array_equal(t, M.forward_table(M.JFIF))
    want = np.asarray(Image.fromarray(rgb, "RGB").convert("YCbCr"))
    got = M.convert(t, rgb)
    for c in range(3):
        diff = int((got[c] != want[..., c]).sum())
        assert diff == 0, (c, diff)


@pytest.mark.parametrize("name,std", [("bt601", M.BT601), ("bt709", M.BT709)])
def test_limited_range_forward_tables(name, std):
    t = L.ycc_table_forward(name)
    assert np.array_equal(t, M.forward_table(std)) and np.array_equal(t, L.ycc_table_forward(std))
    assert int(t[0, 0, 0]) == 16 * 64 + 32 and int(t[1, 0, 0]) == int(t[2, 0, 0]) == 128 * 64 + 32   # the offsets ride on R
    rgb = _all_rgb()
    worst = 0
    for r0 in range(0, 4096, 512):
        s = slice(r0, r0 + 512)
        got = np.stack(M.convert(t, rgb[s]), -1).astype(np.int16)
        want = M.forward_matrix_f64(std, rgb[s][..., 0], rgb[s][..., 1], rgb[s][..., 2]).astype(np.int16)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst
    corners = np.array([[0, 0, 0], [255, 255, 255], [0, 0, 255], [255, 255, 0], [255, 0, 0], [0, 255, 255]], dtype=np.uint8)
    y, cb, cr = M.convert(t, corners)                               # black, white, blue, yellow, red, cyan: the range's ends
    assert (y[0], cb[0], cr[0]) == (16, 128, 128) and (y[1], cb[1], cr[1]) == (235, 128, 128)
    assert (cb[2], cb[3], cr[4], cr[5]) == (240, 16, 240, 16)


def test_reduce_rule_is_pillows_reduce_on_odd_and_even_frames():
    from PIL import Image
    rng = np.random.default_rng(4)
    for w, h in ((37, 23), (36, 22), (1, 1), (2, 1), (1, 2), (2, 2), (5, 1)):
        p = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for sx, sy in ((1, 1), (1, 0), (0, 1), (0, 0)):
            want = np.asarray(Image.fromarray(p, "L").reduce((1 << sx, 1 << sy))) if sx or sy else p
            assert np.array_equal(M.reduce_plane(p, sx, sy), want), (w, h, sx, sy)


def test_model_reproduces_pillows_fixture():
    z = np.load(GOLDEN)
    for k, p in zip(("y", "cb", "cr"), M.make_planes(M.CASES[0])):
        assert np.array_equal(z[f"input_check_{k}"], p), k          # the seeded generators are the fixture's
    assert np.array_equal(z["input_check_rgb"], M.make_rgb(M.RGB_CASES[1]))
    pairs = set()
    for c in M.CASES:
        got = M.compose_case(c, M.make_planes(c))
        ocw, och = M.out_chroma_size(c.out_w, c.out_h, c.dsx, c.dsy)
        for k, (name, shape) in enumerate((("y", (c.out_h, c.out_w)), ("cb", (och, ocw)), ("cr", (och, ocw)))):
            want = z[f"{c.name}_{name}"]
            assert got[k].shape == want.shape == (M.FRAMES,) + shape and np.array_equal(got[k], want), (c.name, name)
        pairs.add((c.ssx, c.ssy, c.dsx, c.dsy))
    assert len(pairs) == 9
    for c in M.RGB_CASES:
        x = M.make_rgb(c)
        for sub, (dsx, dsy) in M.SUBS.items():
            got = M.rgb_to_ycc(x, dsx, dsy, c.out_w, c.out_h, c.filt)
            for k, key in enumerate((f"{c.name}_y", f"{c.name}_{sub}_cb", f"{c.name}_{sub}_cr")):
                assert got[k].shape == z[key].shape and np.array_equal(got[k], z[key]), key
    # the contents do what they are there for: the gapped case reduces both planes, the blocks reach the ends of the outputs' range
    import resize_filters_model as F
    c = M.CASE["420_to_420_gap2"]
    assert F.gap_plan(0, c.in_w, c.in_h, c.out_w, c.out_h, None, 2.0)[:2] == (4, 4)
    assert F.gap_plan(0, 41, 25, 5, 3, None, 2.0)[:2] == (4, 4)
    assert z["rgb_up_y"].min() == 0 and z["rgb_up_y"].max() >= 254 and z["rgb_up_444_cb"].min() <= 1 and z["rgb_up_444_cr"].max() >= 254


def test_model_equals_installed_pillow():
    """live: windows, the source's box scaling, and RGB windows at odd origins with every subsampling"""
    from PIL import Image
    c = M.CASE["420_to_444_box"]
    y, cb, cr = M.make_planes(c, 1)
    got = M.compose_case(c, (y, cb, cr), window=(3, 2, 9, 7))
    filt = Image.Resampling.BICUBIC
    bc = Y.chroma_box(c.box, c.in_w, c.in_h, c.ssx, c.ssy)
    want = [np.asarray(Image.fromarray(p[0], "L").resize((c.out_w, c.out_h), filt, box=b))[2:9, 3:12] for p, b in ((y, c.box), (cb, bc), (cr, bc))]
    assert all(np.array_equal(g[0], w) for g, w in zip(got, want))
    rc = M.RGB_CASE["rgb_down"]
    x = M.make_rgb(rc, 1)
    for (dsx, dsy) in M.SUBS.values():
        for win in ((1, 1, 9, 7), (3, 2, 4, 4), (21, 13, 1, 1)):
            got = M.rgb_to_ycc(x, dsx, dsy, rc.out_w, rc.out_h, window=win)
            im = Image.fromarray(x[0], "RGB").resize((rc.out_w, rc.out_h), Image.Resampling.LANCZOS)
            im = im.crop((win[0], win[1], win[0] + win[2], win[1] + win[3]))
            yy, b, r = im.convert("YCbCr").split()
            if dsx or dsy:
                b, r = b.reduce((1 << dsx, 1 << dsy)), r.reduce((1 << dsx, 1 << dsy))
            assert all(np.array_equal(g[0], np.asarray(w)) for g, w in zip(got, (yy, b, r))), (dsx, dsy, win)


def test_clip_table_and_frames_do_what_they_are_there_for():
    t = M.clip_table()
    sums = lambda px: [int(t[c, 0][px[0]]) + int(t[c, 1][px[1]]) + int(t[c, 2][px[2]]) for c in range(3)]
    assert all(s > 16383 for s in sums(M.CLIP_HIGH)) and all(0 <= s <= 16383 for s in sums(M.CLIP_MID)) and all(s < 0 for s in sums(M.CLIP_LOW))
    x = M.clip_frames()
    yy, cb, cr = M.convert(t, x)
    for p in (yy, cb, cr):                                            # in a thread's dword: two clipped, two not, and the reverse
        assert (p[0, 0, 0:4] == 255)[:2].all() and (p[0, 0, 2:4] < 255).all() and (p[0, 1, 0:2] < 255).all() and (p[0, 1, 2:4] == 255).all()
        assert (p[0, 4, 0:2] == 0).all() and (p[0, 4, 2:4] > 0).all() and (p[0, 5, 2:4] == 0).all() and (p[0, 5, 0:2] > 0).all()


def test_expected_buffers_keep_the_noise_of_unnamed_bytes():
    """M.before_and_expected: the two buffers differ exactly in the bytes the layout names"""
    c = M.CASE["420_to_420_down"]
    planes = M.compose_case(c, M.make_planes(c))
    for layout, kw in (("nv12", dict(y_row_stride=29, c_row_stride=25, base=1, gap=3, frame_gap=1)), ("i420", dict(c_row_stride=13, gap=2))):
        before, want = M.before_and_expected(planes, layout, **kw)
        named = np.zeros(before.buf.shape, bool)
        cw, ch = planes[1].shape[-1], planes[1].shape[-2]
        for f in range(M.FRAMES):
            o = want.at + f * want.frame_stride
            for r in range(c.out_h):
                named[o + r * want.y_row_stride:][:c.out_w] = True
            for r in range(ch):
                if layout == "nv12":
                    named[o + want.cb_offset + r * want.c_row_stride:][:2 * cw] = True
                else:
                    named[o + want.cb_offset + r * want.c_row_stride:][:cw] = True
                    named[o + want.cr_offset + r * want.c_row_stride:][:cw] = True
        assert np.array_equal(before.buf[~named], want.buf[~named]) and (before.buf[named] != want.buf[named]).all()
        assert (~named).sum() > 2 * Y.MARGIN
