"""Host checks of lanczos_resize_ycc16 (no GPU): the numpy model (tests/resize_ycc16_model.py) against Pillow's committed fixture
and against the installed Pillow, the ABI against the header, every refusal the entry makes from its arguments alone by its code
(lanczos_ycc16_request_validate is what the entry runs before it touches a device), and lanczos_ycc16_matrix_init against its
derivation for every standard, depth, alignment and range."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor_norm_model as TN
import resize_ycc16_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc16.npz")
W, H, OW, OH = 37, 23, 22, 14
NEW = ("lanczos_ycc16_matrix_init", "lanczos_ycc16_matrix_validate", "lanczos_ycc16_source_init", "lanczos_ycc16_source_validate",
       "lanczos_ycc16_dest_init", "lanczos_ycc16_dest_validate", "lanczos_ycc16_request_validate", "lanczos_resize_ycc16",
       "lanczos_last_ycc16_info")


def _desc(c=3, bits=16, **kw):
    return L.resize_desc(W, H, OW, OH, c, bits=bits, **kw)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_model_reproduces_pillows_fixture():
    z = np.load(GOLDEN)
    for k, p in zip(("y", "cb", "cr"), M.make_planes(M.CASES[0])):
        assert np.array_equal(z[f"input_check_{k}"], p), k              # the seeded generator is the fixture's
    wrapped = 0
    for c in M.CASES:
        planes = M.make_planes(c)
        for kind, got in (("rgb", M.case_planes_rgb(c, planes)), ("ycc", M.case_planes_ycc(c, planes))):
            want = M.golden_planes(z, c, kind)
            for k in range(3):
                assert got[k].dtype == want[k].dtype == np.uint16 and got[k].shape == want[k].shape, (c.name, kind, k)
                assert np.array_equal(got[k], want[k]), (c.name, kind, k)
        sat = M.resize_plane_saturating(planes[0], c.filt, c.out_w, c.out_h, c.box)
        wrapped += int((sat != z[f"{c.name}_y"]).sum())
    assert wrapped > 100                                                 # the fixture holds words only the I;16 store explains
    assert len({(c.ssx, c.ssy, c.dsx, c.dsy) for c in M.CASES}) == 5
    assert z["420_same_y"].shape == (M.FRAMES, 22, 36) and np.array_equal(z["420_same_dcb"], M.make_planes(M.CASE["420_same"])[1])


def test_model_equals_installed_pillow():
    """live: a window with a fractional box into another subsampling, bicubic, on MSB-aligned hard edges"""
    from PIL import Image
    c = M.CASE["420_box"]._replace(filt="bicubic", content="edges_msb10", dsx=1, dsy=0)
    y, cb, cr = M.make_planes(c, 1)
    win = (2, 3, 9, 7)
    got = M.case_planes_ycc(c, (y, cb, cr), window=win)
    bc = M.chroma_box(c.box, c.in_w, c.in_h, c.ssx, c.ssy)
    ocw, och = M.out_chroma_size(c.out_w, c.out_h, 1, 0)

    def pil(p, ow, oh, b):
        return np.asarray(Image.fromarray(p, "I;16").resize((ow, oh), Image.Resampling.BICUBIC, box=b)).astype(np.uint16)
    want = [pil(y[0], c.out_w, c.out_h, c.box)[3:10, 2:11], pil(cb[0], ocw, och, bc)[3:10, 1:6], pil(cr[0], ocw, och, bc)[3:10, 1:6]]
    assert all(np.array_equal(g[0], w) for g, w in zip(got, want))
    got = M.case_planes_rgb(c, (y, cb, cr), window=win)
    want = [pil(p[0], c.out_w, c.out_h, b)[3:10, 2:11] for p, b in ((y, c.box), (cb, bc), (cr, bc))]
    assert all(np.array_equal(g[0], w) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="wrong mode"):                  # why a reducing_gap stays refused
        Image.fromarray(y[0], "I;16").reduce(2)


def test_expected_dest_keeps_the_noise_of_unnamed_words():
    c = M.CASE["420_down_odd"]
    planes = M.case_planes_ycc(c, M.make_planes(c))
    for layout, kw in (("p010", dict(y_row_stride=21, c_row_stride=23, base=1, gap=3, frame_gap=1)), ("i420", dict(c_row_stride=13, gap=2))):
        before, want = M.expected_dest(planes, layout, **kw)
        named = np.zeros(before.buf.shape, bool)
        cw, ch = planes[1].shape[-1], planes[1].shape[-2]
        for f in range(M.FRAMES):
            o = want.at + f * want.frame_stride
            for r in range(c.out_h):
                named[o + r * want.y_row_stride:][:c.out_w] = True
            for r in range(ch):
                if layout == "p010":
                    named[o + want.cb_offset + r * want.c_row_stride:][:2 * cw] = True
                else:
                    named[o + want.cb_offset + r * want.c_row_stride:][:cw] = True
                    named[o + want.cr_offset + r * want.c_row_stride:][:cw] = True
        assert np.array_equal(before.buf[~named], want.buf[~named]) and (before.buf[named] != want.buf[named]).all()
        assert (~named).sum() > 2 * M.MARGIN


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_structs_and_names_match_the_header():
    with open(os.path.join(ROOT, "include", "lanczos_hip.h")) as f:
        header = f.read()
    Mx = L.Ycc16Matrix
    assert ctypes.sizeof(Mx) == (9 + 3 + 1 + 1 + 4) * 4
    assert (Mx.k.offset, Mx.sub.offset, Mx.shift.offset, Mx.max.offset, Mx.reserved.offset) == (0, 36, 48, 52, 56)
    Rq = L.Ycc16Request
    names = ("d", "opts", "win", "src", "dst", "matrix", "norm", "in_", "out")
    assert [getattr(Rq, n).offset for n in names] == list(range(0, 72, 8))
    assert (Rq.frames.offset, Rq.memory.offset, Rq.in_frame_stride.offset, Rq.out_frame_stride.offset, Rq.stream.offset,
            Rq.reserved.offset) == (72, 76, 80, 88, 96, 104) and ctypes.sizeof(Rq) == 120
    body = re.search(r"typedef struct lanczos_ycc16_request \{(.*?)\} lanczos_ycc16_request;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[\d+\]", "", decl.split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip()]
    assert fields == ["d", "opts", "win", "src", "dst", "matrix", "norm", "in", "out", "frames", "memory", "in_frame_stride",
                      "out_frame_stride", "stream", "reserved"], fields
    assert ctypes.sizeof(L.Ycc16InfoC) == 8 * 4 and [n for n, _ in L.Ycc16InfoC._fields_[:6]] == list(L.Ycc16Info._fields)
    assert re.search(r"int32_t luma_kernel, chroma_kernel, split, join, merge, launches;\s*int32_t reserved\[2\];\s*\} lanczos_ycc16_info", header)
    assert "#define LANCZOS_YCC_BT2020 3" in header and L.YCC_BT2020 == 3 and L.YCC16_STANDARDS["bt2020"] == 3
    for name in NEW:
        assert name in header and name in L.ABI_SYMBOLS and name in L._SIGNATURES and getattr(L._lib(), name).argtypes, name
        assert not name.endswith(("_host", "_device", "_host_ex", "_device_ex")), name
    assert not set(NEW) & set(__import__("binding_calls_cfg").launching(L))
    assert "P010 / P016 are not built" not in header
    assert L._lib().lanczos_last_ycc16_info(None, None) == L.ERR_BAD_ARG
    for name in ("p010", "p016"):
        assert L.YCC16_LAYOUTS[name] == L.YCC_LAYOUTS["nv12"]
    for name in ("p210", "p216", "nv16"):
        assert L.YCC16_LAYOUTS[name] == (L.YCC_NV12, 1, 0)
    assert all(L.YCC16_LAYOUTS[k] == v for k, v in L.YCC_LAYOUTS.items())


def test_init_is_the_tight_layout_in_bytes():
    d = _desc()
    for sx, sy in itertools.product((0, 1), repeat=2):
        cw, ch = M.chroma_size(W, H, sx, sy)
        s = L.YccSource()
        assert L._lib().lanczos_ycc16_source_init(ctypes.byref(s), ctypes.byref(d), L.YCC_PLANAR, sx, sy) == L.OK
        assert (s.y_row_stride, s.c_row_stride, s.cb_offset, s.cr_offset) == (2 * W, 2 * cw, 2 * W * H, 2 * (W * H + cw * ch))
        assert L.ycc_frame_bytes(d, s) == 2 * (W * H + 2 * cw * ch)
        for layout in (L.YCC_NV12, L.YCC_NV21):
            rc = L._lib().lanczos_ycc16_source_init(ctypes.byref(s), ctypes.byref(d), layout, sx, sy)
            assert rc == (L.OK if sx == 1 else L.ERR_BAD_ARG)
            if sx == 1:
                assert (s.y_row_stride, s.c_row_stride, s.cb_offset, s.cr_offset) == (2 * W, 4 * cw, 2 * W * H, 2 * W * H)
        for win, (w, h) in ((None, (OW, OH)), ((2, 4, 7, 5), (7, 5))):
            ocw, och = M.out_chroma_size(w, h, sx, sy)
            t = L.ycc16_dest(d, L.YCC_PLANAR, win, sx, sy)
            assert (t.y_row_stride, t.c_row_stride, t.cb_offset, t.cr_offset) == (2 * w, 2 * ocw, 2 * w * h, 2 * (w * h + ocw * och))
            assert L.ycc_dest_frame_bytes(d, t, win) == 2 * (w * h + 2 * ocw * och)
    for name, (layout, sx, sy) in L.YCC16_LAYOUTS.items():
        s, t = L.ycc16_source(d, name), L.ycc16_dest(d, name)
        assert (s.layout, s.sub_x, s.sub_y) == (t.layout, t.sub_x, t.sub_y) == (layout, sx, sy), name


def _src_code(d, s):
    return L._lib().lanczos_ycc16_source_validate(ctypes.byref(d) if d is not None else None, ctypes.byref(s) if s is not None else None)


def _dst_code(d, t, win=None):
    return L._lib().lanczos_ycc16_dest_validate(ctypes.byref(d) if d is not None else None, ctypes.byref(win) if win is not None else None,
                                                ctypes.byref(t) if t is not None else None)


@pytest.mark.parametrize("side", ["source", "dest"])
def test_layout_refusals_by_code(side):
    d = _desc()
    w, h = (W, H) if side == "source" else (OW, OH)
    cw, ch = M.chroma_size(w, h, 1, 1)
    make = L.ycc16_source if side == "source" else L.ycc16_dest
    code = _src_code if side == "source" else _dst_code

    def mk(name, **kw):
        s = make(d, name)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    planar, nv = (lambda **kw: mk("i420", **kw)), (lambda **kw: mk("p010", **kw))
    luma = 2 * w * h
    assert code(d, planar()) == L.OK and code(d, nv()) == L.OK
    assert code(d, None) == L.ERR_BAD_ARG and code(None, planar()) == L.ERR_BAD_ARG
    # pitched and spaced planes at multiples of 2 are fine, 2 mod 4 included
    assert code(d, planar(y_row_stride=2 * w + 2, c_row_stride=2 * cw + 6, cb_offset=(2 * w + 2) * h + 2,
                          cr_offset=(2 * w + 2) * h + 2 + (2 * cw + 6) * ch + 2)) == L.OK
    assert code(d, nv(y_row_stride=2 * w + 6, c_row_stride=4 * cw + 2, cb_offset=(2 * w + 6) * h + 2, cr_offset=(2 * w + 6) * h + 2)) == L.OK
    bad = [planar(layout=3), planar(layout=-1), planar(sub_x=2), planar(sub_y=-1),
           nv(sub_x=0), nv(layout=L.YCC_NV21, sub_x=0), nv(cr_offset=luma + 2),                        # NV: sub_x != 1, two offsets
           planar(y_row_stride=2 * w - 2), planar(c_row_stride=2 * cw - 2), nv(c_row_stride=4 * cw - 2), planar(y_row_stride=0),
           planar(y_row_stride=w), planar(c_row_stride=cw), nv(c_row_stride=2 * cw),                   # a row counted in words
           planar(y_row_stride=(1 << 40) + 2), planar(cb_offset=-2), planar(cr_offset=-2),
           planar(cb_offset=luma - 2), planar(cr_offset=luma + 2 * cw * ch - 2), planar(cr_offset=luma),   # overlapping planes
           planar(y_row_stride=2 * w + 2), nv(cb_offset=luma - 2, cr_offset=luma - 2),
           planar(y_row_stride=2 * w + 1, cb_offset=(2 * w + 1) * h + 1, cr_offset=(2 * w + 1) * h + 1 + 2 * cw * ch),   # odd strides,
           planar(c_row_stride=2 * cw + 1, cr_offset=luma + (2 * cw + 1) * ch + 1),                                      # offsets
           planar(cb_offset=luma + 2 * cw * ch + 1, cr_offset=luma), nv(cb_offset=luma + 1, cr_offset=luma + 1)]
    for i, s in enumerate(bad):
        assert code(d, s) == L.ERR_BAD_ARG, i
    for i in range(5):
        s = planar()
        s.reserved[i] = 1
        assert code(d, s) == L.ERR_BAD_ARG, i
    # the descriptor: three channels of 16-bit words, and nothing else
    assert code(_desc(bits=8), make(d, "i420")) == L.ERR_UNSUPPORTED                                    # a missing LANCZOS_RESIZE_U16
    assert code(L.resize_desc(W, H, OW, OH, 3, f32=True), make(d, "i420")) == L.ERR_UNSUPPORTED
    da = _desc()
    da.reserved[0] |= L.RESIZE_ALPHA
    assert code(da, make(d, "i420")) == L.ERR_UNSUPPORTED
    for c in (1, 4):
        assert code(_desc(c), make(d, "i420")) == L.ERR_BAD_ARG
    dn = L.resize_desc(W, H, OW, OH, 3, filter="nearest")
    dn.reserved[0] |= L.RESIZE_U16
    assert code(dn, make(d, "i420")) == L.ERR_UNSUPPORTED                                               # LANCZOS_FILTER_NEAREST on words
    for filt in ("lanczos", "box", "bilinear", "hamming", "bicubic"):
        assert code(_desc(filter=filt), make(d, "i420")) == L.OK, filt
    if side == "dest":   # the window's origin against the destination's subsampling; sizes may be odd
        for name, ok, refused in (("i420", [(2, 4), (0, 0), (20, 12)], [(1, 0), (0, 1), (3, 3)]), ("i422", [(2, 1)], [(1, 0), (3, 2)]),
                                  ("i444", [(1, 1), (3, 2)], []), ("p010", [(4, 2)], [(1, 2), (2, 1)]), ("p210", [(2, 1)], [(1, 1)])):
            for x0, y0 in ok:
                win = L.resize_window(d, (x0, y0, 1, 1))
                assert _dst_code(d, L.ycc16_dest(d, name, win), win) == L.OK, (name, x0, y0)
            for x0, y0 in refused:
                win = L.resize_window(d, (x0, y0, 1, 1))
                t = L.ycc16_dest(d, name, (0, 0, 1, 1))
                assert _dst_code(d, t, win) == L.ERR_BAD_ARG, (name, x0, y0)
                with pytest.raises(L.LanczosError):
                    L.ycc16_dest(d, name, win)


def test_matrix_refusals_by_code():
    ok = L.ycc16_matrix("bt2020")
    v = lambda m: L._lib().lanczos_ycc16_matrix_validate(ctypes.byref(m) if m is not None else None)
    assert v(ok) == L.OK and v(None) == L.ERR_BAD_ARG

    def changed(**kw):
        m = L.ycc16_matrix("bt2020")
        for k, val in kw.items():
            if k == "k":
                m.k[val[0]][val[1]] = val[2]
            elif k in ("sub", "reserved"):
                getattr(m, k)[val[0]] = val[1]
            else:
                setattr(m, k, val)
        return m
    for c, j in itertools.product(range(3), repeat=2):
        assert v(changed(k=(c, j, (1 << 24) - 1))) == L.OK and v(changed(k=(c, j, -(1 << 24) + 1))) == L.OK
        assert v(changed(k=(c, j, 1 << 24))) == L.ERR_BAD_ARG and v(changed(k=(c, j, -(1 << 24)))) == L.ERR_BAD_ARG
    for i in range(3):
        assert v(changed(sub=(i, 65535))) == L.OK and v(changed(sub=(i, 65536))) == L.ERR_BAD_ARG and v(changed(sub=(i, -1))) == L.ERR_BAD_ARG
    assert v(changed(shift=0)) == L.OK and v(changed(shift=30)) == L.OK and v(changed(shift=31)) == L.ERR_BAD_ARG and v(changed(shift=-1)) == L.ERR_BAD_ARG
    assert v(changed(max=0)) == L.OK and v(changed(max=65536)) == L.ERR_BAD_ARG and v(changed(max=-1)) == L.ERR_BAD_ARG
    for i in range(4):
        assert v(changed(reserved=(i, 1))) == L.ERR_BAD_ARG
    m = L.Ycc16Matrix()
    init = L._lib().lanczos_ycc16_matrix_init
    assert init(None, 0, 10, 1, 0) == L.ERR_BAD_ARG
    for std, depth in ((4, 10), (-1, 10), (0, 7), (0, 17)):
        assert init(ctypes.byref(m), std, depth, 1, 0) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.ycc16_matrix("bt2100")


def test_request_refusals_by_code():
    """what lanczos_resize_ycc16 refuses before it touches a device: lanczos_ycc16_request_validate is that code"""
    d = _desc()
    s, t, m = L.ycc16_source(d, "p010"), L.ycc16_dest(d, "p010"), L.ycc16_matrix()
    n = L.tensor_norm(TN.strides("chw", OW, OH, 3))
    buf = np.zeros(1 << 14, np.uint16)
    v = lambda rq: L._lib().lanczos_ycc16_request_validate(ctypes.byref(rq) if rq is not None else None)
    mk = lambda dd=d, ss=s, **kw: L.ycc16_request(dd, ss, buf.ctypes.data, buf.ctypes.data, 2, **kw)
    assert v(mk(dest=t)) == L.OK and v(mk(matrix=m)) == L.OK and v(mk(matrix=m, norm=n)) == L.OK
    assert v(mk(dest=t, memory=L.MEM_HOST)) == L.OK
    assert L._lib().lanczos_resize_ycc16(None, ctypes.byref(mk(dest=t))) == L.ERR_BAD_ARG      # a null context
    assert v(None) == L.ERR_BAD_ARG
    # the pointer combinations
    for kw in ({}, dict(dest=t, matrix=m), dict(dest=t, norm=n), dict(norm=n), dict(dest=t, matrix=m, norm=n)):
        assert v(mk(**kw)) == L.ERR_BAD_ARG, kw
    for field in ("d", "src", "in_", "out"):
        rq = mk(dest=t)
        setattr(rq, field, None)
        assert v(rq) == L.ERR_BAD_ARG, field
    rq = mk(dest=t)
    rq.frames = 0
    assert v(rq) == L.ERR_BAD_ARG
    assert v(mk(dest=t, memory=2)) == L.ERR_BAD_ARG
    for i in range(4):
        rq = mk(dest=t)
        rq.reserved[i] = 1
        assert v(rq) == L.ERR_BAD_ARG
    # the descriptor
    assert v(mk(_desc(bits=8), dest=t)) == L.ERR_UNSUPPORTED
    assert v(mk(L.resize_desc(W, H, OW, OH, 3, f32=True), dest=t)) == L.ERR_UNSUPPORTED
    da = _desc()
    da.reserved[0] |= L.RESIZE_ALPHA
    assert v(mk(da, dest=t)) == L.ERR_UNSUPPORTED
    dn = L.resize_desc(W, H, OW, OH, 3, filter="nearest")
    dn.reserved[0] |= L.RESIZE_U16
    assert v(mk(dn, dest=t)) == L.ERR_UNSUPPORTED
    assert v(mk(_desc(1), dest=t)) == L.ERR_BAD_ARG
    # a reducing_gap; a box alone is fine
    gap = L.resize_opts(L.resize_desc(W, H, OW, OH, 3), None, 2.0)
    assert v(mk(dest=t, opts=gap)) == L.ERR_BAD_ARG and v(mk(matrix=m, opts=gap)) == L.ERR_BAD_ARG
    assert v(mk(dest=t, opts=L.resize_opts(L.resize_desc(W, H, OW, OH, 3), (3.5, 2.25, 33.75, 20.5), None))) == L.OK
    # layouts, matrix, norm
    bad_s = L.ycc16_source(d, "p010")
    bad_s.c_row_stride += 1
    bad_t = L.ycc16_dest(d, "p010")
    bad_t.y_row_stride = 2 * OW - 2
    bad_m = L.ycc16_matrix()
    bad_m.shift = 31
    bad_n = L.tensor_norm((1, 1, 1))
    assert v(mk(ss=bad_s, dest=t)) == L.ERR_BAD_ARG and v(mk(dest=bad_t)) == L.ERR_BAD_ARG and v(mk(matrix=bad_m)) == L.ERR_BAD_ARG
    assert v(mk(matrix=m, norm=bad_n)) == L.ERR_BAD_ARG
    odd = L.resize_window(d, (1, 0, 5, 5))
    assert v(mk(dest=L.ycc16_dest(d, "p010", (0, 0, 5, 5)), window=odd)) == L.ERR_BAD_ARG      # a window origin off the subsampling
    assert v(mk(matrix=m, window=odd)) == L.OK                                                 # ... which RGB output does not have
    # bases and frame strides
    for kw in (dict(dest=t, in_frame_stride=2 * (1 << 12) + 1), dict(dest=t, out_frame_stride=2 * (1 << 12) + 1),
               dict(matrix=m, out_frame_stride=2 * (1 << 12) + 2), dict(matrix=m, norm=n, out_frame_stride=4 * (1 << 12) + 2),
               dict(dest=t, memory=L.MEM_HOST, in_frame_stride=1 << 13), dict(dest=t, memory=L.MEM_HOST, out_frame_stride=1 << 13)):
        assert v(mk(**kw)) == L.ERR_BAD_ARG, kw
    for field, off, kw in (("in_", 1, dict(dest=t)), ("out", 1, dict(dest=t)), ("out", 2, dict(matrix=m)), ("out", 2, dict(matrix=m, norm=n))):
        rq = mk(**kw)
        setattr(rq, field, buf.ctypes.data + off)
        assert v(rq) == L.ERR_BAD_ARG, (field, off)
    rq = mk(matrix=m, memory=L.MEM_HOST)                                                       # host RGB frames lie back to back: words
    rq.out = buf.ctypes.data + 2
    assert v(rq) == L.OK


# ---- lanczos_ycc16_matrix_init ---------------------------------------------------------------------------------------------------
COMBOS = list(itertools.product((M.JFIF, M.BT601, M.BT709, M.BT2020), (8, 10, 12, 16), (False, True), (False, True)))


def _sample(depth, msb, n=300_000, seed=0):
    """seeded (y, cb, cr) words of the depth and alignment, and the eight corners of the cube behind them"""
    rng = np.random.default_rng([7, depth, int(msb), seed])
    sh = 16 - depth if msb else 0
    top = (1 << depth) - 1
    v = rng.integers(0, top + 1, (3, n)) << sh
    corners = np.array(list(itertools.product((0, top << sh), repeat=3))).T
    return np.concatenate([v, corners], axis=1).astype(np.uint16)


@pytest.mark.parametrize("standard,depth,msb,full", COMBOS)
def test_matrix_init_against_its_derivation(standard, depth, msb, full):
    got = M.matrix_of_struct(L.ycc16_matrix(standard, depth, msb, full))
    want = M.matrix(standard, depth, msb, full)
    assert np.array_equal(got.k, want.k) and (got.sub, got.shift, got.max) == (want.sub, want.shift, 65535)
    coef, sub = M.real_matrix(standard, depth, msb, full)
    # the shift rule: every entry below 2^23, and one more bit would not fit
    assert 13 <= got.shift <= 22 and (np.abs(got.k) < (1 << 23)).all()
    assert (np.abs(np.floor(np.abs(coef) * float(1 << (got.shift + 1)) + 0.5)) >= (1 << 23)).any()
    unit = (1 << (16 - depth)) if msb else 1
    assert sub == [0 if full else (16 << (depth - 8)) * unit, (1 << (depth - 1)) * unit, (1 << (depth - 1)) * unit]
    y, cb, cr = _sample(depth, msb)
    real, rounded = M.convert_f64(standard, depth, msb, full, y, cb, cr)
    # the derived bound: an entry is off its real value by at most 0.5, so the unrounded integer sum is off the real one by at
    # most sum_j 0.5 |v_j - sub_j| / 2^shift (float64 carries both sides far below that)
    exact = (M.sums(got, y, cb, cr) - (1 << (got.shift - 1))).astype(np.float64) / float(1 << got.shift)
    v = np.stack([np.abs(p.astype(np.float64) - s) for p, s in zip((y, cb, cr), sub)], -1)
    bound = 0.5 * v.sum(-1) / float(1 << got.shift)
    assert bound.max() < 0.5, bound.max()
    assert (np.abs(exact - real) <= bound[:, None] + 1e-6).all()
    assert np.abs(M.convert(got, y, cb, cr).astype(np.int64) - rounded).max() <= 1
    if standard == M.JFIF:
        assert np.array_equal(got.k, M.matrix(M.BT601, depth, msb, full).k)
    # the ends of the range: black, white and the chroma mid-point land on 0, 65535 and grey
    black, white = sub[0], sub[0] + (((1 << depth) - 1 if full else 219 << (depth - 8)) * unit)
    mid = np.array([sub[1]], dtype=np.uint16)
    assert M.convert(got, np.array([black], np.uint16), mid, mid).tolist() == [[0, 0, 0]]
    assert M.convert(got, np.array([white], np.uint16), mid, mid).tolist() == [[65535, 65535, 65535]]
