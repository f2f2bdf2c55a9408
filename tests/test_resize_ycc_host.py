"""Host checks of lanczos_resize_ycc_* (no GPU): the ABI, lanczos_ycc_source_init / _validate, the three standard colour
tables -- JFIF against the installed Pillow over all 2^24 (y, cb, cr) triples, the limited-range ones against their formula and
the float64 matrix -- and the numpy model (tests/resize_ycc_model.py) against Pillow's committed fixture."""
import ctypes
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_ycc_model as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc.npz")
W, H = 37, 23


def _desc(w=W, h=H, c=3, **kw):
    return L.resize_desc(w, h, 19, 13, c, **kw)


def _code(d, s):
    return L._lib().lanczos_ycc_source_validate(ctypes.byref(d) if d is not None else None, ctypes.byref(s) if s is not None else None)


def _init(d, layout, sx, sy):
    s = L.YccSource()
    for i in range(5):
        s.reserved[i] = 9                                          # init clears them
    rc = L._lib().lanczos_ycc_source_init(ctypes.byref(s), ctypes.byref(d), layout, sx, sy)
    return rc, s


def test_abi_structs_match_the_header():
    S = L.YccSource
    assert ctypes.sizeof(S) == 4 * 8 + 3 * 4 + 5 * 4
    assert (S.y_row_stride.offset, S.c_row_stride.offset, S.cb_offset.offset, S.cr_offset.offset) == (0, 8, 16, 24)
    assert (S.layout.offset, S.sub_x.offset, S.sub_y.offset, S.reserved.offset) == (32, 36, 40, 44)
    assert ctypes.sizeof(L.YccInfoC) == 8 * 4
    assert (L.YCC_PLANAR, L.YCC_NV12, L.YCC_NV21) == (0, 1, 2) and (L.YCC_JFIF, L.YCC_BT601, L.YCC_BT709) == (0, 1, 2)
    with open(os.path.join(ROOT, "include", "lanczos_hip.h")) as f:
        header = f.read()
    for macro, value in (("LANCZOS_YCC_PLANAR", 0), ("LANCZOS_YCC_NV12", 1), ("LANCZOS_YCC_NV21", 2), ("LANCZOS_YCC_JFIF", 0),
                         ("LANCZOS_YCC_BT601", 1), ("LANCZOS_YCC_BT709", 2)):
        assert "#define %s %d" % (macro, value) in header, macro
    for name in ("lanczos_ycc_source_init", "lanczos_ycc_source_validate", "lanczos_ycc_table", "lanczos_resize_ycc_device",
                 "lanczos_resize_ycc_tensor_device", "lanczos_resize_ycc_host", "lanczos_resize_ycc_tensor_host",
                 "lanczos_last_ycc_info"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name), name
    assert L._lib().lanczos_last_ycc_info(None, None) == L.ERR_BAD_ARG


@pytest.mark.parametrize("w,h", [(37, 23), (40, 24), (1, 1), (2, 3)])
def test_init_is_the_tight_layout(w, h):
    d = _desc(w, h)
    for sx in (0, 1):
        for sy in (0, 1):
            cw, ch = (w + sx) >> sx, (h + sy) >> sy
            assert (cw, ch) == Y.chroma_size(w, h, sx, sy)
            rc, s = _init(d, L.YCC_PLANAR, sx, sy)
            assert rc == L.OK and _code(d, s) == L.OK
            assert (s.y_row_stride, s.c_row_stride, s.cb_offset, s.cr_offset) == (w, cw, w * h, w * h + cw * ch)
            assert (s.layout, s.sub_x, s.sub_y, list(s.reserved)) == (L.YCC_PLANAR, sx, sy, [0] * 5)
            assert L.ycc_frame_bytes(d, s) == w * h + 2 * cw * ch
            for layout in (L.YCC_NV12, L.YCC_NV21):
                rc, s = _init(d, layout, sx, sy)
                if sx != 1:
                    assert rc == L.ERR_BAD_ARG                      # interleaved chroma is horizontally subsampled
                    continue
                assert rc == L.OK and _code(d, s) == L.OK
                assert (s.y_row_stride, s.c_row_stride, s.cb_offset, s.cr_offset) == (w, 2 * cw, w * h, w * h)
                assert L.ycc_frame_bytes(d, s) == w * h + 2 * cw * ch
    for name, (layout, sx, sy) in L.YCC_LAYOUTS.items():
        s = L.ycc_source(d, name)
        assert (s.layout, s.sub_x, s.sub_y) == (layout, sx, sy), name


def test_init_refusals():
    d = _desc()
    assert L._lib().lanczos_ycc_source_init(None, ctypes.byref(d), 0, 1, 1) == L.ERR_BAD_ARG
    assert L._lib().lanczos_ycc_source_init(ctypes.byref(L.YccSource()), None, 0, 1, 1) == L.ERR_BAD_ARG
    for layout, sx, sy in ((3, 1, 1), (-1, 1, 1), (0, 2, 0), (0, 0, 2), (0, -1, 0), (0, 1, -1), (1, 0, 1), (2, 0, 0)):
        assert _init(d, layout, sx, sy)[0] == L.ERR_BAD_ARG, (layout, sx, sy)


def test_validate_refusals_by_code():
    d = _desc()
    cw, ch = Y.chroma_size(W, H, 1, 1)
    ok = lambda **kw: L.ycc_source(d, "i420", **kw)
    assert _code(d, ok()) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG and _code(None, ok()) == L.ERR_BAD_ARG

    def planar(**kw):
        s = L.ycc_source(d, "i420")
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def nv(**kw):
        s = L.ycc_source(d, "nv12")
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    # pitched and spaced planes are fine
    assert _code(d, planar(y_row_stride=48, c_row_stride=24, cb_offset=48 * H + 3, cr_offset=48 * H + 3 + 24 * ch + 1)) == L.OK
    assert _code(d, planar(cb_offset=W * H + cw * ch, cr_offset=W * H)) == L.OK                     # Cr in front of Cb (YV12)
    assert _code(d, nv(y_row_stride=48, c_row_stride=44, cb_offset=48 * H + 5, cr_offset=48 * H + 5)) == L.OK
    bad = [planar(y_row_stride=W - 1), planar(c_row_stride=cw - 1), nv(c_row_stride=2 * cw - 1), planar(y_row_stride=0),
           planar(y_row_stride=(1 << 40) + 1),
           planar(cb_offset=W * H - 1),                                                             # Cb inside the luma plane
           planar(cr_offset=W * H + cw * ch - 1),                                                   # Cr over Cb's last byte
           planar(cr_offset=W * H),                                                                 # Cr on top of Cb
           planar(y_row_stride=W + 1),                                                              # pitched luma runs into Cb
           planar(cb_offset=-1), nv(cb_offset=W * H - 1, cr_offset=W * H - 1),
           nv(cr_offset=W * H + 1),                                                                 # two offsets for one plane
           planar(sub_x=2), planar(sub_y=-1), planar(layout=3), nv(sub_x=0), nv(layout=L.YCC_NV21, sub_x=0)]
    for i, s in enumerate(bad):
        assert _code(d, s) == L.ERR_BAD_ARG, i
    for i in range(5):
        s = planar()
        s.reserved[i] = 1
        assert _code(d, s) == L.ERR_BAD_ARG, i
    # the descriptor: three channels (the RGB result); alpha, 16-bit and float samples are not built
    for c in (1, 4):
        assert _code(_desc(c=c), ok()) == L.ERR_BAD_ARG
    for kw in ({"bits": 16}, {"f32": True}):
        assert _code(_desc(**kw), ok()) == L.ERR_UNSUPPORTED, kw
    da = _desc()
    da.reserved[0] |= L.RESIZE_ALPHA
    assert _code(da, ok()) == L.ERR_UNSUPPORTED
    # every filter and every a is allowed, NEAREST included
    for filt in L.FILTER_NAMES:
        assert _code(_desc(filter=filt), ok()) == L.OK, filt
    for a in (2, 4):
        assert _code(_desc(a=a), ok()) == L.OK, a
    # two-channel frames stay refused everywhere
    with pytest.raises(L.LanczosError):
        L.resize_desc(W, H, 19, 13, 2)


def test_table_refusals():
    t = np.zeros((3, 3, 256), np.int32)
    assert L._lib().lanczos_ycc_table(0, None) == L.ERR_BAD_ARG
    for std in (-1, 3, 99):
        assert L._lib().lanczos_ycc_table(std, t.ctypes.data) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.ycc_table("bt2020")


def test_jfif_table_is_pillows_convert_over_all_triples():
    from PIL import Image
    y, cb, cr = Y.all_triples()
    t = L.ycc_table("jfif")
    assert np.array_equal(t, Y.table(Y.JFIF))
    want = np.asarray(Image.merge("YCbCr", [Image.fromarray(p, "L") for p in (y, cb, cr)]).convert("RGB"))
    for c in range(3):
        got = np.clip((t[c, 0][y] + t[c, 1][cb] + t[c, 2][cr]) >> 6, 0, 255).astype(np.uint8)
        diff = int((got != want[..., c]).sum())
        assert diff == 0, (c, diff)
    # ... and the recipe as the contract words it, without a table, on a slice
    assert np.array_equal(Y.pillow_recipe(y[::16, ::16], cb[::16, ::16], cr[::16, ::16]), want[::16, ::16])


@pytest.mark.parametrize("name,std", [("bt601", Y.BT601), ("bt709", Y.BT709)])
def test_limited_range_tables(name, std):
    t = L.ycc_table(name)
    assert t.dtype == np.int32 and t.shape == (3, 3, 256)
    assert np.array_equal(t, Y.table(std))                                  # the restated formula, exactly
    assert np.array_equal(t, L.ycc_table(std))
    assert not t[0, 1].any() and not t[2, 2].any()                          # R does not read cb, B does not read cr
    y, cb, cr = Y.all_triples()
    worst = 0
    for r0 in range(0, 4096, 512):                                          # (in slabs: float64 over 2^24 triples at once is 400 MB)
        s = slice(r0, r0 + 512)
        got = Y.convert(t, y[s], cb[s], cr[s]).astype(np.int16)
        want = Y.matrix_f64(std, y[s], cb[s], cr[s]).astype(np.int16)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst                                                # the derived bound: entry rounding adds at most 1.5 / 64


def test_model_reproduces_pillows_fixture():
    z = np.load(GOLDEN)
    assert sorted(k[:-4] for k in z.files if k.endswith("_out")) == sorted(c.name for c in Y.CASES)
    for k, p in zip(("y", "cb", "cr"), Y.make_planes(Y.CASES[0], 2)):
        assert np.array_equal(z[f"input_check_{k}"], p), k                  # the seeded generator is the fixture's
    subs = set()
    for c in Y.CASES:
        y, cb, cr = Y.make_planes(c, 2)
        got = Y.compose(y, cb, cr, c.sx, c.sy, c.out_w, c.out_h, c.filt, c.box, c.gap)
        want = z[f"{c.name}_out"]
        assert got.shape == want.shape == (2, c.out_h, c.out_w, 3) and np.array_equal(got, want), c.name
        subs.add((c.sx, c.sy))
    assert subs == {(1, 1), (1, 0), (0, 0)}
    # the contents do what they are there for: clip8 works on all three outputs, and the gapped cases reduce
    for name in ("i444_up", "i420_edges_down", "i420_extreme"):
        out = z[f"{name}_out"]
        assert all((out[..., ch] == 0).any() and (out[..., ch] == 255).any() for ch in range(3)), name
    import resize_filters_model as F
    c = Y.CASE["i420_gap2_both"]
    cw, ch = Y.chroma_size(c.in_w, c.in_h, 1, 1)
    assert F.gap_plan(0, c.in_w, c.in_h, c.out_w, c.out_h, None, 2.0)[:2] == (8, 8) and F.gap_plan(0, cw, ch, c.out_w, c.out_h, None, 2.0)[:2] == (4, 4)
    c = Y.CASE["i420_gap2_luma"]
    assert F.gap_plan(0, c.in_w, c.in_h, c.out_w, c.out_h, None, 2.0)[:2] == (3, 2) and F.gap_plan(0, 19, 12, c.out_w, c.out_h, None, 2.0)[:2] == (1, 1)


def test_chroma_box_is_exact():
    assert Y.chroma_box(None, 37, 23, 1, 1) == (0.0, 0.0, 18.5, 11.5)
    assert Y.chroma_box(None, 37, 23, 1, 0) == (0.0, 0.0, 18.5, 23.0)
    assert Y.chroma_box((3.5, 2.25, 33.75, 20.5), 37, 23, 1, 1) == (1.75, 1.125, 16.875, 10.25)
    assert Y.chroma_box((3.5, 2.25, 33.75, 20.5), 37, 23, 0, 0) == (3.5, 2.25, 33.75, 20.5)


# ---- the yardsticks of tests/test_resize_ycc_edges_gpu.py, pinned without a GPU ------------------------------------------------
def _pillow(shape, y, cb, cr):
    """the header's recipe on one frame with the installed Pillow: three "L" resizes, chroma with box = Y.chroma_box(...)"""
    from PIL import Image
    filt = {"lanczos": Image.Resampling.LANCZOS, "bicubic": Image.Resampling.BICUBIC}[shape.filt]
    size = (shape.out_w, shape.out_h)
    bl = (0.0, 0.0, float(shape.in_w), float(shape.in_h))
    bc = Y.chroma_box(None, shape.in_w, shape.in_h, shape.sx, shape.sy)
    planes = [Image.fromarray(p).resize(size, filt, box=b) for p, b in ((y, bl), (cb, bc), (cr, bc))]
    assert all(p.mode == "L" for p in planes)
    return np.asarray(Image.merge("YCbCr", planes).convert("RGB"))


def _pillow_cases():
    shapes = Y.narrow_shapes(subs=((1, 1), (1, 0)), outs=((3, 2), (1, 1), None))
    assert len(shapes) == 162
    shapes += [Y.split_alone_shape(cw) for cw in Y.SPLIT_WIDE_CW] + [Y.SPLIT_ODD_WIDE, Y.MANY_FRAMES]
    shapes += [Y.Shape(0, 0, w, h, w, h, "lanczos") for w, h in Y.MERGE_ONLY]
    return shapes


def test_model_equals_installed_pillow_on_the_edge_shapes():
    """every shape class the GPU edge tests compare with Y.compose: narrow frames (rows of 1 .. 5 chroma pairs), the wide rows
    of the split, the odd wide one, the frames of the 65 537-frame batch and the frames that keep their size"""
    for shape in _pillow_cases():
        frames = 12 if shape == Y.MANY_FRAMES else 1
        y, cb, cr = Y.noise_planes(shape, frames, seed=1)
        got = Y.compose_shape(shape, y, cb, cr)
        for f in range(frames):
            want = _pillow(shape, y[f], cb[f], cr[f])
            assert got[f].shape == want.shape and np.array_equal(got[f], want), (shape, f)
        if (shape.sx, shape.sy, shape.out_w, shape.out_h) == (0, 0, shape.in_w, shape.in_h):   # nothing resizes: the conversion alone
            assert np.array_equal(got, Y.convert(Y.table(Y.JFIF), y, cb, cr)), shape


def test_yv12_and_nv16_builders_lay_the_planes_out_as_named():
    """Y.build's plane-order switch (YV12) and NV12 / NV21 with sub_y = 0 (NV16 / NV61): the offsets pass the validator and the
    bytes at them are the planes"""
    case = Y.CASE["i420_down"]
    y, cb, cr = Y.make_planes(case, 2)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
    s = Y.build(y, cb, cr, Y.PLANAR, c_row_stride=21, gap=3, base=1, cr_first=True)
    assert s.cr_offset < s.cb_offset
    src = L.ycc_source(d, "i420", y_row_stride=s.y_row_stride, c_row_stride=21, cb_offset=s.cb_offset, cr_offset=s.cr_offset)
    assert _code(d, src) == L.OK and L.ycc_frame_bytes(d, src) <= s.frame_stride
    for f in range(2):
        o = s.at + f * s.frame_stride
        for r in range(12):
            assert np.array_equal(s.buf[o + s.cb_offset + 21 * r:][:19], cb[f, r]) and np.array_equal(s.buf[o + s.cr_offset + 21 * r:][:19], cr[f, r])
    plain = Y.build(y, cb, cr, Y.PLANAR, c_row_stride=21, gap=3, base=1)
    assert (plain.cb_offset, plain.cr_offset) == (s.cr_offset, s.cb_offset) and plain.frame_stride == s.frame_stride
    case = Y.CASE["i422_down"]
    y, cb, cr = Y.make_planes(case, 2)
    assert cb.shape == (2, case.in_h, 17)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
    for layout, code, first in ((Y.NV12, L.YCC_NV12, cb), (Y.NV21, L.YCC_NV21, cr)):
        s = Y.build(y, cb, cr, layout, c_row_stride=37, base=2)
        src = L.ycc_source(d, code, 1, 0, c_row_stride=37, cb_offset=s.cb_offset)
        assert _code(d, src) == L.OK and (src.sub_x, src.sub_y, src.cr_offset) == (1, 0, s.cb_offset)
        assert L.ycc_frame_bytes(d, src) == s.frame_stride == case.in_w * case.in_h + 37 * case.in_h
        assert np.array_equal(s.buf[s.at + s.cb_offset + 37 * 30:][:34:2], first[0, 30])
        src.cr_offset += 1                                                  # two offsets for one plane, also at sub_y = 0
        assert _code(d, src) == L.ERR_BAD_ARG


def test_passthrough_table_hands_the_planes_through():
    t = Y.passthrough_table()
    assert t.dtype == np.int32 and t.shape == (3, 3, 256) and np.count_nonzero(t) == 3 * 255
    v = np.arange(256, dtype=np.uint8)
    y, cb, cr = np.meshgrid(v, v[::5], v[::7], indexing="ij")
    out = Y.convert(t, y, cb, cr)
    assert np.array_equal(out[..., 0], cb) and np.array_equal(out[..., 1], y) and np.array_equal(out[..., 2], cr)


@pytest.mark.parametrize("name", ["boundary", "wide"])
def test_hostile_tables_keep_the_contracts_condition(name):
    """in int64 over all 2^24 triples: no sum leaves int32 (the header's condition on a caller's table); the boundary table's
    sums take every value of Y.BOUNDARY_SUMS in every channel; the wide table's reach both halves of int32's range"""
    t = Y.boundary_table() if name == "boundary" else Y.wide_table()
    assert t.dtype == np.int32 and t.shape == (3, 3, 256)
    assert np.array_equal(t, Y.boundary_table() if name == "boundary" else Y.wide_table())       # seeded: the same every time
    for c in range(3):
        s = Y.table_sums(t, c)
        assert s.dtype == np.int64 and s.shape == (256, 256, 256)
        lo, hi = int(s.min()), int(s.max())
        assert Y.INT32_MIN <= lo and hi <= Y.INT32_MAX, (c, lo, hi)
        if name == "boundary":
            hit = np.isin(np.asarray(Y.BOUNDARY_SUMS, dtype=np.int64), s)
            assert hit.all(), (c, [v for v, h in zip(Y.BOUNDARY_SUMS, hit) if not h])
            assert (lo, hi) == (Y.INT32_MIN, Y.INT32_MAX)
        else:
            assert np.abs(t[c].astype(np.int64)).max() <= 700_000_000
            assert lo < -(1 << 30) and hi > (1 << 30), (c, lo, hi)
        if name == "boundary":                                              # its small entries: every byte value out of every channel
            assert len(np.unique(s[(s >= 0) & (s <= 16383)] >> 6)) == 256, c


@pytest.mark.parametrize("std", [Y.JFIF, Y.BT601, Y.BT709])
def test_standard_tables_clip_at_both_ends_in_every_channel(std):
    t = Y.table(std)
    for c in range(3):
        s = Y.table_sums(t, c)
        assert Y.INT32_MIN <= int(s.min()) and int(s.max()) <= Y.INT32_MAX
        assert int(s.min()) < 0 and int(s.max()) > 16383                    # the clamp works at both ends ...
    y, cb, cr = (p[::8] for p in Y.all_triples())
    out = Y.convert(t, y, cb, cr)
    assert all((out[..., c] == 0).any() and (out[..., c] == 255).any() for c in range(3))   # ... and outputs 0 and 255


def test_convert_over_all_triples_is_the_table_sums():
    """Y.convert on the all-triples image, the yardstick of the GPU merge tests, against the sums restated on the cube"""
    t = Y.boundary_table()
    y, cb, cr = Y.all_triples()
    got = Y.convert(t, y, cb, cr)
    for c in range(3):
        assert np.array_equal(got[..., c].reshape(256, 256, 256), np.clip(Y.table_sums(t, c) >> 6, 0, 255).astype(np.uint8)), c


def test_chw_words_is_the_view_model():
    """Y.chw_words, which the all-triples tensor case compares with, equals resize_tensor_view_model.view"""
    import resize_tensor16_model as T16
    import resize_tensor_model as T32
    import resize_tensor_view_model as V
    rgb = np.random.default_rng(3).integers(0, 256, (7, 5, 3), dtype=np.uint8)
    for lut in (T32.identity_lut(3), T16.identity_lut16(3), T32.identity_lut(2)):
        for src in ((2, 1, 0), (0, 1, 2), (2, 0)):
            if len(src) != lut.shape[0]:
                continue
            for flip in range(4):
                assert np.array_equal(Y.chw_words(rgb, lut, src, flip), V.view(rgb, lut, src, flip, "chw")), (src, flip)


def test_split_cover_names_every_workgroup_the_wide_rows_use():
    """the row cover as k_rs_ycc_split's contract words it, in plain arithmetic: which widths and residues give a dword or a
    tail byte to the second workgroup, and work to the third"""
    (head, nd, rest), who = Y.split_cover(0, 511)                           # 1022 bytes: 255 dwords, the two tail bytes are items 255, 256
    assert (head, nd, rest) == (0, 255, 2) and who == {("dword", 0), ("byte", 0), ("byte", 1)}
    (head, nd, rest), who = Y.split_cover(1, 512)                           # 3 + 4 * 255 + 1
    assert (head, nd, rest) == (3, 255, 1) and who == {("dword", 0), ("byte", 0), ("byte", 1)}
    assert Y.split_cover(0, 512) == ((0, 256, 0), {("dword", 0)})           # exactly one workgroup of dwords
    assert Y.split_cover(0, 513) == ((0, 256, 2), {("dword", 0), ("byte", 1)})
    assert Y.split_cover(0, 516) == ((0, 258, 0), {("dword", 0), ("dword", 1)})
    assert Y.split_cover(2, 1030)[1] == {("dword", 0), ("dword", 1), ("dword", 2), ("byte", 2)}
    for addr in range(4):                                                   # rows shorter than the way to the next dword
        (head, nd, rest), who = Y.split_cover(addr, 1)
        assert (head, nd, rest) == ((0, 0, 2), (2, 0, 0), (2, 0, 0), (1, 0, 1))[addr] and who == {("byte", 0)}
    for addr in range(8):
        for cw in range(1, 40):
            (head, nd, rest), _ = Y.split_cover(addr, cw)
            assert head + 4 * nd + rest == 2 * cw and (nd == 0 or (addr + head) % 4 == 0) and head < 4 and rest < 4
