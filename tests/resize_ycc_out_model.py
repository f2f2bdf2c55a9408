"""Numpy model of lanczos_resize_ycc_out (include/lanczos_hip.h): resize INTO YCbCr frames.

Two contracts, both compositions of Pillow calls.  From YCbCr planes, plane by plane and without a colour conversion:

    Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
    Cbo = Image.fromarray(Cb, "L").resize((OCW, OCH), filt, box=bc, reducing_gap=g)          (Cr likewise)

with (OCW, OCH) the full output's chroma size under the DESTINATION's subsampling and bc the luma box scaled by the SOURCE's.
A window (x0, y0, w, h) in luma pixels, its origin a multiple of the destination's subsampling, stores luma [y0:y0+h, x0:x0+w]
and chroma [(y0 >> dsy):.. + och, (x0 >> dsx):.. + ocw], ocw = (w + dsx) >> dsx.  From RGB frames:

    rgb = Image.fromarray(x, "RGB").resize((out_w, out_h), filt, box=b, reducing_gap=g)[.crop(window)]
    Y, Cb, Cr = rgb.convert("YCbCr").split();  Cb, Cr = Cb.reduce((1 << dsx, 1 << dsy)), Cr.reduce(...)

through a table int32 [3][3][256] and the reduce rule ((sum + d / 2) * floor(2^24 / d)) >> 24.  The plane resizes are the
existing models' (resize_filters_model.resize); restated here from the contract: the sizes, the windows, the forward tables from
their formulas, the conversion and the ragged average.  CASES / RGB_CASES list the committed fixture
(tests/golden/resize_pillow_ycc_out.npz, written by tests/golden/make_resize_ycc_out_golden.py with Pillow itself).  The whole
destination buffer, noise in unnamed bytes included, is resize_ycc_model.build of the expected planes: `before` and `expected`
share the seed, so they agree in every byte the layout does not name.
"""
import collections

import numpy as np

import resize_filters_model as F
import resize_ycc_model as Y

PLANAR, NV12, NV21 = Y.PLANAR, Y.NV12, Y.NV21
JFIF, BT601, BT709 = Y.JFIF, Y.BT601, Y.BT709
LAYOUTS = {"i420": (PLANAR, 1, 1), "i422": (PLANAR, 1, 0), "i444": (PLANAR, 0, 0), "nv12": (NV12, 1, 1), "nv21": (NV21, 1, 1)}
SUBS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
SUB_NAME = {v: k for k, v in SUBS.items()}


def sub_of(layout):
    return LAYOUTS[layout][1:]


# ---- the forward tables ------------------------------------------------------------------------------------------------------
def _entries(k):
    """(int)(k * i * 64 + 0.5) for i = 0 .. 255: in double, truncated toward zero (Python's int() is C's cast)"""
    return np.array([int(k * i * 64 + 0.5) for i in range(256)], dtype=np.int64)


def forward_coefficients(standard):
    """(k [3][3], offsets [3]) of out = offsets + k @ (R, G, B) in real numbers"""
    if standard == JFIF:
        return np.array([[0.299, 0.587, 0.114], [-0.16874, -0.33126, 0.5], [0.5, -0.41869, -0.08131]]), np.array([0.0, 128.0, 128.0])
    kr, kb = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}[standard]
    kg, sy, sc = 1.0 - kr - kb, 219.0 / 255.0, 224.0 / 255.0
    ub, ur = 2.0 * (1.0 - kb), 2.0 * (1.0 - kr)
    k = np.array([[kr * sy, kg * sy, kb * sy], [-kr / ub * sc, -kg / ub * sc, 0.5 * sc], [0.5 * sc, -kg / ur * sc, -kb / ur * sc]])
    return k, np.array([16.0, 128.0, 128.0])


def forward_table(standard):
    """int32 [3][3][256]: t[c][0] over R, t[c][1] over G, t[c][2] over B, rows c = Y, Cb, Cr; the offsets (and, for the
    limited-range standards, the + 32 that makes the shift round) ride on the R entries"""
    k, off = forward_coefficients(standard)
    t = np.stack([np.stack([_entries(k[c][j]) for j in range(3)]) for c in range(3)])
    for c in range(3):
        t[c, 0] += int(off[c]) * 64 + (0 if standard == JFIF else 32)
    return t.astype(np.int32)


def forward_matrix_f64(standard, r, g, b):
    """the matrix in float64, rounded to nearest and clipped: what the limited-range tables stay within 1 of; [..][3]"""
    k, off = forward_coefficients(standard)
    r, g, b = (p.astype(np.float64) for p in (r, g, b))
    out = np.stack([off[c] + k[c][0] * r + k[c][1] * g + k[c][2] * b for c in range(3)], -1)
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def convert(t, rgb):
    """(Y, Cb, Cr) planes of rgb [..][3]: clip8((t[c][0][R] + t[c][1][G] + t[c][2][B]) >> 6), >> arithmetic"""
    t = np.asarray(t).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return tuple(np.clip((t[c, 0][r] + t[c, 1][g] + t[c, 2][b]) >> 6, 0, 255).astype(np.uint8) for c in range(3))


def reduce_plane(p, sx, sy):
    """Image.reduce((1 << sx, 1 << sy)) of planes [..][h][w]: every block divides by the d = 1, 2 or 4 bytes it holds,
    ((sum + d / 2) * floor(2^24 / d)) >> 24 in unsigned 32-bit"""
    if not (sx or sy):
        return p
    h, w = p.shape[-2:]
    fx, fy = 1 << sx, 1 << sy
    ow, oh = (w + fx - 1) // fx, (h + fy - 1) // fy
    pad = np.zeros(p.shape[:-2] + (oh * fy, ow * fx), dtype=np.uint64)
    pad[..., :h, :w] = p
    s = pad.reshape(p.shape[:-2] + (oh, fy, ow, fx)).sum(axis=(-3, -1))
    ny = np.minimum(fy, h - fy * np.arange(oh))[:, None]
    nx = np.minimum(fx, w - fx * np.arange(ow))[None, :]
    d = (ny * nx).astype(np.uint64)
    out = ((s + d // 2) * ((1 << 24) // d)) >> 24
    assert (((s + d // 2) * ((1 << 24) // d)) < (1 << 32)).all()
    return out.astype(np.uint8)


# ---- the two compositions ----------------------------------------------------------------------------------------------------
def out_chroma_size(w, h, dsx, dsy):
    return (w + dsx) >> dsx, (h + dsy) >> dsy


def ycc_to_ycc(y, cb, cr, ssx, ssy, dsx, dsy, out_w, out_h, filt="lanczos", box=None, gap=None, a=3, window=None):
    """(Yo, Cbo, Cro) of planes [F][h][w]: the stored frame (the window, or the whole output)"""
    f = Y.filter_code(filt)
    in_h, in_w = y.shape[-2:]
    assert cb.shape[-2:] == cr.shape[-2:] == Y.chroma_size(in_w, in_h, ssx, ssy)[::-1]
    ocw_full, och_full = out_chroma_size(out_w, out_h, dsx, dsy)
    bc = Y.chroma_box(box, in_w, in_h, ssx, ssy)
    one = lambda p, ow, oh, b: F.resize(p[..., None], f, ow, oh, b, gap, a)[..., 0]
    yo, cbo, cro = one(y, out_w, out_h, box), one(cb, ocw_full, och_full, bc), one(cr, ocw_full, och_full, bc)
    if window is not None:
        x0, y0, w, h = window
        assert x0 % (1 << dsx) == 0 and y0 % (1 << dsy) == 0 and x0 + w <= out_w and y0 + h <= out_h
        ocw, och = out_chroma_size(w, h, dsx, dsy)
        cx, cy = x0 >> dsx, y0 >> dsy
        assert cx + ocw <= ocw_full and cy + och <= och_full
        yo = yo[..., y0:y0 + h, x0:x0 + w]
        cbo, cro = cbo[..., cy:cy + och, cx:cx + ocw], cro[..., cy:cy + och, cx:cx + ocw]
    return yo, cbo, cro


def rgb_to_ycc(x, dsx, dsy, out_w, out_h, filt="lanczos", box=None, gap=None, a=3, window=None, t=None):
    """(Yo, Cbo, Cro) of RGB frames [F][h][w][3]: resize, cut the window, convert, average the chroma blocks"""
    rgb = F.resize(x, Y.filter_code(filt), out_w, out_h, box, gap, a)
    if window is not None:
        x0, y0, w, h = window
        rgb = rgb[..., y0:y0 + h, x0:x0 + w, :]
    yo, cbo, cro = convert(forward_table(JFIF) if t is None else t, rgb)
    return yo, reduce_plane(cbo, dsx, dsy), reduce_plane(cro, dsx, dsy)


# ---- the destination as it lies in memory ------------------------------------------------------------------------------------
def layout_code(layout):
    return LAYOUTS[layout][0]


def build(planes, layout, **kw):
    """resize_ycc_model.build of (Yo, Cbo, Cro) in a layout of LAYOUTS: the whole buffer with noise in every unnamed byte"""
    return Y.build(*planes, layout_code(layout), **kw)


def before_and_expected(planes, layout, seed=5, **kw):
    """(before, expected): two Frames with the same noise in the unnamed bytes; before holds other planes (the complement)"""
    other = tuple((255 - p).astype(np.uint8) for p in planes)
    return build(other, layout, seed=seed, **kw), build(planes, layout, seed=seed, **kw)


def tight(planes, layout):
    return Y.tight(*planes, layout_code(layout))


# ---- the fixture's cases -----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name ssx ssy dsx dsy in_w in_h out_w out_h filt box gap content")
CASES = []
for _s, (_ssx, _ssy) in SUBS.items():
    for _d, (_dsx, _dsy) in SUBS.items():
        CASES.append(Case(f"{_s}_to_{_d}_down", _ssx, _ssy, _dsx, _dsy, 37, 23, 22, 14, "lanczos", None, None, "noise"))
        CASES.append(Case(f"{_s}_to_{_d}_up", _ssx, _ssy, _dsx, _dsy, 37, 23, 50, 31, "lanczos", None, None, "noise"))
CASES += [
    Case("420_to_420_gap2", 1, 1, 1, 1, 81, 49, 10, 6, "lanczos", None, 2.0, "noise"),       # luma reduces by 4, chroma by 4 too
    Case("420_to_420_nearest", 1, 1, 1, 1, 37, 23, 22, 14, "nearest", None, None, "noise"),
    Case("420_to_444_box", 1, 1, 0, 0, 37, 23, 22, 14, "bicubic", (3.5, 2.25, 33.75, 20.5), None, "edges"),
    Case("420_to_420_same", 1, 1, 1, 1, 36, 22, 36, 22, "lanczos", None, None, "noise"),     # every plane keeps its size: a re-layout
    Case("420_to_420_same_odd", 1, 1, 1, 1, 37, 23, 37, 23, "lanczos", None, None, "noise"), # the chroma box is 18.5 x 11.5: chroma is filtered
    Case("420_to_420_wide", 1, 1, 1, 1, 2058, 6, 1029, 3, "lanczos", None, None, "noise"),   # 515 chroma pairs per row
]
CASE = {c.name: c for c in CASES}

RgbCase = collections.namedtuple("RgbCase", "name in_w in_h out_w out_h filt content")
RGB_CASES = [
    RgbCase("rgb_down", 37, 23, 22, 14, "lanczos", "noise"),
    RgbCase("rgb_up", 37, 23, 51, 31, "lanczos", "blocks"),
    RgbCase("rgb_same", 37, 23, 37, 23, "lanczos", "noise"),
    RgbCase("rgb_same_blocks", 37, 23, 37, 23, "lanczos", "blocks"),
    RgbCase("rgb_1x1", 1, 1, 1, 1, "lanczos", "noise"),
    RgbCase("rgb_2x1", 2, 1, 2, 1, "lanczos", "noise"),
    RgbCase("rgb_1x2", 1, 2, 1, 2, "lanczos", "noise"),
    RgbCase("rgb_wide_same", 2053, 5, 2053, 5, "lanczos", "noise"),                          # 514 groups of four pixels per row
]
RGB_CASE = {c.name: c for c in RGB_CASES}
FRAMES = 2


def make_planes(case, frames=FRAMES, seed=0):
    """seeded source planes of a Case (resize_ycc_model.make_planes's contents on this list's seeds)"""
    rng = np.random.default_rng(9500 + 31 * CASES.index(case) + seed)
    cw, ch = Y.chroma_size(case.in_w, case.in_h, case.ssx, case.ssy)
    shapes = ((frames, case.in_h, case.in_w), (frames, ch, cw), (frames, ch, cw))
    if case.content == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
    out = []
    for k, s in enumerate(shapes):       # edges: blocks of 3 .. 5 samples, another phase per plane
        yy, xx = np.mgrid[0:s[1], 0:s[2]]
        p = ((((xx + k) // (3 + k)) + ((yy + 2 * k) // (3 + k))) & 1) * 255
        out.append(np.where(rng.integers(0, 2, (frames, 1, 1)), 255 - p, p).astype(np.uint8))
    return tuple(out)


def make_rgb(case, frames=FRAMES, seed=0):
    """seeded RGB frames [F][h][w][3]: noise, or blocks of 0 / 255 per channel, three pixels wide, another phase per channel"""
    rng = np.random.default_rng(9700 + 31 * RGB_CASES.index(case) + seed)
    if case.content == "noise":
        return rng.integers(0, 256, (frames, case.in_h, case.in_w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:case.in_h, 0:case.in_w]
    x = np.stack([((((xx + c) // 3) + ((yy + 2 * c) // 3)) & 1) * 255 for c in range(3)], -1)
    return np.where(rng.integers(0, 2, (frames, 1, 1, 1)), 255 - x, x).astype(np.uint8)


def compose_case(case, planes, window=None, dsub=None):
    dsx, dsy = (case.dsx, case.dsy) if dsub is None else dsub
    return ycc_to_ycc(*planes, case.ssx, case.ssy, dsx, dsy, case.out_w, case.out_h, case.filt, case.box, case.gap, window=window)


# ---- a caller's table whose sums leave [0, 16383] on both sides --------------------------------------------------------------
def clip_table():
    """Y = clip8(4 R - 2 G - 128), Cb = clip8(3 G - B - 100), Cr = clip8(2 B + 2 R - 300): sums far outside [0, 16383] at both
    ends in every channel, bytes in between where the operands are moderate"""
    i = np.arange(256, dtype=np.int64)
    t = np.zeros((3, 3, 256), dtype=np.int64)
    t[0, 0], t[0, 1] = 64 * (4 * i - 128), -64 * 2 * i
    t[1, 1], t[1, 2] = 64 * (3 * i - 100), -64 * i
    t[2, 0], t[2, 2] = 64 * (2 * i - 300), 64 * 2 * i
    return t.astype(np.int32)


CLIP_HIGH, CLIP_MID, CLIP_LOW = (255, 200, 100), (120, 60, 50), (0, 10, 100)   # (R, G, B): every sum above 16383 / inside / below 0


def clip_frames(w=37, h=23, frames=FRAMES):
    """RGB frames for clip_table.  A thread converts pixels 4 k .. 4 k + 3 of a row into one dword of Y: rows 0 .. 3 hold
    (high, high, in range, in range) and the reverse in every such group, rows 4 .. 7 the same with sums below 0, in all three
    outputs at once; the rest is noise"""
    rng = np.random.default_rng(9900)
    x = rng.integers(0, 256, (frames, h, w, 3), dtype=np.uint8)
    for r in range(min(h, 8)):
        out = CLIP_HIGH if r < 4 else CLIP_LOW
        pat = (out, out, CLIP_MID, CLIP_MID) if r % 2 == 0 else (CLIP_MID, CLIP_MID, out, out)
        for px in range(w):
            x[:, r, px] = pat[px % 4]
    return x
