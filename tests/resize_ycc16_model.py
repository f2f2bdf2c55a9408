"""Numpy model of lanczos_resize_ycc16 (include/lanczos_hip.h): YCbCr frames of 16-bit words into wide YCbCr
frames, packed RGB words and normalised tensor elements.

The planes are Pillow's mode I;16 on the raw words, each plane on its own:

    Yo  = Image.fromarray(Y,  "I;16").resize((out_w, out_h), filt, box=bl)
    Cbo = Image.fromarray(Cb, "I;16").resize((CW, CH), filt, box=bc)                 (Cr likewise)

bc is bl scaled by the SOURCE's subsampling on its doubles; (CW, CH) is (out_w, out_h) for RGB and tensor output and the full
output's chroma size under the DESTINATION's subsampling for YCbCr output.  The resize of one plane is the existing models'
(resize_filters_model.resize, which runs uint16 frames through resize16_model's double tables, truncating rounding and the I;16
store: a sum above 65535 stores 0xFF00 | low byte).  Restated here from the contract, not from the library's code: the sizes,
boxes and windows, the integer matrix with its derivation from a standard, and the layouts in memory.  The elements are
resize_tensor_norm_model's over the RGB words.  CASES is the list of the committed fixture
(tests/golden/resize_pillow_ycc16.npz, written by tests/golden/make_resize_ycc16_golden.py with Pillow itself).

Buffers here are uint16 arrays and every stride, offset and base of a Frames is in WORDS (the C structs take bytes: twice
that); a base of 1 word puts the frame at 2 mod 4.
"""
import collections

import numpy as np

import resize16_model as M16
import resize_filters_model as F
import resize_model as M8
import resize_box_model as MB
import resize_ycc_model as Y

PLANAR, NV12, NV21 = Y.PLANAR, Y.NV12, Y.NV21
JFIF, BT601, BT709, BT2020 = 0, 1, 2, 3
# (layout code, sub_x, sub_y); "nv61" is the pair-swapped 4:2:2 shape, which has no name in the binding: code NV21 with (1, 0)
LAYOUTS = {"i420": (PLANAR, 1, 1), "i422": (PLANAR, 1, 0), "i444": (PLANAR, 0, 0), "nv12": (NV12, 1, 1), "nv21": (NV21, 1, 1),
           "p010": (NV12, 1, 1), "p016": (NV12, 1, 1), "nv16": (NV12, 1, 0), "p210": (NV12, 1, 0), "p216": (NV12, 1, 0),
           "nv61": (NV21, 1, 0)}
SUB_PLANAR = {(1, 1): "i420", (1, 0): "i422", (0, 0): "i444"}
SUB_PAIRS = {(1, 1): "p010", (1, 0): "p210"}
SUB_PAIRS_SWAPPED = {(1, 1): "nv21", (1, 0): "nv61"}


def sub_of(layout):
    return LAYOUTS[layout][1:]


def layout_code(layout):
    return LAYOUTS[layout][0]


chroma_size = Y.chroma_size
chroma_box = Y.chroma_box


def out_chroma_size(w, h, dsx, dsy):
    return (w + dsx) >> dsx, (h + dsy) >> dsy


# ---- the planes --------------------------------------------------------------------------------------------------------------
def resize_plane(p, filt, out_w, out_h, box=None, a=3):
    """planes [F][h][w] uint16 -> [F][out_h][out_w]: Image.resize on mode I;16"""
    assert p.dtype == np.uint16
    return F.resize(p[..., None], Y.filter_code(filt), out_w, out_h, box, None, a)[..., 0]


def resize_plane_saturating(p, filt, out_w, out_h, box=None, a=3):
    """the near miss: the same passes with a store that clamps to 65535 where Pillow stores 0xFF00 | low byte"""
    f = Y.filter_code(filt)
    in_h, in_w = p.shape[-2:]
    x0, y0, x1, y1 = box if box is not None else (0, 0, in_w, in_h)
    spans = {2: (MB.axis_runs(in_w, out_w, x0, x1), in_w, out_w, x0, x1), 1: (MB.axis_runs(in_h, out_h, y0, y1), in_h, out_h, y0, y1)}
    y = p.astype(np.int64)
    for axis in M8.pass_order(in_w, in_h, out_h, None):
        run, in_n, out_n, b0, b1 = spans[axis]
        if run:
            fi, c, k = F.axis_tables(f, in_n, out_n, b0, b1, a, f64=True)
            y = M16.store(M16.pass_sums(y.astype(np.float64), axis, fi, c, k), saturate=True)
    return y.astype(np.uint16)


def planes_rgb(y, cb, cr, ssx, ssy, out_w, out_h, filt="lanczos", box=None, a=3, window=None):
    """(Yo, Cbo, Cro), all out_w x out_h (cut to the window): what the matrix converts"""
    in_h, in_w = y.shape[-2:]
    assert cb.shape[-2:] == cr.shape[-2:] == chroma_size(in_w, in_h, ssx, ssy)[::-1]
    bc = chroma_box(box, in_w, in_h, ssx, ssy)
    out = [resize_plane(y, filt, out_w, out_h, box, a), resize_plane(cb, filt, out_w, out_h, bc, a), resize_plane(cr, filt, out_w, out_h, bc, a)]
    if window is not None:
        x0, y0, w, h = window
        out = [p[..., y0:y0 + h, x0:x0 + w] for p in out]
    return tuple(out)


def planes_ycc(y, cb, cr, ssx, ssy, dsx, dsy, out_w, out_h, filt="lanczos", box=None, a=3, window=None):
    """(Yo, Cbo, Cro) of the stored frame: chroma at the destination's subsampling; a window in luma pixels, origin a multiple of it"""
    in_h, in_w = y.shape[-2:]
    assert cb.shape[-2:] == cr.shape[-2:] == chroma_size(in_w, in_h, ssx, ssy)[::-1]
    ocw_full, och_full = out_chroma_size(out_w, out_h, dsx, dsy)
    bc = chroma_box(box, in_w, in_h, ssx, ssy)
    yo = resize_plane(y, filt, out_w, out_h, box, a)
    cbo, cro = resize_plane(cb, filt, ocw_full, och_full, bc, a), resize_plane(cr, filt, ocw_full, och_full, bc, a)
    if window is not None:
        x0, y0, w, h = window
        assert x0 % (1 << dsx) == 0 and y0 % (1 << dsy) == 0 and x0 + w <= out_w and y0 + h <= out_h
        ocw, och = out_chroma_size(w, h, dsx, dsy)
        cx, cy = x0 >> dsx, y0 >> dsy
        assert cx + ocw <= ocw_full and cy + och <= och_full
        yo = yo[..., y0:y0 + h, x0:x0 + w]
        cbo, cro = cbo[..., cy:cy + och, cx:cx + ocw], cro[..., cy:cy + och, cx:cx + ocw]
    return yo, cbo, cro


# ---- the matrix --------------------------------------------------------------------------------------------------------------
Matrix = collections.namedtuple("Matrix", "k sub shift max")   # k: int64 [3][3]; sub: three ints
KR_KB = {JFIF: (0.299, 0.114), BT601: (0.299, 0.114), BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}


def real_matrix(standard, depth=10, msb_aligned=True, full_range=False):
    """(coefficients float64 [3][3], sub [3]) of RGB = coefficients @ ((y, cb, cr) - sub), scaled to 0 .. 65535"""
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    unit = float(1 << (16 - depth)) if msb_aligned else 1.0
    full = float((1 << depth) - 1)
    ky = 65535.0 / ((full if full_range else float(219 << (depth - 8))) * unit)
    kc = 65535.0 / ((full if full_range else float(224 << (depth - 8))) * unit)
    coef = np.array([[ky, 0.0, 2.0 * (1.0 - kr) * kc],
                     [ky, -2.0 * (1.0 - kb) * kb / kg * kc, -2.0 * (1.0 - kr) * kr / kg * kc],
                     [ky, 2.0 * (1.0 - kb) * kc, 0.0]])
    mid = (1 << (depth - 1)) * int(unit)
    return coef, [0 if full_range else (16 << (depth - 8)) * int(unit), mid, mid]


def _nearest(x):
    """round to nearest, halves away from zero (no coefficient of a standard lands on one)"""
    return np.where(x < 0, -np.floor(-x + 0.5), np.floor(x + 0.5)).astype(np.int64)


def matrix(standard, depth=10, msb_aligned=True, full_range=False):
    """the rule of lanczos_ycc16_matrix_init: the largest shift <= 30 that keeps every rounded entry below 2^23 in magnitude"""
    coef, sub = real_matrix(standard, depth, msb_aligned, full_range)
    for shift in range(30, -1, -1):
        k = _nearest(coef * float(1 << shift))
        if (np.abs(k) < (1 << 23)).all():
            return Matrix(k, sub, shift, 65535)
    raise AssertionError("no shift fits")


def passthrough_matrix():
    """R = cb, G = y, B = cr, words as they are"""
    return Matrix(np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.int64), [0, 0, 0], 0, 65535)


def sums(m, y, cb, cr):
    """the int64 sums of the three channels, rounding term included: [..][3]"""
    v = [p.astype(np.int64) - s for p, s in zip((y, cb, cr), m.sub)]
    rnd = (1 << (m.shift - 1)) if m.shift else 0
    k = np.asarray(m.k, dtype=np.int64)
    return np.stack([k[c][0] * v[0] + k[c][1] * v[1] + k[c][2] * v[2] + rnd for c in range(3)], -1)


def convert(m, y, cb, cr):
    """clamp(sum >> shift, 0, max) (>> arithmetic: numpy's on int64 floors): uint16 [..][3]"""
    return np.clip(sums(m, y, cb, cr) >> m.shift, 0, m.max).astype(np.uint16)


def convert_f64(standard, depth, msb_aligned, full_range, y, cb, cr):
    """the real matrix in float64: (the unrounded values [..][3], rounded to nearest and clipped to 0 .. 65535)"""
    coef, sub = real_matrix(standard, depth, msb_aligned, full_range)
    v = np.stack([p.astype(np.float64) - s for p, s in zip((y, cb, cr), sub)], -1)
    real = v @ coef.T
    return real, np.clip(np.floor(real + 0.5), 0, 65535).astype(np.int64)


def matrix_struct(L, m):
    """a Matrix as the binding's Ycc16Matrix"""
    s = L.Ycc16Matrix()
    for c in range(3):
        for j in range(3):
            s.k[c][j] = int(m.k[c][j])
        s.sub[c] = int(m.sub[c])
    s.shift, s.max = int(m.shift), int(m.max)
    return s


def matrix_of_struct(s):
    return Matrix(np.array([[s.k[c][j] for j in range(3)] for c in range(3)], dtype=np.int64), [s.sub[c] for c in range(3)], s.shift, s.max)


def rgb16(m, planes):
    """packed RGB words [F][h][w][3] of resized planes"""
    return convert(m, *planes)


# ---- frames as they lie in memory: WORDS -------------------------------------------------------------------------------------
Frames = collections.namedtuple("Frames", "buf at frame_stride y_row_stride c_row_stride cb_offset cr_offset layout")
MARGIN = 32


def build(y, cb, cr, layout=PLANAR, y_row_stride=None, c_row_stride=None, base=0, gap=0, frame_gap=0, seed=1):
    """The planes [F][h][w] laid out as frames of words: Y rows y_row_stride apart, `gap` words, then the chroma planes (PLANAR:
    Cb, gap, Cr) or the interleaved plane of word pairs (NV12: Cb first, NV21: Cr first), rows c_row_stride apart; frames
    frame_gap words past the extent apart; the first frame MARGIN + base words into the buffer.  Every word the layout does not
    name is noise."""
    f, h, w = y.shape
    _, ch, cw = cb.shape
    crow = cw if layout == PLANAR else 2 * cw
    yrs = w if y_row_stride is None else y_row_stride
    crs = crow if c_row_stride is None else c_row_stride
    cb_off = h * yrs + gap
    cr_off = cb_off + ch * crs + gap if layout == PLANAR else cb_off
    extent = cr_off + ch * crs
    fs = extent + frame_gap
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 65536, MARGIN + base + (f - 1) * fs + extent + MARGIN, dtype=np.uint16)
    at = MARGIN + base
    for k in range(f):
        o = at + k * fs
        for r in range(h):
            buf[o + r * yrs:o + r * yrs + w] = y[k, r]
        for r in range(ch):
            if layout == PLANAR:
                buf[o + cb_off + r * crs:o + cb_off + r * crs + cw] = cb[k, r]
                buf[o + cr_off + r * crs:o + cr_off + r * crs + cw] = cr[k, r]
            else:
                first, second = (cb, cr) if layout == NV12 else (cr, cb)
                buf[o + cb_off + r * crs:o + cb_off + r * crs + 2 * cw:2] = first[k, r]
                buf[o + cb_off + r * crs + 1:o + cb_off + r * crs + 2 * cw:2] = second[k, r]
    return Frames(buf, at, fs, yrs, crs, cb_off, cr_off, layout)


def expected_dest(planes, layout, seed=5, **kw):
    """(before, expected): two Frames of a whole destination buffer with the same noise in every unnamed word; `before` holds
    the complement of the planes, so every named word has to change"""
    code = layout_code(layout) if isinstance(layout, str) else layout
    other = tuple((p ^ np.uint16(0xFFFF)).astype(np.uint16) for p in planes)
    return build(*other, code, seed=seed, **kw), build(*planes, code, seed=seed, **kw)


def tight(y, cb, cr, layout):
    """[F][W] uint16: the frames back to back in the tight layout, as Context.resize_ycc16_* take them"""
    s = build(y, cb, cr, layout_code(layout) if isinstance(layout, str) else layout)
    return s.buf[s.at:s.at + y.shape[0] * s.frame_stride].reshape(y.shape[0], s.frame_stride).copy()


def byte_strides(fr):
    """the keyword arguments of L.ycc16_source / L.ycc16_dest for a Frames: bytes"""
    return dict(y_row_stride=2 * fr.y_row_stride, c_row_stride=2 * fr.c_row_stride, cb_offset=2 * fr.cb_offset, cr_offset=2 * fr.cr_offset)


# ---- the cover arithmetic of the kernels, as their contracts word it ---------------------------------------------------------
PAIRS_THREADS = 256            # threads of a workgroup of k_rs_ycc_split16 / k_rs_ycc_join16: one dword of a tight plane each
PAIRS_PER_WORKGROUP = 512      # ... which is two pairs
MERGE_GROUP = 2                # pixels per thread of k_rs_ycc16_merge
MERGE_BLOCK = 512              # pixels per workgroup


def pairs_cover(row, cw):
    """(head, nd, rest) of chroma row `row` of cw pairs: the row's words [row * cw, row * cw + cw) of a tight plane are the nd
    dwords at dword-aligned offsets inside them and the single words in front (head) and behind (rest)"""
    head = (row * cw) & 1
    nd = (cw - head) >> 1
    rest = cw - head - 2 * nd
    assert head + 2 * nd + rest == cw and rest in (0, 1)
    return head, nd, rest


# ---- the fixture's cases -----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name ssx ssy dsx dsy in_w in_h out_w out_h filt box window content")
CASES = [
    Case("420_down_odd", 1, 1, 1, 1, 37, 23, 19, 13, "lanczos", None, None, "noise16"),          # odd sizes on both sides
    Case("422_down", 1, 0, 1, 0, 33, 31, 20, 30, "lanczos", None, None, "limited10_msb"),
    Case("444_up", 0, 0, 0, 0, 16, 16, 40, 24, "lanczos", None, None, "edges16"),
    Case("420_1x1", 1, 1, 1, 1, 37, 23, 1, 1, "lanczos", None, None, "noise16"),
    Case("420_up_bicubic", 1, 1, 1, 1, 37, 23, 45, 29, "bicubic", None, None, "edges_msb10"),
    Case("420_box", 1, 1, 1, 1, 37, 23, 19, 13, "lanczos", (3.5, 2.25, 33.75, 20.5), None, "limited10_msb"),
    Case("420_same", 1, 1, 1, 1, 36, 22, 36, 22, "lanczos", None, None, "noise16"),               # into YCbCr: a pure re-layout
    Case("420_same_odd", 1, 1, 1, 1, 37, 23, 37, 23, "lanczos", None, None, "limited10_lsb"),     # luma a copy, chroma filtered
    Case("420_edges_msb", 1, 1, 1, 1, 37, 23, 19, 13, "lanczos", None, None, "edges_msb10"),      # hard edges, MSB-aligned full range
    Case("420_limited_bilinear", 1, 1, 1, 1, 40, 24, 19, 13, "bilinear", None, None, "limited10_lsb"),
    Case("420_window", 1, 1, 1, 1, 37, 23, 30, 20, "lanczos", None, (2, 4, 17, 9), "noise16"),
    Case("420_to_444", 1, 1, 0, 0, 37, 23, 22, 14, "hamming", None, None, "limited10_msb"),
    Case("444_to_420", 0, 0, 1, 1, 37, 23, 22, 14, "lanczos", None, None, "noise16"),
]
CASE = {c.name: c for c in CASES}
FRAMES = 2


def make_planes(case, frames=FRAMES, seed=0):
    """seeded source planes (Y [F][h][w], Cb [F][ch][cw], Cr) of a Case, uint16.  noise16: every word; limited10_msb / _lsb:
    limited-range 10-bit noise (luma 64 .. 940, chroma 64 .. 960), in the high or the low bits; edges16 / edges_msb10: blocks
    of 0 and 65535 / 0xFFC0, where the filters overshoot on both sides and the I;16 store wraps its low byte"""
    rng = np.random.default_rng([9600, [c.name for c in CASES].index(case.name), seed])
    cw, ch = chroma_size(case.in_w, case.in_h, case.ssx, case.ssy)
    shapes = ((frames, case.in_h, case.in_w), (frames, ch, cw), (frames, ch, cw))
    c = case.content
    if c == "noise16":
        return tuple(rng.integers(0, 65536, s, dtype=np.uint16) for s in shapes)
    if c.startswith("limited10"):
        sh = 6 if c.endswith("msb") else 0
        return tuple((rng.integers(64, 941 if k == 0 else 961, s) << sh).astype(np.uint16) for k, s in enumerate(shapes))
    top = 65535 if c == "edges16" else 0xFFC0
    out = []
    for k, s in enumerate(shapes):       # blocks of 3 .. 5 samples, another phase per plane
        yy, xx = np.mgrid[0:s[1], 0:s[2]]
        p = ((((xx + k) // (3 + k)) + ((yy + 2 * k) // (3 + k))) & 1) * top
        out.append(np.where(rng.integers(0, 2, (frames, 1, 1)), top - p, p).astype(np.uint16))
    return tuple(out)


def case_planes_rgb(case, planes, window="case"):
    win = case.window if window == "case" else window
    return planes_rgb(*planes, case.ssx, case.ssy, case.out_w, case.out_h, case.filt, case.box, window=win)


def case_planes_ycc(case, planes, window="case", dsub=None):
    win = case.window if window == "case" else window
    dsx, dsy = (case.dsx, case.dsy) if dsub is None else dsub
    return planes_ycc(*planes, case.ssx, case.ssy, dsx, dsy, case.out_w, case.out_h, case.filt, case.box, window=win)


def golden_planes(z, case, kind):
    """the fixture's planes of a case: kind "rgb" (chroma at the luma size) or "ycc" (at the destination's), cut to the case's window"""
    yo = z[f"{case.name}_y"]
    cbo, cro = (z[f"{case.name}_cb"], z[f"{case.name}_cr"]) if kind == "rgb" else (z[f"{case.name}_dcb"], z[f"{case.name}_dcr"])
    if case.window is not None:
        x0, y0, w, h = case.window
        yo = yo[:, y0:y0 + h, x0:x0 + w]
        if kind == "rgb":
            cbo, cro = cbo[:, y0:y0 + h, x0:x0 + w], cro[:, y0:y0 + h, x0:x0 + w]
        else:
            ocw, och = out_chroma_size(w, h, case.dsx, case.dsy)
            cx, cy = x0 >> case.dsx, y0 >> case.dsy
            cbo, cro = cbo[:, cy:cy + och, cx:cx + ocw], cro[:, cy:cy + och, cx:cx + ocw]
    return yo, cbo, cro
