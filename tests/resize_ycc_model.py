"""Numpy model of lanczos_resize_ycc_* (include/lanczos_hip.h): YCbCr frames with subsampled chroma into RGB.

The contract is a composition of Pillow calls:

    Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
    Cbo = Image.fromarray(Cb, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
    Cro = Image.fromarray(Cr, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
    rgb = Image.merge("YCbCr", (Yo, Cbo, Cro)).convert("RGB")

The resize of one plane is the existing models' (resize_filters_model.resize, which stands on resize_model and
resize_box_model; a window is a crop of its result, as resize_window_model pins it).  What is restated here from the
contract, not from the library's code: the chroma plane's size and box, the conversion recipe through a table
int32 [3][3][256], and the three standard tables from their formulas.  CASES is the list of the committed fixture
(tests/golden/resize_pillow_ycc.npz, written by tests/golden/make_resize_ycc_golden.py with Pillow itself), and the buffer
builders lay planes out as I420 / NV12 / NV21 frames with noise in every byte the layout does not name.
"""
import collections

import numpy as np

import resize_filters_model as F

PLANAR, NV12, NV21 = 0, 1, 2
JFIF, BT601, BT709 = 0, 1, 2


def chroma_size(in_w, in_h, sx, sy):
    return (in_w + sx) >> sx, (in_h + sy) >> sy


def chroma_box(box, in_w, in_h, sx, sy):
    """the luma box (None: the whole frame) scaled to the chroma plane, on its float values: halving a double is exact"""
    x0, y0, x1, y1 = (float(v) for v in (box if box is not None else (0, 0, in_w, in_h)))
    kx, ky = (0.5 if sx else 1.0), (0.5 if sy else 1.0)
    return (x0 * kx, y0 * ky, x1 * kx, y1 * ky)


def _entries(k, off):
    """(int)(k * (i - off) * 64 + 0.5) for i = 0 .. 255: in double, truncated toward zero (Python's int() is C's cast)"""
    return np.array([int(k * (i - off) * 64 + 0.5) for i in range(256)], dtype=np.int64)


def table(standard):
    """int32 [3][3][256]: t[c][0] over y, t[c][1] over cb, t[c][2] over cr"""
    t = np.zeros((3, 3, 256), dtype=np.int64)
    if standard == JFIF:     # Pillow's convert("RGB"): the luma entry is 64 y, a multiple of 64, so the shift takes it out whole
        t[:, 0] = 64 * np.arange(256)
        t[0, 2] = _entries(1.402, 128)
        t[1, 1], t[1, 2] = _entries(-0.34414, 128), _entries(-0.71414, 128)
        t[2, 1] = _entries(1.772, 128)
    else:                    # limited range: luma 16 .. 235, chroma 16 .. 240; + 32 on the luma entry makes the shift round
        kr, kb = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}[standard]
        kg, ky, kc = 1.0 - kr - kb, 255.0 / 219.0, 255.0 / 224.0
        t[:, 0] = _entries(ky, 16) + 32
        t[0, 2] = _entries(2.0 * (1.0 - kr) * kc, 128)
        t[1, 1] = _entries(-2.0 * (1.0 - kb) * kb / kg * kc, 128)
        t[1, 2] = _entries(-2.0 * (1.0 - kr) * kr / kg * kc, 128)
        t[2, 1] = _entries(2.0 * (1.0 - kb) * kc, 128)
    return t.astype(np.int32)


def matrix_f64(standard, y, cb, cr):
    """the limited-range matrix in float64, rounded to nearest and clipped: what the two tables stay within 1 of"""
    kr, kb = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}[standard]
    kg, ky, kc = 1.0 - kr - kb, 255.0 / 219.0, 255.0 / 224.0
    yy, u, v = ky * (y.astype(np.float64) - 16), kc * (cb.astype(np.float64) - 128), kc * (cr.astype(np.float64) - 128)
    rgb = np.stack([yy + 2 * (1 - kr) * v, yy - 2 * (1 - kb) * kb / kg * u - 2 * (1 - kr) * kr / kg * v, yy + 2 * (1 - kb) * u], -1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def convert(t, y, cb, cr):
    """out[..., c] = clip8((t[c][0][y] + t[c][1][cb] + t[c][2][cr]) >> 6), >> arithmetic"""
    t = np.asarray(t).astype(np.int64)
    out = [np.clip((t[c, 0][y] + t[c, 1][cb] + t[c, 2][cr]) >> 6, 0, 255) for c in range(3)]
    return np.stack(out, axis=-1).astype(np.uint8)


def pillow_recipe(y, cb, cr):
    """Pillow's convert("RGB") as the contract states it, without a table"""
    T = lambda k, v: np.array([int(k * (i - 128) * 64 + 0.5) for i in range(256)], dtype=np.int64)[v]
    y = y.astype(np.int64)
    r = y + (T(1.402, cr) >> 6)
    g = y + ((T(-0.34414, cb) + T(-0.71414, cr)) >> 6)
    b = y + (T(1.772, cb) >> 6)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def all_triples():
    """a 4096 x 4096 image holding every (y, cb, cr) once: pixel i = y << 16 | cb << 8 | cr"""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return (i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)


def passthrough_table():
    """R = cb, G = y, B = cr: entries 64 i where a channel reads its plane, 0 elsewhere, so that the shift gives i back"""
    t = np.zeros((3, 3, 256), dtype=np.int32)
    t[0, 1] = t[1, 0] = t[2, 2] = 64 * np.arange(256)
    return t


INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# where clip8(sum >> 6) changes its behaviour: the ends of int32, the shift's steps around 0, the last sums that give 254 and
# 255 unclamped (16319 / 16320, 16383) and the first ones the clamp holds (16384 ...), and one full step beyond either end
BOUNDARY_SUMS = (INT32_MIN, -16384, -65, -64, -63, -1, 0, 1, 63, 64, 65, 16319, 16320, 16383, 16384, 16447, 16448, INT32_MAX)


def boundary_table(seed=7):
    """A caller's table at the edge of what the contract allows ("entries must keep the sum inside int32"): luma entries lie in
    [-2^30, 2^30 - 1] and chroma entries in [-2^29, 2^29], so no sum leaves int32 and both of its ends are reached.  For every
    channel and every v of BOUNDARY_SUMS one (y, cb, cr) is planted whose three entries add up to v, each of them large; the
    triples differ from channel to channel.  The other entries are half small (sums around the shift's range) and half wide."""
    rng = np.random.default_rng(seed)
    t = np.zeros((3, 3, 256), dtype=np.int64)
    n = len(BOUNDARY_SUMS)
    for c in range(3):
        small = rng.integers(-20000, 20001, (3, 256))
        wide = np.stack([rng.integers(-(1 << 30), 1 << 30, 256), rng.integers(-(1 << 29), (1 << 29) + 1, 256),
                         rng.integers(-(1 << 29), (1 << 29) + 1, 256)])
        t[c] = np.where(rng.integers(0, 2, (3, 256)) == 1, small, wide)
        iy, ib, ir = (rng.permutation(256)[:n] for _ in range(3))
        for k, v in enumerate(BOUNDARY_SUMS):
            if v == INT32_MIN:
                p, q = -(1 << 29), -(1 << 29)
            elif v == INT32_MAX:
                p, q = 1 << 29, 1 << 29
            else:
                p, q = (int(x) for x in rng.integers(-(1 << 29) + (1 << 15), (1 << 29) - (1 << 15), 2))
            t[c, 1, ib[k]], t[c, 2, ir[k]], t[c, 0, iy[k]] = p, q, v - p - q
    assert (np.abs(t[:, 0] + 0.5) < (1 << 30)).all() and (np.abs(t[:, 1:]) <= (1 << 29)).all()
    return t.astype(np.int32)


def wide_table(seed=8):
    """seeded entries in +-7e8: three of them add up to at most 2.1e9 < 2^31 - 1, so sums range over nearly all of int32"""
    return np.random.default_rng(seed).integers(-700_000_000, 700_000_001, (3, 3, 256)).astype(np.int32)


def table_sums(t, c):
    """int64 [256][256][256]: the sum of channel c for every (y, cb, cr), in the order of all_triples()"""
    t = np.asarray(t).astype(np.int64)
    return t[c, 0][:, None, None] + t[c, 1][None, :, None] + t[c, 2][None, None, :]


def chw_words(rgb, lut, src, flip):
    """the words of one tight CHW frame under the view contract (resize_tensor_view_model.view for one frame), plane by plane
    and without index arrays, for frames as large as all_triples(): [OC][h][w] of the table's word"""
    lb = np.ascontiguousarray(lut)
    lb = lb.view({4: np.uint32, 2: np.uint16}[lb.dtype.itemsize]).reshape(len(src), 256)
    b = rgb[::-1] if flip & 2 else rgb
    b = b[:, ::-1] if flip & 1 else b
    return np.stack([lb[oc][b[..., s]] for oc, s in enumerate(src)])


# ---- the row cover of the chroma split ------------------------------------------------------------------------------------------
SPLIT_THREADS = 256


def split_cover(addr, cw):
    """Who moves the 2 cw bytes of an interleaved chroma row at byte address `addr`, as the split's contract words it: the
    dwords at dword-aligned addresses inside the row, one per work item, then the `head` bytes in front of the first of them
    and the `rest` bytes behind the last, one per work item, SPLIT_THREADS items to a workgroup.  Returns (head, nd, rest) and
    the set of (kind, workgroup) pairs that have work, kind "dword" or "byte"."""
    n = 2 * cw
    head = min(-addr & 3, n)
    nd = (n - head) >> 2
    rest = n - head - 4 * nd
    assert 0 <= rest < 4 and head + 4 * nd + rest == n
    who = {("dword", k // SPLIT_THREADS) for k in range(nd)} | {("byte", k // SPLIT_THREADS) for k in range(nd, nd + head + rest)}
    return (head, nd, rest), who


def filter_code(filt):
    return F.NAMES.index(filt) if isinstance(filt, str) else int(filt)


def resize_planes(y, cb, cr, sx, sy, out_w, out_h, filt="lanczos", box=None, gap=None, a=3, window=None):
    """(Yo, Cbo, Cro): each plane [H][W] or [F][H][W] resized on its own, chroma with the scaled box; cropped to the window"""
    f = filter_code(filt)
    in_h, in_w = y.shape[-2:]
    assert cb.shape[-2:] == cr.shape[-2:] == chroma_size(in_w, in_h, sx, sy)[::-1]
    bc = chroma_box(box, in_w, in_h, sx, sy)
    one = lambda p, b: F.resize(p[..., None], f, out_w, out_h, b, gap, a)[..., 0]
    out = [one(y, box), one(cb, bc), one(cr, bc)]
    if window is not None:
        x0, y0, w, h = window
        out = [p[..., y0:y0 + h, x0:x0 + w] for p in out]
    return out


def compose(y, cb, cr, sx, sy, out_w, out_h, filt="lanczos", box=None, gap=None, a=3, window=None, t=None):
    """the whole contract: [..][h][w][3] uint8"""
    yo, cbo, cro = resize_planes(y, cb, cr, sx, sy, out_w, out_h, filt, box, gap, a, window)
    return convert(table(JFIF) if t is None else t, yo, cbo, cro)


# ---- the fixture's cases -----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name sx sy in_w in_h out_w out_h filt box gap content")
CASES = [
    Case("i420_down", 1, 1, 37, 23, 19, 13, "lanczos", None, None, "noise"),             # odd in_w and in_h; 247 pixels: a tail of 3
    Case("i420_1x1", 1, 1, 37, 23, 1, 1, "lanczos", None, None, "noise"),
    Case("i422_down", 1, 0, 33, 31, 20, 30, "lanczos", None, None, "noise"),
    Case("i444_up", 0, 0, 16, 16, 40, 24, "lanczos", None, None, "edges"),
    Case("i420_up_bicubic", 1, 1, 37, 23, 61, 40, "bicubic", None, None, "edges"),
    Case("i420_nearest", 1, 1, 37, 23, 19, 13, "nearest", None, None, "noise"),
    Case("i420_box", 1, 1, 37, 23, 19, 13, "lanczos", (3.5, 2.25, 33.75, 20.5), None, "noise"),
    Case("i420_gap2_both", 1, 1, 81, 49, 5, 3, "lanczos", None, 2.0, "noise"),          # luma reduces by 8, chroma by 4
    Case("i420_gap2_luma", 1, 1, 37, 23, 6, 4, "lanczos", None, 2.0, "noise"),          # luma reduces by 3 x 2, chroma does not
    Case("i420_same", 1, 1, 37, 23, 37, 23, "lanczos", None, None, "noise"),            # luma is a copy, chroma still resizes
    Case("i420_extreme", 1, 1, 37, 23, 19, 13, "lanczos", None, None, "extreme"),
    Case("i420_edges_down", 1, 1, 37, 23, 19, 13, "lanczos", None, None, "edges"),
    Case("i420_even_bilinear", 1, 1, 40, 24, 19, 13, "bilinear", None, None, "noise"),
]
CASE = {c.name: c for c in CASES}


def make_planes(case, frames=1, seed=0):
    """seeded planes of a case: (Y [F][H][W], Cb [F][ch][cw], Cr).  noise; full-range hard edges (blocks of 0 and 255 in all
    three planes, where the filters ring and clip8 works on every output); extreme chroma (cb, cr in {0, 255} over noise luma)"""
    rng = np.random.default_rng(9100 + 17 * CASES.index(case) + seed)
    cw, ch = chroma_size(case.in_w, case.in_h, case.sx, case.sy)
    shapes = ((frames, case.in_h, case.in_w), (frames, ch, cw), (frames, ch, cw))
    if case.content == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
    if case.content == "extreme":
        return (rng.integers(0, 256, shapes[0], dtype=np.uint8),) + tuple(
            (rng.integers(0, 2, s, dtype=np.uint8) * 255).astype(np.uint8) for s in shapes[1:])
    out = []
    for k, s in enumerate(shapes):       # edges: blocks of 3 .. 5 samples, another phase per plane
        yy, xx = np.mgrid[0:s[1], 0:s[2]]
        b = 3 + k
        p = ((((xx + k) // b) + ((yy + 2 * k) // b)) & 1) * 255
        flip = rng.integers(0, 2, (frames, 1, 1))
        out.append(np.where(flip, 255 - p, p).astype(np.uint8))
    return tuple(out)


# ---- frames as they lie in memory ---------------------------------------------------------------------------------------------
Frames = collections.namedtuple("Frames", "buf at frame_stride y_row_stride c_row_stride cb_offset cr_offset layout")
MARGIN = 64


def build(y, cb, cr, layout=PLANAR, y_row_stride=None, c_row_stride=None, base=0, gap=0, frame_gap=0, seed=1, cr_first=False):
    """The planes [F][h][w] laid out as frames: Y rows y_row_stride apart, `gap` bytes, then the chroma planes (PLANAR: Cb, gap,
    Cr; with cr_first Cr, gap, Cb, which is YV12) or the interleaved plane (NV12: Cb first, NV21: Cr first), rows c_row_stride
    apart; frames frame_gap bytes past the extent apart; the first frame MARGIN + base bytes into the buffer.  Every byte the
    layout does not name is noise."""
    f, h, w = y.shape
    _, ch, cw = cb.shape
    crow = cw if layout == PLANAR else 2 * cw
    yrs = w if y_row_stride is None else y_row_stride
    crs = crow if c_row_stride is None else c_row_stride
    assert not cr_first or layout == PLANAR
    cb_off = h * yrs + gap
    cr_off = cb_off + ch * crs + gap if layout == PLANAR else cb_off
    extent = cr_off + ch * crs
    if cr_first:
        cb_off, cr_off = cr_off, cb_off
    fs = extent + frame_gap
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, MARGIN + base + (f - 1) * fs + extent + MARGIN, dtype=np.uint8)
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


def tight(y, cb, cr, layout=PLANAR):
    """[F][B] uint8: the frames back to back in the tight layout, as Context.resize_ycc takes them"""
    s = build(y, cb, cr, layout)
    return s.buf[s.at:s.at + y.shape[0] * s.frame_stride].reshape(y.shape[0], s.frame_stride).copy()


# ---- the shapes of tests/test_resize_ycc_edges_gpu.py, each pinned to the installed Pillow by tests/test_resize_ycc_host.py ------
Shape = collections.namedtuple("Shape", "sx sy in_w in_h out_w out_h filt")
SPLIT_WIDE_CW = (511, 512, 513, 516, 1030)                  # chroma pairs per row around one, two and three workgroups' worth
SPLIT_ODD_WIDE = Shape(1, 1, 1031, 3, 516, 2, "lanczos")    # cw = 516 from an odd width: the chroma pass runs
MERGE_ONLY = ((1, 1500), (2500, 1), (1100, 3))              # 4:4:4 frames that keep their size: w == 1, one long row, rem0 != 0
MANY_FRAMES = Shape(1, 1, 4, 2, 3, 2, "lanczos")


def split_alone_shape(cw):
    """NV12 / NV21 frames of 2 cw x 4 halved: the chroma box is the chroma plane, so chroma is a copy of what the split wrote"""
    return Shape(1, 1, 2 * cw, 4, cw, 2, "lanczos")


def narrow_shapes(subs=((1, 1),), outs=((3, 2), None)):
    """in_w 1 .. 9 x in_h 1 .. 3 (cw 1 .. 5: rows shorter than the way to the next dword), to every size of outs (None: same)"""
    return [Shape(sx, sy, w, h, *(o if o is not None else (w, h)), "lanczos")
            for sx, sy in subs for w in range(1, 10) for h in range(1, 4) for o in outs]


def noise_planes(shape, frames=1, seed=0):
    """seeded noise planes (Y, Cb, Cr) of a Shape, [F][h][w] each"""
    rng = np.random.default_rng([9300, shape.in_w, shape.in_h, shape.sx, shape.sy, seed])
    cw, ch = chroma_size(shape.in_w, shape.in_h, shape.sx, shape.sy)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((frames, shape.in_h, shape.in_w), (frames, ch, cw), (frames, ch, cw)))


def compose_shape(shape, y, cb, cr, **kw):
    return compose(y, cb, cr, shape.sx, shape.sy, shape.out_w, shape.out_h, shape.filt, **kw)
