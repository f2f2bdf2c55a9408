"""The resize dispatcher over the cross product of its options (tests/test_resize_matrix_cfg.py, tests/test_resize_matrix_gpu.py):
the case generator, the legality rules and the route decision (rs_route) restated in plain Python, and the CPU reference of every
case.  No GPU is needed to import this module or to compute an expected array.

A case is one value of every dimension: the sample kind, the geometry, the filter, the options (box / reducing_gap), the window,
the output (bytes or one of the tensor forms), the source layout and the forced path.  cases() is the full product; legality()
sorts it into requests that run (None), requests an entry refuses (the LANCZOS_ERR_* code) and combinations that are no request
at all (NA: no entry takes them, or the value names nothing of its own for that kind).  predict() says which kernels a legal case
launches, written from the conditions of rs_route (csrc/lanczos_resize_route.cpp), against which tests/test_resize_matrix_cfg.py
holds it case by case on the host; predict_dest() says the same of a destination layout.  predict() asks the host planners
(resize_window_plan_host, resize_crops_plan_host) for `fused`, `pass_h`, `pass_v` and `fx` / `fy` and hard-codes none of them.
A destination layout is one more dimension, kept beside the Case tuple: dest_cases() pairs every bytes-out request with pitched
rows and with planes, dest_legality() / DEST_RULES sort the pairs, dest_layout() is the buffer and expected_dest() what a legal
pair leaves in it.  The host entries (tests/test_resize_matrix_host_gpu.py) take the same cases on tight buffers: expected_host(),
host_out_bytes(), host_origins_of(), host_source_of().

Nothing in the reference comes from the code under test: the full bytes of a (kind, geometry, filter, options) are
resize_filters_model.resize's, and everything else is numpy indexing on them with the models of the window, the tensor view, the
crops and the source layout.  The tables are resize_tensor_model.identity_lut / resize_tensor16_model.identity_lut16: every
(output channel, byte) has a word of its own that names both."""
import collections
import functools
import itertools

import numpy as np

import lanczos_hls_amd as L
import patterns as P
import resize_crops_model as RC
import resize_dest_model as DM
import resize_filters_model as F
import resize_source_model as SM
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V

FRAMES = 3
GUARD = 64          # sentinel elements in front of the first output frame and behind the last
FRAME_GAP = 7       # sentinel elements between two output frames
SENTINEL = 0xA5     # every byte of it
NA = "n/a"

Kind = collections.namedtuple("Kind", "channels bps alpha dtype")
KINDS = collections.OrderedDict([
    ("u8x1", Kind(1, 1, False, np.uint8)), ("u8x3", Kind(3, 1, False, np.uint8)), ("u8x4", Kind(4, 1, False, np.uint8)),
    ("rgba", Kind(4, 1, True, np.uint8)),
    ("u16x1", Kind(1, 2, False, np.uint16)), ("u16x3", Kind(3, 2, False, np.uint16)), ("u16x4", Kind(4, 2, False, np.uint16)),
    ("f32x1", Kind(1, 4, False, np.float32)), ("f32x3", Kind(3, 4, False, np.float32)), ("f32x4", Kind(4, 4, False, np.float32))])
U8_KINDS = ("u8x1", "u8x3", "u8x4", "rgba")

# name -> (in_w, in_h, out_w, out_h)
GEOMETRIES = collections.OrderedDict([
    ("down", (61, 47, 37, 29)), ("up", (37, 29, 61, 47)), ("wideK", (90, 40, 20, 17)), ("strips", (523, 37, 300, 21)),
    ("h", (61, 47, 37, 47)), ("v", (61, 47, 61, 29)), ("none", (61, 47, 61, 47)),
    # more than 100 times as tall as wide and shrinking in height: the pass kernels, vertical first (Pillow's order rule)
    ("tall", (7, 750, 13, 77))])
FILTERS = ("lanczos", "bicubic", "nearest")
OPTIONS = ("none", "fbox", "ibox", "gap")
WINDOWS = ("whole", "sub")
SOURCES = ("none", "pitched", "planar")
FORCES = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS, L.RESIZE_CONVERT)
FORCE_NAMES = {L.RESIZE_AUTO: "AUTO", L.RESIZE_FUSED: "FUSED", L.RESIZE_TWO_PASS: "TWO_PASS", L.RESIZE_CONVERT: "CONVERT"}

# elem: bytes of a stored element, 0 = the samples themselves.  mapped: a channel map (channel_map()), per-frame flips D_FLIP and
# the uniform `flip` XORed with them.  layout: "chw", "hwc", or "chwp", CHW with padded rows and planes.  crop: a crop origin per
# frame (ORIGINS), the frame being crop_size().  The issue's four outputs are bytes, f32, bf16map_* and bf16crop_*; bf16, f32map
# and f32crop are here because three of the fifteen fused families (<1, 2>, <1, 4 + mapped>, <1, 4 + mapped + crops>) have no
# other way in.
Output = collections.namedtuple("Output", "elem mapped layout flip crop")
OUTPUTS = collections.OrderedDict([
    ("bytes", Output(0, False, None, 0, False)),
    ("f32", Output(4, False, "chw", 0, False)),
    ("bf16", Output(2, False, "hwc", 0, False)),
    ("f32map", Output(4, True, "chwp", 3, False)),
    ("bf16map_hwc", Output(2, True, "hwc", 1, False)),
    ("bf16map_chwp", Output(2, True, "chwp", 2, False)),
    ("f32crop", Output(4, True, "hwc", 2, True)),
    ("bf16crop_hwc", Output(2, True, "hwc", 3, True)),
    ("bf16crop_chwp", Output(2, True, "chwp", 1, True))])
D_FLIP = (0, 1, 2)

Case = collections.namedtuple("Case", "kind geo filt opt win out src force")


def describe(case):
    return "/".join(str(v) for v in case[:-1]) + "/" + FORCE_NAMES[case.force]


def cases(kinds=None, geos=None):
    """the full product, in the order the GPU test walks it: the forced path changes fastest, then the source"""
    for k, g in itertools.product(kinds or KINDS, geos or GEOMETRIES):
        for rest in itertools.product(FILTERS, OPTIONS, WINDOWS, OUTPUTS, SOURCES, FORCES):
            yield Case(k, g, *rest)


# ---- the arguments of a case ------------------------------------------------------------------------------------------

def box_of(case):
    """the source box: a fractional one; an integer one over the full extent of one axis, the idle one where there is one"""
    iw, ih, _, _ = GEOMETRIES[case.geo]
    if case.opt == "fbox":
        return (1.25, 2.5, iw - 3.75, ih - 1.125)
    if case.opt == "ibox":
        return (0, 3, iw, ih - 3) if case.geo == "v" else (3, 0, iw - 3, ih)
    return None


def gap_of(case):
    return 2.0 if case.opt == "gap" else None


def _odd(n):
    return n if n % 2 else n - 1


def window_size(geo):
    """(w, h) of the sub-window, both odd; on `strips` still wider than one strip of any kind (the widest is 256 columns)"""
    _, _, ow, oh = GEOMETRIES[geo]
    return (271 if geo == "strips" else _odd(ow - 6)), _odd(oh - 8)


def window_of(case):
    """(x0, y0, w, h) with an odd origin and an odd size, or None"""
    return (3, 5) + window_size(case.geo) if case.win == "sub" else None


def crop_size(geo):
    return window_size(geo)


def origins_of(geo):
    """the far corner, one the kernels must clamp on both axes, one odd interior origin"""
    _, _, ow, oh = GEOMETRIES[geo]
    w, h = crop_size(geo)
    assert ow - w >= 2 and oh - h >= 4
    return np.array([(ow - w, oh - h), (ow, -3), (1, 3)], dtype=np.int32)


def channel_map(channels):
    """a map that reorders; of four channels it also drops one"""
    return {1: (0,), 3: (2, 0, 1), 4: (2, 0, 3)}[channels]


def out_channels(case):
    c = KINDS[case.kind].channels
    return channel_map(c) if OUTPUTS[case.out].mapped else tuple(range(c))


def flips_of(case):
    """the flip of every frame as the kernels see it: the uniform one XOR the frame's byte"""
    o = OUTPUTS[case.out]
    return [o.flip ^ f for f in D_FLIP] if o.mapped else [0] * FRAMES


def frame_size(case):
    """(w, h) of a stored frame"""
    _, _, ow, oh = GEOMETRIES[case.geo]
    if OUTPUTS[case.out].crop:
        return crop_size(case.geo)
    return window_size(case.geo) if case.win == "sub" else (ow, oh)


def tensor_strides(case):
    """(chan_stride, row_stride, pix_stride) in elements"""
    w, h = frame_size(case)
    oc = len(out_channels(case))
    lay = OUTPUTS[case.out].layout
    if lay == "chwp":
        return h * (w + 3) + 5, w + 3, 1
    return V.strides(lay, w, h, oc)


def out_geometry(case):
    """(element bytes, elements of a frame's extent, frame stride in elements, elements of the whole buffer)"""
    k, o = KINDS[case.kind], OUTPUTS[case.out]
    w, h = frame_size(case)
    if o.elem:
        item, n = o.elem, V.extent(w, h, len(out_channels(case)), tensor_strides(case))
    else:
        item, n = k.bps, w * h * k.channels
    fs = n + FRAME_GAP
    return item, n, fs, GUARD + (FRAMES - 1) * fs + n + GUARD


def lut_of(case):
    o = OUTPUTS[case.out]
    oc = len(out_channels(case))
    return T32.identity_lut(oc) if o.elem == 4 else T16.identity_lut16(oc)


# ---- contents ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def frames_of(kind, geo):
    """[FRAMES][in_h][in_w][C]: noise and gradient noise with a seed per frame; float frames are unit noise with one inf, one NaN
    and one denormal near the centre, inside the support of the sub-window"""
    k = KINDS[kind]
    iw, ih, _, _ = GEOMETRIES[geo]
    seed = 1000 * list(KINDS).index(kind) + 10 * list(GEOMETRIES).index(geo)
    if k.dtype == np.float32:
        x = np.random.default_rng(seed).standard_normal((FRAMES, ih, iw, k.channels)).astype(np.float32)
        for f in range(FRAMES):
            cy, cx = ih // 2 + f, iw // 2 - f
            x[f, cy, cx, 0] = np.inf
            x[f, cy - 5, (cx + 7) % iw, k.channels - 1] = np.nan      # (the columns wrap on the 7 columns of `tall` alone)
            x[f, cy + 4, (cx - 6) % iw, 0] = np.float32(1e-41)
    elif k.dtype == np.uint16:
        x = np.stack([P.noise(ih, iw, k.channels, seed=seed + f, dtype=np.uint16) for f in range(FRAMES)])
    else:
        x = np.stack([(P.gradient_noise if f == 1 else P.noise)(ih, iw, k.channels, seed=seed + f) for f in range(FRAMES)])
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def source_of(kind, geo, src):
    """the resize_source_model.Source of a layout, every byte it does not name noise.  pitched: rows 7 samples longer, the base 3
    samples off a dword, the frame stride one sample past the extent (in bytes for 8-bit frames, where this is the row-shift
    family of RGBA; wider samples keep their alignment).  planar: odd row and plane strides."""
    k = KINDS[kind]
    x = frames_of(kind, geo)
    ih = GEOMETRIES[geo][1]
    rs, cs, _ = source_strides(kind, geo, src)
    if src == "pitched":
        return SM.build(x, "interleaved", rs, base=(3 * k.bps) % 4, frame_stride=ih * rs + k.bps, seed=3)
    assert src == "planar" and k.bps == 1 and k.channels > 1
    assert rs % 2 and cs % 2
    return SM.build(x, "planar", rs, cs, base=1, frame_stride=k.channels * cs + 1, seed=4)


def source_strides(kind, geo, src):
    """(row_stride, chan_stride, pix_stride) in bytes of source_of()'s layout, without building its frames"""
    k = KINDS[kind]
    iw, ih, _, _ = GEOMETRIES[geo]
    if src == "pitched":
        return (iw * k.channels + 7) * k.bps, k.bps, k.channels * k.bps
    rs = iw + 3 + (iw % 2)
    return rs, ih * rs + 1 + (ih * rs) % 2, k.bps


def source_struct(case, s=None):
    """the ResizeSource of a case, written field by field (a refused layout has to reach the entry)"""
    k = KINDS[case.kind]
    iw, ih, _, _ = GEOMETRIES[case.geo]
    r = L.ResizeSource()
    if case.src == "pitched":
        r.row_stride, r.chan_stride, r.pix_stride = s.row_stride if s else (iw * k.channels + 7) * k.bps, k.bps, k.channels * k.bps
    else:
        rs = s.row_stride if s else (iw + 3) * k.bps
        r.row_stride, r.chan_stride, r.pix_stride = rs, s.chan_stride if s else ih * rs, k.bps
    return r


# ---- legality ---------------------------------------------------------------------------------------------------------

def desc_of(case):
    """the descriptor, its filter set without validation (a refused one has to reach the entry)"""
    k = KINDS[case.kind]
    iw, ih, ow, oh = GEOMETRIES[case.geo]
    d = L.resize_desc(iw, ih, ow, oh, k.channels, 3, alpha=k.alpha, bits=16 if k.bps == 2 else 8, f32=k.bps == 4)
    d.reserved[0] |= L.filter_code(case.filt) << 8
    return d


@functools.lru_cache(maxsize=None)
def _plan(kind, geo, filt, opt, where):
    """the host planners' answer for the whole output, the sub-window or the crop: (fused, pass_h, pass_v, reduces, K, strips,
    chunks, factors, the size of the frame the resize reads)"""
    case = Case(kind, geo, filt, opt, "sub" if where == "sub" else "whole", "bytes", "none", L.RESIZE_AUTO)
    d = desc_of(case)
    if where == "crop":
        p = L.resize_crops_plan_host(d, crop_size(geo), FRAMES, box=box_of(case), reducing_gap=gap_of(case))
    else:
        p = L.resize_window_plan_host(d, window_of(case), FRAMES, box=box_of(case), reducing_gap=gap_of(case))
    return (bool(p.inner.fused), bool(p.pass_h), bool(p.pass_v), p.fx > 1 or p.fy > 1, p.inner.K, p.inner.strips, p.inner.chunks,
            (p.fx, p.fy), (p.reduced_w, p.reduced_h))


Plan = collections.namedtuple("Plan", "fused pass_h pass_v reduces K strips chunks factors reduced")


def plan(case, where=None):
    if where is None:
        where = "crop" if OUTPUTS[case.out].crop else case.win
    return Plan(*_plan(case.kind, case.geo, case.filt, case.opt, where))


# The rules, in the order the entries apply them; the first that holds decides.  NA: no entry takes the combination, or the value
# names nothing of its own there (one plane is a pitched source).
RULES = (
    ("a window together with crops is not a request", lambda c, k, o: o.crop and c.win != "whole", NA),
    ("crops need a tensor output", lambda c, k, o: o.crop and not o.elem, NA),
    ("a planar source needs 3 or 4 channels", lambda c, k, o: c.src == "planar" and k.channels == 1, NA),
    ("nearest is refused for u16", lambda c, k, o: c.filt == "nearest" and k.bps == 2, L.ERR_UNSUPPORTED),
    ("tensor outputs are 8-bit only", lambda c, k, o: o.elem and k.bps != 1, L.ERR_UNSUPPORTED),
    ("planar sources are 8-bit only", lambda c, k, o: c.src == "planar" and k.bps != 1, L.ERR_UNSUPPORTED),
    ("a gap is refused for alpha, u16, f32 and nearest",
     lambda c, k, o: c.opt == "gap" and (k.alpha or k.bps != 1 or c.filt == "nearest"), L.ERR_BAD_ARG),
    ("forced FUSED needs a plan", lambda c, k, o: c.force == L.RESIZE_FUSED and not plan(c).fused, L.ERR_UNSUPPORTED),
)


def legality(case):
    """None: the case runs.  NA: it is no request.  Otherwise the code its entry returns."""
    k, o = KINDS[case.kind], OUTPUTS[case.out]
    for _, holds, verdict in RULES:
        if holds(case, k, o):
            return verdict
    return None


# ---- the dispatcher restated --------------------------------------------------------------------------------------------

PLANAR_OUT = 128            # kRsPlanarOut in the flag word of a fused instance
NORM = 256                  # kRsNorm: the flag word of the lanczos_tensor_norm instances
AUTO_PLANAR_DIRECT = True   # kRsPlanarAutoDirect: under AUTO the fused kernel reads planes as they lie
Pred = collections.namedtuple("Pred", "main alpha reduce pack follower last_kernel tensor_route source_route")
_FLAGS = ((8, "mapped"), (16, "crops"), (32, "planar"), (64, "rowshift"), (PLANAR_OUT, "planar_out"))


def family(bps, tensor):
    """the name of rs_launch_fused<bps, tensor>"""
    return f"fused<{bps}, {' + '.join([str(tensor & 7)] + [n for b, n in _FLAGS if tensor & b])}>"


FUSED_FAMILIES = tuple(family(b, t) for b, t in ((1, 0), (2, 0), (4, 0), (1, 4), (1, 2), (1, 12), (1, 10), (1, 28), (1, 26), (1, 32),
                                                 (1, 44), (1, 42), (1, 64), (1, 76), (1, 74)))


def predict(case):
    """What a legal case launches: the main kernel (a fused family, nearest, copy, crop, pass_h_only, pass_v_only, two_pass,
    v_first -- the two passes in Pillow's order for a tall frame -- or none where the crops gather reads the caller's frames), the alpha pass kernels with their `only`, whether k_reduce runs, the
    pack kernel, the tensor follower, and the three values the context reports (source_route None: the call has no source and
    leaves the last one)."""
    k, o = KINDS[case.kind], OUTPUTS[case.out]
    p = plan(case)
    need_h, need_v = p.pass_h, p.pass_v
    nearest = case.filt == "nearest" and (need_h or need_v)
    force, tensor, crops = case.force, bool(o.elem), o.crop
    pack_kernel = {"none": None, "pitched": "pack_rows", "planar": f"pack<{k.channels}>"}[case.src]
    src, pack, route = (None if case.src == "none" else case.src), None, None
    if src and p.reduces:                          # the reduction reads packed frames
        pack, route, src = pack_kernel, L.SOURCE_PACKED, None
    had_source = src is not None
    rowshift = src == "pitched" and k.alpha        # the pitch of source_of() is no dword multiple
    if src and (force in (L.RESIZE_CONVERT, L.RESIZE_TWO_PASS) or (rowshift and crops) or
                (src == "planar" and (crops or (force == L.RESIZE_AUTO and not AUTO_PLANAR_DIRECT)))):
        src = None
    # the order rule on the frame the resize reads (rs_vertical_first); the planners report fused = 0 for it
    v_first = (need_h and need_v and case.filt != "nearest" and p.reduced[1] > 100 * p.reduced[0] and
               GEOMETRIES[case.geo][3] < p.reduced[1])
    assert not (v_first and p.fused)
    fused_ok = p.fused and not nearest and need_h and need_v and not v_first
    assert not (force == L.RESIZE_FUSED and not fused_ok), "refused: legality() comes first"
    fused = fused_ok and force != L.RESIZE_TWO_PASS
    t_fused = tensor and fused and force != L.RESIZE_CONVERT
    crops_gather = crops and not t_fused
    if had_source:
        if crops_gather or not fused:
            src = None                             # the fused kernel alone reads a source as it lies
        route = L.SOURCE_DIRECT if src else L.SOURCE_PACKED
        if not src:
            pack = pack_kernel
    crops_direct = crops_gather and not nearest and not need_h and not need_v
    whole = case.win == "whole"
    if crops_gather:                               # the bytes of the whole output, by the plan of the whole output
        whole = True
        fused = (plan(case, "whole").fused and not nearest and need_h and need_v and not v_first and
                 force != L.RESIZE_TWO_PASS)
    alpha = ()
    if fused:
        t = o.elem if t_fused else 0
        if src == "planar":
            t = (t + 8 if t else 0) + 32
        elif src and rowshift:
            t = (t + 8 if t else 0) + 64
        elif t_fused and crops:
            t += 8 + 16
        elif t_fused and o.mapped:
            t += 8
        main, last = family(1 if (t or k.bps == 1) else k.bps, t), L.KERNEL_RESIZE_FUSED
    elif nearest:
        main, last = "nearest", L.KERNEL_RESIZE_NEAREST
    elif not need_h and not need_v:
        main, last = ("none" if crops_direct else "copy" if whole else "crop"), L.KERNEL_RESIZE_TWO_PASS
    elif v_first:
        main, last = "v_first", L.KERNEL_RESIZE_TWO_PASS
        if k.alpha:
            alpha = ("v_alpha_first", "h_alpha_last")
    else:
        main, last = ("two_pass" if need_h and need_v else "pass_h_only" if need_h else "pass_v_only"), L.KERNEL_RESIZE_TWO_PASS
        if k.alpha:
            alpha = tuple(f"{ax}_alpha<{'true' if only else 'false'}>" for ax, runs, only in
                          (("h", need_h, not need_v), ("v", need_v, not need_h)) if runs)
    follower = None
    if tensor:
        follower = ("crops_direct" if crops_direct else "crops_scratch" if crops_gather else
                    None if t_fused else "to_tensor_map" if o.mapped else "to_tensor")
    troute = 0 if not tensor else L.TENSOR_FUSED if t_fused else L.TENSOR_CONVERTED
    return Pred(main, alpha, p.reduces, pack, follower, last, troute, route)


DESTS = ("pitched", "planar")
DEST_DIM = ("none",) + DESTS   # the destination dimension; "none" is the case itself, as cases() yields it


def dest_strides(case, dest):
    """(row_stride, chan_stride, pix_stride) in bytes of a destination for the frame of a bytes-out case: pitched rows whose pitch
    is no dword multiple, or planes with padded rows and a padded plane stride"""
    k = KINDS[case.kind]
    w, h = frame_size(case)
    if dest == "pitched":
        rs = w * k.channels * k.bps + k.bps
        return rs + (k.bps if rs % 4 == 0 else 0), k.bps, k.channels * k.bps
    return (w + 3) * k.bps, (h * (w + 3) + 5) * k.bps, k.bps


def dest_cases(kinds=None, geos=None):
    """The destination dimension as (case, dest) pairs, dest in DESTS, over every bytes-out case that is a request, legal or
    refused, in the order of cases() with the destination changing fastest.  A destination with a tensor output is NA (no entry
    takes it), so the Case tuple and the product of cases() stay what they are."""
    for case in cases(kinds, geos):
        if case.out == "bytes" and legality(case) != NA:
            for dest in DESTS:
                yield case, dest


# The rules of a case with a destination, in the order the entry applies them (resize_bytes: the descriptor, the source, the
# destination; then the options and the route inside resize_device): RULES with one row behind the source's.  One plane is the
# pitched shape whatever the sample width (resize_dest_resolve looks at the channel count first, as tests/test_resize_dest_host.py
# holds it to), so planes of wide samples are refused only where there are three or four of them.
_DEST_AFTER = "planar sources are 8-bit only"
DEST_RULES = tuple(
    row for name, holds, verdict in RULES for row in
    [(name, (lambda c, k, o, dest, holds=holds: holds(c, k, o)), verdict)] +
    ([("planar destinations are 8-bit only", lambda c, k, o, dest: dest == "planar" and k.bps != 1 and k.channels > 1,
       L.ERR_UNSUPPORTED)] if name == _DEST_AFTER else []))
assert len(DEST_RULES) == len(RULES) + 1


def dest_legality(case, dest):
    """legality() of a bytes-out case with a destination"""
    assert case.out == "bytes" and dest in DESTS
    k, o = KINDS[case.kind], OUTPUTS[case.out]
    for _, holds, verdict in DEST_RULES:
        if holds(case, k, o, dest):
            return verdict
    return None


def dest_shape(case, dest):
    """"planar" or "interleaved": the shape the library resolves a destination to.  One plane is pitched rows."""
    return "planar" if dest == "planar" and KINDS[case.kind].channels > 1 else "interleaved"


def dest_layout(case, dest, tight=False):
    """The buffer of a destination as a resize_dest_model.Dest full of sentinels: dest_strides(), the first byte of frame 0 at
    residue (3 * bps) % 4 behind GUARD elements, the frames FRAME_GAP elements further apart than the layout's own extent, GUARD
    elements behind the last named byte of the last frame (the padding behind the last row is not part of the buffer).  tight: as
    the host entry takes it, which has no frame stride: the frames at the layout's own extent, no guard, the first byte at 0."""
    k = KINDS[case.kind]
    w, h = frame_size(case)
    rs, cs, _ = dest_strides(case, dest)
    shape = dest_shape(case, dest)
    rs, cs, ps, extent, named = DM.strides((FRAMES, h, w, k.channels), k.bps, shape, rs, cs if shape == "planar" else None)
    at = 0 if tight else GUARD * k.bps + (3 * k.bps) % 4
    fs = extent if tight else extent + FRAME_GAP * k.bps
    total = at + (FRAMES - 1) * fs + named + (0 if tight else GUARD * k.bps)
    return DM.Dest(np.full(total, SENTINEL, dtype=np.uint8), at, shape, rs, cs, ps, fs, extent, named)


def dest_struct(case, dest):
    """the ResizeDest of a case, written field by field (a refused layout has to reach the entry)"""
    r = L.ResizeDest()
    r.row_stride, r.chan_stride, r.pix_stride = dest_strides(case, dest)
    return r


def predict_dest(case, dest):
    """The destination route of a legal bytes-out case, from the contract of lanczos_resize_dest (include/lanczos_hip.h): DIRECT
    where the fused kernel runs, except behind a reducing gap, under forced CONVERT (forced TWO_PASS runs no fused kernel), and
    into planes from RGBA rows it reads as they lie off a dword pitch; UNPACKED everything else.  (No frame here names 2^31 bytes.)"""
    p = predict(case)
    rowshift_direct = KINDS[case.kind].alpha and case.src == "pitched" and p.source_route == L.SOURCE_DIRECT
    direct = (p.main.startswith("fused<") and not p.reduce and case.force != L.RESIZE_CONVERT and
              not (dest == "planar" and rowshift_direct))
    return L.DEST_DIRECT if direct else L.DEST_UNPACKED


def predict_dest_main(case, dest):
    """(the main kernel, the unpack kernel or None) of a legal bytes-out case with a destination.  A destination changes nothing in
    front of the store: the main kernel is predict()'s, except that planes stored DIRECT take the planar-out instance of the
    fused kernel, which exists over an interleaved source (pitched rows included) and over a planar one.  UNPACKED: k_rs_unpack_dest
    of the channel count for planes, k_rs_unpack_dest_rows for every pitched shape."""
    k = KINDS[case.kind]
    p = predict(case)
    planes = dest_shape(case, dest) == "planar"
    if predict_dest(case, dest) == L.DEST_UNPACKED:
        return p.main, f"unpack<{k.channels}>" if planes else "unpack_rows"
    if not planes:
        return p.main, None
    assert p.main in (family(1, 0), family(1, 32)), (describe(case), dest, p.main)
    return family(1, PLANAR_OUT + (32 if p.main == family(1, 32) else 0)), None


def route_line(case, dest=None):
    """the request of a case as tests/native/resize_route_check.hip reads it"""
    k, o = KINDS[case.kind], OUTPUTS[case.out]
    d = desc_of(case)
    box, win = box_of(case), window_of(case)
    iw, ih, _, _ = GEOMETRIES[case.geo]
    f = [d.in_w, d.in_h, d.out_w, d.out_h, d.channels, d.a, d.reserved[0]]
    f += [int(case.opt != "none")] + [repr(float(v)) for v in (box or (0, 0, iw, ih))] + [repr(gap_of(case) or 0.0)]
    f += [1, 0, 0, *crop_size(case.geo), 1] if o.crop else [1, *win, 0] if win else [0, 0, 0, 0, 0, 0]
    f += [o.elem, int(o.mapped), *tensor_strides(case), len(out_channels(case))] if o.elem else [0, 0, 0, 0, 0, 0]
    f += [1, *source_strides(case.kind, case.geo, case.src)] if case.src != "none" else [0, 0, 0, 0]
    f += [1, *dest_strides(case, dest)] if dest else [0, 0, 0, 0]
    return " ".join(str(v) for v in f + [case.force, FRAMES])


MAINS = ("nearest", "copy", "crop", "pass_h_only", "pass_v_only", "two_pass", "v_first", "none")
ALPHA_LEAVES = ("h_alpha<true>", "h_alpha<false>", "v_alpha<true>", "v_alpha<false>", "v_alpha_first", "h_alpha_last")
PACKS = ("pack<3>", "pack<4>", "pack_rows")
FOLLOWERS = ("to_tensor", "to_tensor_map", "crops_scratch", "crops_direct")
_WIDE = tuple(KINDS)
_PLANAR = ("u8x3", "u8x4", "rgba")
# leaf -> the kinds that can reach it (every one of them must)
LEAVES = collections.OrderedDict(
    [(family(1, 0), U8_KINDS), (family(2, 0), ("u16x1", "u16x3", "u16x4")), (family(4, 0), ("f32x1", "f32x3", "f32x4"))] +
    [(family(1, t), U8_KINDS) for t in (4, 2, 12, 10, 28, 26)] +
    [(family(1, t), _PLANAR) for t in (32, 44, 42)] + [(family(1, t), ("rgba",)) for t in (64, 76, 74)] +
    [("nearest", tuple(n for n in KINDS if KINDS[n].bps != 2))] +
    [(m, _WIDE) for m in ("copy", "crop", "pass_h_only", "pass_v_only", "two_pass", "v_first")] + [("none", U8_KINDS)] +
    [(a, ("rgba",)) for a in ALPHA_LEAVES] + [("reduce", ("u8x1", "u8x3", "u8x4"))] +
    [("pack<3>", ("u8x3",)), ("pack<4>", ("u8x4", "rgba")), ("pack_rows", _WIDE)] + [(f, U8_KINDS) for f in FOLLOWERS] +
    # what a destination adds (dest_cases()): the scatter kernels of the UNPACKED route and the planar-out fused families
    [("unpack<3>", ("u8x3",)), ("unpack<4>", ("u8x4", "rgba")), ("unpack_rows", _WIDE)] +
    [(family(1, PLANAR_OUT), _PLANAR), (family(1, PLANAR_OUT + 32), _PLANAR)])
UNPACKS = ("unpack<3>", "unpack<4>", "unpack_rows")
PLANAR_OUT_FAMILIES = (family(1, PLANAR_OUT), family(1, PLANAR_OUT + 32))
DEST_LEAVES = UNPACKS + PLANAR_OUT_FAMILIES


def dest_pairs(kind):
    """the (dest, route) pairs a kind can reach: both routes of pitched rows, and of planes where the validator takes them"""
    k = KINDS[kind]
    return {(d, r) for d in DESTS for r in (L.DEST_DIRECT, L.DEST_UNPACKED) if d == "pitched" or k.bps == 1 or k.channels == 1}


def leaves_of(pred):
    """the names of LEAVES a prediction reaches"""
    out = [pred.main] + list(pred.alpha)
    if pred.reduce:
        out.append("reduce")
    if pred.pack:
        out.append(pred.pack)
    if pred.follower:
        out.append(pred.follower)
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def full_bytes(kind, geo, filt, opt):
    """[FRAMES][out_h][out_w][C]: the whole output of every frame, by the numpy model of Pillow's resize"""
    case = Case(kind, geo, filt, opt, "whole", "bytes", "none", L.RESIZE_AUTO)
    _, _, ow, oh = GEOMETRIES[geo]
    y = F.resize(frames_of(kind, geo), F.NAMES.index(filt), ow, oh, box_of(case), gap_of(case), a=3, alpha=KINDS[kind].alpha)
    y = np.ascontiguousarray(y)
    y.setflags(write=False)
    return y


def cut_of(full, window=None, crop=None, origins=None):
    """the frames a call stores, [FRAMES][h][w][C]: the window slice or the per-frame crops of `full`, or `full`"""
    if crop is not None:
        return RC.slices(full, crop[0], crop[1], origins)
    if window is not None:
        x0, y0, w, h = window
        return full[:, y0:y0 + h, x0:x0 + w]
    return full


def compose(full, window=None, crop=None, origins=None, lut=None, src=None, flips=None, strides=None, base=0,
            frame_stride=None, out=None):
    """The composition every expected array is made by, arguments spelled out (the fixture checks call it directly): the window
    slice or the per-frame crops of `full`, then -- with a table -- the view's scatter into `out`, else the samples themselves."""
    cut = cut_of(full, window, crop, origins)
    if lut is None:
        n = cut[0].size
        for f in range(cut.shape[0]):
            out[base + f * frame_stride:base + f * frame_stride + n] = np.ascontiguousarray(cut[f]).reshape(-1).view(out.dtype)
        return cut.shape[0] * n
    return V.scatter(out, base, cut, lut, src, flips, strides, frame_stride)


def _compose_case(case, base, fs, total, origins):
    """the output buffer of a legal case without a destination: `total` elements of sentinels, the frames `fs` elements apart from
    element `base` on"""
    o = OUTPUTS[case.out]
    item, n, _, _ = out_geometry(case)
    want = np.full(total * item, SENTINEL, dtype=np.uint8).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[item])
    full = full_bytes(case.kind, case.geo, case.filt, case.opt)
    w, h = frame_size(case)
    if o.elem:
        wrote = compose(full, window_of(case), crop_size(case.geo) if o.crop else None, origins if o.crop else None,
                        lut_of(case), out_channels(case), flips_of(case), tensor_strides(case), base, fs, want)
        assert wrote == FRAMES * len(out_channels(case)) * w * h
    else:
        wrote = compose(full, window_of(case), base=base, frame_stride=fs, out=want)
        assert wrote == FRAMES * n
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _expected(kind, geo, filt, opt, win, out):
    case = Case(kind, geo, filt, opt, win, out, "none", L.RESIZE_AUTO)
    _, _, fs, total = out_geometry(case)
    return _compose_case(case, GUARD, fs, total, origins_of(geo))


def expected(case):
    """the whole output buffer of a legal case as elements: sentinels in front, between the frames, behind, and at every element
    of a tensor frame its strides do not name.  It depends on neither the source layout nor the forced path."""
    return _expected(*case[:6])


@functools.lru_cache(maxsize=None)
def _expected_dest(kind, geo, filt, opt, win, dest, tight):
    case = Case(kind, geo, filt, opt, win, "bytes", "none", L.RESIZE_AUTO)
    t = dest_layout(case, dest, tight)
    want = DM.pack(t, cut_of(full_bytes(kind, geo, filt, opt), window_of(case)))
    want.setflags(write=False)
    return want


def expected_dest(case, dest):
    """The whole buffer of dest_layout() as bytes after a legal bytes-out case: sentinels, with the frames compose() stores for the
    case put where the formula of tests/resize_dest_model.py names (its offsets, not restated here).  The guard, the frame gaps,
    row padding and plane padding keep the sentinel."""
    return _expected_dest(*case[:5], dest, False)


# ---- the host entries ---------------------------------------------------------------------------------------------------
#
# lanczos_resize_dest_host takes every bytes-out case, lanczos_resize_tensor_source_host every tensor case.  A host entry has no
# frame stride: the frames lie the layout's own extent apart, and the buffers are exactly as long as include/lanczos_hip.h says:
# extent * FRAMES elements of a tensor, extent * (FRAMES - 1) + named bytes of a destination, w * h * C * bps * FRAMES otherwise.
# The origins rule: the host entry validates its origin array and refuses an origin outside the output with ERR_BAD_ARG, where
# the device entries clamp.  The host walk therefore passes origins_of() after the clamp (host_origins_of(): the same windows,
# so the same expected frames) and keeps origins_of() itself as one refused request per crop output.

def host_origins_of(geo):
    """origins_of() as the kernels clamp them: every origin inside the output, the same crops"""
    _, _, ow, oh = GEOMETRIES[geo]
    w, h = crop_size(geo)
    inside = RC.clamp(origins_of(geo), ow, oh, w, h).astype(np.int32)
    assert not np.array_equal(inside, origins_of(geo))
    return np.ascontiguousarray(inside)


def host_out_bytes(case, dest=None):
    """the size of `out` as the header states it"""
    if dest:
        t = dest_layout(case, dest, tight=True)
        return t.extent * (FRAMES - 1) + t.named
    item, n, _, _ = out_geometry(case)
    return item * n * FRAMES


@functools.lru_cache(maxsize=None)
def _expected_host(kind, geo, filt, opt, win, out):
    case = Case(kind, geo, filt, opt, win, out, "none", L.RESIZE_AUTO)
    _, n, _, _ = out_geometry(case)
    return _compose_case(case, 0, n, n * FRAMES, origins_of(geo)).view(np.uint8)


def expected_host(case, dest=None):
    """the bytes of `out` after a legal case through its host entry: the composition of expected() / expected_dest() on the tight
    strides.  What the strides do not name -- padded tensor rows and planes, destination padding -- holds the sentinel."""
    if dest:
        return _expected_dest(*case[:5], dest, True)
    return _expected_host(*case[:6])


@functools.lru_cache(maxsize=None)
def host_source_of(kind, geo, src):
    """source_of()'s frames and strides re-laid as the host entry reads them: the layout's own extent apart, the first byte on a
    dword"""
    k = KINDS[kind]
    rs, cs, _ = source_strides(kind, geo, src)
    return SM.build(frames_of(kind, geo), "interleaved" if src == "pitched" else "planar", rs, cs if src == "planar" else None,
                    base=0, seed=5)


def first_difference(got, want, f32):
    """None, or (index, got, want) of the first element that differs; float samples by the rule of resize32_model.same"""
    if f32:
        g, w = got.view(np.float32), want.view(np.float32)
        gn, wn = np.isnan(g), np.isnan(w)
        bad = (gn != wn) | (~gn & ~wn & (got != want))
    else:
        bad = got != want
    if not bad.any():
        return None
    i = int(np.argmax(bad))
    return i - GUARD, int(got[i]), int(want[i])
