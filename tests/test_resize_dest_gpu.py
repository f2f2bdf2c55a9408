"""GPU checks of a destination layout (lanczos_resize_dest, lanczos_resize_dest_device / _host): planar and row-pitched result
frames stored by the library.  The yardsticks are the entries WITHOUT a destination, Context.resize / resize_f32 on tightly packed
interleaved frames (themselves pinned to Pillow), and Pillow's fixtures directly; the new path is never compared with itself.
Everything is compared as bytes.  The destination buffers come from tests/resize_dest_model.py: every byte of them holds noise
before the call, and every call is checked twice -- the named bytes are the yardstick's, and EVERY OTHER BYTE STILL HOLDS ITS
NOISE: row padding, plane padding, the gaps between frames, the margins.  With row_stride == w a store one byte too wide lands in a
neighbour's sample, in the padded layouts in the noise; either shows."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_dest_model as DM
import resize_source_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the route AUTO takes for a planar destination the fused kernel can store ("Destinations")
PLANAR_ROUTE = L.DEST_DIRECT


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _dest(d, t, window=None):
    dst = L.resize_dest(d, t.layout, t.row_stride, t.chan_stride if t.layout == "planar" else None, window=window)
    L.resize_dest_validate(d, dst, window=window)
    return dst


def _store(ctx, d, t, x, frames, shape, dtype=np.uint8, path=L.RESIZE_AUTO, source=None, **kw):
    """lanczos_resize_dest_device into the model's buffer.  x: the packed input frames (an array) or a Source of the source model.
    Returns the frames the buffer holds afterwards, after checking that no byte the layout does not name has changed"""
    import torch
    if isinstance(x, SM.Source):
        xd, x_at, in_fs = torch.from_numpy(x.buf).cuda(), x.at, x.frame_stride
        source = L.resize_source(d, x.layout, x.row_stride, x.chan_stride if x.layout == "planar" else None)
    else:
        xd, x_at, in_fs = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).cuda(), 0, 0
    y = torch.from_numpy(t.buf).cuda()
    assert y.data_ptr() % 4 == 0 and xd.data_ptr() % 4 == 0
    ctx.resize_force(path)
    try:
        ctx.resize_device(d, xd.data_ptr() + x_at, y.data_ptr() + t.at, frames, in_frame_stride=in_fs,
                          out_frame_stride=t.frame_stride, stream=torch.cuda.current_stream().cuda_stream, source=source,
                          dest=_dest(d, t, kw.get("window")), **kw)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    raw = y.cpu().numpy()
    item = np.dtype(dtype).itemsize
    full = (frames,) + tuple(shape)
    m = DM.named_mask(t, full, item)
    if not np.array_equal(raw[~m], t.buf[~m]):
        bad = np.flatnonzero((raw != t.buf) & ~m)
        raise AssertionError(f"{len(bad)} bytes the layout does not name were written, first at {int(bad[0]) - t.at} of the frames")
    return DM.unpack(t, full, dtype, raw)


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


# K -> (filter, a, in_w, out_w): _instance_shape of tests/test_resize_source_gpu.py
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 6
    a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    return "lanczos", a, iw, 261


def _planar_layouts(shape, seed=0):
    """four planar destinations for frames of `shape`: base residue 0..3 x row padding 0..3 (one with row_stride == w), plane and
    frame strides off 4 -- between them every residue of a plane row's first byte"""
    n, h, w, c = shape
    out = []
    for k in range(4):
        rs = w + k
        cs = h * rs + (k + 1 - h * rs) % 4                                  # plane strides with residues 1, 2, 3, 0
        gap = (k + 1 - c * cs) % 4                                         # frame strides with residues 1, 2, 3, 0
        out.append(DM.build(shape, "planar", rs, cs, base=(4 - k) % 4, frame_stride=c * cs + gap, seed=seed + k))
    residues = {(t.at + f * t.frame_stride + ch * t.chan_stride + y * t.row_stride) % 4
                for t in out for f in range(n) for ch in range(c) for y in range(h)}
    assert residues == {0, 1, 2, 3} and any(t.chan_stride % 4 for t in out) and any(t.frame_stride % 4 for t in out)
    assert any(t.row_stride == w for t in out) and {t.at % 4 for t in out} == {0, 1, 2, 3}
    return out


PATHS = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_CONVERT)


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_planar_destinations_of_every_fused_instance(ctx, K):
    """k_rs_fused<C, K, ALPHA, kRsPlanarOut> and <..., kRsPlanar + kRsPlanarOut> for C = 3, 4 and alpha: more than one strip with a
    ragged last one, 75 output rows, more than one chunk, four frames, into four planar destinations that between them start a
    plane row at every residue.  DIRECT under AUTO and forced FUSED, UNPACKED under forced CONVERT.  An ALPHA source whose rows
    are pitched off a dword keeps its own direct staging and is unpacked."""
    ih, oh, frames = 37, 75, 4
    for c, alpha in ((3, False), (4, False), (4, True)):
        filt, a, iw, ow = _instance_shape(K, c)
        d = L.resize_desc(iw, ih, ow, oh, c, a, alpha=alpha, filter=filt)
        p = L.resize_plan_host(d, frames)
        assert p.fused and p.K == K and p.strips > 1 and p.chunks > 1 and ow % 2, (c, K, p.K)
        imgs = np.stack([P.noise(ih, iw, c, seed=47 * K + c + 7 * k) for k in range(frames)])
        ref = ctx.resize(imgs, ow, oh, a, alpha=alpha, filter=filt)          # the yardstick: the entry without a destination
        psrc = SM.build(imgs, "planar", iw + 3, ih * (iw + 3) + 1, base=1, frame_stride=c * (ih * (iw + 3) + 1) + 2, seed=K)
        for i, t in enumerate(_planar_layouts((frames, oh, ow, c), seed=K)):
            for path in PATHS:
                for sname, x in (("interleaved", imgs), ("planar", psrc)):
                    before = ctx.last_source_route()
                    got = _store(ctx, d, t, x, frames, (oh, ow, c), path=path)
                    _eq(got, ref, f"K={K} C={c} alpha={alpha} layout {i} path {path} source {sname}")
                    route = L.DEST_UNPACKED if path == L.RESIZE_CONVERT else L.DEST_DIRECT if path == L.RESIZE_FUSED else PLANAR_ROUTE
                    assert ctx.last_dest_route() == route and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, (K, c, path)
                    want = before if sname == "interleaved" else L.SOURCE_PACKED if path == L.RESIZE_CONVERT else L.SOURCE_DIRECT
                    assert ctx.last_source_route() == want, (K, c, path, sname)
        if alpha:   # rows 1 and 2 past a dword: the kRsRowShift staging, and no planar-out instance of it
            t = _planar_layouts((frames, oh, ow, c), seed=K + 9)[1]
            for pad in (1, 2):
                s = SM.build(imgs, "interleaved", iw * c + pad, base=pad, frame_stride=ih * (iw * c + pad) + 3, seed=pad)
                for path in PATHS:
                    _eq(_store(ctx, d, t, s, frames, (oh, ow, c), path=path), ref, f"K={K} alpha rows +{pad} path {path}")
                    assert ctx.last_dest_route() == L.DEST_UNPACKED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
                    assert ctx.last_source_route() == (L.SOURCE_PACKED if path == L.RESIZE_CONVERT else L.SOURCE_DIRECT)


@pytest.mark.parametrize("c,widths", [(3, (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257)), (4, (1, 2, 3, 4, 5, 63, 64, 65, 67))])
def test_widths_around_the_dword_grid(ctx, c, widths):
    """one-strip and two-strip outputs whose plane rows end anywhere in a dword, at all four base residues, with tight rows and
    with padded ones: the partial dwords at both ends of a row, and the rows that are shorter than a dword"""
    ih, oh, frames = 9, 11, 2
    for w in widths:
        iw = w // 2 + 1 if w > 5 else w + 3
        d = L.resize_desc(iw, ih, w, oh, c)
        imgs = np.stack([P.noise(ih, iw, c, seed=3 * w + k) for k in range(frames)])
        ref = ctx.resize(imgs, w, oh)
        assert L.resize_plan_host(d, frames).fused
        for base in range(4):
            for pad in (0, 1 + base % 3):
                rs = w + pad
                cs = oh * rs + (base + 1) % 4
                t = DM.build((frames, oh, w, c), "planar", rs, cs, base=base, frame_stride=c * cs + base, seed=w + base)
                for path in (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_CONVERT):
                    _eq(_store(ctx, d, t, imgs, frames, (oh, w, c), path=path), ref, f"C={c} w={w} base {base} pad {pad} path {path}")
                    assert ctx.last_dest_route() == (L.DEST_UNPACKED if path == L.RESIZE_CONVERT else
                                                     L.DEST_DIRECT if path == L.RESIZE_FUSED else PLANAR_ROUTE)
            # pitched interleaved rows of the same widths: pitches 0..3 past the row
            rs = w * c + base
            t = DM.build((frames, oh, w, c), "interleaved", rs, base=(base + 1) % 4, frame_stride=oh * rs + 1, seed=w)
            for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                _eq(_store(ctx, d, t, imgs, frames, (oh, w, c), path=path), ref, f"C={c} w={w} pitched +{base} path {path}")


def test_pitched_interleaved_is_direct_on_the_fused_kernel(ctx):
    """one shape per sample type; byte pitches a dword multiple and 1..3 off it, 16-bit pitches odd in samples, float pitches
    multiples of 4.  DIRECT on the fused kernel, UNPACKED under CONVERT, the same bytes; the padding keeps its noise"""
    iw, ih, ow, oh, frames = 90, 41, 70, 35, 3
    rng = np.random.default_rng(8)
    cases = [(1, {}, np.uint8), (3, {}, np.uint8), (4, {}, np.uint8), (4, {"alpha": True}, np.uint8), (3, {"bits": 16}, np.uint16),
             (3, {"f32": True}, np.float32), (1, {"f32": True}, np.float32)]
    for c, kw, dtype in cases:
        b = np.dtype(dtype).itemsize
        d = L.resize_desc(iw, ih, ow, oh, c, **kw)
        assert L.resize_plan_host(d, frames).fused
        if dtype == np.float32:
            imgs = rng.standard_normal((frames, ih, iw, c)).astype(np.float32)
            ref = ctx.resize_f32(imgs, ow, oh)
        else:
            imgs = rng.integers(0, 256 ** b, (frames, ih, iw, c)).astype(dtype)
            ref = ctx.resize(imgs, ow, oh, **{k: v for k, v in kw.items() if k == "alpha"})
        tight = ow * c * b
        for pad, base in (((-tight) % 4 + 8, 0), (13, 1), (1, 2), (2, 3), (3, 0), (0, 3)):
            if base % b or (b == 4 and (pad * b) % 4):
                continue
            rs = tight + pad * b
            t = DM.build((frames, oh, ow, c), "interleaved", rs, base=base, frame_stride=oh * rs + 3 * b, seed=pad, itemsize=b)
            # (a tight destination is the call without one, DIRECT whatever is forced)
            for path, route in ((L.RESIZE_AUTO, L.DEST_DIRECT), (L.RESIZE_FUSED, L.DEST_DIRECT),
                                (L.RESIZE_CONVERT, L.DEST_UNPACKED if pad else L.DEST_DIRECT)):
                got = _store(ctx, d, t, imgs, frames, (oh, ow, c), dtype, path=path)
                _eq(got, ref, f"C={c} {kw} pad {pad} base {base} path {path}")
                assert ctx.last_dest_route() == route and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, (c, kw, pad, path)
        # ... from a planar and from a pitched source as well (8-bit, three or four channels)
        if b == 1 and c >= 3:
            rs = tight + 5
            t = DM.build((frames, oh, ow, c), "interleaved", rs, base=1, frame_stride=oh * rs + 2, seed=9)
            for s in (SM.build(imgs, "planar", iw + 3, ih * (iw + 3) + 1, base=1, seed=5),
                      SM.build(imgs, "interleaved", iw * c + 7, base=3, seed=6)):
                _eq(_store(ctx, d, t, s, frames, (oh, ow, c)), ref, f"C={c} {kw} source {s.layout}")
                assert ctx.last_dest_route() == L.DEST_DIRECT and ctx.last_source_route() == L.SOURCE_DIRECT


def _two_dests(shape, itemsize=1):
    n, h, w, c = shape
    out = {"pitched": DM.build(shape, "interleaved", (w * c + 7) * itemsize, base=(3 * itemsize) % 4,
                               frame_stride=(h * (w * c + 7) + 1) * itemsize, seed=6, itemsize=itemsize)}
    if itemsize == 1 and c >= 3:
        out["planar"] = DM.build(shape, "planar", w + 3, h * (w + 3) + 1, base=1, frame_stride=c * (h * (w + 3) + 1) + 2, seed=5)
    return out


def test_unpacked_routes(ctx):
    """everything the fused kernel does not run stores its packed result in scratch, and the scatter follows"""
    frames = 3
    imgs = np.stack([P.gradient_noise(120, 160, 3, seed=12 + k) for k in range(frames)])
    big = np.stack([P.noise(300, 400, 3, seed=2 + k) for k in range(frames)])
    rgba = np.stack([P.noise(120, 160, 4, seed=5 + k) for k in range(frames)])
    #        name, frames, out_w, out_h, path, keywords, UNPACKED by definition
    cases = [("two pass", imgs, 64, 48, L.RESIZE_TWO_PASS, {}, True), ("h only", imgs, 77, 120, L.RESIZE_AUTO, {}, True),
             ("v only", imgs, 160, 50, L.RESIZE_AUTO, {}, True), ("nearest", imgs, 71, 53, L.RESIZE_AUTO, {"filter": "nearest"}, True),
             ("copy", imgs, 160, 120, L.RESIZE_AUTO, {}, True), ("crop", imgs, 160, 120, L.RESIZE_AUTO, {"window": (7, 5, 101, 77)}, True),
             ("gap 2", big, 40, 30, L.RESIZE_AUTO, {"reducing_gap": 2.0}, True),
             ("alpha two pass", rgba, 64, 48, L.RESIZE_TWO_PASS, {"alpha": True}, True),
             ("box", imgs, 64, 48, L.RESIZE_AUTO, {"box": (10.25, 7.5, 131.75, 99.125)}, False),
             ("box", imgs, 64, 48, L.RESIZE_CONVERT, {"box": (10.25, 7.5, 131.75, 99.125)}, True)]
    for name, x, ow, oh, path, kw, unpacked in cases:
        _, ih, iw, c = x.shape
        ctx.resize_force(path)
        try:
            ref = ctx.resize(x, ow, oh, **kw)
        finally:
            ctx.resize_force(L.RESIZE_AUTO)
        dkw = {k: v for k, v in kw.items() if k not in ("filter", "alpha")}
        d = L.resize_desc(iw, ih, ow, oh, c, alpha=kw.get("alpha", False), filter=kw.get("filter", "lanczos"))
        for lname, t in _two_dests(ref.shape).items():
            got = _store(ctx, d, t, x, frames, ref.shape[1:], path=path, **dkw)
            _eq(got, ref, f"{name} {lname}")
            if unpacked or lname == "planar":
                assert ctx.last_dest_route() == (L.DEST_UNPACKED if unpacked else PLANAR_ROUTE), (name, lname)
            else:
                assert ctx.last_dest_route() == L.DEST_DIRECT, (name, lname)
            if name == "nearest":
                assert ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
            if name == "gap 2":
                assert L.resize_plan_host(d, frames, reducing_gap=2.0).fx > 1
    # 16-bit and float samples on the two-pass kernels into pitched rows
    rng = np.random.default_rng(3)
    for kw, dtype in (({"bits": 16}, np.uint16), ({"f32": True}, np.float32)):
        x = rng.integers(0, 60000, (frames, 41, 90, 3)).astype(dtype)
        ref = ctx.resize_f32(x, 70, 35) if dtype == np.float32 else ctx.resize(x, 70, 35)
        d = L.resize_desc(90, 41, 70, 35, 3, **kw)
        t = _two_dests(ref.shape, np.dtype(dtype).itemsize)["pitched"]
        _eq(_store(ctx, d, t, x, frames, ref.shape[1:], dtype, path=L.RESIZE_TWO_PASS), ref, f"two pass {kw}")
        assert ctx.last_dest_route() == L.DEST_UNPACKED and ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS


def test_a_window_into_planes(ctx):
    """341 x 256, the centre 224 x 224: a destination shaped for the window, tight (N x C x 224 x 224) and padded"""
    frames, iw, ih, ow, oh = 3, 500, 375, 341, 256
    win = L.center_window(ow, oh, 224, 224)
    imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=60 + k) for k in range(frames)])
    ref = ctx.resize(imgs, ow, oh, window=win)
    d = L.resize_desc(iw, ih, ow, oh, 3)
    assert L.resize_window_plan_host(d, win, frames).inner.fused
    shape = (frames, 224, 224, 3)
    for t in (DM.build(shape, "planar", seed=1), DM.build(shape, "planar", 227, 224 * 227 + 3, base=3, seed=2),
              DM.build(shape, "interleaved", 224 * 3 + 5, base=1, seed=3)):
        for path in PATHS:
            _eq(_store(ctx, d, t, imgs, frames, shape[1:], path=path, window=win), ref, f"window {t.layout} {t.row_stride} path {path}")
            direct = t.layout == "interleaved" and path != L.RESIZE_CONVERT
            assert ctx.last_dest_route() == (L.DEST_DIRECT if direct else L.DEST_UNPACKED if t.layout == "interleaved" or
                                             path == L.RESIZE_CONVERT else PLANAR_ROUTE)
    # the tight planar destination is torch's N x C x H x W
    import torch
    y = torch.zeros((frames, 3, 224, 224), dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(imgs).cuda()
    ctx.resize_device(d, x.data_ptr(), y.data_ptr(), frames, window=win, dest=L.resize_dest(d, "planar", window=win))
    torch.cuda.synchronize()
    _eq(y.permute(0, 2, 3, 1).contiguous().cpu().numpy(), ref, "N x C x H x W")


@pytest.mark.parametrize("fixture,alpha", [("resize_pillow.npz", False), ("resize_pillow_alpha.npz", True)])
def test_pillow_directly(ctx, fixture, alpha):
    """Pillow's images straight into padded planes (one plane: pitched rows): the bytes are Pillow's outputs"""
    z = np.load(os.path.join(GOLDEN, fixture))
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 12
    for i, name in enumerate(names):
        img, out = z[f"{name}_in"], z[f"{name}_out"]
        img3, out3 = (img[..., None], out[..., None]) if img.ndim == 2 else (img, out)
        (ih, iw, c), (oh, ow) = img3.shape, out3.shape[:2]
        d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
        rs = ow + 1 + i % 3
        t = DM.build((1, oh, ow, c), "planar", rs, oh * rs + i % 2, base=i % 4, seed=i)
        _eq(_store(ctx, d, t, img3[None], 1, (oh, ow, c))[0], out3, f"{fixture} {name}")
        if c >= 3:   # the host entry
            _eq(ctx.resize(img3, ow, oh, alpha=alpha, planar_out=True), out3.transpose(2, 0, 1), f"host {name}")


def test_both_ends_planar(ctx):
    """N x C x H x W in, N x C x h x w out, and the result of one call is the source of the next"""
    frames = 3
    imgs = np.stack([P.gradient_noise(96, 130, 3, seed=70 + k) for k in range(frames)])
    mid = ctx.resize(imgs, 77, 59)
    ref = ctx.resize(mid, 131, 90)
    d1, d2 = L.resize_desc(130, 96, 77, 59, 3), L.resize_desc(77, 59, 131, 90, 3)
    s = SM.build(imgs, "planar", 133, 96 * 133 + 1, base=3, seed=1)
    t1 = DM.build((frames, 59, 77, 3), "planar", 79, 59 * 79 + 2, base=1, frame_stride=3 * (59 * 79 + 2) + 1, seed=2)
    _eq(_store(ctx, d1, t1, s, frames, (59, 77, 3)), mid, "first call")
    assert ctx.last_source_route() == L.SOURCE_DIRECT and ctx.last_dest_route() == PLANAR_ROUTE
    s2 = DM.as_source(t1)._replace(buf=DM.pack(t1, mid))                 # the first call's destination, as it was left
    t2 = DM.build((frames, 90, 131, 3), "planar", 131, 90 * 131 + 3, base=2, seed=3)
    _eq(_store(ctx, d2, t2, s2, frames, (90, 131, 3)), ref, "second call")


def test_host_entries(ctx):
    """planar_out=True on Context.resize, alone and with planar=True; lanczos_resize_dest_host keeps the unnamed bytes of `out`"""
    import ctypes
    imgs = np.stack([P.noise(41, 90, 3, seed=k) for k in range(3)])
    chw = np.ascontiguousarray(imgs.transpose(0, 3, 1, 2))
    for ow, oh, kw in ((70, 35, {}), (70, 41, {}), (70, 35, {"window": (3, 2, 60, 29)}), (30, 14, {"reducing_gap": 1.5})):
        want = ctx.resize(imgs, ow, oh, **kw).transpose(0, 3, 1, 2)
        _eq(ctx.resize(imgs, ow, oh, planar_out=True, **kw), want, f"host {ow}x{oh} {kw}")
        _eq(ctx.resize(chw, ow, oh, planar=True, planar_out=True, **kw), want, f"host planar in {ow}x{oh} {kw}")
        _eq(ctx.resize(imgs[0], ow, oh, planar_out=True, **kw), want[0], "one frame")
    rgba = np.stack([P.noise(41, 90, 4, seed=9 + k) for k in range(2)])
    _eq(ctx.resize(rgba, 70, 35, alpha=True, planar_out=True), ctx.resize(rgba, 70, 35, alpha=True).transpose(0, 3, 1, 2), "alpha")
    with pytest.raises(L.LanczosError):
        ctx.resize(imgs.astype(np.uint16), 70, 35, planar_out=True)
    # the C entry on the model's buffers: the host array's padding keeps its noise, the last frame ends at its last named byte
    d = L.resize_desc(90, 41, 70, 35, 3)
    ref = ctx.resize(imgs, 70, 35)
    for t in _two_dests(ref.shape).values():
        t = DM.build(ref.shape, t.layout, t.row_stride, t.chan_stride if t.layout == "planar" else None, base=t.at % 4, seed=4)
        buf = t.buf.copy()
        rc = L._lib().lanczos_resize_dest_host(ctx._h, ctypes.byref(d), None, None, None, ctypes.byref(_dest(d, t)),
                                               imgs.ctypes.data, buf.ctypes.data + t.at, 3)
        assert rc == L.OK
        m = DM.named_mask(t, ref.shape)
        assert np.array_equal(buf[~m], t.buf[~m])
        _eq(DM.unpack(t, ref.shape, buf=buf), ref, f"dest_host {t.layout}")
    # 16-bit samples into pitched rows
    x16 = np.random.default_rng(1).integers(0, 65536, (2, 41, 90, 3)).astype(np.uint16)
    d16, ref16 = L.resize_desc(90, 41, 70, 35, 3, bits=16), ctx.resize(x16, 70, 35)
    t = DM.build(ref16.shape, "interleaved", 70 * 3 * 2 + 6, seed=8, itemsize=2)
    buf = t.buf.copy()
    rc = L._lib().lanczos_resize_dest_host(ctx._h, ctypes.byref(d16), None, None, None, ctypes.byref(_dest(d16, t)),
                                           x16.ctypes.data, buf.ctypes.data + t.at, 2)
    m = DM.named_mask(t, ref16.shape, 2)
    assert rc == L.OK and np.array_equal(buf[~m], t.buf[~m])
    _eq(DM.unpack(t, ref16.shape, np.uint16, buf), ref16, "dest_host u16")


def test_device_argument_checks(ctx):
    import ctypes
    import torch
    iw, ih, ow, oh = 90, 41, 70, 35
    d = L.resize_desc(iw, ih, ow, oh, 3)
    imgs = np.stack([P.noise(ih, iw, 3, seed=k) for k in range(2)])
    x = torch.from_numpy(imgs).cuda()
    y = torch.zeros(2 * ow * oh * 3 + 4096, dtype=torch.uint8, device="cuda")
    before = ctx.last_dest_route()

    def dst(rs=ow, cs=ow * oh, ps=1, reserved=0):
        t = L.ResizeDest()
        t.row_stride, t.chan_stride, t.pix_stride = rs, cs, ps
        t.reserved[1] = reserved
        return t
    pitched = L.resize_dest(d, "interleaved", row_stride=3 * ow + 2)
    bad = [dict(dest=dst(rs=ow - 1)), dict(dest=dst(cs=ow * oh - 1)), dict(dest=dst(ps=3)), dict(dest=dst(reserved=1)),
           dict(dest=dst(), out_frame_stride=3 * ow * oh - 1),                                # a frame stride below the named bytes
           dict(dest=dst(rs=ow + 5, cs=oh * (ow + 5)), out_frame_stride=2 * oh * (ow + 5) + (oh - 1) * (ow + 5) + ow - 1),
           dict(dest=pitched, out_frame_stride=(oh - 1) * (3 * ow + 2) + 3 * ow - 1)]
    for kw in bad:
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
    # ... the last named byte + 1 is enough: frames may lie in each other's padding
    ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, dest=pitched, out_frame_stride=(oh - 1) * (3 * ow + 2) + 3 * ow)
    ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, dest=dst(rs=ow + 5, cs=oh * (ow + 5)),
                      out_frame_stride=2 * oh * (ow + 5) + (oh - 1) * (ow + 5) + ow)
    torch.cuda.synchronize()
    before = ctx.last_dest_route()
    assert before == PLANAR_ROUTE
    # floats: a pitch, a base or a frame stride off 4; 16-bit: off 2; planar wide samples
    df, d16 = L.resize_desc(iw, ih, ow, oh, 3, f32=True), L.resize_desc(iw, ih, ow, oh, 3, bits=16)
    xf = torch.zeros(2 * iw * ih * 3, dtype=torch.float32, device="cuda")
    yf = torch.zeros(2 * (ow * 3 + 4) * oh + 64, dtype=torch.float32, device="cuda")
    tf = L.ResizeDest()
    for rs, off, fs, code in ((ow * 12 + 2, 0, 0, L.ERR_BAD_ARG), (ow * 12 + 8, 2, 0, L.ERR_BAD_ARG),
                              (ow * 12 + 8, 0, oh * (ow * 12 + 8) + 2, L.ERR_BAD_ARG)):
        tf.row_stride, tf.chan_stride, tf.pix_stride = rs, 4, 12
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(df, xf.data_ptr(), yf.data_ptr() + off, 2, dest=tf, out_frame_stride=fs)
        assert e.value.code == code, (rs, off, fs)
    tf.row_stride, tf.chan_stride, tf.pix_stride = ow * 6 + 1, 2, 6
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_device(d16, xf.data_ptr(), yf.data_ptr(), 2, dest=tf)
    assert e.value.code == L.ERR_BAD_ARG
    tf.row_stride, tf.chan_stride, tf.pix_stride = ow * 6 + 2, 2, 6
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_device(d16, xf.data_ptr(), yf.data_ptr() + 1, 2, dest=tf)
    assert e.value.code == L.ERR_BAD_ARG
    tf.row_stride, tf.chan_stride, tf.pix_stride = ow * 2, ow * oh * 2, 2
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_device(d16, xf.data_ptr(), yf.data_ptr(), 2, dest=tf)
    assert e.value.code == L.ERR_UNSUPPORTED
    assert ctx.last_dest_route() == before                                  # a refused call leaves the route of the last good one
    # a tight interleaved destination is the call without one: the plan's kernel, DIRECT, the same bytes, under CONVERT too
    ya, yb = torch.zeros_like(y), torch.zeros_like(y)
    ctx.resize_force(L.RESIZE_CONVERT)
    try:
        ctx.resize_device(d, x.data_ptr(), ya.data_ptr(), 2, dest=L.resize_dest(d, "interleaved"))
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    ka, ra = ctx.last_kernel(), ctx.last_dest_route()
    ctx.resize_device(d, x.data_ptr(), yb.data_ptr(), 2)
    torch.cuda.synchronize()
    assert ka == ctx.last_kernel() == L.KERNEL_RESIZE_FUSED and ra == L.DEST_DIRECT and ctx.last_dest_route() == L.DEST_DIRECT
    assert torch.equal(ya, yb) and ya.any()
    # a NULL destination is lanczos_resize_source_device: the same bytes, and the last destination route stays what it was
    ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, dest=dst())
    assert ctx.last_dest_route() == PLANAR_ROUTE
    xs = torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 3, 1, 2))).cuda()
    y2, y3 = torch.zeros_like(y), torch.zeros_like(y)
    src = L.resize_source(d, "planar")
    rc = L._lib().lanczos_resize_dest_device(ctx._h, ctypes.byref(d), None, None, ctypes.byref(src), None, xs.data_ptr(),
                                             y2.data_ptr(), 2, 0, 0, None)
    ctx.resize_device(d, xs.data_ptr(), y3.data_ptr(), 2, source=src)
    torch.cuda.synchronize()
    assert rc == L.OK and ctx.last_dest_route() == PLANAR_ROUTE and torch.equal(y2, y3) and torch.equal(y2, yb)


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_CONVERT])
def test_capture_replay_with_a_destination(path):
    """A captured call with a destination, pitched rows (DIRECT under FUSED, UNPACKED under CONVERT) and planes, replays right after
    the destination was overwritten; an eager call of a larger shape on the same context afterwards is right as well"""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow, frames = 93 + path, 139, 47, 61, 3      # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3)
        assert L.resize_plan_host(d, frames).fused
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=9 + k) for k in range(frames)])
        ref = c.resize(imgs, ow, oh)
        c.close()
        c = L.Context(0)                                        # a context that has not seen the shape
        c.resize_force(path)
        shape = (frames, oh, ow, 3)
        x = torch.from_numpy(imgs).cuda()
        for t in (DM.build(shape, "interleaved", ow * 3 + 5, base=1, seed=4), DM.build(shape, "planar", ow + 3, oh * (ow + 3) + 1, base=3, seed=5)):
            m = DM.named_mask(t, shape)
            y = torch.from_numpy(t.buf).cuda()
            g = torch.cuda.CUDAGraph()
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="relaxed"):
                c.resize_device(d, x.data_ptr(), y.data_ptr() + t.at, frames, out_frame_stride=t.frame_stride,
                                stream=torch.cuda.current_stream().cuda_stream, dest=_dest(d, t))
            direct = t.layout == "interleaved" and path == L.RESIZE_FUSED
            assert c.last_dest_route() == (L.DEST_DIRECT if direct else L.DEST_UNPACKED if t.layout == "interleaved" or
                                           path == L.RESIZE_CONVERT else PLANAR_ROUTE)
            torch.cuda.synchronize()
            assert np.array_equal(y.cpu().numpy(), t.buf)           # captured, not run
            for k in range(2):
                noise = np.random.default_rng(k).integers(1, 256, t.buf.size, dtype=np.uint8)
                y.copy_(torch.from_numpy(noise))                    # the destination overwritten
                g.replay()
                torch.cuda.synchronize()
                raw = y.cpu().numpy()
                assert np.array_equal(raw[~m], noise[~m]), "replay wrote bytes the layout does not name"
                _eq(DM.unpack(t, shape, buf=raw), ref, f"replay {k} {t.layout}")
            # eager, a larger result (larger scratch on the UNPACKED route), the same context: the graph's blocks stay alive
            big = np.stack([P.noise(ih + 40, iw + 60, 3, seed=k) for k in range(frames)])
            c.resize_force(L.RESIZE_AUTO)
            want = c.resize(big, ow + 50, oh + 30)
            c.resize_force(path)
            _eq(c.resize(big, ow + 50, oh + 30, planar_out=True), want.transpose(0, 3, 1, 2), "eager after the capture")
            y.copy_(torch.from_numpy(t.buf))
            g.replay()
            torch.cuda.synchronize()
            _eq(DM.unpack(t, shape, buf=y.cpu().numpy()), ref, "replay after the eager call")
            del g
    finally:
        c.close()
