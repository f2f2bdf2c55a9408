"""GPU checks of a source layout (lanczos_resize_source, lanczos_resize_source_* / lanczos_resize_tensor_source_*): planar and
row-pitched frames read as they lie.  The yardsticks are the entries WITHOUT a source, Context.resize / resize_f32 on the tightly
packed interleaved copy (themselves pinned to Pillow), the view model over those bytes, and Pillow's fixtures directly; the new
path is never compared with itself.  Everything is compared as bytes or bit patterns.  The source buffers come from
tests/resize_source_model.py: every byte the layout does not name holds noise, and the outputs lie between sentinels."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_crops_model as RC
import resize_source_model as SM
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLIPS = [0, 1, 2, 3]
MAPS = {3: ((2, 1, 0), (2, 0)), 4: ((2, 1, 0), (3, 0, 1, 2))}   # one that reorders, one that drops (C = 4: one that rotates)
# the route AUTO takes for a planar source the fused kernel can run ("Sources": the measurements behind it)
AUTO_PLANAR = L.SOURCE_DIRECT
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _lut(oc, dtype):
    return T32.identity_lut(oc) if dtype == "float32" else T16.identity_lut16(oc)


def _source(d, s):
    src = L.resize_source(d, s.layout, s.row_stride, s.chan_stride if s.layout == "planar" else None)
    L.resize_source_validate(d, src)
    return src


def _bytes(ctx, d, s, frames, shape, dtype=np.uint8, path=L.RESIZE_AUTO, **kw):
    """lanczos_resize_source_device on the model's buffer, into frames of `shape` between sentinels, 3 elements apart"""
    import torch
    n = int(np.prod(shape))
    item = np.dtype(dtype).itemsize
    fs = n + 3
    total = GUARD + (frames - 1) * fs + n + GUARD
    y = torch.full((total * item,), 0xA5, dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(s.buf).cuda()
    assert x.data_ptr() % 4 == 0
    ctx.resize_force(path)
    try:
        ctx.resize_device(d, x.data_ptr() + s.at, y.data_ptr() + GUARD * item, frames, in_frame_stride=s.frame_stride,
                          out_frame_stride=fs * item, stream=torch.cuda.current_stream().cuda_stream, source=_source(d, s), **kw)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    raw = y.cpu().numpy()
    keep = np.zeros(total * item, dtype=bool)
    out = []
    for f in range(frames):
        a = (GUARD + f * fs) * item
        keep[a:a + n * item] = True
        out.append(raw[a:a + n * item].view(dtype).reshape(shape))
    assert (raw[~keep] == 0xA5).all(), "a byte outside the output frames was written"
    return np.stack(out)


def _tensor(ctx, d, s, frames, ref, lut, src, flips, layout, dtype, path=L.RESIZE_AUTO, **kw):
    """lanczos_resize_tensor_source_device into sentinels; returns the words [F][...] as Context.resize_tensor shapes them, after
    checking that every word the view does not name still holds the sentinel (the model's scatter over `ref` names them)"""
    import torch
    elem = 4 if dtype == "float32" else 2
    word, signed, SENT = (np.uint32, np.int32, 0xA5A5A5A5) if elem == 4 else (np.uint16, np.int16, 0xA5A5)
    _, h, w, _ = ref.shape
    oc = len(src)
    st = V.strides(layout, w, h, oc)
    n = V.extent(w, h, oc, st)
    fs = n + 5
    total = GUARD + (frames - 1) * fs + n + GUARD
    want = np.full(total, SENT, dtype=word)
    assert V.scatter(want, GUARD, ref, lut, src, flips, st, fs) == frames * oc * h * w
    y = torch.from_numpy(np.full(total, SENT, dtype=word).view(signed)).cuda()
    x = torch.from_numpy(s.buf).cuda()
    dl = torch.from_numpy(V.words(lut).view(signed)).cuda()
    df = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_tensor_device(d, x.data_ptr() + s.at, y.data_ptr() + elem * GUARD, frames, dl.data_ptr(), st,
                                 in_frame_stride=s.frame_stride, out_frame_stride=elem * fs,
                                 stream=torch.cuda.current_stream().cuda_stream, dtype=dtype, channels_out=src,
                                 d_flip=df.data_ptr(), source=_source(d, s), **kw)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    got = y.cpu().numpy().view(word)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} words differ, first at {int(bad[0][0]) - GUARD}: {int(got[bad[0][0]]):#x} != "
                             f"{int(want[bad[0][0]]):#x}")


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


# K -> (filter, a, in_w, out_w): _instance_shape of tests/test_resize_tensor_view_gpu.py
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 6
    a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    return "lanczos", a, iw, 261


def _planar_layouts(imgs):
    """four planar sources of the same frames: base residue 0..3 x row padding 0..3, plane and frame strides off 4 -- between
    them every residue of a plane row's first byte"""
    _, ih, iw, c = imgs.shape
    out = []
    for k in range(4):
        rs = iw + k
        cs = ih * rs + (0, 1, 2, 3)[(k + 1) % 4]
        out.append(SM.build(imgs, "planar", rs, cs, base=(4 - k) % 4, frame_stride=c * cs + (3, 1, 2, 0)[k], seed=k))
    residues = {(s.at + ch * s.chan_stride + y * s.row_stride) % 4 for s in out for ch in range(c) for y in range(ih)}
    assert residues == {0, 1, 2, 3} and any(s.chan_stride % 4 for s in out) and any(s.frame_stride % 4 for s in out)
    assert any(s.row_stride == iw for s in out) and {s.at % 4 for s in out} == {0, 1, 2, 3}
    return out


ROUTES = ((L.RESIZE_AUTO, AUTO_PLANAR), (L.RESIZE_FUSED, L.SOURCE_DIRECT), (L.RESIZE_CONVERT, L.SOURCE_PACKED))


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_every_planar_fused_instance(ctx, K):
    """k_rs_fused<C, K, ALPHA, kRsPlanar>, <..., 4 + 8 + 32> and <..., 2 + 8 + 32> for C = 3, 4 and alpha: more than one strip
    with a ragged last one, 75 output rows, more than one chunk; four frames (flips 0..3) in four planar layouts.  Bytes equal
    Context.resize of the packed copy, tensors the view model over those bytes, under AUTO, forced FUSED and forced CONVERT."""
    ih, oh, frames = 37, 75, 4
    for c, alpha in ((3, False), (4, False), (4, True)):
        filt, a, iw, ow = _instance_shape(K, c)
        d = L.resize_desc(iw, ih, ow, oh, c, a, alpha=alpha, filter=filt)
        p = L.resize_plan_host(d, frames)
        assert p.fused and p.K == K and p.strips > 1 and p.chunks > 1 and ow % 2, (c, K, p.K)
        imgs = np.stack([P.noise(ih, iw, c, seed=41 * K + c + 7 * k) for k in range(frames)])
        ref = ctx.resize(imgs, ow, oh, a, alpha=alpha, filter=filt)          # the yardstick: the entry without a source
        layouts = _planar_layouts(imgs)
        combos = [(dt, lay, m) for dt in ("float32", "bfloat16") for lay in ("chw", "hwc") for m in MAPS[c]]
        for i, s in enumerate(layouts):
            assert np.array_equal(SM.unpack(s, imgs.shape), imgs)
            for path, route in ROUTES:
                _eq(_bytes(ctx, d, s, frames, (oh, ow, c), path=path), ref, f"K={K} C={c} alpha={alpha} layout {i} path {path}")
                assert ctx.last_source_route() == route and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, (K, c, path)
                for dt, lay, m in combos[i::4]:   # eight combinations over the four layouts, alpha included
                    lut = _lut(len(m), dt)
                    _tensor(ctx, d, s, frames, ref, lut, m, FLIPS, lay, dt, path=path)
                    assert ctx.last_source_route() == route, (K, c, path, dt)
                    assert ctx.last_tensor_route() == (L.TENSOR_CONVERTED if path == L.RESIZE_CONVERT else L.TENSOR_FUSED)


def test_pitched_interleaved_is_direct_on_the_fused_kernel(ctx):
    """one shape per sample type; byte pitches odd, 16-bit pitches odd in samples, float pitches multiples of 4"""
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
        for pad, base in ((7, 0), (13, 1), (1, 2), (0, 3)):
            if base % b:
                continue
            rs = iw * c * b + pad * b
            s = SM.build(imgs, "interleaved", rs, base=base, frame_stride=ih * rs + 3 * b, seed=pad)
            # (a tight source is the call without one, DIRECT whatever is forced)
            for path, route in ((L.RESIZE_AUTO, L.SOURCE_DIRECT), (L.RESIZE_FUSED, L.SOURCE_DIRECT),
                                (L.RESIZE_CONVERT, L.SOURCE_PACKED if pad else L.SOURCE_DIRECT)):
                _eq(_bytes(ctx, d, s, frames, (oh, ow, c), dtype, path=path), ref, f"C={c} {kw} pad {pad} base {base} path {path}")
                assert ctx.last_source_route() == route and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, (c, kw, pad, path)
    # a tensor out of a pitched source, with a window: the instances of the view as they are
    d = L.resize_desc(iw, ih, ow, oh, 3)
    imgs = rng.integers(0, 256, (frames, ih, iw, 3), dtype=np.uint8)
    win = (3, 2, 60, 29)
    ref = ctx.resize(imgs, ow, oh, window=win)
    s = SM.build(imgs, "interleaved", iw * 3 + 5, base=1, seed=3)
    for dt in ("float32", "bfloat16"):
        _tensor(ctx, d, s, frames, ref, _lut(2, dt), (2, 0), FLIPS[:3], "chw", dt, window=win)
        assert ctx.last_source_route() == L.SOURCE_DIRECT and ctx.last_tensor_route() == L.TENSOR_FUSED


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_alpha_rows_off_a_dword(ctx, K):
    """k_rs_fused<4, K, true, kRsRowShift>, <..., 4 + 8 + 64> and <..., 2 + 8 + 64>: LANCZOS_RESIZE_ALPHA over interleaved rows
    whose pitch is no multiple of 4, where every row has another residue and the existing ALPHA staging (one shift per frame)
    does not apply.  The planar test's shapes; pitches 1, 2 and 3 past a dword with every base residue; bytes, and tensors of
    both dtypes, both layouts, a reordering and a dropping map, flips 0..3; AUTO and forced FUSED are DIRECT, CONVERT is
    PACKED.  A pitch that is a dword multiple runs the existing instances, DIRECT as well.  Crops of such rows are PACKED."""
    import torch
    ih, oh, frames, c = 37, 75, 4, 4
    filt, a, iw, ow = _instance_shape(K, c)
    d = L.resize_desc(iw, ih, ow, oh, c, a, alpha=True, filter=filt)
    p = L.resize_plan_host(d, frames)
    assert p.fused and p.K == K and p.strips > 1 and p.chunks > 1
    imgs = np.stack([P.noise(ih, iw, c, seed=43 * K + 7 * k) for k in range(frames)])
    ref = ctx.resize(imgs, ow, oh, a, alpha=True, filter=filt)             # the yardstick: the entry without a source
    combos = [(dt, lay, m) for dt in ("float32", "bfloat16") for lay in ("chw", "hwc") for m in ((2, 1, 0), (0, 1, 2))]
    layouts = [SM.build(imgs, "interleaved", iw * c + pad, base=base, frame_stride=ih * (iw * c + pad) + gap, seed=pad)
               for pad, base, gap in ((1, 0, 3), (2, 3, 0), (3, 1, 2), (7, 2, 1), (8, 1, 4))]
    for i, s in enumerate(layouts):
        assert np.array_equal(SM.unpack(s, imgs.shape), imgs)
        assert len({(s.at + y * s.row_stride) % 4 for y in range(ih)}) == (4, 2, 4, 4, 1)[i]   # the residues its rows start at
        for path, route in ROUTES[1:] + ((L.RESIZE_AUTO, L.SOURCE_DIRECT),):
            _eq(_bytes(ctx, d, s, frames, (oh, ow, c), path=path), ref, f"K={K} layout {i} path {path}")
            assert ctx.last_source_route() == route and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, (K, i, path)
            for dt, lay, m in combos[(2 * i) % 8:(2 * i) % 8 + 2]:
                _tensor(ctx, d, s, frames, ref, _lut(3, dt), m, FLIPS, lay, dt, path=path)
                assert ctx.last_source_route() == route, (K, i, path, dt)
                assert ctx.last_tensor_route() == (L.TENSOR_CONVERTED if path == L.RESIZE_CONVERT else L.TENSOR_FUSED)
    # a crop origin per frame: there are no such crops instances, the rows are packed first; with a dword pitch they ride
    w, h = ow - 37, oh - 14
    dw = L.resize_desc(iw, ih, ow, oh, c, a, alpha=True, filter=filt)
    fused = bool(L.resize_crops_plan_host(dw, (w, h), frames).inner.fused)
    origins = np.array([(0, 0), (ow - w, oh - h), (ow - w, 1), (3, oh - h)], dtype=np.int32)
    do = torch.from_numpy(origins).cuda()
    cref = np.stack([ref[f, y0:y0 + h, x0:x0 + w] for f, (x0, y0) in enumerate(origins)])
    for s, route in ((layouts[0], L.SOURCE_PACKED), (layouts[4], L.SOURCE_DIRECT if fused else L.SOURCE_PACKED)):
        for dt in ("float32", "bfloat16"):
            _tensor(ctx, dw, s, frames, cref, _lut(3, dt), (2, 1, 0), FLIPS, "chw", dt, crop=(w, h), d_origin=do.data_ptr())
            assert ctx.last_source_route() == route, (K, dt, route)
            assert ctx.last_tensor_route() == (L.TENSOR_FUSED if fused else L.TENSOR_CONVERTED)


def _two_sources(imgs):
    _, ih, iw, c = imgs.shape
    return {"planar": SM.build(imgs, "planar", iw + 3, ih * (iw + 3) + 1, base=1, frame_stride=c * (ih * (iw + 3) + 1) + 2, seed=5),
            "pitched": SM.build(imgs, "interleaved", iw * c + 7, base=3, frame_stride=ih * (iw * c + 7) + 1, seed=6)}


def test_packed_routes(ctx):
    """everything the fused kernel does not run gets the source packed first: the result is the packed call's"""
    frames = 3
    imgs = np.stack([P.gradient_noise(120, 160, 3, seed=12 + k) for k in range(frames)])
    big = np.stack([P.noise(300, 400, 3, seed=2 + k) for k in range(frames)])
    #        name, frames, out_w, out_h, path, keywords, PACKED by definition
    cases = [("two pass", imgs, 64, 48, L.RESIZE_TWO_PASS, {}, True), ("h only", imgs, 77, 120, L.RESIZE_AUTO, {}, True),
             ("v only", imgs, 160, 50, L.RESIZE_AUTO, {}, True), ("nearest", imgs, 71, 53, L.RESIZE_AUTO, {"filter": "nearest"}, True),
             ("copy", imgs, 160, 120, L.RESIZE_AUTO, {}, True), ("crop", imgs, 160, 120, L.RESIZE_AUTO, {"window": (7, 5, 101, 77)}, True),
             ("gap 2", big, 40, 30, L.RESIZE_AUTO, {"reducing_gap": 2.0}, True),
             ("box", imgs, 64, 48, L.RESIZE_AUTO, {"box": (10.25, 7.5, 131.75, 99.125)}, False),
             ("box", imgs, 64, 48, L.RESIZE_CONVERT, {"box": (10.25, 7.5, 131.75, 99.125)}, True)]
    for name, x, ow, oh, path, kw, packed in cases:
        _, ih, iw, c = x.shape
        ctx.resize_force(path)
        try:
            ref = ctx.resize(x, ow, oh, **kw)
        finally:
            ctx.resize_force(L.RESIZE_AUTO)
        dkw = {k: v for k, v in kw.items() if k != "filter"}
        d = L.resize_desc(iw, ih, ow, oh, c, filter=kw.get("filter", "lanczos"))
        for lname, s in _two_sources(x).items():
            got = _bytes(ctx, d, s, frames, ref.shape[1:], path=path, **dkw)
            _eq(got, ref, f"{name} {lname}")
            if packed:
                assert ctx.last_source_route() == L.SOURCE_PACKED, (name, lname)
            if name == "nearest":
                assert ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
            if name == "gap 2":
                assert L.resize_plan_host(d, frames, reducing_gap=2.0).fx > 1


def test_packed_crops(ctx):
    """a crop origin per frame, origins at the plan's maxima: a planar source is packed, a pitched one rides the crops instances;
    frames kept at size gather from the packed copy"""
    import torch
    frames = 5
    for name, (iw, ih, ow, oh, w, h) in {"fused": (160, 120, 64, 48, 41, 29), "at size": (341, 47, 341, 47, 224, 30)}.items():
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=30 + k) for k in range(frames)])
        d = L.resize_desc(iw, ih, ow, oh, 3)
        p = L.resize_crops_plan_host(d, (w, h), frames).inner
        mx, my = ow - w, oh - h
        if p.fused:
            sd = [L.resize_window_plan_host(d, (x, 0, w, h), frames).inner.stage_dw for x in range(mx + 1)]
            rr = [L.resize_window_plan_host(d, (0, y, w, h), frames).inner.ring_rows for y in range(my + 1)]
            bx, by = int(np.argmax(sd)), int(np.argmax(rr))
            assert sd[bx] == p.stage_dw and rr[by] == p.ring_rows
        else:
            bx, by = mx // 2 | 1, my // 2 | 1
        origins = np.array([(0, 0), (mx, my), (bx, 1), (2, by), (bx, by)], dtype=np.int32)
        full = ctx.resize(imgs, ow, oh)
        do = torch.from_numpy(origins).cuda()
        flips = [0, 1, 2, 3, 1]
        for lname, s in _two_sources(imgs).items():
            for dt in ("float32", "bfloat16"):
                src = (2, 1, 0)
                lut = _lut(3, dt)
                want = RC.crops(full, lut, w, h, origins, src, flips, "chw")
                # the crops model gives the words; the device helper wants the bytes they are made of: frame f's window
                ref = np.stack([full[f, y0:y0 + h, x0:x0 + w] for f, (x0, y0) in enumerate(origins)])
                assert np.array_equal(V.view(ref, lut, src, flips, "chw"), want)
                _tensor(ctx, d, s, frames, ref, lut, src, flips, "chw", dt, crop=(w, h), d_origin=do.data_ptr())
                direct = lname == "pitched" and p.fused
                assert ctx.last_source_route() == (L.SOURCE_DIRECT if direct else L.SOURCE_PACKED), (name, lname)
                assert ctx.last_tensor_route() == (L.TENSOR_FUSED if p.fused else L.TENSOR_CONVERTED)


@pytest.mark.parametrize("fixture,alpha", [("resize_pillow.npz", False), ("resize_pillow_alpha.npz", True)])
def test_pillow_directly(ctx, fixture, alpha):
    """Pillow's images as planes with padded rows: the bytes are Pillow's outputs"""
    z = np.load(os.path.join(GOLDEN, fixture))
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 12
    seen = set()
    for i, name in enumerate(names):
        img, out = z[f"{name}_in"], z[f"{name}_out"]
        img3, out3 = (img[..., None], out[..., None]) if img.ndim == 2 else (img, out)
        (ih, iw, c), (oh, ow) = img3.shape, out3.shape[:2]
        d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
        rs = iw + 1 + i % 3
        s = SM.build(img3[None], "planar", rs, ih * rs + i % 2, base=i % 4, seed=i)
        got = _bytes(ctx, d, s, 1, (oh, ow, c))
        _eq(got[0], out3, f"{fixture} {name}")
        seen.add(ctx.last_source_route())
        if c == 3:   # the host entry on tight planes
            _eq(ctx.resize(np.ascontiguousarray(img3.transpose(2, 0, 1)), ow, oh, alpha=alpha, planar=True), out3, f"host {name}")
    assert seen == {L.SOURCE_DIRECT, L.SOURCE_PACKED} or not alpha, seen


def test_unnamed_bytes_do_not_matter(ctx):
    """two buffers that differ only in the bytes the layout does not name give identical results, on every route"""
    frames = 2
    imgs = np.stack([P.noise(41, 90, 4, seed=k) for k in range(frames)])
    for ow, oh, alpha in ((70, 35, False), (70, 35, True), (70, 41, False), (180, 82, False)):
        d = L.resize_desc(90, 41, ow, oh, 4, alpha=alpha)
        ref = ctx.resize(imgs, ow, oh, alpha=alpha)
        for layout, rs, cs in (("planar", 93, 41 * 93 + 2), ("interleaved", 90 * 4 + 9, None)):
            a = SM.build(imgs, layout, rs, cs, base=1, frame_stride=None if cs is None else 4 * cs + 6, seed=1)
            b = SM.build(imgs, layout, rs, cs, base=1, frame_stride=None if cs is None else 4 * cs + 6, seed=1, fill_seed=77)
            m = SM.named_mask(a, imgs.shape)
            assert np.array_equal(a.buf[m], b.buf[m]) and not np.array_equal(a.buf[~m], b.buf[~m])
            for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                ga, gb = (_bytes(ctx, d, s, frames, (oh, ow, 4), path=path) for s in (a, b))
                _eq(ga, ref, f"{layout} {ow}x{oh} alpha={alpha} path {path}")
                _eq(gb, ga, f"{layout} {ow}x{oh}: the padding reached the result")


def test_host_entries(ctx):
    """planar=True on Context.resize and Context.resize_tensor: (C, H, W) and (N, C, H, W)"""
    imgs = np.stack([P.noise(41, 90, 3, seed=k) for k in range(3)])
    chw = np.ascontiguousarray(imgs.transpose(0, 3, 1, 2))
    for ow, oh, kw in ((70, 35, {}), (70, 41, {}), (70, 35, {"window": (3, 2, 60, 29)}), (30, 14, {"reducing_gap": 1.5})):
        _eq(ctx.resize(chw, ow, oh, planar=True, **kw), ctx.resize(imgs, ow, oh, **kw), f"host {ow}x{oh} {kw}")
        _eq(ctx.resize(chw[0], ow, oh, planar=True, **kw), ctx.resize(imgs[0], ow, oh, **kw), "one frame")
    for dt in ("float32", "float16"):
        for kw in ({}, {"channels_out": (2, 0), "flip": [1, 2, 3]}, {"crop": (33, 21), "origins": [(0, 0), (37, 14), (5, 3)]}):
            mean, std = ((0.4, 0.5), (0.2, 0.3)) if "channels_out" in kw else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
            want = ctx.resize_tensor(imgs, 70, 35, mean=mean, std=std, dtype=dt, **kw)
            got = ctx.resize_tensor(chw, 70, 35, mean=mean, std=std, dtype=dt, planar=True, **kw)
            _eq(V.words(got), V.words(want), f"tensor host {dt} {kw}")
    with pytest.raises(L.LanczosError):
        ctx.resize(imgs.astype(np.uint16).transpose(0, 3, 1, 2), 70, 35, planar=True)


def test_device_argument_checks(ctx):
    import torch
    iw, ih, ow, oh = 90, 41, 70, 35
    d = L.resize_desc(iw, ih, ow, oh, 3)
    imgs = np.stack([P.noise(ih, iw, 3, seed=k) for k in range(2)])
    x = torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 3, 1, 2))).cuda()
    y = torch.zeros(2 * ow * oh * 3 + 16, dtype=torch.uint8, device="cuda")
    t = torch.zeros(2 * ow * oh * 3 + 16, dtype=torch.float32, device="cuda")
    dl = torch.from_numpy(T32.identity_lut(3)).cuda()
    st = V.strides("chw", ow, oh, 3)
    before = ctx.last_source_route()

    def src(rs=iw, cs=iw * ih, ps=1, reserved=0):
        s = L.ResizeSource()
        s.row_stride, s.chan_stride, s.pix_stride = rs, cs, ps
        s.reserved[1] = reserved
        return s
    bad = [dict(source=src(rs=iw - 1)), dict(source=src(cs=iw * ih - 1)), dict(source=src(ps=3)), dict(source=src(reserved=1)),
           dict(source=src(), in_frame_stride=3 * iw * ih - 1), dict(source=src(cs=iw * ih + 5), in_frame_stride=3 * iw * ih + 14),
           dict(source=L.resize_source(d, "interleaved", row_stride=3 * iw + 2), in_frame_stride=ih * (3 * iw + 2) - 1)]
    for kw in bad:
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), t.data_ptr(), 2, dl.data_ptr(), st, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
    assert ctx.last_source_route() == before
    # a window together with crops
    org = torch.zeros(4, dtype=torch.int32, device="cuda")
    v = L.tensor_view(dl.data_ptr(), V.strides("chw", 33, 21, 3), 4, (0, 1, 2))
    cr, win = L.resize_crops(33, 21, org.data_ptr()), L.resize_window(d, (0, 0, 33, 21))
    import ctypes
    rc = L._lib().lanczos_resize_tensor_source_device(ctx._h, ctypes.byref(d), None, ctypes.byref(win), ctypes.byref(cr),
                                                      ctypes.byref(src()), ctypes.byref(v), x.data_ptr(), t.data_ptr(), 2, 0, 0, None)
    assert rc == L.ERR_BAD_ARG
    rc = L._lib().lanczos_resize_tensor_source_device(ctx._h, ctypes.byref(d), None, ctypes.byref(win), ctypes.byref(cr), None,
                                                      ctypes.byref(v), x.data_ptr(), t.data_ptr(), 2, 0, 0, None)
    assert rc == L.ERR_BAD_ARG
    # a refused call leaves the route of the last good one, also where the source is the tight one
    ctx.resize_force(L.RESIZE_CONVERT)
    try:
        ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, source=src())
        assert ctx.last_source_route() == L.SOURCE_PACKED
        with pytest.raises(L.LanczosError):
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, source=L.resize_source(d, "interleaved"), in_frame_stride=3 * iw * ih - 1)
        assert ctx.last_source_route() == L.SOURCE_PACKED
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    # a tight interleaved source is the call without one: the plan's kernel, DIRECT, the same bytes
    xt = torch.from_numpy(imgs).cuda()
    ya, yb = torch.zeros_like(y), torch.zeros_like(y)
    ctx.resize_device(d, xt.data_ptr(), ya.data_ptr(), 2, source=L.resize_source(d, "interleaved"))
    ka, ra = ctx.last_kernel(), ctx.last_source_route()
    ctx.resize_device(d, xt.data_ptr(), yb.data_ptr(), 2)
    torch.cuda.synchronize()
    assert ka == ctx.last_kernel() == L.KERNEL_RESIZE_FUSED and L.resize_plan_host(d, 2).fused and ra == L.SOURCE_DIRECT
    assert torch.equal(ya, yb) and ya.any()
    # a NULL source is the existing entry: the same bytes, and the last source route stays what it was
    ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, source=src())
    torch.cuda.synchronize()
    assert ctx.last_source_route() == AUTO_PLANAR
    xi = torch.from_numpy(imgs).cuda()
    y2 = torch.zeros_like(y)
    for route_before in (AUTO_PLANAR,):
        rc = L._lib().lanczos_resize_source_device(ctx._h, ctypes.byref(d), None, None, None, xi.data_ptr(), y2.data_ptr(), 2, 0, 0,
                                                   None)
        torch.cuda.synchronize()
        assert rc == L.OK and ctx.last_source_route() == route_before
    y3 = torch.zeros_like(y)
    ctx.resize_device(d, xi.data_ptr(), y3.data_ptr(), 2)
    torch.cuda.synchronize()
    assert torch.equal(y2, y3) and torch.equal(y2, y) and y.any()
    t2, t3 = torch.zeros_like(t), torch.zeros_like(t)
    vv = L.tensor_view(dl.data_ptr(), st, 4, (0, 1, 2))
    rc = L._lib().lanczos_resize_tensor_source_device(ctx._h, ctypes.byref(d), None, None, None, None, ctypes.byref(vv), xi.data_ptr(),
                                                      t2.data_ptr(), 2, 0, 0, None)
    ctx.resize_tensor_device(d, xi.data_ptr(), t3.data_ptr(), 2, dl.data_ptr(), vv)
    torch.cuda.synchronize()
    assert rc == L.OK and torch.equal(t2.view(torch.int32), t3.view(torch.int32)) and t2.view(torch.int32).any()
    assert ctx.last_source_route() == AUTO_PLANAR


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_CONVERT])
def test_capture_replay_follows_the_source(path):
    """A captured planar tensor call, once on the DIRECT and once on the PACKED route, replays right and follows the source's
    contents of the moment; an eager call of another shape on the same context afterwards is right as well"""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow, frames = 91 + path, 137, 47, 61, 3      # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3)
        assert L.resize_plan_host(d, frames).fused
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=9 + k) for k in range(frames)])
        imgs2 = np.stack([P.noise(ih, iw, 3, seed=19 + k) for k in range(frames)])
        ref, ref2 = c.resize(imgs, ow, oh), c.resize(imgs2, ow, oh)
        c.close()
        c = L.Context(0)                                        # a context that has not seen the shape
        c.resize_force(path)
        s, s2 = (SM.build(v, "planar", iw + 3, ih * (iw + 3) + 1, base=1, seed=4) for v in (imgs, imgs2))
        src = L.resize_source(d, "planar", s.row_stride, s.chan_stride)
        lut = T32.identity_lut(3)
        st = V.strides("chw", ow, oh, 3)
        x = torch.from_numpy(s.buf).cuda()
        dl = torch.from_numpy(lut).cuda()
        y = torch.zeros((frames, 3, oh, ow), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="relaxed"):
            c.resize_tensor_device(d, x.data_ptr() + s.at, y.data_ptr(), frames, dl.data_ptr(), st,
                                   stream=torch.cuda.current_stream().cuda_stream, source=src)
        assert c.last_source_route() == (L.SOURCE_DIRECT if path == L.RESIZE_FUSED else L.SOURCE_PACKED)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()                    # captured, not run
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(y.cpu().numpy()), V.view(ref, lut), "first replay")
        x.copy_(torch.from_numpy(s2.buf))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(y.cpu().numpy()), V.view(ref2, lut), "replay after the source changed")
        # eager, another shape (larger scratch on the PACKED route), the same context: the graph's blocks stay alive
        big = np.stack([P.noise(ih + 40, iw + 60, 3, seed=k) for k in range(frames)])
        assert L.resize_plan_host(L.resize_desc(iw + 60, ih + 40, ow, oh, 3), frames).fused
        c.resize_force(L.RESIZE_AUTO)
        want = c.resize(big, ow, oh)
        c.resize_force(path)
        _eq(c.resize(np.ascontiguousarray(big.transpose(0, 3, 1, 2)), ow, oh, planar=True), want, "eager after the capture")
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(y.cpu().numpy()), V.view(ref2, lut), "replay after the eager call")
        del g
    finally:
        c.close()
