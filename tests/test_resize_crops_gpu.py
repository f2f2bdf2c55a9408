"""GPU checks of a tensor view with a crop origin per frame (lanczos_resize_crops, lanczos_resize_tensor_crops_*): 8-bit frames
resized straight into float32 or 16-bit tensors, every frame storing the w x h window of its resize at an origin of its own that
the kernels read from device memory.  Everything is compared as 32-bit or 16-bit patterns, never within a tolerance: against the
numpy model (tests/resize_crops_model.py) over slices of Context.resize's FULL bytes and, for Pillow's fixture, against torch's own
indexing, flip and normalise arithmetic on the CPU.  Every crops fused instance runs at origins that reach its plan's maxima; the
route is asserted against the plan query; the device tests check that no word the strides do not name is touched and that an
origin outside the output is clamped."""
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_crops_model as RC
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
PATHS = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS)
DTYPES = ("float32", "bfloat16")
FLIPS = [0, 1, 2, 3, 1]
MAPS = {1: ((0,),), 3: ((2, 1, 0), (2, 0)), 4: ((2, 1, 0), (3, 0, 1, 2))}
NOT_FITTING = (1018, 367, 300, 43, 3, 259, 11)   # tests/test_resize_crops_host.py: the window at (0, 0) is fused, the crops are not


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize_crops_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_crops_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _lut(oc, dtype):
    """a table that names output channel and byte"""
    return T32.identity_lut(oc) if dtype == "float32" else T16.identity_lut16(oc)


def _eq(got, want, what):
    got, want = V.words(np.asarray(got)), V.words(np.asarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}: "
                             f"{int(got[tuple(bad[0])]):#x} != {int(want[tuple(bad[0])]):#x}")


def _routes(ctx, img, ow, oh, lut, want, fused, what, paths=PATHS, dtype="float32", **kw):
    """AUTO, forced FUSED (refused exactly where the crops plan is not fused) and forced TWO_PASS / CONVERT: the same words, and
    the route the plan implies."""
    try:
        for path in paths:
            ctx.resize_force(path)
            if path == L.RESIZE_FUSED and not fused:
                with pytest.raises(L.LanczosError) as e:
                    ctx.resize_tensor(img, ow, oh, lut=lut, dtype=dtype, **kw)
                assert e.value.code == L.ERR_UNSUPPORTED, what
                continue
            got = ctx.resize_tensor(img, ow, oh, lut=lut, dtype=dtype, **kw)
            _eq(got, want, f"{what} path {path}")
            expect = L.TENSOR_FUSED if fused and path not in (L.RESIZE_TWO_PASS, L.RESIZE_CONVERT) else L.TENSOR_CONVERTED
            assert ctx.last_tensor_route() == expect, (what, path, ctx.last_tensor_route())
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


# K -> (filter, a, in_w, out_w, crop w): _instance_shape of tests/test_resize_tensor_view_gpu.py with its output as the crop and the
# output widened by 37 pixels at the same scale, so that origins have room
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        filt, a, iw, cw = ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 6
    else:
        filt, cw = "lanczos", 261
        a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    ow = cw + 37
    return filt, a, (iw * ow) // cw, ow, cw


def _origins(d, w, h, frames):
    """(0, 0), the far corner, an origin that reaches the plan's stage_dw, one that reaches its ring_rows, an odd interior one;
    and the crops plan"""
    p = L.resize_crops_plan_host(d, (w, h), frames).inner
    mx, my = d.out_w - w, d.out_h - h
    sd = [L.resize_window_plan_host(d, (x, 0, w, h), frames).inner.stage_dw for x in range(mx + 1)]
    rr = [L.resize_window_plan_host(d, (0, y, w, h), frames).inner.ring_rows for y in range(my + 1)]
    assert max(sd) == p.stage_dw and max(rr) == p.ring_rows
    xs = [x for x in range(mx + 1) if sd[x] == p.stage_dw]
    ys = [y for y in range(my + 1) if rr[y] == p.ring_rows]
    # the largest ones away from the edges where there is one, with any origin on the other axis
    o = [(0, 0), (mx, my), (xs[len(xs) // 2], 1), (2, ys[len(ys) // 2]), ((mx // 2) | 1, (my // 2) | 1)]
    return np.array(o, dtype=np.int32), p, min(sd) < p.stage_dw or min(rr) < p.ring_rows


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_every_crops_fused_instance(ctx, K):
    """k_rs_fused<C, K, false, 4 + 8 + 16> and <..., 2 + 8 + 16> for C = 1, 3, 4: 37 input rows, a crop of more than one strip
    with a ragged last one and 43 rows (a last block of 3, two chunks), five frames at origins that reach the plan's maxima,
    flipped 0, 1, 2, 3, 1; maps that reorder and drop; CHW and HWC.  The words name the output channel and the byte Context.resize
    stores at the frame's origin plus (x, y)."""
    ih, oh, h = 37, 61, 43
    for c in (1, 3, 4):
        filt, a, iw, ow, w = _instance_shape(K, c)
        sw = 64 if c == 4 else 256
        d = L.resize_desc(iw, ih, ow, oh, c, a, filter=filt)
        origins, p, tells = _origins(d, w, h, 5)
        assert p.fused and p.K == K and p.strips > 1 and w % sw and w % 2 and h % 8 == 3 and p.chunks > 1, (c, K, p.K, w)
        assert tells, "every origin has the same plan: the shape shows nothing"
        imgs = np.stack([P.noise(ih, iw, c, seed=37 * K + c + 7 * k) for k in range(5)])
        full = ctx.resize(imgs, ow, oh, a, filter=filt)
        for src in MAPS[c]:
            for dtype in DTYPES:
                lut = _lut(len(src), dtype)
                for layout in ("chw", "hwc"):
                    _routes(ctx, imgs, ow, oh, lut, RC.crops(full, lut, w, h, origins, src, FLIPS, layout), True,
                            f"K={K} C={c} {src} {dtype} {layout}", dtype=dtype, a=a, filter=filt, layout=layout,
                            channels_out=src, flip=FLIPS, crop=(w, h), origins=origins)


def test_alpha_instances(ctx):
    """LANCZOS_RESIZE_ALPHA with alpha dropped: k_rs_fused<4, K, true, 4 + 8 + 16> and <..., 2 + 8 + 16> at one shape per K"""
    rng = np.random.default_rng(5)
    ih, oh, h = 37, 61, 43
    for K in (3, 5, 7, 9, 11, 13, 17, 25):
        filt, a, iw, ow, w = _instance_shape(K, 4)
        d = L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True, filter=filt)
        origins, p, _ = _origins(d, w, h, 5)
        assert p.fused and p.K == K and p.chunks > 1
        imgs = rng.integers(0, 256, (5, ih, iw, 4), dtype=np.uint8)
        full = ctx.resize(imgs, ow, oh, a, alpha=True, filter=filt)
        for dtype in DTYPES:
            lut = _lut(3, dtype)
            _routes(ctx, imgs, ow, oh, lut, RC.crops(full, lut, w, h, origins, (0, 1, 2), FLIPS), True, f"alpha K={K} {dtype}",
                    dtype=dtype, a=a, filter=filt, alpha=True, channels_out=(0, 1, 2), flip=FLIPS, crop=(w, h), origins=origins)


def _torch_want(stored, src, mean, std, dtype, flip=0):
    """torch on the CPU over Pillow's bytes [h][w][C]: the channels indexed, flipped, normalised with mean / std in output order,
    cast -- as words [OC][h][w]"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(stored)).permute(2, 0, 1)[list(src)]
    dims = [dim for dim, bit in ((-1, 1), (-2, 2)) if flip & bit]
    x = x.flip(dims) if dims else x
    x = x.float().div(255).sub(torch.tensor(mean, dtype=torch.float32)[:, None, None])
    x = x.div(torch.tensor(std, dtype=torch.float32)[:, None, None]).contiguous()
    if dtype == "float32":
        return x.view(torch.int32).numpy().view(np.uint32)
    return x.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


def test_pillow_then_torch(ctx):
    """Pillow's resize(...).crop(frame's window).transpose(frame's flip) then torch's div / sub / div, bit for bit; the call
    without flips is torch's .flip of the same.  RGB in BGR order, RGBA without its alpha."""
    cases = _golden().load()
    routes = set()
    for name, (case, imgs, origins, flips, stored) in cases.items():
        _, mode, filt, iw, ih, ow, oh, box, gap, (w, h) = case
        x = imgs[..., None] if imgs.ndim == 3 else imgs
        st = stored[..., None] if stored.ndim == 3 else stored
        c = x.shape[-1]
        src = (0, 1, 2) if c == 4 else (2, 1, 0) if c == 3 else (0,)
        mean, std = MEAN[:len(src)], STD[:len(src)]
        kw = dict(mean=mean, std=std, alpha=mode == "RGBA", filter=filt, box=box, reducing_gap=gap, channels_out=src, crop=(w, h),
                  origins=origins)
        for dtype in ("float32", "bfloat16", "float16"):
            for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
                ctx.resize_force(path)
                try:
                    got = ctx.resize_tensor(x, ow, oh, dtype=dtype, flip=flips, **kw)
                    routes.add(ctx.last_tensor_route())
                    plain = ctx.resize_tensor(x, ow, oh, dtype=dtype, **kw)
                finally:
                    ctx.resize_force(L.RESIZE_AUTO)
                for k in range(len(x)):
                    _eq(got[k], _torch_want(st[k], src, mean, std, dtype), f"{name} frame {k} {dtype} path {path}")
                    _eq(plain[k], _torch_want(st[k], src, mean, std, dtype, int(flips[k])), f"{name} frame {k} {dtype} unflipped")
    assert routes == {L.TENSOR_FUSED, L.TENSOR_CONVERTED}


def test_converted_routes(ctx):
    """one pass (each axis idle in turn), NEAREST, both idle over a 341-pixel RGB source (rows of 1023 bytes: every window row
    starts at another byte of its dword), a reducing gap, a plan that does not fit, and forced CONVERT"""
    rng = np.random.default_rng(21)
    #        name, in_w, in_h, out_w, out_h, crop, keywords, fused
    cases = [("h only", 160, 120, 77, 120, (51, 97), {}, False), ("v only", 160, 120, 160, 50, (131, 33), {}, False),
             ("nearest", 160, 120, 71, 53, (40, 31), {"filter": "nearest"}, False),
             ("both idle", 341, 47, 341, 47, (224, 30), {}, False),
             ("gap 2", 160, 120, 20, 15, (13, 9), {"reducing_gap": 2.0}, True),
             ("not fitting", *NOT_FITTING[:4], NOT_FITTING[5:], {}, False),
             ("fused", 160, 120, 64, 48, (41, 29), {}, True)]
    for name, iw, ih, ow, oh, (w, h), kw, fused in cases:
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=12 + k) for k in range(5)])
        d = L.resize_desc(iw, ih, ow, oh, 3, filter=kw.get("filter", "lanczos"))
        opts = {k: v for k, v in kw.items() if k != "filter"}
        assert bool(L.resize_crops_plan_host(d, (w, h), 5, **opts).inner.fused) == fused, name
        mx, my = ow - w, oh - h
        origins = np.array([(0, 0), (mx, my), (1, my), (mx, 1), (int(rng.integers(0, mx + 1)) | 1, int(rng.integers(0, my + 1)))],
                           dtype=np.int32)
        origins = RC.clamp(origins, ow, oh, w, h).astype(np.int32)
        full = ctx.resize(imgs, ow, oh, **kw)
        for dtype in DTYPES:
            for src in ((2, 1, 0), (2, 0)):
                lut = _lut(len(src), dtype)
                for layout in ("chw", "hwc"):
                    paths = (L.RESIZE_AUTO,) if name == "nearest" else (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_CONVERT)
                    _routes(ctx, imgs, ow, oh, lut, RC.crops(full, lut, w, h, origins, src, FLIPS, layout), fused,
                            f"{name} {dtype} {src} {layout}", paths=paths, dtype=dtype, layout=layout, channels_out=src, flip=FLIPS,
                            crop=(w, h), origins=origins, **kw)
        if name == "nearest":
            assert ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
    # one channel and four at size, the identity view, no flips, a single frame
    for c in (1, 4):
        img = P.noise(33, 59, c, seed=c)
        lut = _lut(c, "float32")
        got = ctx.resize_tensor(img, 59, 33, lut=lut, crop=(31, 20), origins=[(13, 7)])
        assert got.shape == (c, 20, 31) and ctx.last_tensor_route() == L.TENSOR_CONVERTED
        x = img if img.ndim == 3 else img[..., None]
        _eq(got, V.view(x[7:27, 13:44], lut), f"one frame C={c}")


def test_host_entry_refusals(ctx):
    """the host entry validates its host array instead of clamping; crop= and window= exclude each other"""
    imgs = np.stack([P.noise(41, 90, 3, seed=k) for k in range(2)])
    ok = dict(crop=(33, 21), origins=[(0, 0), (37, 14)])
    assert ctx.resize_tensor(imgs, 70, 35, **ok).shape == (2, 3, 21, 33)
    for org in ([(0, 0), (38, 14)], [(0, 0), (37, 15)], [(-1, 0), (0, 0)], [(0, -1), (0, 0)], [(0, 0), (1 << 30, 0)]):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor(imgs, 70, 35, crop=(33, 21), origins=org)
        assert e.value.code == L.ERR_BAD_ARG, org
    for bad in (dict(crop=(33, 21)), dict(origins=[(0, 0), (1, 1)]), dict(crop=(33, 21), origins=[(0, 0)]),
                dict(crop=(33, 21), origins=[(0, 0), (1, 1)], window=(0, 0, 33, 21)), dict(crop=(71, 21), origins=[(0, 0), (0, 0)]),
                dict(crop=(33, 21), origins=[(0.5, 0), (1, 1)])):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor(imgs, 70, 35, **bad)
        assert e.value.code == L.ERR_BAD_ARG, bad


def _device_case(ctx, elem, d, imgs, full, w, h, origins, src, st, frame_stride, path, what, in_off=0, in_gap=0):
    """One device call into a guarded buffer of sentinels: every element the contract names has its value, every other word of
    the buffer -- guards in front and behind, row, plane and frame padding -- still holds the sentinel.  16-bit frames start 2 bytes
    past a dword, the source frames in_off bytes past one and in_gap bytes apart.  Flips (junk in bits 2..7) and origins come from
    device memory; the origins are given as they are and expected as the contract clamps them."""
    import torch
    word = np.uint32 if elem == 4 else np.uint16
    SENTINEL, GUARD = (0xA5A5A5A5, 64) if elem == 4 else (0xA5A5, 65)
    lut = _lut(len(src), "float32" if elem == 4 else "bfloat16")       # no entry is the sentinel
    frames = len(imgs)
    flips = np.array([(0xFC, 0x05, 0x82, 0x7F, 0x40)[k % 5] for k in range(frames)], dtype=np.uint8)
    n = V.extent(w, h, len(src), st)
    fs = frame_stride or n
    total = GUARD + (frames - 1) * fs + n + GUARD
    want = np.full(total, SENTINEL, dtype=word)
    assert RC.scatter(want, GUARD, full, lut, w, h, origins, src, flips, st, fs) == frames * len(src) * h * w
    signed = np.int32 if elem == 4 else np.int16
    y = torch.from_numpy(np.full(total, SENTINEL, dtype=word).view(signed)).cuda()
    in_frame = imgs[0].size
    in_fs = in_frame + in_gap
    xb = np.full(in_off + frames * in_fs + 8, 0x5A, dtype=np.uint8)
    for k in range(frames):
        xb[in_off + k * in_fs:in_off + k * in_fs + in_frame] = imgs[k].reshape(-1)
    x = torch.from_numpy(xb).cuda()
    assert x.data_ptr() % 4 == 0
    dl = torch.from_numpy(V.words(lut).view(signed)).cuda()
    df = torch.from_numpy(flips).cuda()
    do = torch.from_numpy(np.ascontiguousarray(origins, dtype=np.int32)).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_tensor_device(d, x.data_ptr() + in_off, y.data_ptr() + elem * GUARD, frames, dl.data_ptr(), st,
                                 in_frame_stride=in_fs if in_gap else 0, out_frame_stride=elem * frame_stride,
                                 stream=torch.cuda.current_stream().cuda_stream, dtype="float32" if elem == 4 else "bfloat16",
                                 channels_out=src, d_flip=df.data_ptr(), crop=(w, h), d_origin=do.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    _eq(y.cpu().numpy().view(word), want, what)
    return ctx.last_tensor_route()


@pytest.mark.parametrize("elem", [4, 2])
def test_nothing_else_is_written_and_origins_are_clamped(ctx, elem):
    """A fused shape, a one-pass shape and frames at size; out_channels below channels; tight and padded rows and planes, a slice
    of a larger tensor, a gap between the frames; source frames off a dword and apart; origins slightly and wildly outside the
    output: the named elements of the clamped origins and no other word, on both routes."""
    iw, ih = 90, 41
    for c, src in ((3, (2, 1, 0)), (4, (2, 0, 1)), (3, (1,))):
        oc = len(src)
        for ow, oh, w, h, fused in ((71, 35, 60, 29, True), (71, ih, 33, 30, False), (iw, ih, 61, 30, False)):
            d = L.resize_desc(iw, ih, ow, oh, c)
            assert bool(L.resize_crops_plan_host(d, (w, h), 5).inner.fused) == fused
            imgs = np.stack([P.noise(ih, iw, c, seed=70 + 5 * k + c) for k in range(5)])
            full = ctx.resize(imgs, ow, oh)     # the bytes every layout below is made of
            mx, my = ow - w, oh - h
            origins = np.array([(-3, 2), (mx + 5, my), (3, my + 1), (-(1 << 31), (1 << 31) - 1), (mx // 2 | 1, -1)], dtype=np.int64)
            assert (RC.clamp(origins, ow, oh, w, h) != origins).any(axis=1).all()
            row = w + 3
            layouts = {"chw": V.strides("chw", w, h, oc), "hwc": V.strides("hwc", w, h, oc),
                       "padded chw": (h * row + 5, row, 1), "padded hwc": (1, w * oc + 7, oc),
                       "planes of a larger tensor": (2 * h * w, w, 1), "pixels of a larger tensor": (1, w * (oc + 2), oc + 2)}
            for i, (name, st) in enumerate(layouts.items()):
                gap = V.extent(w, h, oc, st) + 11          # odd for the tight layouts: 16-bit frames alternate in alignment
                for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                    got = _device_case(ctx, elem, d, imgs, full, w, h, origins, src, st, gap, path,
                                       f"elem {elem} C={c} {src} {ow}x{oh} {name} path {path}", in_off=i % 4, in_gap=(0, 5, 7)[i % 3])
                    assert got == (L.TENSOR_FUSED if fused and path == L.RESIZE_AUTO else L.TENSOR_CONVERTED), (name, path)


def test_device_argument_checks(ctx):
    import torch
    d = L.resize_desc(90, 41, 70, 35, 3)
    x = torch.zeros(90 * 41 * 3, dtype=torch.uint8, device="cuda")
    y = torch.zeros(33 * 21 * 3 + 8, dtype=torch.float32, device="cuda")
    do = torch.zeros(4, dtype=torch.int32, device="cuda")
    dl = torch.from_numpy(T32.identity_lut(3)).cuda()
    st = V.strides("chw", 33, 21, 3)
    ext = 4 * 33 * 21 * 3
    bad = [dict(crop=(33, 21)), dict(d_origin=do.data_ptr()), dict(crop=(33, 21), d_origin=do.data_ptr(), window=(0, 0, 33, 21)),
           dict(crop=(71, 21), d_origin=do.data_ptr()), dict(crop=(33, 21), d_origin=do.data_ptr() + 2),
           dict(crop=(33, 21), d_origin=do.data_ptr(), out_frame_stride=ext - 4)]
    for kw in bad:
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 2, dl.data_ptr(), st, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
    # the extent is the crop's: a frame stride of exactly one crop frame is enough
    ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), st, out_frame_stride=ext, crop=(33, 21),
                             d_origin=do.data_ptr())
    torch.cuda.synchronize()
    assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


def test_equal_origins_are_the_window(ctx):
    """every frame at (x0, y0): the words and the route of the view call with the window (x0, y0, w, h)"""
    imgs = np.stack([P.noise(41, 90, 3, seed=4 + k) for k in range(3)])
    flips = [1, 2, 0]
    for ow, oh, fused in ((70, 35, True), (70, 41, False), (90, 41, False)):
        for x0, y0, w, h in ((0, 0, 33, 21), (37, oh - 21, 33, 21), (5, 3, 60, 30)):
            for dtype in ("float32", "bfloat16", "float16"):
                lut = L.normalize_lut(3, MEAN[:3], STD[:3], dtype=dtype)
                for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                    ctx.resize_force(path)
                    try:
                        want = ctx.resize_tensor(imgs, ow, oh, lut=lut, dtype=dtype, window=(x0, y0, w, h), channels_out=(2, 1, 0),
                                                 flip=flips)
                        route = ctx.last_tensor_route()
                        got = ctx.resize_tensor(imgs, ow, oh, lut=lut, dtype=dtype, crop=(w, h), origins=[(x0, y0)] * 3,
                                                channels_out=(2, 1, 0), flip=flips)
                        assert ctx.last_tensor_route() == route == (L.TENSOR_FUSED if fused and path == L.RESIZE_AUTO
                                                                     else L.TENSOR_CONVERTED)
                        _eq(got, want, f"{ow}x{oh} ({x0}, {y0}, {w}, {h}) {dtype} path {path}")
                    finally:
                        ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_capture_replay_follows_origins_and_flips(path):
    """A captured crops call replays right; the kernels read origins and flips when they run, so a replay after both were
    overwritten follows the new contents."""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow, frames, w, h = 95 + path, 141, 47, 61, 4, 40, 27      # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3)
        assert L.resize_crops_plan_host(d, (w, h), frames).inner.fused
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=9 + k) for k in range(frames)])
        src = (2, 1, 0)
        lut = T32.identity_lut(3)
        flips, flips2 = np.array([0, 1, 2, 3], dtype=np.uint8), np.array([3, 3, 0, 1], dtype=np.uint8)
        org = np.array([(0, 0), (21, 20), (7, 3), (13, 11)], dtype=np.int32)
        org2 = np.array([(20, 1), (0, 19), (25, 20), (3, 3)], dtype=np.int32)     # (25, 20) is clamped to (21, 20)
        full = c.resize(imgs, ow, oh)
        c.close()
        c = L.Context(0)                                        # a context that has not seen the shape
        c.resize_force(path)
        st = V.strides("chw", w, h, 3)
        x = torch.from_numpy(imgs).cuda()
        dl, df, do = torch.from_numpy(lut).cuda(), torch.from_numpy(flips).cuda(), torch.from_numpy(org).cuda()
        y = torch.zeros((frames, 3, h, w), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), frames, dl.data_ptr(), st,
                                   stream=torch.cuda.current_stream().cuda_stream, channels_out=src, d_flip=df.data_ptr(),
                                   crop=(w, h), d_origin=do.data_ptr())
        assert c.last_tensor_route() == (L.TENSOR_FUSED if path == L.RESIZE_FUSED else L.TENSOR_CONVERTED)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()                    # captured, not run
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), RC.crops(full, lut, w, h, org, src, flips), "first replay")
        do.copy_(torch.from_numpy(org2))
        df.copy_(torch.from_numpy(flips2))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), RC.crops(full, lut, w, h, org2, src, flips2), "replay after the origins and the flips changed")
        del g
    finally:
        c.close()
