"""GPU checks of the tensor view (lanczos_tensor_view, lanczos_resize_tensor_view_*): 8-bit frames resized straight into float32
or 16-bit tensors through a channel map and per-frame flips.  Everything is compared as 32-bit or 16-bit patterns, never within
a tolerance: against the numpy model (tests/resize_tensor_view_model.py) over Context.resize's bytes and, for Pillow's fixtures,
against torch's own indexing, flip and normalise arithmetic on the CPU.  Every mapped fused instance runs with tables that name
output channel and byte; the route is asserted against the plan query; the device tests check that no word the strides do not
name is touched."""
import ctypes
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
PATHS = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS)
DTYPES = ("float32", "bfloat16")
FLIPS = [0, 1, 2, 3]
MAPS = {1: ((0,),), 3: ((2, 1, 0), (2, 0)), 4: ((2, 1, 0), (3, 0, 1, 2))}


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


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
    """AUTO, forced FUSED (refused exactly where the plan says the byte request is not fused) and forced TWO_PASS: the same
    words, and the route the plan implies."""
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


# K -> (filter, a, in_w, out_w): the shapes of tests/test_resize_tensor16_gpu.py, the width odd
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 6
    a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    return "lanczos", a, iw, 261


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_every_mapped_fused_instance(ctx, K):
    """k_rs_fused<C, K, false, 4 + 8> and <..., 2 + 8> for C = 1, 3, 4: more than one strip with a ragged last one, 75 output
    rows (a last block of 3), more than one chunk, an odd out_w; four frames flipped 0, 1, 2, 3; maps that reorder and drop; CHW
    and HWC.  The result's words are the output channel and the byte of Context.resize."""
    ih, oh = 37, 75
    for c in (1, 3, 4):
        filt, a, iw, ow = _instance_shape(K, c)
        sw = 64 if c == 4 else 256
        d = L.resize_desc(iw, ih, ow, oh, c, a, filter=filt)
        p = L.resize_plan_host(d, 4)
        assert p.fused and p.K == K and p.strips > 1 and ow % sw and ow % 2 and oh % 8 == 3 and p.chunks > 1, (c, K, p.K, ow)
        imgs = np.stack([P.noise(ih, iw, c, seed=31 * K + c + 7 * k) for k in range(4)])
        ref = ctx.resize(imgs, ow, oh, a, filter=filt)
        for src in MAPS[c]:
            for dtype in DTYPES:
                lut = _lut(len(src), dtype)
                for layout in ("chw", "hwc"):
                    _routes(ctx, imgs, ow, oh, lut, V.view(ref, lut, src, FLIPS, layout), True,
                            f"K={K} C={c} {src} {dtype} {layout}", dtype=dtype, a=a, filter=filt, layout=layout,
                            channels_out=src, flip=FLIPS)


def test_alpha_instances(ctx):
    """LANCZOS_RESIZE_ALPHA with alpha dropped: k_rs_fused<4, K, true, 4 + 8> and <..., 2 + 8> at one shape per K; the colours
    are un-premultiplied as in the byte request"""
    rng = np.random.default_rng(3)
    ih, oh = 37, 75
    for K in (3, 5, 7, 9, 11, 13, 17, 25):
        filt, a, iw, ow = _instance_shape(K, 4)
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True, filter=filt), 4)
        assert p.fused and p.K == K
        imgs = rng.integers(0, 256, (4, ih, iw, 4), dtype=np.uint8)
        ref = ctx.resize(imgs, ow, oh, a, alpha=True, filter=filt)
        for dtype in DTYPES:
            lut = _lut(3, dtype)
            _routes(ctx, imgs, ow, oh, lut, V.view(ref, lut, (0, 1, 2), FLIPS), True, f"alpha K={K} {dtype}", dtype=dtype, a=a,
                    filter=filt, alpha=True, channels_out=(0, 1, 2), flip=FLIPS)


def test_an_identity_view_is_the_call_without_one(ctx):
    """the words and the route of the float32 and the 16-bit call, with and without a window, fused and converted"""
    img = np.stack([P.noise(41, 90, 3, seed=4), P.gradient_noise(41, 90, 3, seed=5)])
    for ow, oh, fused in ((70, 35, True), (70, 41, False)):
        for window in (None, L.center_window(ow, oh, 33, 21)):
            for dtype in ("float32", "bfloat16", "float16"):
                lut = L.normalize_lut(3, MEAN[:3], STD[:3], dtype=dtype)
                for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                    ctx.resize_force(path)
                    try:
                        want = ctx.resize_tensor(img, ow, oh, lut=lut, dtype=dtype, window=window)
                        route = ctx.last_tensor_route()
                        got = ctx.resize_tensor(img, ow, oh, lut=lut, dtype=dtype, window=window, channels_out=(0, 1, 2))
                        assert ctx.last_tensor_route() == route == (L.TENSOR_FUSED if fused and path == L.RESIZE_AUTO
                                                                     else L.TENSOR_CONVERTED)
                        _eq(got, want, f"identity {ow}x{oh} {window} {dtype} path {path}")
                        _eq(ctx.resize_tensor(img, ow, oh, lut=lut, dtype=dtype, window=window, flip=[0, 0]), want, "no flips")
                    finally:
                        ctx.resize_force(L.RESIZE_AUTO)


def test_converted_routes(ctx):
    """one pass (each axis idle in turn), NEAREST, the plain copy, the crop copy, a reducing gap and forced CONVERT: each with a
    window from center_window, a reversed map and flips"""
    imgs = np.stack([P.gradient_noise(120, 160, 3, seed=12 + k) for k in range(4)])
    #        name, out_w, out_h, window (w, h), keywords, fused
    cases = [("h only", 77, 120, (51, 97), {}, False), ("v only", 160, 50, (131, 33), {}, False),
             ("nearest", 71, 53, (40, 31), {"filter": "nearest"}, False),
             ("copy", 160, 120, (160, 120), {}, False), ("crop copy", 160, 120, (101, 77), {}, False),
             ("gap 2", 20, 15, (13, 9), {"reducing_gap": 2.0}, True),
             ("fused", 64, 48, (41, 29), {}, True)]
    for name, ow, oh, (ww, wh), kw, fused in cases:
        win = L.center_window(ow, oh, ww, wh)
        d = L.resize_desc(160, 120, ow, oh, 3, filter=kw.get("filter", "lanczos"))
        opts = {k: v for k, v in kw.items() if k != "filter"}
        assert bool(L.resize_window_plan_host(d, win, 4, **opts).inner.fused) == fused, name
        ref = ctx.resize(imgs, ow, oh, window=win, **kw)
        assert ref.shape == (4, wh, ww, 3)
        for dtype in DTYPES:
            for src in ((2, 1, 0), (2, 0)):
                lut = _lut(len(src), dtype)
                for layout in ("chw", "hwc"):
                    paths = (L.RESIZE_AUTO,) if name == "nearest" else (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_CONVERT)
                    _routes(ctx, imgs, ow, oh, lut, V.view(ref, lut, src, FLIPS, layout), fused,
                            f"{name} {dtype} {src} {layout}", paths=paths, dtype=dtype, layout=layout, window=win,
                            channels_out=src, flip=FLIPS, **kw)
        if name == "nearest":
            assert ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
    # a string flips every frame, and a single frame keeps Context.resize's shapes
    lut = _lut(3, "float32")
    got = ctx.resize_tensor(imgs[0], 64, 48, lut=lut, channels_out=(2, 1, 0), flip="hv")
    assert got.shape == (3, 48, 64)
    _eq(got, V.view(ctx.resize(imgs[0], 64, 48), lut, (2, 1, 0), 3), "one frame")
    # two output channels: mean / std in output order, the rows of two one-channel tables
    got = ctx.resize_tensor(imgs[0], 64, 48, mean=(0.4, 0.5), std=(0.2, 0.3), channels_out=(2, 0), dtype="float16")
    lut2 = np.concatenate([L.normalize_lut(1, m, s, dtype="float16") for m, s in ((0.4, 0.2), (0.5, 0.3))])
    _eq(got, V.view(ctx.resize(imgs[0], 64, 48), lut2, (2, 0)), "two channels, normalised")
    for bad in ({"flip": "x"}, {"flip": [0, 1]}, {"flip": [0, 4, 0, 0]}, {"channels_out": ()}, {"channels_out": (0, 1, 2, 0)}):
        with pytest.raises(L.LanczosError):
            ctx.resize_tensor(imgs, 64, 48, **bad)
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_tensor(imgs, 64, 48, channels_out=(1, 1))
    assert e.value.code == L.ERR_BAD_ARG


def _torch_want(pillow_out, src, dtype):
    """torch on the CPU over Pillow's bytes: the channels indexed, flipped horizontally, normalised with mean / std in output
    order, cast -- as words [OC][H][W]"""
    import torch
    oc = len(src)
    mean = torch.tensor(MEAN[:oc], dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD[:oc], dtype=torch.float32)[:, None, None]
    x = torch.from_numpy(np.ascontiguousarray(pillow_out)).permute(2, 0, 1)[list(src)].flip(-1)
    x = x.float().div(255).sub(mean).div(std).contiguous()
    if dtype == "float32":
        return x.view(torch.int32).numpy().view(np.uint32)
    return x.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("fixture,alpha", [("resize_pillow.npz", False), ("resize_pillow_alpha.npz", True)])
def test_pillow_then_torch(ctx, fixture, alpha):
    """BGR order (alpha fixture: [:, :3]), mirrored, normalised: torch's arithmetic on Pillow's bytes, bit for bit"""
    z = np.load(os.path.join(GOLDEN, fixture))
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 12
    fused = 0
    for name in names:
        img, out = z[f"{name}_in"], z[f"{name}_out"]
        img3, out3 = (img[..., None], out[..., None]) if img.ndim == 2 else (img, out)
        (ih, iw, c), (oh, ow) = img3.shape, out3.shape[:2]
        src = (0, 1, 2) if alpha else (2, 1, 0) if c >= 3 else (0,)
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, alpha=alpha), 1)
        fused += p.fused
        for dtype in ("float32", "bfloat16", "float16"):
            want = _torch_want(out3, src, dtype)
            for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
                ctx.resize_force(path)
                try:
                    got = ctx.resize_tensor(img3, ow, oh, mean=MEAN[:len(src)], std=STD[:len(src)], alpha=alpha, dtype=dtype,
                                            channels_out=src, flip="h")
                finally:
                    ctx.resize_force(L.RESIZE_AUTO)
                _eq(got, want, f"{fixture} {name} {dtype} path {path}")
                assert ctx.last_tensor_route() == (L.TENSOR_FUSED if p.fused and path == L.RESIZE_AUTO
                                                   else L.TENSOR_CONVERTED), name
    assert fused >= 6, fused


def _device_case(ctx, elem, d, imgs, ref, src, window, st, frame_stride, path, what):
    """One device call into a guarded buffer of sentinels: every element the contract names has its value, every other word of
    the buffer -- guards in front and behind, row, plane and frame padding, the planes of a larger tensor -- still holds the
    sentinel.  16-bit frames start 2 bytes past a dword.  The flips come from device memory with junk in bits 2..7."""
    import torch
    word = np.uint32 if elem == 4 else np.uint16
    SENTINEL, GUARD = (0xA5A5A5A5, 64) if elem == 4 else (0xA5A5, 65)
    lut = _lut(len(src), "float32" if elem == 4 else "bfloat16")       # no entry is the sentinel
    frames, wh, ww = ref.shape[:3]
    flips = np.array([(0xFC, 0x05, 0x82, 0x7F, 0x40)[k % 5] for k in range(frames)], dtype=np.uint8)
    n = V.extent(ww, wh, len(src), st)
    fs = frame_stride or n
    total = GUARD + (frames - 1) * fs + n + GUARD
    want = np.full(total, SENTINEL, dtype=word)
    assert V.scatter(want, GUARD, ref, lut, src, flips, st, fs) == frames * len(src) * wh * ww
    signed = np.int32 if elem == 4 else np.int16
    y = torch.from_numpy(np.full(total, SENTINEL, dtype=word).view(signed)).cuda()
    if elem == 2:
        assert y.data_ptr() % 4 == 0 and (y.data_ptr() + 2 * GUARD) % 4 == 2
    x = torch.from_numpy(imgs).cuda()
    dl = torch.from_numpy(V.words(lut).view(signed)).cuda()
    df = torch.from_numpy(flips).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr() + elem * GUARD, frames, dl.data_ptr(), st,
                                 out_frame_stride=elem * frame_stride, stream=torch.cuda.current_stream().cuda_stream,
                                 dtype="float32" if elem == 4 else "bfloat16", window=window, channels_out=src,
                                 d_flip=df.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    _eq(y.cpu().numpy().view(word), want, what)
    return ctx.last_tensor_route()


@pytest.mark.parametrize("elem", [4, 2])
def test_nothing_else_is_written(ctx, elem):
    """A fused shape and one that is not, a window and none, out_channels below channels, tight and padded rows and planes, a
    slice of a larger tensor (the planes of four channels under three stored ones), a gap between the frames: the named
    elements and no other word, on both routes."""
    iw, ih = 90, 41
    for c, src in ((3, (2, 1, 0)), (4, (2, 0, 1)), (3, (1,))):
        oc = len(src)
        for ow, oh, window, fused in ((71, 35, None, True), (71, 35, (3, 2, 60, 29), True), (71, ih, None, False)):
            assert bool(L.resize_window_plan_host(L.resize_desc(iw, ih, ow, oh, c), window, 3).inner.fused) == fused
            w, h = (window[2], window[3]) if window else (ow, oh)
            d = L.resize_desc(iw, ih, ow, oh, c)
            imgs = np.stack([P.noise(ih, iw, c, seed=70 + 5 * k + c) for k in range(3)])
            ref = ctx.resize(imgs, ow, oh, window=window)     # the bytes every layout below is made of
            row = w + 3
            layouts = {"chw": V.strides("chw", w, h, oc), "hwc": V.strides("hwc", w, h, oc),
                       "padded chw": (h * row + 5, row, 1), "padded hwc": (1, w * oc + 7, oc),
                       "planes of a larger tensor": (2 * h * w, w, 1), "pixels of a larger tensor": (1, w * (oc + 2), oc + 2)}
            for name, st in layouts.items():
                gap = V.extent(w, h, oc, st) + 11          # odd for the tight layouts: 16-bit frames alternate in alignment
                for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                    got = _device_case(ctx, elem, d, imgs, ref, src, window, st, gap, path,
                                       f"elem {elem} C={c} {src} {ow}x{oh} {window} {name} path {path}")
                    assert got == (L.TENSOR_FUSED if fused and path == L.RESIZE_AUTO else L.TENSOR_CONVERTED), (name, path)


def test_device_argument_checks(ctx):
    import torch
    d = L.resize_desc(90, 41, 70, 35, 4)
    x = torch.zeros(90 * 41 * 4, dtype=torch.uint8, device="cuda")
    y = torch.zeros(70 * 35 * 3 + 8, dtype=torch.float32, device="cuda")
    dl = torch.from_numpy(T32.identity_lut(3)).cuda()
    st = V.strides("chw", 70, 35, 3)
    ext = 4 * 70 * 35 * 3
    for elem, kw, ptr in ((4, {}, y.data_ptr() + 2), (2, {}, y.data_ptr() + 1), (4, {"out_frame_stride": ext + 2}, y.data_ptr()),
                          (4, {"out_frame_stride": ext - 4}, y.data_ptr()), (2, {"out_frame_stride": ext // 2 + 1}, y.data_ptr())):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), ptr, 1, None, L.tensor_view(dl.data_ptr(), st, elem, (0, 1, 2)), **kw)
        assert e.value.code == L.ERR_BAD_ARG, (elem, kw)
        assert ctx.last_tensor_route() == 0
    # the extent counts out_channels: three planes fit where four would not
    ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), st, out_frame_stride=ext, channels_out=(0, 1, 2))
    torch.cuda.synchronize()
    assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


def _hip():
    """the HIP runtime this process already runs on"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def _captured_chain(ctx, stream, call):
    """Captures `call` on `stream` with the runtime's own API and returns (nodes, edges) of the graph, which is never run"""
    hip = _hip()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipStreamBeginCapture.argtypes = [vp, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, ctypes.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphDestroy.argtypes = [vp]
    graph = vp()
    assert hip.hipStreamBeginCapture(stream, 2) == 0                    # hipStreamCaptureModeRelaxed
    try:
        call()
    finally:
        assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    try:
        n, m = sz(), sz()
        assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
        assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(m)) == 0
        src, dst = (vp * max(m.value, 1))(), (vp * max(m.value, 1))()
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(m)) == 0
        return n.value, [(src[i], dst[i]) for i in range(m.value)]
    finally:
        assert hip.hipGraphDestroy(graph) == 0


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_capture_replay_and_flip_update(path):
    """A captured view call replays right; the kernels read the table and the flips when they run, so a replay after both were
    overwritten follows the new contents.  The captured graph is a single chain: no node has two successors or predecessors."""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow, frames = 93 + path, 139, 47, 61, 4      # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3)
        assert L.resize_plan_host(d, frames).fused
        imgs = np.stack([P.gradient_noise(ih, iw, 3, seed=9 + k) for k in range(frames)])
        src = (2, 1, 0)
        lut, lut2 = T32.identity_lut(3), L.normalize_lut(3, MEAN[:3], STD[:3])
        flips, flips2 = np.array([0, 1, 2, 3], dtype=np.uint8), np.array([3, 3, 0, 1], dtype=np.uint8)
        ref = c.resize(imgs, ow, oh)
        c.close()
        c = L.Context(0)                                        # a context that has not seen the shape
        c.resize_force(path)
        st = V.strides("chw", ow, oh, 3)
        x = torch.from_numpy(imgs).cuda()
        dl, df = torch.from_numpy(lut).cuda(), torch.from_numpy(flips).cuda()
        y = torch.zeros((frames, 3, oh, ow), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()

        def call():
            c.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), frames, dl.data_ptr(), st,
                                   stream=torch.cuda.current_stream().cuda_stream, channels_out=src, d_flip=df.data_ptr())
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            call()
        assert c.last_tensor_route() == (L.TENSOR_FUSED if path == L.RESIZE_FUSED else L.TENSOR_CONVERTED)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()                    # captured, not run
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), V.view(ref, lut, src, flips), "first replay")
        dl.copy_(torch.from_numpy(lut2))
        df.copy_(torch.from_numpy(flips2))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), V.view(ref, lut2, src, flips2), "replay after the table and the flips changed")
        del g
        # the topology, from a capture of the same call through the runtime's own API
        y.zero_()
        with torch.cuda.stream(s):
            nodes, edges = _captured_chain(c, s.cuda_stream, call)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()
        assert nodes >= (1 if path == L.RESIZE_FUSED else 3) and len(edges) == nodes - 1, (nodes, edges)
        assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges), edges
    finally:
        c.close()
