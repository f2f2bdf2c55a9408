"""GPU checks of the tensor entry (lanczos_resize_tensor_*): 8-bit frames resized straight into float tensors through a table.
Everything is compared as 32-bit patterns, never within a tolerance: against the table applied to Context.resize's bytes
(tests/resize_tensor_model.py) and, for Pillow's fixtures, against torch's own ToTensor() + Normalize() arithmetic.  Every
fused instance runs with a table of NaN payloads that names channel and byte; the route (fused / converted) is asserted
against the plan query."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_tensor_model as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# ImageNet's constants; a fourth channel (RGBX, RGBA) and a single one (L) get constants of their own
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
PATHS = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    got = got.view(np.uint32) if got.dtype == np.float32 else got
    want = want.view(np.uint32) if want.dtype == np.float32 else want
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}: "
                             f"{int(got[tuple(bad[0])]):#010x} != {int(want[tuple(bad[0])]):#010x}")


def _routes(ctx, img, ow, oh, lut, want, fused, what, **kw):
    """AUTO, forced FUSED (refused exactly where the plan says the byte request is not fused) and forced TWO_PASS: the same
    words, and the route the plan implies."""
    try:
        for path in PATHS:
            ctx.resize_force(path)
            if path == L.RESIZE_FUSED and not fused:
                with pytest.raises(L.LanczosError) as e:
                    ctx.resize_tensor(img, ow, oh, lut=lut, **kw)
                assert e.value.code == L.ERR_UNSUPPORTED, what
                continue
            _eq(ctx.resize_tensor(img, ow, oh, lut=lut, **kw), want, f"{what} path {path}")
            expect = L.TENSOR_FUSED if fused and path != L.RESIZE_TWO_PASS else L.TENSOR_CONVERTED
            assert ctx.last_tensor_route() == expect, (what, path, ctx.last_tensor_route())
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


# K -> (filter, a, in_w as a function of the strip width, out_w likewise): the smallest shapes of the instance tests of
# test_resize_filters_gpu.py (K = 3, 5) and test_resize_gpu.py (the Lanczos buckets, out_w = 261)
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 5
    a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    return "lanczos", a, iw, 261


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_every_fused_instance_with_the_identity_table(ctx, K):
    """k_rs_fused<C, K, false, true> for C = 1, 3, 4: more than one strip with a ragged last one, 75 output rows (a last block
    of 3), more than one chunk; CHW and HWC.  The result's payloads are the channel and the byte of Context.resize."""
    for c in (1, 3, 4):
        filt, a, iw, ow = _instance_shape(K, c)
        ih, oh = 37, 75
        d = L.resize_desc(iw, ih, ow, oh, c, a, filter=filt)
        p = L.resize_plan_host(d, 1)
        sw = 64 if c == 4 else 256
        assert p.fused and p.K == K and p.strips > 1 and ow % sw and oh % 8 == 3 and p.chunks > 1, (c, K, p.K, p.strips)
        img = P.noise(ih, iw, c, seed=31 * K + c)
        lut = T.identity_lut(c)
        ref = ctx.resize(img, ow, oh, a, filter=filt)
        assert ctx.last_tensor_route() == 0                    # a byte call is no tensor call
        for layout in ("chw", "hwc"):
            _routes(ctx, img, ow, oh, lut, T.tensor(ref, lut, layout), True, f"K={K} C={c} {layout}", a=a, filter=filt,
                    layout=layout)


def test_tall_single_frame_in_chunks(ctx):
    iw, ih, ow, oh = 40, 150, 70, 301
    p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 3), 1)
    assert p.fused and p.chunks > 4 and oh % p.rows_per_chunk
    img = P.gradient_noise(ih, iw, 3, seed=2)
    lut = T.identity_lut(3)
    _routes(ctx, img, ow, oh, lut, T.tensor(ctx.resize(img, ow, oh), lut), True, "tall")


def test_alpha_instances(ctx):
    """LANCZOS_RESIZE_ALPHA has the epilogue too: k_rs_fused<4, K, true, true> at one shape per K"""
    rng = np.random.default_rng(3)
    for K in (3, 5, 7, 9, 11, 13, 17, 25):
        filt, a, iw, ow = _instance_shape(K, 4)
        ih, oh = 37, 75
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True, filter=filt), 1)
        assert p.fused and p.K == K
        img = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
        lut = T.identity_lut(4)
        ref = ctx.resize(img, ow, oh, a, alpha=True, filter=filt)
        _routes(ctx, img, ow, oh, lut, T.tensor(ref, lut), True, f"alpha K={K}", a=a, filter=filt, alpha=True)


def _torch_want(pillow_out):
    """torchvision's pipeline on the CPU (IEEE division) over Pillow's bytes, as words [C][H][W]"""
    import torch
    c = pillow_out.shape[2]
    mean = torch.tensor(MEAN[:c], dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD[:c], dtype=torch.float32)[:, None, None]
    x = torch.from_numpy(np.ascontiguousarray(pillow_out)).permute(2, 0, 1).float().div(255).sub(mean).div(std)
    return T.bits(x.contiguous().numpy())


@pytest.mark.parametrize("fixture,alpha", [("resize_pillow.npz", False), ("resize_pillow_alpha.npz", True)])
def test_pillow_then_torch(ctx, fixture, alpha):
    z = np.load(os.path.join(GOLDEN, fixture))
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 12
    fused = 0
    for name in names:
        img, out = z[f"{name}_in"], z[f"{name}_out"]
        (ih, iw, c), (oh, ow) = img.shape, out.shape[:2]
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, alpha=alpha), 1)
        if name.startswith(("h_only", "v_only", "identity")):
            assert not p.fused, name                           # one pass or none: the converted route
        fused += p.fused
        lut = L.normalize_lut(c, MEAN[:c], STD[:c])
        _routes(ctx, img, ow, oh, lut, _torch_want(out), bool(p.fused), f"{fixture} {name}", alpha=alpha)
        ctx.resize_force(L.RESIZE_AUTO)                        # mean / std instead of a ready table
        _eq(ctx.resize_tensor(img, ow, oh, mean=MEAN[:c], std=STD[:c], alpha=alpha), _torch_want(out), name)
    assert fused >= 6, fused


def _device_case(ctx, c, ow, oh, st, frames, frame_stride, lead, in_gap, path, what, iw=90, ih=41):
    """One device call into a guarded, sentinel-filled buffer: every word the contract names has its value, every other word
    of the buffer -- guards in front and behind, row, plane and frame padding -- keeps the sentinel."""
    import torch
    SENTINEL, GUARD = 0x5EA1AB1E, 64
    imgs = np.stack([P.noise(ih, iw, c, seed=70 + 5 * k + c) for k in range(frames)])
    lut = T.identity_lut(c)
    d = L.resize_desc(iw, ih, ow, oh, c)
    ctx.resize_force(L.RESIZE_AUTO)
    ref = ctx.resize(imgs, ow, oh)
    in_fb = ih * iw * c
    in_fs = in_fb + in_gap
    x = torch.full((lead + frames * in_fs + 8,), 255, dtype=torch.uint8, device="cuda")
    for k in range(frames):
        x[lead + k * in_fs:lead + k * in_fs + in_fb] = torch.from_numpy(imgs[k].reshape(-1)).cuda()
    n = T.extent(ow, oh, c, st)
    fs = frame_stride or n
    total = GUARD + (frames - 1) * fs + n + GUARD
    want = np.full(total, SENTINEL, dtype=np.uint32)
    named = T.scatter(want, GUARD, ref, lut, st, fs)
    assert named == frames * c * oh * ow
    y = torch.from_numpy(np.full(total, SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    dl = torch.from_numpy(lut).cuda()
    ctx.resize_force(path)
    try:
        s = torch.cuda.current_stream().cuda_stream
        ctx.resize_tensor_device(d, x.data_ptr() + lead, y.data_ptr() + 4 * GUARD, frames, dl.data_ptr(), st,
                                 in_frame_stride=in_fs if in_gap else 0, out_frame_stride=4 * frame_stride, stream=s)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    _eq(y.cpu().numpy().view(np.uint32), want, what)
    return ctx.last_tensor_route()


@pytest.mark.parametrize("c", [1, 3, 4])
def test_layouts_strides_and_guards(ctx, c):
    ow, oh = 70, 35                                       # rows of 70, 210, 280 samples; two strips for four channels
    assert L.resize_plan_host(L.resize_desc(90, 41, ow, oh, c), 3).fused
    row = ow + 3
    plane = oh * row + 5
    padded = (plane, row, 1)
    layouts = {"chw": (T.strides("chw", ow, oh, c), 0), "hwc": (T.strides("hwc", ow, oh, c), 0),
               "padded": (padded, T.extent(ow, oh, c, padded) + 11),
               "padded hwc": ((1, ow * c + 7, c), T.extent(ow, oh, c, (1, ow * c + 7, c)) + 2)}
    for name, (st, fs) in layouts.items():
        for lead, in_gap in ((0, 0), (1, 13)):           # an odd input base (delta != 0 while staging) and a frame stride
            for path, route in ((L.RESIZE_AUTO, L.TENSOR_FUSED), (L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED)):
                got = _device_case(ctx, c, ow, oh, st, 3, fs, lead, in_gap, path, f"C={c} {name} lead {lead} path {path}")
                assert got == route, (name, path, got)


def test_device_argument_checks(ctx):
    import torch
    d = L.resize_desc(90, 41, 70, 35, 3)
    x = torch.zeros(90 * 41 * 3, dtype=torch.uint8, device="cuda")
    y = torch.zeros(70 * 35 * 3 + 8, dtype=torch.float32, device="cuda")
    dl = torch.from_numpy(T.identity_lut(3)).cuda()
    st = T.strides("chw", 70, 35, 3)
    for kw, ptr in (({}, y.data_ptr() + 2), ({"out_frame_stride": 4 * 70 * 35 * 3 + 2}, y.data_ptr()),
                    ({"out_frame_stride": 4 * 70 * 35 * 3 - 4}, y.data_ptr())):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), ptr, 1, dl.data_ptr(), st, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
        assert ctx.last_tensor_route() == 0
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), (1, 1, 1))
    assert e.value.code == L.ERR_BAD_ARG


def test_float_frame_of_2_gib_is_converted(ctx):
    """Planes 2^28 floats apart: the float frame spans 2 GiB, past the fused store's 32-bit buffer offsets.  AUTO converts (64-bit
    addresses in k_rs_to_tensor), although the byte request plans fused; forced FUSED is refused."""
    import torch
    iw, ih, ow, oh, c = 90, 41, 70, 35, 3
    cs = 1 << 28
    d = L.resize_desc(iw, ih, ow, oh, c)
    assert L.resize_plan_host(d, 1).fused and T.extent(ow, oh, c, (cs, ow, 1)) * 4 >= 1 << 31
    img = P.noise(ih, iw, c, seed=8)
    lut = T.identity_lut(c)
    want = T.tensor(ctx.resize(img, ow, oh), lut)
    x = torch.from_numpy(img).cuda()
    dl = torch.from_numpy(lut).cuda()
    y = torch.empty(2 * cs + oh * ow, dtype=torch.int32, device="cuda")
    for k in range(c):
        y[k * cs:k * cs + oh * ow] = 0
    try:
        ctx.resize_force(L.RESIZE_FUSED)
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), (cs, ow, 1))
        assert e.value.code == L.ERR_UNSUPPORTED
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), (cs, ow, 1))
        torch.cuda.synchronize()
        assert ctx.last_tensor_route() == L.TENSOR_CONVERTED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
        got = np.stack([y[k * cs:k * cs + oh * ow].cpu().numpy().view(np.uint32).reshape(oh, ow) for k in range(c)])
        _eq(got, want, "planes 1 GiB apart")
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        del y
        torch.cuda.empty_cache()


def test_other_routes(ctx):
    """nearest, a box, reducing_gap (one whose reduced frame already has the target size, so the inner resize is the plain
    copy), one-axis resizes and the copy itself: the table over Context.resize's bytes."""
    img = P.gradient_noise(120, 160, 3, seed=12)
    lut = L.normalize_lut(3, MEAN[:3], STD[:3])
    cases = [("nearest", 71, 53, {"filter": "nearest"}, False),
             ("box", 64, 48, {"box": (10.5, 7.25, 130.0, 99.5)}, True),
             ("box bicubic", 200, 150, {"box": (10.5, 7.25, 130.0, 99.5), "filter": "bicubic"}, True),
             ("gap 2", 20, 15, {"reducing_gap": 2.0}, True),
             ("gap whose reduction is the result", 40, 30, {"reducing_gap": 1.0, "filter": "box"}, False),
             ("h only", 77, 120, {}, False), ("v only", 160, 50, {}, False), ("copy", 160, 120, {}, False)]
    for name, ow, oh, kw, fused in cases:
        d = L.resize_desc(160, 120, ow, oh, 3, filter=kw.get("filter", "lanczos"))
        opts = {k: v for k, v in kw.items() if k != "filter"}
        p = L.resize_plan_host(d, 1, **opts)
        inner = p.inner if opts else p
        assert bool(inner.fused) == fused, name
        if name.startswith("gap"):
            assert p.fx > 1 and p.fy > 1
        if name == "gap whose reduction is the result":
            assert (p.reduced_w, p.reduced_h) == (ow, oh) and not p.pass_h and not p.pass_v
        ref = ctx.resize(img, ow, oh, **kw)
        for layout in ("chw", "hwc"):
            if kw.get("filter") == "nearest":             # one path: forced FUSED is refused for it, as for the bytes
                ctx.resize_force(L.RESIZE_AUTO)
                _eq(ctx.resize_tensor(img, ow, oh, lut=lut, layout=layout, **kw), T.tensor(ref, lut, layout), name)
                assert ctx.last_tensor_route() == L.TENSOR_CONVERTED and ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
            else:
                _routes(ctx, img, ow, oh, lut, T.tensor(ref, lut, layout), fused, f"{name} {layout}", layout=layout, **kw)
    # batches and 2-D input keep Context.resize's shapes
    batch = np.stack([img, img[::-1]])
    got = ctx.resize_tensor(batch, 64, 48, lut=lut)
    assert got.shape == (2, 3, 48, 64)
    _eq(got, T.tensor(ctx.resize(batch, 64, 48), lut), "batch")
    grey = img[..., 0].copy()
    got = ctx.resize_tensor(grey, 64, 48, mean=0.5, std=0.5, layout="hwc")
    assert got.shape == (48, 64, 1)
    _eq(got[..., 0], T.tensor(ctx.resize(grey, 64, 48), L.normalize_lut(1, 0.5, 0.5))[0], "2-D input")


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_capture_replay_and_table_update(path):
    """A captured tensor call replays right; the kernels read the table when they run, so a replay after the table and the
    input were overwritten gives the new table over the new bytes.  An eager call between capture and first replay (first use
    of the shape inside the capture) does not disturb it."""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow = 91 + path, 137, 47, 61           # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3)
        assert L.resize_plan_host(d, 1).fused             # the fused kernel runs this width
        img, img2 = P.gradient_noise(ih, iw, 3, seed=9), P.noise(ih, iw, 3, seed=10)
        lut, lut2 = T.identity_lut(3), L.normalize_lut(3, MEAN[:3], STD[:3])
        ref, ref2 = c.resize(img, ow, oh), c.resize(img2, ow, oh)
        c.close()
        c = L.Context(0)                                  # a context that has not seen the shape
        c.resize_force(path)
        st = T.strides("chw", ow, oh, 3)
        x = torch.from_numpy(img).cuda()
        dl = torch.from_numpy(lut).cuda()
        y = torch.zeros((3, oh, ow), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), st,
                                   stream=torch.cuda.current_stream().cuda_stream)
        assert c.last_tensor_route() == (L.TENSOR_FUSED if path == L.RESIZE_FUSED else L.TENSOR_CONVERTED)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()              # captured, not run
        y2 = torch.zeros_like(y)
        c.resize_tensor_device(d, x.data_ptr(), y2.data_ptr(), 1, dl.data_ptr(), st,
                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _eq(y2.cpu().numpy(), T.tensor(ref, lut), "eager call before any replay")
        assert not y.view(torch.int32).any()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), T.tensor(ref, lut), "first replay")
        x.copy_(torch.from_numpy(img2))
        dl.copy_(torch.from_numpy(lut2))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), T.tensor(ref2, lut2), "replay after the table and the input changed")
        del g
    finally:
        c.close()
