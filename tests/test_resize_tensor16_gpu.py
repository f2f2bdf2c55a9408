"""GPU checks of the 16-bit tensor entry (lanczos_resize_tensor16_*): 8-bit frames resized straight into bfloat16 / float16
tensors through a table of 16-bit words.  Everything is compared as 16-bit patterns, never within a tolerance: against the
table applied to Context.resize's bytes (tests/resize_tensor16_model.py) and, for Pillow's fixtures, against torch's own
ToTensor() + Normalize() arithmetic cast by torch on the CPU.  Every fused instance runs with tables that name channel and
byte; the route (fused / converted) is asserted against the plan query; the device tests check that no 16-bit word the
strides do not name is touched, with frames that start 2 bytes past a dword."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_tensor16_model as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# ImageNet's constants; a fourth channel (RGBX, RGBA) and a single one (L) get constants of their own
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
PATHS = (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS)
DTYPES = ("bfloat16", "float16")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _eq(got, want, what):
    got, want = T.words(np.asarray(got)), T.words(np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {tuple(bad[0])}: "
                             f"{int(got[tuple(bad[0])]):#06x} != {int(want[tuple(bad[0])]):#06x}")


def _routes(ctx, img, ow, oh, lut, want, fused, what, paths=PATHS, dtype="bfloat16", **kw):
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
            assert got.dtype == (np.float16 if dtype == "float16" else np.uint16)
            _eq(got, want, f"{what} path {path}")
            expect = L.TENSOR_FUSED if fused and path not in (L.RESIZE_TWO_PASS, L.RESIZE_CONVERT) else L.TENSOR_CONVERTED
            assert ctx.last_tensor_route() == expect, (what, path, ctx.last_tensor_route())
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


# K -> (filter, a, in_w as a function of the strip width, out_w likewise): the shapes of tests/test_resize_tensor_gpu.py
def _instance_shape(K, c):
    sw = 64 if c == 4 else 256
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, (sw + sw // 3) // 2 + 2, sw + sw // 3 + 5
    a, iw = {7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 17: (4, 496), 25: (3, 1018)}[K]
    return "lanczos", a, iw, 261


@pytest.mark.parametrize("K", [3, 5, 7, 9, 11, 13, 17, 25])
def test_every_fused_instance_with_the_identity_table(ctx, K):
    """k_rs_fused<C, K, false, 2> for C = 1, 3, 4: more than one strip with a ragged last one, 75 output rows (a last block of
    3), more than one chunk, an odd out_w (rows and planes of a CHW frame start on 2-byte, not 4-byte, multiples); CHW and
    HWC.  The result's words are the channel and the byte of Context.resize."""
    for c in (1, 3, 4):
        filt, a, iw, ow0 = _instance_shape(K, c)
        ih, oh = 37, 75
        sw = 64 if c == 4 else 256
        # the widths of the short filters' shapes are even (346, 90): they run as they are and one pixel wider
        for ow in (ow0,) if ow0 % 2 else (ow0, ow0 + 1):
            d = L.resize_desc(iw, ih, ow, oh, c, a, filter=filt)
            p = L.resize_plan_host(d, 1)
            assert p.fused and p.K == K and p.strips > 1 and ow % sw and oh % 8 == 3 and p.chunks > 1, (c, K, p.K, ow)
            img = P.noise(ih, iw, c, seed=31 * K + c)
            ref = ctx.resize(img, ow, oh, a, filter=filt)
            assert ctx.last_tensor_route() == 0                    # a byte call is no tensor call
            for layout, lut in (("chw", T.identity_lut16(c)), ("hwc", T.special_lut16(c))):
                _routes(ctx, img, ow, oh, lut, T.tensor16(ref, lut, layout), True, f"K={K} C={c} {ow} {layout}", a=a,
                        filter=filt, layout=layout)
        assert ow % 2                                              # an odd width ran


def test_alpha_instances(ctx):
    """LANCZOS_RESIZE_ALPHA has the epilogue too: k_rs_fused<4, K, true, 2> at one shape per K"""
    rng = np.random.default_rng(3)
    for K in (3, 5, 7, 9, 11, 13, 17, 25):
        filt, a, iw, ow = _instance_shape(K, 4)
        ih, oh = 37, 75
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True, filter=filt), 1)
        assert p.fused and p.K == K
        img = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
        lut = T.identity_lut16(4)
        ref = ctx.resize(img, ow, oh, a, alpha=True, filter=filt)
        _routes(ctx, img, ow, oh, lut, T.tensor16(ref, lut), True, f"alpha K={K}", a=a, filter=filt, alpha=True)


def test_the_table_is_moved_not_computed_on(ctx):
    """zeros, subnormals, infs and NaNs of both formats arrive as they are, a float16 table as well as a uint16 one, on the
    fused and on the converted route (forced CONVERT: the resize as AUTO plans it, then k_rs_to_tensor16)"""
    img = P.noise(41, 90, 3, seed=4)
    ref = ctx.resize(img, 70, 35)
    for lut in (T.identity_lut16(3), T.special_lut16(3), T.special_lut16(3).view(np.float16)):
        for dtype in DTYPES:
            _routes(ctx, img, 70, 35, lut, T.tensor16(ref, lut), True, f"special {lut.dtype} {dtype}",
                    paths=(L.RESIZE_AUTO, L.RESIZE_CONVERT), dtype=dtype)
    with pytest.raises(L.LanczosError):                        # a float32 table is not a 16-bit one, and the reverse
        ctx.resize_tensor(img, 70, 35, lut=np.zeros((3, 256), dtype=np.float32), dtype="bfloat16")
    with pytest.raises(L.LanczosError):
        ctx.resize_tensor(img, 70, 35, lut=T.identity_lut16(3))
    with pytest.raises(L.LanczosError):
        ctx.resize_tensor(img, 70, 35, dtype="int8")


def _device_case(ctx, c, iw, ih, ow, oh, st, frames, frame_stride, lead, in_gap, path, what):
    """One device call into a guarded buffer filled with 0xA5A5 whose frames start 2 bytes past a dword: every element the
    contract names has its value, every other 16-bit word of the buffer -- guards in front and behind, row, plane and frame
    padding -- still holds 0xA5A5."""
    import torch
    SENTINEL, GUARD = 0xA5A5, 65                               # an odd guard: the first frame is 2 bytes past a dword
    imgs = np.stack([P.noise(ih, iw, c, seed=70 + 5 * k + c) for k in range(frames)])
    lut = T.identity_lut16(c)                                  # no entry is 0xA5A5
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
    want = np.full(total, SENTINEL, dtype=np.uint16)
    named = T.scatter(want, GUARD, ref, lut, st, fs)
    assert named == frames * c * oh * ow
    y = torch.from_numpy(np.full(total, SENTINEL, dtype=np.uint16).view(np.int16)).cuda()
    assert y.data_ptr() % 4 == 0 and (y.data_ptr() + 2 * GUARD) % 4 == 2
    dl = torch.from_numpy(lut.view(np.int16)).cuda()
    ctx.resize_force(path)
    try:
        s = torch.cuda.current_stream().cuda_stream
        ctx.resize_tensor_device(d, x.data_ptr() + lead, y.data_ptr() + 2 * GUARD, frames, dl.data_ptr(), st,
                                 in_frame_stride=in_fs if in_gap else 0, out_frame_stride=2 * frame_stride, stream=s,
                                 dtype="bfloat16")
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    _eq(y.cpu().numpy().view(np.uint16), want, what)
    return ctx.last_tensor_route()


@pytest.mark.parametrize("c", [1, 3, 4])
def test_nothing_else_is_written(ctx, c):
    """A fused shape and one that is not (a horizontal pass only), out_w odd and even, padded rows (out_w + 3) and planes, CHW
    and HWC, the frame 2 bytes past a dword: the named elements and no other 16-bit word."""
    iw, ih = 90, 41
    for ow in (70, 71):
        for oh, fused in ((35, True), (ih, False)):
            assert bool(L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c), 1).fused) == fused
            row = ow + 3
            padded = (oh * row + 5, row, 1)
            layouts = {"chw": T.strides("chw", ow, oh, c), "hwc": T.strides("hwc", ow, oh, c), "padded chw": padded,
                       "padded hwc": (1, ow * c + 7, c)}
            for name, st in layouts.items():
                for path in (L.RESIZE_AUTO, L.RESIZE_CONVERT):
                    got = _device_case(ctx, c, iw, ih, ow, oh, st, 1, 0, 0, 0, path, f"C={c} {ow}x{oh} {name} path {path}")
                    assert got == (L.TENSOR_FUSED if fused and path == L.RESIZE_AUTO else L.TENSOR_CONVERTED), (name, path)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_a_batch_with_frame_strides(ctx, c):
    """5 frames, both frame strides larger than tight, the output one an odd number of elements (2 bytes times an odd number: a
    multiple of 2 and not of 4), an odd input base; both routes"""
    iw, ih, ow, oh = 90, 41, 71, 35
    assert L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c), 5).fused
    for name, st in (("chw", T.strides("chw", ow, oh, c)), ("padded hwc", (1, ow * c + 7, c))):
        fs = T.extent(ow, oh, c, st) + 10
        fs += 1 - fs % 2
        assert (2 * fs) % 4 == 2
        for path, route in ((L.RESIZE_AUTO, L.TENSOR_FUSED), (L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED)):
            got = _device_case(ctx, c, iw, ih, ow, oh, st, 5, fs, 1, 13, path, f"batch C={c} {name} path {path}")
            assert got == route, (name, path, got)


def test_device_argument_checks(ctx):
    import torch
    d = L.resize_desc(90, 41, 70, 35, 3)
    x = torch.zeros(90 * 41 * 3, dtype=torch.uint8, device="cuda")
    y = torch.zeros(70 * 35 * 3 + 8, dtype=torch.int16, device="cuda")
    dl = torch.from_numpy(T.identity_lut16(3).view(np.int16)).cuda()
    st = T.strides("chw", 70, 35, 3)
    for kw, ptr in (({}, y.data_ptr() + 1), ({"out_frame_stride": 2 * 70 * 35 * 3 + 1}, y.data_ptr()),
                    ({"out_frame_stride": 2 * 70 * 35 * 3 - 2}, y.data_ptr())):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_device(d, x.data_ptr(), ptr, 1, dl.data_ptr(), st, dtype="float16", **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
        assert ctx.last_tensor_route() == 0
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), (1, 1, 1), dtype="float16")
    assert e.value.code == L.ERR_BAD_ARG
    # a ready TensorOut16 needs no dtype; a frame 2 bytes past a dword is fine
    ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr() + 2, 1, None, L.tensor16_out(dl.data_ptr(), st))
    torch.cuda.synchronize()
    assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


def _torch_want(pillow_out, dtype):
    """torchvision's pipeline on the CPU (IEEE division) over Pillow's bytes, cast by torch, as words [C][H][W]"""
    import torch
    c = pillow_out.shape[2]
    mean = torch.tensor(MEAN[:c], dtype=torch.float32)[:, None, None]
    std = torch.tensor(STD[:c], dtype=torch.float32)[:, None, None]
    x = torch.from_numpy(np.ascontiguousarray(pillow_out)).permute(2, 0, 1).float().div(255).sub(mean).div(std)
    return x.contiguous().to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


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
        for dtype in DTYPES:
            want = _torch_want(out, dtype)
            got = ctx.resize_tensor(img, ow, oh, mean=MEAN[:c], std=STD[:c], alpha=alpha, dtype=dtype)
            _eq(got, want, f"{fixture} {name} {dtype}")
            assert ctx.last_tensor_route() == (L.TENSOR_FUSED if p.fused else L.TENSOR_CONVERTED), name
            lut = L.normalize_lut(c, MEAN[:c], STD[:c], dtype=dtype)
            _routes(ctx, img, ow, oh, lut, want, bool(p.fused), f"{fixture} {name} {dtype}", paths=(L.RESIZE_TWO_PASS,),
                    dtype=dtype, alpha=alpha)
    assert fused >= 6, fused
    # the one-liner of Context.resize_tensor's docstring: the bfloat16 words are the tensor torch would hold
    import torch
    got = ctx.resize_tensor(img, ow, oh, mean=MEAN[:c], std=STD[:c], alpha=alpha, dtype="bfloat16")
    t = torch.from_numpy(got.view(np.int16)).view(torch.bfloat16)
    want = torch.from_numpy(_torch_want(out, "bfloat16").view(np.int16)).view(torch.bfloat16)
    assert t.dtype == torch.bfloat16 and torch.equal(t, want)


def test_other_routes(ctx):
    """nearest, a box, reducing_gap that reduces, one-axis resizes and the copy itself: the table over Context.resize's bytes"""
    img = P.gradient_noise(120, 160, 3, seed=12)
    lut = L.normalize_lut(3, MEAN[:3], STD[:3], dtype="bfloat16")
    cases = [("nearest", 71, 53, {"filter": "nearest"}, False),
             ("box", 64, 48, {"box": (10.5, 7.25, 130.0, 99.5)}, True),
             ("gap 2", 20, 15, {"reducing_gap": 2.0}, True),
             ("h only", 77, 120, {}, False), ("v only", 160, 50, {}, False), ("copy", 160, 120, {}, False)]
    for name, ow, oh, kw, fused in cases:
        d = L.resize_desc(160, 120, ow, oh, 3, filter=kw.get("filter", "lanczos"))
        opts = {k: v for k, v in kw.items() if k != "filter"}
        p = L.resize_plan_host(d, 1, **opts)
        inner = p.inner if opts else p
        assert bool(inner.fused) == fused, name
        if name.startswith("gap"):
            assert p.fx > 1 and p.fy > 1
        ref = ctx.resize(img, ow, oh, **kw)
        for layout in ("chw", "hwc"):
            if kw.get("filter") == "nearest":             # one path: forced FUSED is refused for it, as for the bytes
                ctx.resize_force(L.RESIZE_AUTO)
                _eq(ctx.resize_tensor(img, ow, oh, lut=lut, layout=layout, dtype="bfloat16", **kw),
                    T.tensor16(ref, lut, layout), name)
                assert ctx.last_tensor_route() == L.TENSOR_CONVERTED and ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
            else:
                _routes(ctx, img, ow, oh, lut, T.tensor16(ref, lut, layout), fused, f"{name} {layout}", layout=layout, **kw)
    # batches and 2-D input keep Context.resize's shapes
    batch = np.stack([img, img[::-1]])
    got = ctx.resize_tensor(batch, 64, 48, lut=lut, dtype="bfloat16")
    assert got.shape == (2, 3, 48, 64) and got.dtype == np.uint16
    _eq(got, T.tensor16(ctx.resize(batch, 64, 48), lut), "batch")
    grey = img[..., 0].copy()
    got = ctx.resize_tensor(grey, 64, 48, mean=0.5, std=0.5, layout="hwc", dtype="float16")
    assert got.shape == (48, 64, 1) and got.dtype == np.float16
    _eq(got[..., 0], T.tensor16(ctx.resize(grey, 64, 48), L.normalize_lut(1, 0.5, 0.5, dtype="float16"))[0], "2-D input")
