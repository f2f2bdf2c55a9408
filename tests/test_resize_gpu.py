"""GPU checks of the resize-to-any-size entry (lanczos_resize_*): every byte identical to Pillow's fixture and to the numpy
model of the contract (tests/resize_model.py), no tolerance -- full-size shapes, both kernel paths, batches with frame
strides on a non-default stream, first use inside stream capture, and the CLI."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _checker(h, w, c, cell=1):
    y, x = np.mgrid[0:h, 0:w]
    v = (((y // cell) + (x // cell)) & 1) * 255
    return np.repeat(v[..., None], c, axis=2).astype(np.uint8)


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def test_pillow_fixture(ctx):
    z = np.load(GOLDEN)
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 12
    for name in names:
        img, want = z[f"{name}_in"], z[f"{name}_out"]
        oh, ow = want.shape[:2]
        for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
            ctx.resize_force(path)
            _eq(ctx.resize(img, ow, oh, 3), want, f"{name} path {path}")
    ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("pattern", ["gradient", "noise", "blocks", "checker"])
def test_4k_to_1080p(ctx, pattern):
    h, w, c = 2160, 3840, 3
    img = {"gradient": lambda: P.gradient_noise(h, w, c, seed=3), "noise": lambda: P.noise(h, w, c, seed=4),
           "blocks": lambda: P.blocks(h, w, c), "checker": lambda: _checker(h, w, c, cell=8)}[pattern]()
    out = ctx.resize(img, 1920, 1080, 3)
    _eq(out, M.resize(img, 1920, 1080, 3), pattern)
    assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
    if pattern == "checker":   # the ringing at every 0/255 edge saturates at both ends
        assert out.min() == 0 and out.max() == 255


@pytest.mark.parametrize("shape", [
    (7680, 4320, 1920, 1080), (1920, 1080, 1280, 720), (1920, 1080, 1366, 768), (3840, 2160, 160, 90),
    (1280, 720, 1920, 1080), (1920, 1080, 1920, 540), (1920, 1080, 1000, 1080)])
def test_full_size_shapes(ctx, shape):
    iw, ih, ow, oh = shape
    img = P.gradient_noise(ih, iw, 3, seed=iw + oh)
    _eq(ctx.resize(img, ow, oh, 3), M.resize(img, ow, oh, 3), str(shape))
    both = iw != ow and ih != oh
    if (iw, ih, ow, oh) == (3840, 2160, 160, 90):
        assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS   # ksize 145: the fused ring does not fit
    elif both:
        assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("a", [2, 3, 4])
def test_channels_and_a(ctx, channels, a):
    img = P.noise(600, 801, channels, seed=channels * 10 + a)
    want = M.resize(img, 517, 389, a)
    for path in (L.RESIZE_FUSED, L.RESIZE_TWO_PASS):
        ctx.resize_force(path)
        _eq(ctx.resize(img, 517, 389, a), want, f"C={channels} a={a} path {path}")
    ctx.resize_force(L.RESIZE_AUTO)
    if channels == 1:
        _eq(ctx.resize(img[..., 0], 517, 389, a), want[..., 0], "2-D input")


@pytest.mark.parametrize("shape", [
    (801, 600, 517, 389), (1920, 1080, 1280, 720), (640, 480, 1000, 701), (1000, 300, 333, 700), (999, 701, 1001, 350),
    (1024, 768, 256, 192), (257, 3, 100, 2), (5, 300, 2, 77)])
def test_both_paths_forced(ctx, shape):
    iw, ih, ow, oh = shape
    for c in (3, 4):
        img = P.gradient_noise(ih, iw, c, seed=iw * 7 + c)
        want = M.resize(img, ow, oh, 3)
        for path, family in ((L.RESIZE_FUSED, L.KERNEL_RESIZE_FUSED), (L.RESIZE_TWO_PASS, L.KERNEL_RESIZE_TWO_PASS)):
            ctx.resize_force(path)
            _eq(ctx.resize(img, ow, oh, 3), want, f"{shape} C={c} path {path}")
            assert ctx.last_kernel() == family
    ctx.resize_force(L.RESIZE_AUTO)


def test_fused_refused_where_it_cannot_run(ctx):
    img = P.noise(2160, 400, 3, seed=1)
    ctx.resize_force(L.RESIZE_FUSED)
    try:
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(img, 200, 90, 3)          # vertical ksize 145: the ring does not fit
        assert e.value.code == L.ERR_UNSUPPORTED
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(img, 200, 2160, 3)        # one axis only: nothing to fuse
        assert e.value.code == L.ERR_UNSUPPORTED
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


def test_batches_with_frame_strides_on_a_stream(ctx):
    import torch
    f, ih, iw, c, ow, oh = 5, 270, 481, 3, 200, 150
    frames = np.stack([P.gradient_noise(ih, iw, c, seed=50 + k) for k in range(f)])
    want = M.resize(frames, ow, oh, 3)
    in_fb, out_fb = ih * iw * c, oh * ow * c
    in_fs, out_fs = in_fb + 13, out_fb + 7            # odd strides: unaligned frame starts
    x = torch.zeros(f * in_fs + 64, dtype=torch.uint8, device="cuda")
    for k in range(f):
        x[k * in_fs:k * in_fs + in_fb] = torch.from_numpy(frames[k].reshape(-1)).cuda()
    s = torch.cuda.Stream()
    d = L.resize_desc(iw, ih, ow, oh, c, 3)
    for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED):
        ctx.resize_force(path)
        y = torch.full((f * out_fs + 64,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), f, in_fs, out_fs, s.cuda_stream)
        s.synchronize()
        got = y.cpu().numpy()
        for k in range(f):
            _eq(got[k * out_fs:k * out_fs + out_fb].reshape(oh, ow, c), want[k], f"frame {k} path {path}")
            assert (got[k * out_fs + out_fb:(k + 1) * out_fs] == 77).all(), "wrote into the gap between frames"
        assert (got[f * out_fs:] == 77).all()
    ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_first_use_inside_capture_then_eager_before_replay(path):
    """The tables of a shape first used inside stream capture are valid at once: an eager call BEFORE any replay gives the
    right bytes, and the graph replays right afterwards (and after a later eager call of other shapes)."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 83 + path, 131, 47, 61       # shapes no other test of this module uses
        img, img2 = P.gradient_noise(ih, iw, 3, seed=9), P.noise(ih, iw, 3, seed=10)
        d = L.resize_desc(iw, ih, ow, oh, 3, 3)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(y.max()) == 0                          # captured, not run
        y2 = torch.zeros_like(y)
        c.resize_device(d, x.data_ptr(), y2.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _eq(y2.cpu().numpy(), M.resize(img, ow, oh, 3), "eager call before any replay")
        assert int(y.max()) == 0
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img2, ow, oh, 3), "replay")
        big = P.noise(300, 400, 3, seed=11)               # another shape: may grow the two-pass scratch
        _eq(c.resize(big, 170, 120, 3), M.resize(big, 170, 120, 3), "other shape")
        x.copy_(torch.from_numpy(img))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img, ow, oh, 3), "replay after other work")
        del g
    finally:
        c.close()


def _write_png(path, img):
    h, w, c = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    ctype = {1: 0, 3: 2, 4: 6}[c]
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(maxsplit=4)
    assert parts[0] in (b"P6", b"P5")
    w, h = int(parts[1]), int(parts[2])
    c = 3 if parts[0] == b"P6" else 1
    return np.frombuffer(parts[4][:w * h * c], np.uint8).reshape(h, w, c)


def test_cli_resize_png(tmp_path):
    exe = os.path.join(ROOT, "lanczos-hls_amd", "lanczos_upscale")
    img = P.gradient_noise(150, 237, 3, seed=21)
    src = str(tmp_path / "in.png")
    _write_png(src, img)
    out = str(tmp_path / "out.ppm")
    r = subprocess.run([exe, src, out, "--size", "101x64", "--a", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kernel family" in r.stdout
    _eq(_read_ppm(out), M.resize(img, 101, 64, 3), "CLI")
    r = subprocess.run([exe, src, str(tmp_path / "o.png"), "--size", "0x64"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
