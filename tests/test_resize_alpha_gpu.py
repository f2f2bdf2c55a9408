"""GPU checks of LANCZOS_RESIZE_ALPHA (four channels with straight alpha resized as Pillow's mode RGBA, premultiplied and
un-premultiplied inside the kernels): every byte identical to Pillow's fixture (tests/golden/resize_pillow_alpha.npz) or to
the numpy model of the contract (tests/resize_alpha_model.py), no tolerance anywhere.  Both kernel paths, every fused
instance at both edges of its bucket (coverage asserted through the plan query), full-size frames, one-axis resizes, the
identity copy, strided batches on a stream with unaligned frame bases, stream capture, two metamorphic checks that need no
model, the clamp of the un-premultiply, the device helpers over every (value, alpha) pair, and the CLI."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_alpha_model as A
import resize_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_alpha.npz")
FUSED_K = (7, 9, 11, 13, 17, 25)
PATHS = ((L.RESIZE_FUSED, L.KERNEL_RESIZE_FUSED), (L.RESIZE_TWO_PASS, L.KERNEL_RESIZE_TWO_PASS))


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _rgba(h, w, seed, alpha="noise"):
    """Noise colour under noise alpha that has runs of 0, runs of 255 and everything between."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha == "noise":
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        y, x = np.mgrid[0:h, 0:w]
        a[(x // 5 + y // 3) % 4 == 0] = 0
        a[(x // 5 + y // 3) % 4 == 1] = 255
        img[..., 3] = a
    else:
        img[..., 3] = alpha
    return img


def _plan(iw, ih, ow, oh, a, frames=1):
    return L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True), frames)


def _hks(iw, ow, a):
    return L.resize_taps_host(L.resize_desc(iw, 1, ow, 1, 1, a), 0)[2].shape[1]


def _forced(ctx, img, ow, oh, a, what, want=None):
    """Both forced paths and AUTO against `want` (the model by default); returns the plan."""
    ih, iw = img.shape[-3], img.shape[-2]
    want = A.resize(img, ow, oh, a) if want is None else want
    p = _plan(iw, ih, ow, oh, a)
    try:
        for path, family in PATHS:
            ctx.resize_force(path)
            if path == L.RESIZE_FUSED and not p.fused:
                with pytest.raises(L.LanczosError) as e:
                    ctx.resize(img, ow, oh, a, alpha=True)
                assert e.value.code == L.ERR_UNSUPPORTED, what
                continue
            _eq(ctx.resize(img, ow, oh, a, alpha=True), want, f"{what} path {path}")
            assert ctx.last_kernel() == family, what
        ctx.resize_force(L.RESIZE_AUTO)
        _eq(ctx.resize(img, ow, oh, a, alpha=True), want, f"{what} auto")
        assert ctx.last_kernel() == (L.KERNEL_RESIZE_FUSED if p.fused else L.KERNEL_RESIZE_TWO_PASS), what
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return p


def test_pillow_fixture(ctx):
    z = np.load(GOLDEN)
    names = sorted(k[:-3] for k in z.files if k.endswith("_in"))
    assert len(names) >= 16
    for name in names:
        img, want = z[f"{name}_in"], z[f"{name}_out"]
        oh, ow = want.shape[:2]
        for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
            ctx.resize_force(path)
            _eq(ctx.resize(img, ow, oh, 3, alpha=True), want, f"{name} path {path}")
    ctx.resize_force(L.RESIZE_AUTO)


def test_flag_is_off_by_default_and_refused_without_four_channels(ctx):
    img = _rgba(40, 50, 1)
    _eq(ctx.resize(img, 23, 31, 3), M.resize(img, 23, 31, 3), "default is RGBX")
    assert not np.array_equal(M.resize(img, 23, 31, 3), A.resize(img, 23, 31, 3))
    for c in (1, 3):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(img[..., :c], 23, 31, 3, alpha=True)
        assert e.value.code == L.ERR_BAD_ARG


# horizontal ksize -> (a, in_w) at out_w = 261 (64 * 4 + 5 columns): both edges of every K bucket (5 | 7, 9, 11, 13,
# 15 | 17, 19 | 25), as tests/test_resize_gpu.py
H_KSIZE = {5: (2, 200), 7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 15: (3, 574), 17: (4, 496), 19: (3, 757),
           25: (3, 1018)}
V25 = {2: 21, 3: 31, 4: 41}     # out_h at in_h = 120 with a vertical ksize of 25


def test_every_fused_alpha_instance(ctx):
    """k_rs_fused<4, K, alpha> for every K at both edges of its bucket, each with a vertical upscale and a vertical ksize of 25."""
    ow, ih = 261, 120
    seen = set()
    for hk, (a, iw) in H_KSIZE.items():
        assert _hks(iw, ow, a) == hk                       # from the public query, not recomputed
        k = next(b for b in FUSED_K if b >= hk)
        img = _rgba(ih, iw, seed=hk)
        for oh in (131, V25[a]):
            if oh == V25[a]:
                assert _hks(ih, oh, a) == 25
            p = _forced(ctx, img, ow, oh, a, f"hk={hk} oh={oh}")
            assert p.fused and p.K == k and p.strips > 1, (hk, oh, p.K)
            seen.add((p.K, hk))
    assert {k for k, _ in seen} == set(FUSED_K)
    for lo, hi in ((5, 7), (15, 17), (19, 25)):            # both edges of the buckets that have two
        assert (hi, lo) in seen and (hi, hi) in seen


@pytest.mark.parametrize("shape", [(3840, 2160, 1920, 1080), (1920, 1080, 3840, 2160)])
def test_full_size_rgba(ctx, shape):
    iw, ih, ow, oh = shape
    img = P.gradient_noise(ih, iw, 4, seed=iw + oh)
    img[..., 3] = _rgba(ih, iw, seed=ow)[..., 3]
    _eq(ctx.resize(img, ow, oh, 3, alpha=True), A.resize(img, ow, oh, 3), str(shape))
    assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


@pytest.mark.parametrize("shape", [(801, 300, 517, 300), (300, 801, 300, 517), (300, 200, 1000, 200), (300, 200, 300, 777),
                                   (1920, 1080, 1920, 540), (1920, 1080, 1000, 1080)])
def test_one_axis_only(ctx, shape):
    """H-only and V-only: the one two-pass kernel that runs premultiplies and un-premultiplies; the fused kernel refuses."""
    iw, ih, ow, oh = shape
    img = _rgba(ih, iw, seed=iw + 2 * oh)
    p = _forced(ctx, img, ow, oh, 3, str(shape))
    assert not p.fused


def test_two_pass_with_more_taps_than_any_fused_instance(ctx):
    img = _rgba(400, 1100, seed=5)
    p = _forced(ctx, img, 261, 23, 3, "ksize 27 x 107")     # both kernels of the two-pass path, premultiplied scratch
    assert not p.fused and _hks(1100, 261, 3) == 27


def test_identity_is_a_copy(ctx):
    img = _rgba(57, 83, seed=6)
    assert not np.array_equal(A.unpremultiply(A.premultiply(img)), img)    # a round trip would show
    for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
        ctx.resize_force(path)
        _eq(ctx.resize(img, 83, 57, 3, alpha=True), img, f"identity path {path}")
    ctx.resize_force(L.RESIZE_AUTO)
    _eq(ctx.resize(np.stack([img, img[::-1]]), 83, 57, 3, alpha=True), np.stack([img, img[::-1]]), "identity batch")


def test_batches_with_frame_strides_on_a_stream(ctx):
    """Odd frame strides, poison in every gap, base leads of 0..3 bytes, a non-default stream, all three forced paths.  With a
    lead the pixels of a frame straddle the dwords the fused kernel stages: it shifts them out before it premultiplies."""
    import torch
    f, ih, iw, ow, oh, c = 5, 270, 481, 200, 150, 4
    frames = np.stack([_rgba(ih, iw, seed=50 + k) for k in range(f)])
    want = A.resize(frames, ow, oh, 3)
    in_fb, out_fb = ih * iw * c, oh * ow * c
    in_fs, out_fs = in_fb + 13, out_fb + 7            # odd strides: unaligned frame starts
    s = torch.cuda.Stream()
    d = L.resize_desc(iw, ih, ow, oh, c, 3, alpha=True)
    assert _plan(iw, ih, ow, oh, 3, f).fused
    try:
        for lead, poison in ((0, "255"), (1, "noise"), (2, "255"), (3, "noise")):
            n = lead + f * in_fs + 64
            if poison == "255":
                x = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
            else:
                x = torch.from_numpy(np.random.default_rng(lead).integers(0, 256, n, dtype=np.uint8)).cuda()
            for k in range(f):
                x[lead + k * in_fs:lead + k * in_fs + in_fb] = torch.from_numpy(frames[k].reshape(-1)).cuda()
            for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED):
                ctx.resize_force(path)
                y = torch.full((f * out_fs + 64,), 77, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    ctx.resize_device(d, x.data_ptr() + lead, y.data_ptr(), f, in_fs, out_fs, s.cuda_stream)
                s.synchronize()
                got = y.cpu().numpy()
                for k in range(f):
                    _eq(got[k * out_fs:k * out_fs + out_fb].reshape(oh, ow, c), want[k],
                        f"frame {k} path {path} lead {lead} {poison}")
                    assert (got[k * out_fs + out_fb:(k + 1) * out_fs] == 77).all(), "wrote into the gap between frames"
                assert (got[f * out_fs:] == 77).all()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_first_use_inside_capture_then_eager_then_replay(path):
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 85 + path, 133, 49, 63       # shapes no other test of this module uses
        img, img2 = _rgba(ih, iw, seed=9), _rgba(ih, iw, seed=10)
        d = L.resize_desc(iw, ih, ow, oh, 4, 3, alpha=True)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 4), dtype=torch.uint8, device="cuda")
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
        _eq(y2.cpu().numpy(), A.resize(img, ow, oh, 3), "eager call before any replay")
        assert int(y.max()) == 0
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), A.resize(img2, ow, oh, 3), "replay")
        # the same shape without the flag shares the cached tables
        _eq(c.resize(img, ow, oh, 3), M.resize(img, ow, oh, 3), "the same shape as RGBX")
        x.copy_(torch.from_numpy(img))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), A.resize(img, ow, oh, 3), "replay after other work")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("shape", [(301, 200, 173, 119), (120, 90, 317, 211)])
def test_opaque_frame_equals_rgbx(ctx, shape):
    """Alpha 255 everywhere: a constant 255 channel stays 255 through the tables (asserted through the model for this shape),
    premultiplying by 255 is the identity, and the result is exactly the RGBX one -- GPU against GPU, no model involved."""
    iw, ih, ow, oh = shape
    img = _rgba(ih, iw, seed=iw, alpha=255)
    assert (M.resize(img[..., 3], ow, oh, 3) == 255).all()
    assert np.array_equal(A.premultiply(img), img)
    for path, _ in PATHS:
        ctx.resize_force(path)
        rgbx = ctx.resize(img, ow, oh, 3)
        _eq(ctx.resize(img, ow, oh, 3, alpha=True), rgbx, f"{shape} path {path}")
        assert (rgbx[..., 3] == 255).all()
    ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("shape", [(301, 200, 173, 119), (120, 90, 317, 211)])
def test_transparent_frame_stays_transparent(ctx, shape):
    iw, ih, ow, oh = shape
    img = _rgba(ih, iw, seed=iw + 1, alpha=0)
    want = A.resize(img, ow, oh, 3)
    for path, _ in PATHS:
        ctx.resize_force(path)
        out = ctx.resize(img, ow, oh, 3, alpha=True)
        assert (out[..., 3] == 0).all()
        _eq(out, want, f"{shape} path {path}")
    ctx.resize_force(L.RESIZE_AUTO)
    assert (want[..., :3] == 0).all()                     # nothing of the hidden colour survives


def test_premultiplied_colour_above_alpha_is_clamped(ctx):
    """A soft-edged opaque disc of noise colour on a transparent ground, up- and downscaled: dark opaque pixels under the
    negative lobes pull alpha down further than the colour next to them, c' > A occurs at the output and the min() of the
    un-premultiply decides those samples.  Asserted through the model so that the case cannot be lost."""
    h, w = 90, 120
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot(x - w / 2, y - h / 2)
    img = _rgba(h, w, seed=7)
    img[..., 3] = np.clip((30 - r) * 60, 0, 255).astype(np.uint8)
    for ow, oh in ((317, 211), (77, 61)):
        assert A.clamp_hits(img, ow, oh, 3) > 0, (ow, oh)
        _forced(ctx, img, ow, oh, 3, f"disc -> {ow}x{oh}")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_device_helpers_exact_on_every_pair(tmp_path):
    """rs_premul_px / rs_unpremul_px (lanczos_alpha.hpp) on the device over all 65 536 (value, alpha) pairs each, against the
    literal integer formulas (tests/native/resize_alpha_check.hip): exhaustive, so this is the proof of the f32 division."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "resize_alpha_check")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "lanczos-hls_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "resize_alpha_check.hip"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "premultiply: all 65536 pairs exact" in r.stdout and "un-premultiply: all 65536 pairs exact" in r.stdout


def _write_png(path, img):
    h, w, c = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    ctype = {1: 0, 3: 2, 4: 6}[c]
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _read_png_rgba(path):
    """An 8-bit RGBA PNG without interlace, every filter type (the CLI's encoder may pick any)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, t = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if t == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        elif t == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert (depth, ctype, interlace) == (8, 6, 0), hdr
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * 4)
    out = np.zeros((h, w * 4), np.int64)
    for y in range(h):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(w * 4, np.int64)
        if ft == 0:
            out[y] = line
        elif ft == 2:
            out[y] = (line + up) & 255
        else:
            for i in range(w * 4):
                left = out[y, i - 4] if i >= 4 else 0
                ul = up[i - 4] if i >= 4 else 0
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + up[i]) >> 1
                else:
                    pa, pb, pc = abs(up[i] - ul), abs(left - ul), abs(left + up[i] - 2 * ul)
                    pred = left if pa <= pb and pa <= pc else (up[i] if pb <= pc else ul)
                out[y, i] = (line[i] + pred) & 255
    return out.astype(np.uint8).reshape(h, w, 4)


def test_cli_alpha(tmp_path):
    exe = os.path.join(ROOT, "lanczos-hls_amd", "lanczos_upscale")
    img = _rgba(75, 119, seed=21)
    src = str(tmp_path / "in.png")
    _write_png(src, img)
    out = str(tmp_path / "out.png")
    r = subprocess.run([exe, src, out, "--size", "51x32", "--alpha"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "straight alpha" in r.stdout
    _eq(_read_png_rgba(out), A.resize(img, 51, 32, 3), "CLI --alpha")
    r = subprocess.run([exe, src, out, "--size", "51x32", "--alpha", "--channels", "4"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    _eq(_read_png_rgba(out), A.resize(img, 51, 32, 3), "CLI --alpha --channels 4")
    r = subprocess.run([exe, src, out, "--size", "51x32", "--channels", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    _eq(_read_png_rgba(out), M.resize(img, 51, 32, 3), "CLI without --alpha: RGBX as before")
    for args in (["--alpha"], ["--size", "51x32", "--alpha", "--channels", "3"]):
        r = subprocess.run([exe, src, out] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--alpha needs" in r.stderr, args
    r = subprocess.run([exe, src, str(tmp_path / "out.ppm"), "--size", "51x32", "--alpha"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--alpha needs" in r.stderr
