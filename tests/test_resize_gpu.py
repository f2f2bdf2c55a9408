"""GPU checks of the resize-to-any-size entry (lanczos_resize_*): every byte identical to Pillow's fixture and to the numpy
model of the contract (tests/resize_model.py), no tolerance -- full-size shapes, both kernel paths, batches with frame
strides on a non-default stream, first use inside stream capture, and the CLI.  Every fused kernel instance, the geometry
edges of the fused march, saturating content, more than 65 535 frames and the bounded axis cache are covered on small frames
(the numpy model is the cost), with the coverage asserted through the plan query (lanczos_resize_plan_host).

Frames of 2 GiB and more (the 32-bit-offset fallback to two-pass), the largest frames the fused kernel accepts, frame strides
of 4 GiB and the launchers this file's 65 537 frames do not reach are run by tests/test_resize_wide_addresses_gpu.py, against a
reference that applies the numpy models to the window of the source a request reads (tests/resize_window_model.py)."""
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
    """Every byte around the frames is poison (255, or seeded noise): the gaps between frames, the 64 bytes behind the last
    one and the bytes in front of the first (the base pointer is offset by 0..3 bytes).  The fused kernel reads the
    neighbours that share a dword with a frame or a row and relies on zero coefficients there; a zero neighbour would hide a
    coefficient that is not."""
    for c in (3, 1, 4):
        _strided_batch(ctx, c)
    ctx.resize_force(L.RESIZE_AUTO)


def _strided_batch(ctx, c):
    import torch
    f, ih, iw, ow, oh = 5, 270, 481, 200, 150
    frames = np.stack([P.gradient_noise(ih, iw, c, seed=50 + k) for k in range(f)])
    want = M.resize(frames, ow, oh, 3)
    in_fb, out_fb = ih * iw * c, oh * ow * c
    in_fs, out_fs = in_fb + 13, out_fb + 7            # odd strides: unaligned frame starts
    s = torch.cuda.Stream()
    d = L.resize_desc(iw, ih, ow, oh, c, 3)
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


# ---------------------------------------------------------------------------------------------------------------
# Every fused instance, the edges of the fused march, content, frame loops, the axis cache.  Frames are small; what a
# case covers is asserted through the plan query and the public tables, so a shape list that drifts fails instead of losing
# coverage silently.

FUSED_K = (7, 9, 11, 13, 17, 25)


def _hks(iw, ow, a):
    return L.resize_taps_host(L.resize_desc(iw, 1, ow, 1, 1, a), 0)[2].shape[1]


def _plan(iw, ih, ow, oh, c, a, frames=1):
    return L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, a), frames)


def _all_paths(ctx, img, ow, oh, a, what):
    """FUSED (refused exactly where the plan says two-pass), TWO_PASS and AUTO against the model; returns the plan."""
    ih, iw, c = img.shape
    want = M.resize(img, ow, oh, a)
    p = _plan(iw, ih, ow, oh, c, a)
    try:
        ctx.resize_force(L.RESIZE_FUSED)
        if p.fused:
            _eq(ctx.resize(img, ow, oh, a), want, f"{what} fused")
            assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, what
        else:
            with pytest.raises(L.LanczosError) as e:
                ctx.resize(img, ow, oh, a)
            assert e.value.code == L.ERR_UNSUPPORTED, what
        ctx.resize_force(L.RESIZE_TWO_PASS)
        _eq(ctx.resize(img, ow, oh, a), want, f"{what} two-pass")
        assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS, what
        ctx.resize_force(L.RESIZE_AUTO)
        _eq(ctx.resize(img, ow, oh, a), want, f"{what} auto")
        assert ctx.last_kernel() == (L.KERNEL_RESIZE_FUSED if p.fused else L.KERNEL_RESIZE_TWO_PASS), what
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return p


def _smallest_fused_out_h(iw, ih, ow, c, a):
    """The smallest out_h < in_h (the largest vertical ksize) that still plans fused: its ring just fits the LDS budget."""
    for oh in range(1, ih):
        if _plan(iw, ih, ow, oh, c, a).fused:
            return oh
    raise AssertionError("no vertical downscale of this request plans fused")


# horizontal ksize -> (a, in_w) at out_w = 261: 256 + 5 columns (64 * 4 + 5 for four channels), rows of 261 and 783 bytes
H_KSIZE = {5: (2, 200), 7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 15: (3, 574), 17: (4, 496), 19: (3, 757),
           25: (3, 1018)}
V25 = {2: 21, 3: 31, 4: 41}     # out_h at in_h = 120 with a vertical ksize of 25


def test_every_fused_instance(ctx):
    """k_rs_fused<C, K> for every C in {1, 3, 4} and K in {7, 9, 11, 13, 17, 25}, at both edges of every bucket (ksize 5 | 7,
    15 | 17, 19 | 25), each with a small vertical ksize (an upscale), one of 25, and the largest whose ring still fits."""
    ow, ih = 261, 120
    seen = set()
    for c in (1, 3, 4):
        for hk, (a, iw) in H_KSIZE.items():
            assert _hks(iw, ow, a) == hk                       # from the public query, not recomputed
            k = next(b for b in FUSED_K if b >= hk)
            img = P.noise(ih, iw, c, seed=hk * 8 + c)
            oh_max = _smallest_fused_out_h(iw, ih, ow, c, a)
            for oh in (131, V25[a], oh_max):
                vk = _hks(ih, oh, a)
                if oh == V25[a]:
                    assert vk == 25
                p = _all_paths(ctx, img, ow, oh, a, f"C={c} hk={hk} vk={vk}")
                assert p.fused and p.K == k, (c, hk, vk, p.K)
                assert p.strips > 1 and (ow * c) % 4 != 0 or c == 4
                seen.add((c, p.K))
            assert _hks(ih, oh_max, a) > 25 and (oh_max == 1 or not _plan(iw, ih, ow, oh_max - 1, c, a).fused)
    assert seen == {(C, K) for C in (1, 3, 4) for K in (7, 9, 11, 13, 17, 25)}


def _sw(c):
    return 64 if c == 4 else 256


def _edge_cases(c):
    """(name, in_w, in_h, out_w, out_h, a) of the geometry edges for one channel count."""
    sw = _sw(c)
    cases = []
    for ow in (1, 2, 3, 5, sw - 1, sw, sw + 1, 2 * sw + 1):
        cases.append((f"out_w={ow}", max(2, (ow * 17 + 9) // 10), 40, ow, 23, 3))
    for oh in (1, 7, 8, 9, 31, 32, 33, 65):
        cases.append((f"out_h={oh}", 50, max(2, (oh * 17 + 9) // 10), 37, oh, 3))
    cases += [("in_w=1", 1, 20, 7, 13, 3), ("in_h=1", 20, 1, 13, 7, 3), ("in=1x1", 1, 1, 5, 4, 3),
              ("w 2->1000", 2, 30, 1000, 17, 3), ("h 2->1000", 30, 2, 17, 1000, 3),
              ("w 1000->2", 1000, 30, 2, 17, 3), ("h 1000->2", 30, 1000, 17, 2, 3),
              ("ksize 25", 1018, 40, 261, 23, 3), ("ksize 27", 1100, 40, 261, 23, 3),
              ("staging capped", 1017, 200, 261, 29, 3)]
    oh = _smallest_fused_out_h(300, 400, 261, c, 3)
    cases += [("ring just fits", 300, 400, 261, oh, 3), ("ring just does not fit", 300, 400, 261, oh - 1, 3)]
    return cases


@pytest.mark.parametrize("c", [1, 3, 4])
def test_geometry_edges(ctx, c):
    for name, iw, ih, ow, oh, a in _edge_cases(c):
        img = P.gradient_noise(ih, iw, c, seed=iw + 3 * oh + c)
        p = _all_paths(ctx, img, ow, oh, a, f"C={c} {name} {iw}x{ih}->{ow}x{oh}")
        if name in ("ksize 27", "ring just does not fit", "w 1000->2", "h 1000->2"):
            assert not p.fused, name
        elif name != "staging capped" or c == 3:
            assert p.fused, name
    assert _hks(1018, 261, 3) == 25 and _hks(1100, 261, 3) == 27


def test_geometry_edges_cover_the_branches():
    """What the edge list must contain, from the plan query and the tables (no launch here)."""
    import math
    chunks = strips = capped = unaligned = no_new_row = 0
    for c in (1, 3, 4):
        for name, iw, ih, ow, oh, a in _edge_cases(c):
            p = _plan(iw, ih, ow, oh, c, a)
            if not p.fused:
                continue
            chunks += p.chunks > 1
            strips += p.strips > 1
            capped += p.stage_rows < min(16, math.ceil(8 * ih / oh) + 1)
            # the byte-store path on every strip: the row pitch (frames from the allocator are aligned) is no dword multiple
            unaligned += (ow * c) % 4 != 0
            f, n, _ = L.resize_taps_host(L.resize_desc(iw, ih, ow, oh, c, a), 1)
            for ch in range(p.chunks):
                o_end = min((ch + 1) * p.rows_per_chunk, oh)
                need = [int(f[min(o0 + 8, o_end) - 1] + n[min(o0 + 8, o_end) - 1])
                        for o0 in range(ch * p.rows_per_chunk, o_end, 8)]
                no_new_row += any(b <= a_ for a_, b in zip(need, need[1:]))
    assert chunks and strips and capped and unaligned and no_new_row, (chunks, strips, capped, unaligned, no_new_row)


def _accumulators(img, ow, oh, a):
    """The model's unclipped accumulators of both passes (int64): [in_h][out_w][C] and [out_h][out_w][C]."""
    x = img.astype(np.int64)

    def gather(n_in, n_out):
        f, _, k = M.axis_tables(n_in, n_out, a)
        idx = np.minimum(f[:, None].astype(np.int64) + np.arange(k.shape[1])[None, :], n_in - 1)   # beyond count: coeff 0
        return idx, k.astype(np.int64)
    idx, k = gather(img.shape[1], ow)
    acc_h = (x[:, idx, :] * k[None, :, :, None]).sum(axis=2) + (1 << 21)
    t = np.clip(acc_h >> 22, 0, 255)
    idx, k = gather(img.shape[0], oh)
    acc_v = (t[idx, :, :] * k[:, :, None, None]).sum(axis=1) + (1 << 21)
    return acc_h, acc_v


@pytest.mark.parametrize("c", [1, 3, 4])
def test_content_saturates_both_clamps_of_both_passes(ctx, c):
    """All-0, all-255 and checkers at a down- and an upscale.  A 1-pixel checker saturates at the upscale only: at a downscale
    the filter removes it (the model's accumulators stay within 98..157 of 255 at 90 -> 61 and within 3..252 at 90 -> 89), so
    at the downscale the clamps are exercised by a 2-pixel checker, next to the 1-pixel one."""
    down, up = (90, 70, 61, 47), (61, 47, 90, 70)
    for iw, ih, ow, oh in (down, up):
        for name, img in (("zeros", np.zeros((ih, iw, c), np.uint8)), ("ones", np.full((ih, iw, c), 255, np.uint8))):
            _all_paths(ctx, img, ow, oh, 3, f"C={c} {name}")
            assert (ctx.resize(img, ow, oh, 3) == img[0, 0, 0]).all()
    for (iw, ih, ow, oh), cell in ((down, 1), (up, 1), (down, 2), (up, 2)):
        img = _checker(ih, iw, c, cell)
        _all_paths(ctx, img, ow, oh, 3, f"C={c} checker cell {cell} {iw}->{ow}")
        if (cell, (iw, ih, ow, oh)) == (1, down):
            continue
        out = ctx.resize(img, ow, oh, 3)
        assert out.min() == 0 and out.max() == 255
        for acc in _accumulators(img, ow, oh, 3):
            assert acc.min() < 0 and acc.max() > (255 << 22), (cell, iw, ow)


def test_more_than_65535_frames_in_one_call(ctx):
    """Both launch helpers split at 65 535 frames and re-base their pointers: 65 537 frames, every frame compared."""
    import torch
    f, ih, iw, c, ow, oh = 65537, 10, 12, 3, 7, 5
    base = np.stack([P.noise(ih, iw, c, seed=70 + k) for k in range(8)])
    frames = base[np.arange(f) % 8].copy()
    for j, k in enumerate((0, 65534, 65535, 65536)):
        frames[k] = P.gradient_noise(ih, iw, c, seed=90 + j)
    want8 = M.resize(base, ow, oh, 3)
    want = want8[np.arange(f) % 8].copy()
    for k in (0, 65534, 65535, 65536):
        want[k] = M.resize(frames[k], ow, oh, 3)
    assert len({want[k].tobytes() for k in (0, 65534, 65535, 65536, 1, 2)}) == 6
    x = torch.from_numpy(frames).cuda()
    d = L.resize_desc(iw, ih, ow, oh, c, 3)
    try:
        for path, family in ((L.RESIZE_FUSED, L.KERNEL_RESIZE_FUSED), (L.RESIZE_TWO_PASS, L.KERNEL_RESIZE_TWO_PASS)):
            ctx.resize_force(path)
            y = torch.full((f, oh, ow, c), 77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), f, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert ctx.last_kernel() == family
            _eq(y.cpu().numpy(), want, f"65537 frames path {path}")
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


def test_host_batches_with_growing_staging():
    c = L.Context(0)
    try:
        for f, ih, iw in ((2, 40, 50), (5, 90, 120), (3, 40, 50)):
            frames = np.stack([P.gradient_noise(ih, iw, 3, seed=30 + k) for k in range(f)])
            for path in (L.RESIZE_FUSED, L.RESIZE_TWO_PASS):
                c.resize_force(path)
                _eq(c.resize(frames, 37, 29, 3), M.resize(frames, 37, 29, 3), f"{f} frames of {iw}x{ih} path {path}")
    finally:
        c.close()


def _axis_shapes(n):
    """n requests over 2n distinct axis shapes (no axis repeats, H and V never share one)."""
    return [(20 + k, 90 + k, 31 + k, 57 + k) for k in range(n)]


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_axis_cache_survives_many_shapes(path):
    """More than 2 x kMaxAxes (32) axis shapes through one context, the first ones revisited in between and at the end."""
    c = L.Context(0)
    try:
        c.resize_force(path)
        shapes = _axis_shapes(40)                       # 80 axes
        order = shapes[:20] + shapes[:3] + shapes[20:] + shapes[:3] + shapes[-3:]
        for iw, ih, ow, oh in order:
            img = P.noise(ih, iw, 3, seed=iw)
            _eq(c.resize(img, ow, oh, 3), M.resize(img, ow, oh, 3), f"{iw}x{ih}->{ow}x{oh} path {path}")
    finally:
        c.close()


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_captured_tables_survive_axis_evictions(path):
    """A shape captured into a graph early, 80 other axis shapes afterwards, then the replay: the graph's tables are still there."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 77, 119, 43, 67
        img = P.gradient_noise(ih, iw, 3, seed=12)
        d = L.resize_desc(iw, ih, ow, oh, 3, 3)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for jw, jh, kw, kh in _axis_shapes(40):
            other = P.noise(jh, jw, 3, seed=jw)
            _eq(c.resize(other, kw, kh, 3), M.resize(other, kw, kh, 3), f"{jw}x{jh}->{kw}x{kh}")
        assert int(y.max()) == 0
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img, ow, oh, 3), "replay after 80 other axis shapes")
        _eq(c.resize(img, ow, oh, 3), M.resize(img, ow, oh, 3), "the captured shape, eagerly")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_one_shape_captured_into_two_graphs(path):
    """One shape captured into two graphs of one context (the second capture finds the tables the first one cached), 80 other
    axis shapes afterwards, then both replays and an eager call of the shape."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 77, 119, 43, 67
        img = P.gradient_noise(ih, iw, 3, seed=16)
        want = M.resize(img, ow, oh, 3)
        d = L.resize_desc(iw, ih, ow, oh, 3, 3)
        x = torch.from_numpy(img).cuda()
        ys = [torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        graphs = [torch.cuda.CUDAGraph() for _ in range(2)]
        s = torch.cuda.Stream()
        for g, y in zip(graphs, ys):
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
                c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for jw, jh, kw, kh in _axis_shapes(40):
            other = P.noise(jh, jw, 3, seed=jw)
            _eq(c.resize(other, kw, kh, 3), M.resize(other, kw, kh, 3), f"{jw}x{jh}->{kw}x{kh}")
        assert int(ys[0].max()) == 0 and int(ys[1].max()) == 0
        for k, (g, y) in enumerate(zip(graphs, ys)):
            g.replay()
            torch.cuda.synchronize()
            _eq(y.cpu().numpy(), want, f"replay of graph {k} after 80 other axis shapes")
        _eq(c.resize(img, ow, oh, 3), want, "the captured shape, eagerly")
        del graphs
    finally:
        c.close()


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_square_shape_first_used_inside_capture(path):
    """in_w == in_h and out_w == out_h: both axes are one cache entry.  Capture, eager call before any replay, replay."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        n_in, n_out = 97 + path, 59
        img, img2 = P.gradient_noise(n_in, n_in, 3, seed=13), P.noise(n_in, n_in, 3, seed=14)
        d = L.resize_desc(n_in, n_in, n_out, n_out, 3, 3)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((n_out, n_out, 3), dtype=torch.uint8, device="cuda")
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
        _eq(y2.cpu().numpy(), M.resize(img, n_out, n_out, 3), "eager call before any replay")
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img2, n_out, n_out, 3), "replay")
        big = P.noise(120, 120, 3, seed=15)               # another square shape
        _eq(c.resize(big, 70, 70, 3), M.resize(big, 70, 70, 3), "other square shape")
        x.copy_(torch.from_numpy(img))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img, n_out, n_out, 3), "replay after other work")
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
