"""The resize family at the 32-bit address edges: frames of 2^31 bytes and more, the largest frames the fused kernel accepts,
outputs and two-pass intermediates of 2^31 bytes, frame strides of 4 GiB, and more than 65 535 frames through every launcher
that splits a batch.  Everything is compared exactly (bytes; 32-bit patterns for float), and every route a case was built
for is asserted in the case.

The frames are huge, the work is not: a box or a band of output rows picks which addresses the kernels touch, the content is
generated on the device, and only the rectangles tests/resize_window_model.py asks for are copied to the host -- the
reference applies the numpy models' tables and passes to those.  What is left uncompared is said where it is.

Device memory: at most about 5 GiB at once (the strided cases: one buffer of 4 GiB + 1 MiB for the module, allocated when
the first of them runs; they come last, and the tests before them free what they hold).  Every test prints its duration and
its peak torch allocation.
"""
import time

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize32_model as M32
import resize_box_model as MB
import resize_filters_model as F
import resize_tensor_model as T
import resize_window_model as W
from test_resize_plan import FRAMES_2GIB, OUT_EDGE, corner_box, frames_below_2gib

pytestmark = pytest.mark.gpu

DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}
FAMILY = {"fused": L.KERNEL_RESIZE_FUSED, "two_pass": L.KERNEL_RESIZE_TWO_PASS, "nearest": L.KERNEL_RESIZE_NEAREST}
EDGE = 1 << 31


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _report(request):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[wide addresses] {request.node.name}: {time.perf_counter() - t0:.2f} s, "
          f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.3f} GiB")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _free():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _tdtype(bps):
    import torch
    return {1: torch.uint8, 2: torch.int16, 4: torch.float32}[bps]


def _generate(n, bps, seed):
    """n samples on the device from a seeded generator, filled in place in runs of 2^28 (no temporaries)"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.empty(n, dtype=_tdtype(bps), device="cuda")
    for i in range(0, n, 1 << 28):
        part = x[i:i + (1 << 28)]
        if bps == 4:
            part.normal_(0.0, 1000.0, generator=g)
        elif bps == 2:
            part.random_(-32768, 32768, generator=g)
        else:
            part.random_(0, 256, generator=g)
    return x


def _host(t, bps):
    a = t.contiguous().cpu().numpy()
    return a.view(np.uint16) if bps == 2 else a


def _fetcher(x, bps):
    """fetch(y0, y1, x0, x1) over the device frame x [H][W][C]: only that rectangle crosses to the host"""
    return lambda y0, y1, x0, x1: _host(x[y0:y1, x0:x1], bps)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = M32.differs(got, want) if got.dtype == np.float32 else got != want
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} samples differ, first at {at}: {got[at]} != {want[at]}")


def _bands(n, width, *around):
    """index runs of `width`: the first, the last, and one around each of `around`, clipped to [0, n)"""
    starts = [0, n - width] + [min(max(int(a) - width // 2, 0), n - width) for a in around]
    return [np.arange(s, s + width) for s in sorted(set(starts))]


class Frame:
    """One device frame [H][W][C] and its request, resized through lanczos_resize_device_ex and compared on chosen rows and
    columns with the windowed reference."""

    def __init__(self, spec, seed):
        self.name, self.iw, self.ih, self.c, self.kw, self.bps = spec
        self.dtype = DTYPES[self.bps]
        self.alpha = bool(self.kw.get("alpha"))
        self.pitch = self.iw * self.c * self.bps
        self.bytes = self.ih * self.pitch
        self.x = _generate(self.iw * self.ih * self.c, self.bps, seed).view(self.ih, self.iw, self.c)
        self.fetch = _fetcher(self.x, self.bps)

    def desc(self, ow, oh, filt=F.LANCZOS):
        return L.resize_desc(self.iw, self.ih, ow, oh, self.c, filter=filt, **self.kw)

    def axes(self, ow, oh, rows, cols, filt=F.LANCZOS, box=None):
        return W.axes(self.iw, self.ih, ow, oh, self.dtype, rows, cols, 3, filt, box)

    def run(self, ctx, ow, oh, box, force, family, filt=F.LANCZOS, windows=None, what=""):
        """windows: (rows, cols) index arrays to compare (None: everything).  Returns the device result."""
        import torch
        what = f"{self.name} {self.iw}x{self.ih}->{ow}x{oh} {F.NAMES[filt]} box {box} force {force} {what}"
        y = torch.full((oh, ow, self.c), 77, dtype=_tdtype(self.bps), device="cuda")
        ctx.resize_force(force)
        ctx.resize_device(self.desc(ow, oh, filt), self.x.data_ptr(), y.data_ptr(), 1, stream=_stream(), box=box)
        torch.cuda.synchronize()
        assert ctx.last_kernel() == FAMILY[family], (what, ctx.last_kernel())
        for rows, cols in windows or [(np.arange(oh), np.arange(ow))]:
            want = W.resize(self.fetch, self.iw, self.ih, ow, oh, self.c, self.dtype, rows, cols, 3, filt, self.alpha, box)
            r, q = torch.as_tensor(rows, device="cuda"), torch.as_tensor(cols, device="cuda")
            _same(_host(y[r][:, q], self.bps), want, f"{what} rows {rows[0]}.. cols {cols[0]}..")
        return y

    def refused(self, ctx, ow, oh, box):
        import torch
        y = torch.zeros((oh, ow, self.c), dtype=_tdtype(self.bps), device="cuda")
        ctx.resize_force(L.RESIZE_FUSED)
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(self.desc(ow, oh), self.x.data_ptr(), y.data_ptr(), 1, stream=_stream(), box=box)
        code = e.value.code
        del e                       # (it holds this frame, and with it the device frame, until a collection)
        assert code == L.ERR_UNSUPPORTED, self.name


# ---- a. input frames of 2^31 bytes or more ----------------------------------------------------------------------------------

def boxes_2a(iw, ih, pitch, cb):
    """The three fractional boxes of about 197 x 149 source pixels: top-left, bottom-right, and one whose rows straddle byte
    offset 2^31 of the frame, horizontally around the pixel that byte lies in."""
    row = EDGE // pitch
    col = (EDGE - row * pitch) // cb
    y1 = min(ih - 0.25, row + 74.75)
    x0 = min(max(col - 98.5, 0.25), iw - 198.0)
    return {"top-left": (0.25, 0.5, 197.5, 149.25), "bottom-right": corner_box(iw, ih),
            "straddling": (x0, y1 - 149.25, x0 + 197.25, y1)}


def one_axis_cases(spec):
    """(what, out_w, out_h, box, windows): resizes that change one axis only, the other full and at equal size, narrow outputs.
    Vertical only for every frame -- the box's rows reach the frame's last row, beyond byte 2^31 -- compared on three bands of
    64 columns; horizontal only, compared on three bands of 64 rows (the last ones lie beyond byte 2^31), for the frames with
    alpha and with 16-bit samples."""
    name, iw, ih, c, kw, bps = spec
    cases = [("vertical only", iw, 8, (0, ih - 150.75, iw, ih - 1.75),
              [(np.arange(8), b) for b in _bands(iw, 64, iw // 2)])]
    if name in ("rgba", "u16c3"):
        cases.append(("horizontal only", 8, ih, (iw - 150.75, 0, iw - 1.75, ih),
                      [(b, np.arange(8)) for b in _bands(ih, 64, ih // 2)]))
    return cases


@pytest.mark.parametrize("spec", FRAMES_2GIB, ids=[s[0] for s in FRAMES_2GIB])
def test_input_frames_of_2_gib(ctx, spec):
    """AUTO serves a frame of 2^31 bytes or more with two passes (k_rs_pass_h/_v, k_rs_h_alpha / k_rs_v_alpha), with one
    pass where a box changes one axis only, and with k_rs_nearest: 64-bit addresses throughout.  Forced FUSED is refused.
    Every output sample of the box cases is compared; of the one-axis cases, three bands."""
    name, iw, ih, c, kw, bps = spec
    ow, oh = OUT_EDGE
    fr = Frame(spec, seed=11)
    assert fr.bytes >= EDGE
    try:
        for where, box in boxes_2a(iw, ih, fr.pitch, c * bps).items():
            p = L.resize_plan_host(fr.desc(ow, oh), 1, box=box)
            assert p.pass_h and p.pass_v and not p.inner.fused, (name, where)
            if where == "straddling":      # from the model's tables: the vertical taps read the row that holds byte 2^31
                H, V = fr.axes(ow, oh, np.arange(oh), np.arange(ow), box=box)
                assert V.lo <= EDGE // fr.pitch < V.hi, (name, V.lo, V.hi)
            fr.run(ctx, ow, oh, box, L.RESIZE_AUTO, "two_pass", what=where)
        corner = corner_box(iw, ih)
        fr.refused(ctx, ow, oh, corner)
        for what, w, h, box, windows in one_axis_cases(spec):
            p = L.resize_plan_host(fr.desc(w, h), 1, box=box)
            assert (p.pass_h, p.pass_v) == ((0, 1) if what == "vertical only" else (1, 0)), (name, what)
            fr.run(ctx, w, h, box, L.RESIZE_AUTO, "two_pass", windows=windows, what=what)
        if name in ("u8c1", "u8c4", "f32c3"):
            fr.run(ctx, ow, oh, corner, L.RESIZE_AUTO, "nearest", filt=F.NEAREST)
        if name == "u8c1":
            import torch
            for filt in (F.BILINEAR, F.BICUBIC):
                fr.run(ctx, ow, oh, corner, L.RESIZE_AUTO, "two_pass", filt=filt)
            # the plain copy: equal size, no box -- one hipMemcpy2DAsync row of 2 GiB, compared on the device
            y = torch.zeros_like(fr.x)
            ctx.resize_force(L.RESIZE_AUTO)
            ctx.resize_device(fr.desc(iw, ih), fr.x.data_ptr(), y.data_ptr(), 1, stream=_stream())
            torch.cuda.synchronize()
            assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS
            for r in range(0, ih, 4096):   # (in runs of rows: the comparison's temporaries stay small)
                assert torch.equal(y[r:r + 4096], fr.x[r:r + 4096]), f"the plain copy of 2 GiB, rows from {r}"
            del y
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        del fr
        _free()


# ---- b. the largest frames the fused kernel accepts ---------------------------------------------------------------------------

def fused_strip_width(c, bps):
    """output pixels per strip of k_rs_fused (csrc/lanczos_resize.hpp rs_strip_width, restated)"""
    if bps == 4:
        return 128 if c == 1 else 64
    return 64 if c == 4 else 128 if bps == 2 else 256


def staged_end(spec, ow, oh, box):
    """(the byte offset at which the last staged row of the last strip ends, the frame's bytes), from the plan and the model's
    tables: a strip stages stage_dw dwords of a row from the dword that holds its first input pixel (frames from the allocator
    start on a dword), and the last row staged is the last one the vertical taps read."""
    name, iw, ih, c, kw, bps = spec
    d = L.resize_desc(iw, ih, ow, oh, c, **kw)
    p = L.resize_plan_host(d, 1, box=box).inner
    assert p.fused, (name, ow)
    H, V = W.axes(iw, ih, ow, oh, DTYPES[bps], np.arange(oh), np.arange(ow), box=box)
    sw = fused_strip_width(c, bps)
    assert p.strips == -(-ow // sw), (name, p.strips, sw)
    xs = int(H.first[(p.strips - 1) * sw])
    row = V.hi - 1
    cb = c * bps
    return ((row * iw * cb + xs * cb) & ~3) + 4 * p.stage_dw, iw * ih * cb


BELOW = frames_below_2gib()


@pytest.mark.parametrize("spec", BELOW, ids=[s[0] for s in BELOW])
def test_largest_frames_the_fused_kernel_accepts(ctx, spec):
    """Frames a few bytes below the planner's limit of 2^31 - 4: the fused kernel's 32-bit offsets at their largest.  The
    bottom-right box, to 173 x 131 (one strip; three for four channels) and to 261 x 131 (more than one strip everywhere),
    forced FUSED and forced TWO_PASS against the windowed reference, every sample.  For each request the last strip's last
    staged row must end past the frame's end -- the loads there are out of the buffer's range and must read as 0 under
    zero coefficients; it does for every sample width (asserted; the margins are printed).  8-bit, four channels: one
    tensor request (identity table, CHW) on the same frame must take the fused route."""
    import torch
    name, iw, ih, c, kw, bps = spec
    fr = Frame(spec, seed=23)
    box = corner_box(iw, ih)
    assert EDGE - 32768 <= fr.bytes <= EDGE - 5
    try:
        for ow in (OUT_EDGE[0], 261):
            oh = OUT_EDGE[1]
            end, size = staged_end(spec, ow, oh, box)
            print(f"\n[wide addresses] {name} {iw}x{ih}: {EDGE - size} bytes below 2^31; ->{ow}x{oh}: the last staged row ends "
                  f"{end - size} bytes past the frame's end, {'past' if end - 4 >= EDGE else 'below'} offset 2^31")
            assert end > size, (name, ow, end, size)
            assert L.resize_plan_host(fr.desc(ow, oh), 1, box=box).inner.strips > (1 if ow == 261 or c == 4 else 0)
            fr.run(ctx, ow, oh, box, L.RESIZE_FUSED, "fused")
            fr.run(ctx, ow, oh, box, L.RESIZE_TWO_PASS, "two_pass")
        if name == "u8c4":
            ow, oh = OUT_EDGE
            lut = T.identity_lut(c)
            dl = torch.from_numpy(lut).cuda()
            y = torch.zeros((c, oh, ow), dtype=torch.int32, device="cuda")
            ctx.resize_force(L.RESIZE_AUTO)
            ctx.resize_tensor_device(fr.desc(ow, oh), fr.x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(),
                                     L.tensor_strides("chw", ow, oh, c), stream=_stream(), box=box)
            torch.cuda.synchronize()
            assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
            want = W.resize(fr.fetch, iw, ih, ow, oh, c, np.uint8, np.arange(oh), np.arange(ow), box=box)
            _same(y.cpu().numpy().view(np.uint32), T.tensor(want, lut), "tensor request, fused")
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        del fr
        _free()


# ---- c. outputs and intermediates of 2^31 bytes or more --------------------------------------------------------------------

def _scattered(n, k, seed):
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def test_output_frame_of_2_gib():
    """40 x 30 -> 65535 x 32769, one channel: the output is 2^31 + 32767 bytes, so the plan says two passes (`bytes`), and
    k_rs_pass_v stores above 2^31.  Compared: all columns of rows 0..7, of the 8 rows around byte offset 2^31 of the output
    and of the last 8 rows (the offset lies in the last row, so those two bands overlap), and of 16 scattered rows
    (64 at first: cut down, the test took longer than test_more_than_65535_frames_in_one_call).  Left
    uncompared: every other row -- the bands cap the reference's cost, not the failures seen: a 32-bit offset that wraps shows
    in the straddling band and in everything behind it, which the last band is."""
    import torch
    iw, ih, ow, oh = 40, 30, 65535, 32769
    spec = ("u8c1", iw, ih, 1, {}, 1)
    assert ow * oh >= EDGE and not L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 1), 1).fused
    c = L.Context(0)
    fr = Frame(spec, seed=31)
    try:
        bands = _bands(oh, 8, EDGE // ow)
        assert any(b[0] <= EDGE // ow <= b[-1] for b in bands) and bands[-1][-1] == oh - 1 and bands[0][0] == 0
        rows = np.unique(np.concatenate(bands + [_scattered(oh, 16, 5)]))
        y = fr.run(c, ow, oh, None, L.RESIZE_AUTO, "two_pass", windows=[(rows, np.arange(ow))])
        del y
    finally:
        c.close()
        del fr
        _free()


def test_intermediate_of_2_gib_and_its_tensor():
    """328 x 32769 -> 65535 x 8, one channel: the two-pass intermediate is 32769 rows of 65535 bytes, 2^31 + 32767 bytes of
    context scratch, which k_rs_pass_h writes and k_rs_pass_v reads above 2^31 (every output row's taps reach the last rows).
    (328 columns, not fewer: a frame more than 100 times as tall as wide that shrinks in height runs vertical first, as Pillow
    does, through an intermediate of 8 rows; 32769 <= 100 * 328 keeps this one horizontal first.)
    Compared: all 8 rows at the first, the middle and the last 64 columns and at 16 scattered columns (64 at first: cut down for
    the same reason as above); the other columns are not
    (the reference costs 32769 intermediate rows per column).  Then the same request through the tensor entry (identity table,
    CHW): the converted route, k_rs_to_tensor behind the two passes, on the same columns.  (The byte frame k_rs_to_tensor reads
    here is 512 KiB; one above 2^31 bytes would have a float frame of 8 GiB.)"""
    import torch
    iw, ih, ow, oh = 328, 32769, 65535, 8
    assert ih <= 100 * iw
    spec = ("u8c1", iw, ih, 1, {}, 1)
    p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 1), 1, box=(0, 0, iw, ih))
    assert not p.inner.fused and p.pass_h and p.pass_v and p.mid_rows * ow >= EDGE
    c = L.Context(0)
    fr = Frame(spec, seed=37)
    try:
        cols = np.unique(np.concatenate(_bands(ow, 64, ow // 2) + [_scattered(ow, 16, 6)]))
        y = fr.run(c, ow, oh, None, L.RESIZE_AUTO, "two_pass", windows=[(np.arange(oh), cols)])
        lut = T.identity_lut(1)
        dl = torch.from_numpy(lut).cuda()
        t = torch.zeros((1, oh, ow), dtype=torch.int32, device="cuda")
        c.resize_tensor_device(fr.desc(ow, oh), fr.x.data_ptr(), t.data_ptr(), 1, dl.data_ptr(),
                               L.tensor_strides("chw", ow, oh, 1), stream=_stream())
        torch.cuda.synchronize()
        assert c.last_tensor_route() == L.TENSOR_CONVERTED and c.last_kernel() == L.KERNEL_RESIZE_TWO_PASS
        # the table applied to the bytes the byte request gave (compared with the reference above on `cols`), everywhere
        want = T.tensor(y.cpu().numpy(), lut)
        _same(t.cpu().numpy().view(np.uint32), want, "tensor request, converted")
        del y, t
    finally:
        c.close()
        del fr
        _free()


# ---- e. more than 65 535 frames through the launchers that have never split -----------------------------------------------

MANY = 65537
SPECIAL = (0, 65534, 65535, 65536)


def _many_frames(dtype, c):
    """65 537 frames of 12 x 10 as test_more_than_65535_frames_in_one_call builds them: eight base frames cycled, distinct
    frames at 0, 65534, 65535 and 65536.  Returns (frames, the twelve distinct frames, the index of each frame in them)."""
    def one(seed, gradient=False):
        if dtype == np.uint8:
            return (P.gradient_noise if gradient else P.noise)(10, 12, c, seed=seed)
        if dtype == np.uint16:
            return P.noise(10, 12, c, seed=seed, dtype=np.uint16)
        return (np.random.default_rng(seed).standard_normal((10, 12, c)) * 100).astype(np.float32)
    distinct = np.stack([one(70 + k) for k in range(8)] + [one(90 + j, True) for j in range(4)])
    index = np.arange(MANY) % 8
    index[list(SPECIAL)] = 8 + np.arange(4)
    return distinct[index], distinct, index


MANY_CASES = ["nearest", "reduce", "gap", "alpha two-pass", "u16 fused", "u16 two-pass", "f32 fused", "f32 two-pass",
              "tensor fused", "tensor converted"]


@pytest.mark.parametrize("case", MANY_CASES)
def test_more_than_65535_frames_through_every_launcher(ctx, case):
    """rs_nearest_launch, reduce_launch (alone and in front of a reducing_gap resize), rs_launch_pass with the alpha kernels,
    the 16-bit and float instances of rs_launch_fused and rs_launch_pass, the TENSOR instance of rs_launch_fused and
    rs_to_tensor_launch each split a batch at 65 535 frames and re-base their pointers: 65 537 frames, every frame compared."""
    import torch
    ow, oh = 7, 5
    dtype = np.uint16 if case.startswith("u16") else np.float32 if case.startswith("f32") else np.uint8
    c = 4 if case.startswith("alpha") else 3
    bps = np.dtype(dtype).itemsize
    kw = {"alpha": True} if c == 4 else {"bits": 16} if bps == 2 else {"f32": True} if bps == 4 else {}
    frames, distinct, index = _many_frames(dtype, c)
    x = torch.from_numpy(frames.view(np.int16) if bps == 2 else frames).cuda()
    force, family, filt, gap, tensor = L.RESIZE_AUTO, "fused", F.LANCZOS, None, False
    if case == "nearest":
        family, filt = "nearest", F.NEAREST
    elif case == "gap":
        ow, oh, gap = 3, 2, 2.0
        p = L.resize_plan_host(L.resize_desc(12, 10, ow, oh, c), MANY, reducing_gap=gap)
        assert p.fx > 1 and p.fy > 1 and p.inner.fused, (p.fx, p.fy)
    elif case.endswith("two-pass"):
        force, family = L.RESIZE_TWO_PASS, "two_pass"
    elif case.endswith("fused"):
        force = L.RESIZE_FUSED
    elif case == "tensor converted":
        force = L.RESIZE_CONVERT
    tensor = case.startswith("tensor")
    try:
        if case == "reduce":
            want = MB.reduce(distinct, 2)[index]
            y = torch.full(want.shape, 77, dtype=torch.uint8, device="cuda")
            ctx.reduce_device(12, 10, c, 2, x.data_ptr(), y.data_ptr(), MANY, stream=_stream())
            torch.cuda.synchronize()
            _same(y.cpu().numpy(), want, case)
            return
        want = F.resize(distinct, filt, ow, oh, reducing_gap=gap, alpha=c == 4)
        assert len({w.tobytes() for w in want}) == 12
        d = L.resize_desc(12, 10, ow, oh, c, filter=filt, **kw)
        ctx.resize_force(force)
        if tensor:
            lut = T.identity_lut(c)
            dl = torch.from_numpy(lut).cuda()
            y = torch.zeros((MANY, c, oh, ow), dtype=torch.int32, device="cuda")
            ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), MANY, dl.data_ptr(), L.tensor_strides("chw", ow, oh, c),
                                     stream=_stream())
            torch.cuda.synchronize()
            assert ctx.last_tensor_route() == (L.TENSOR_FUSED if case == "tensor fused" else L.TENSOR_CONVERTED)
            assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
            _same(y.cpu().numpy().view(np.uint32), T.tensor(want, lut)[index], case)
        else:
            y = torch.full((MANY, oh, ow, c), 77, dtype=_tdtype(bps), device="cuda")
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), MANY, stream=_stream(), reducing_gap=gap)
            torch.cuda.synchronize()
            assert ctx.last_kernel() == FAMILY[family], case
            _same(_host(y, bps), want[index], case)
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        del x
        _free()


# ---- d. frame strides of 4 GiB ----------------------------------------------------------------------------------------------

BIG_BYTES = (1 << 32) + (1 << 20)
GUARD = 4096
AT = GUARD          # where the first frame of a strided pair starts in the big buffer


@pytest.fixture(scope="module")
def big():
    """One buffer of 2^32 + 2^20 bytes for the module, never initialised as a whole."""
    import torch
    b = torch.empty(BIG_BYTES, dtype=torch.uint8, device="cuda")
    yield b
    del b
    torch.cuda.empty_cache()


def _stride(bps):
    return (1 << 32) + (13 if bps == 1 else 16)


def _bytes_of(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _place(big, frames, stride, poison):
    """two frames `stride` bytes apart in the big buffer, 4 KiB of poison in front of and behind each; returns the pointer"""
    fb = frames[0].nbytes
    assert len(frames) == 2 and AT + stride + fb + GUARD <= BIG_BYTES
    for k in range(2):
        at = AT + k * stride
        big[at - GUARD:at + fb + GUARD] = poison
        big[at:at + fb] = _bytes_of(frames[k])
    return big.data_ptr() + AT


def _collect(big, shape, dtype, stride, poison, what):
    """the two frames back from the big buffer; the poison around them must be intact"""
    fb = int(np.prod(shape)) * np.dtype(dtype).itemsize
    out = []
    for k in range(2):
        at = AT + k * stride
        raw = big[at - GUARD:at + fb + GUARD].cpu().numpy()
        assert (raw[:GUARD] == poison).all() and (raw[GUARD + fb:] == poison).all(), f"{what}: wrote around frame {k}"
        out.append(raw[GUARD:GUARD + fb].view(dtype).reshape(shape))
    return np.stack(out)


def _strided(big, call, src, out_shape, out_dtype, in_stride, out_stride, what):
    """call(d_in, d_out, in_frame_stride, out_frame_stride) with the big stride first on the input side (tight output), then
    on the output side (tight input); returns the two results [2][...] of out_dtype."""
    import torch
    results = []
    x = _bytes_of(src)
    ob = int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize
    y = torch.full((2 * ob,), 0x5A, dtype=torch.uint8, device="cuda")
    call(_place(big, src, in_stride, 0xA5), y.data_ptr(), in_stride, 0)
    torch.cuda.synchronize()
    results.append(y.cpu().numpy().view(out_dtype).reshape((2,) + tuple(out_shape)))
    blank = np.full((2,) + tuple(out_shape), 0, dtype=out_dtype)
    d_out = _place(big, blank, out_stride, 0x5A)
    call(x.data_ptr(), d_out, 0, out_stride)
    torch.cuda.synchronize()
    results.append(_collect(big, out_shape, out_dtype, out_stride, 0x5A, what))
    return results


def _pair(dtype, c, seed, h=89, w=117):
    if dtype == np.float32:
        return (np.random.default_rng(seed).standard_normal((2, h, w, c)) * 100).astype(np.float32)
    return np.stack([P.noise(h, w, c, seed=seed, dtype=dtype), P.gradient_noise(h, w, c, seed=seed + 1).astype(dtype) * (257 if dtype == np.uint16 else 1)])


# (name, dtype, channels, alpha, filter, force, kernel family)
STRIDED_RESIZES = [
    ("fused u8 c1", np.uint8, 1, False, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("fused u8 c3", np.uint8, 3, False, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("fused u8 c4", np.uint8, 4, False, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("fused rgba", np.uint8, 4, True, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("fused u16", np.uint16, 3, False, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("fused f32", np.float32, 3, False, F.LANCZOS, L.RESIZE_FUSED, "fused"),
    ("two-pass u8", np.uint8, 3, False, F.LANCZOS, L.RESIZE_TWO_PASS, "two_pass"),
    ("two-pass rgba", np.uint8, 4, True, F.LANCZOS, L.RESIZE_TWO_PASS, "two_pass"),
    ("two-pass u16", np.uint16, 3, False, F.LANCZOS, L.RESIZE_TWO_PASS, "two_pass"),
    ("two-pass f32", np.float32, 3, False, F.LANCZOS, L.RESIZE_TWO_PASS, "two_pass"),
    ("nearest u8 c3", np.uint8, 3, False, F.NEAREST, L.RESIZE_AUTO, "nearest"),
    ("nearest f32", np.float32, 3, False, F.NEAREST, L.RESIZE_AUTO, "nearest"),
    ("copy", np.uint8, 3, False, F.LANCZOS, L.RESIZE_AUTO, "two_pass"),
    ("gap", np.uint8, 3, False, F.LANCZOS, L.RESIZE_AUTO, "fused"),
]


@pytest.mark.parametrize("case", STRIDED_RESIZES, ids=[c[0] for c in STRIDED_RESIZES])
def test_resize_with_frames_4_gib_apart(ctx, big, case):
    """Two frames of 117 x 89 with different content, 2^32 + 16 bytes apart (2^32 + 13 for 8-bit: the second frame then starts
    on an odd byte), first on the input side, then on the output side, against the whole-frame numpy models.  Every launcher
    multiplies blockIdx.y or .z by that stride in 64 bits; the poison around the output frames must be intact."""
    name, dtype, c, alpha, filt, force, family = case
    bps = np.dtype(dtype).itemsize
    src = _pair(dtype, c, seed=len(name))
    ih, iw = src.shape[1:3]
    ow, oh, gap = (iw, ih, None) if name == "copy" else (20, 15, 2.0) if name == "gap" else (61, 97, None)
    kw = {"alpha": True} if alpha else {"bits": 16} if bps == 2 else {"f32": True} if bps == 4 else {}
    d = L.resize_desc(iw, ih, ow, oh, c, filter=filt, **kw)
    if name == "gap":
        p = L.resize_plan_host(d, 2, reducing_gap=gap)
        assert p.fx > 1 and p.fy > 1 and p.inner.fused
    want = F.resize(src, filt, ow, oh, reducing_gap=gap, alpha=alpha)

    def call(d_in, d_out, in_fs, out_fs):
        ctx.resize_device(d, d_in, d_out, 2, in_fs, out_fs, _stream(), reducing_gap=gap)
        assert ctx.last_kernel() == FAMILY[family], (name, ctx.last_kernel())
    try:
        ctx.resize_force(force)
        for side, got in zip(("input", "output"), _strided(big, call, src, (oh, ow, c), dtype, _stride(bps), _stride(bps), name)):
            _same(got, want, f"{name}, the stride on the {side} side")
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("route", ["fused", "converted"])
def test_tensor_with_frames_4_gib_apart(ctx, big, route):
    """The tensor entry on both routes: byte frames 2^32 + 13 bytes apart, then float frames 2^32 + 16 bytes apart."""
    c, ow, oh = 3, 61, 97
    src = _pair(np.uint8, c, seed=41)
    ih, iw = src.shape[1:3]
    d = L.resize_desc(iw, ih, ow, oh, c)
    lut = T.identity_lut(c)
    dl = _bytes_of(lut)
    want = T.tensor(F.resize(src, F.LANCZOS, ow, oh), lut)

    def call(d_in, d_out, in_fs, out_fs):
        ctx.resize_tensor_device(d, d_in, d_out, 2, dl.data_ptr(), L.tensor_strides("chw", ow, oh, c), in_fs, out_fs, _stream())
        assert ctx.last_tensor_route() == (L.TENSOR_FUSED if route == "fused" else L.TENSOR_CONVERTED), route
        assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
    try:
        ctx.resize_force(L.RESIZE_AUTO if route == "fused" else L.RESIZE_CONVERT)
        for side, got in zip(("input", "output"), _strided(big, call, src, (c, oh, ow), np.uint32, _stride(1), _stride(4), route)):
            _same(got, want, f"tensor {route}, the stride on the {side} side")
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


@pytest.mark.parametrize("factor", [2, (1366, 4)], ids=["k_reduce", "k_reduce_wide"])
def test_reduce_with_frames_4_gib_apart(ctx, big, factor):
    """lanczos_reduce_device reports no kernel; which one runs follows from the factor alone (reduce_launch: k_reduce_wide
    iff fx * channels is more than the 4096 bytes of a tile, k_reduce otherwise), asserted here on the factor."""
    c = 3
    fx = factor if isinstance(factor, int) else factor[0]
    assert (fx * c > 4096) == (factor != 2)
    src = _pair(np.uint8, c, seed=43, h=90, w=120)
    want = MB.reduce(src, factor)
    ow, oh = L.reduce_size(120, 90, factor)
    assert want.shape == (2, oh, ow, c)

    def call(d_in, d_out, in_fs, out_fs):
        ctx.reduce_device(120, 90, c, factor, d_in, d_out, 2, None, in_fs, out_fs, _stream())
    for side, got in zip(("input", "output"), _strided(big, call, src, (oh, ow, c), np.uint8, _stride(1), _stride(1), "reduce")):
        _same(got, want, f"reduce by {factor}, the stride on the {side} side")


def _upscale_cases():
    """(name, w, h, c, sn, sd, a, mode, main route, prefix route): the routes tests/test_upscale_routes_gpu.py reaches"""
    import test_upscale_routes_gpu as R
    wm, wt = R._width(3, 1, 2, True), R._width(3, 1, 2, False)
    cases = []
    for mode in (L.MODE_EXACT, L.MODE_LSB1):
        cases += [("march + riding", wm, 24, 3, 2, 1, 3, mode, R.MARCH, R.RIDING), ("tile + behind", wt, 24, 3, 2, 1, 3, mode, R.TILE, R.BEHIND),
                  ("ratp", 96, 60, 3, 3, 2, 3, mode, R.RATP, R.BEHIND), ("rat", 96, 60, 3, 5, 3, 3, mode, R.RAT, R.BEHIND),
                  ("generic + streamed", 24, 1000, 1, 1, 1, 3, mode, R.GENERIC, R.STREAMED)]
    return cases + [("hls", 64, 40, 3, 2, 1, 3, L.MODE_HLS, L.ROUTE_MAIN_HLS, R.NONE)]


def test_upscale_with_frames_4_gib_apart(ctx, big):
    """lanczos_resample_device with in / out_frame_stride = 2^32 + 16 on every route of the upscale entry, two frames of
    different content against the CPU oracle: EXACT bit-identical, LSB1 through test_parity_gpu._cmp, HLS mode against its
    model."""
    import oracle_lib as O
    import test_upscale_routes_gpu as R
    stride = (1 << 32) + 16
    oracle = {}
    for name, w, h, c, sn, sd, a, mode, main, prefix in _upscale_cases():
        src = np.stack([P.noise(h, w, c, seed=51), P.dark_noise(h, w, c, seed=52)])
        key = (w, h, c, sn, sd, a, mode == L.MODE_HLS)
        if key not in oracle:
            if mode == L.MODE_HLS:
                cfg = O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)
                oracle[key] = np.stack([O.hls_expected_hwc(cfg, img, 8) for img in src])
            else:
                oracle[key] = np.stack([R._oracle(img, sn, sd, a)[0] for img in src])
        want = oracle[key]
        d = L.make_desc(w, h, c, sn, sd, a, 1, mode)
        what = f"{name} {w}x{h}x{c} {sn}/{sd} a={a} mode {mode}"

        def call(d_in, d_out, in_fs, out_fs):
            ctx.resample_device(d, d_in, d_out, 2, in_fs, out_fs, _stream())
            r = ctx.last_route()
            assert (r.main, r.prefix, r.launches) == (main, prefix, 1), f"{what}: route {r}"
        for side, got in zip(("input", "output"), _strided(big, call, src, want.shape[1:], np.uint8, stride, stride, what)):
            for k in range(2):
                if mode == L.MODE_LSB1:
                    R._cmp(got[k], want[k], mode, f"{what}, frame {k}, {side} side", (src[k], sn, sd, a, ctx.last_kernel()))
                else:
                    _same(got[k], want[k], f"{what}, frame {k}, {side} side")
