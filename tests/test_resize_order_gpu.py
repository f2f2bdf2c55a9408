"""GPU checks of the pass order (Pillow 12.2.0's Image.resize runs a frame with height > 100 * width that shrinks in height
vertical first; include/lanczos_hip.h): every case of tests/golden/resize_pillow_tall.npz against Pillow's
bytes through AUTO, TWO_PASS and FUSED; one tall shape per sample kind through every follower of the byte result (window,
tensors, view, crops, sources, reducing_gap, strided batches, a captured graph) against the numpy models, between sentinels;
and the widest frame the rule can reach, 655 x 65535, with its twin 656 x 65535 on the other side.  The kernel family and the
routes the context reports are asserted throughout."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_box_model as MB
import resize_filters_model as FM
import resize_matrix_cfg as MC
import resize_model as M
import resize_source_model as SM
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V
import resize_window_model as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_tall.npz")
FORCE_NAMES = {L.RESIZE_AUTO: "AUTO", L.RESIZE_TWO_PASS: "TWO_PASS", L.RESIZE_FUSED: "FUSED"}


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize_tall_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_tall_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g, g.load(GOLDEN)


# ---- the fixture: Pillow's bytes -------------------------------------------------------------------------------------------

def _host_call(ctx, f, m, img, ow, oh, box, gap):
    if m == "F":
        return ctx.resize_f32(img, ow, oh, box=box, filter=f)
    return ctx.resize(img, ow, oh, alpha=m == "RGBA", box=box, reducing_gap=gap, filter=f)


def test_fixture_cases_give_pillows_bytes(ctx):
    """171 cases x AUTO and TWO_PASS: Pillow's bytes (mode F: its 32-bit patterns) and the kernel family.  Forcing FUSED
    refuses every case that runs vertical first with LANCZOS_ERR_UNSUPPORTED and still runs, fused, the twins on the other side
    of each edge whose two passes both run.  A wrong result is counted and the walk goes on, so that a failure says how many."""
    g, cases = _golden()
    failures = []
    ran = {"fused": 0, "refused": 0, "v_first": 0}
    for name, case in cases.items():
        f, m, iw, ih, ow, oh, box, gap, img, want = case
        nearest = f == "nearest"
        both = g.both_run(MB, FM, case[:8])
        tall = g.vertical_first(*g.reduced_size(FM, case[:8]), oh)
        v_first = tall and both and not nearest
        ran["v_first"] += v_first
        for force in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED):
            what = f"{name} {FORCE_NAMES[force]}"
            ctx.resize_force(force)
            fusable = both and not nearest and not v_first
            if force == L.RESIZE_FUSED and not fusable:
                try:
                    _host_call(ctx, f, m, img, ow, oh, box, gap)
                    failures.append(f"{what}: not refused")
                except L.LanczosError as e:
                    if e.code != L.ERR_UNSUPPORTED:
                        failures.append(f"{what}: refused with {e.code}")
                ran["refused"] += 1
                continue
            try:
                got = _host_call(ctx, f, m, img, ow, oh, box, gap)
            except L.LanczosError as e:
                failures.append(f"{what}: error {e.code}")
                continue
            if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
                failures.append(f"{what}: {int((got.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ from Pillow's")
            kernel = (L.KERNEL_RESIZE_NEAREST if nearest and any(g.axes_run(MB, FM, case[:8]))
                      else L.KERNEL_RESIZE_FUSED if fusable and force != L.RESIZE_TWO_PASS else L.KERNEL_RESIZE_TWO_PASS)
            if ctx.last_kernel() != kernel:
                failures.append(f"{what}: kernel family {ctx.last_kernel()}, not {kernel}")
            ran["fused"] += force == L.RESIZE_FUSED
    print(f"{len(cases)} cases: {ran}; {len(failures)} failures")
    assert not failures, f"{len(failures)} failures, the first: {failures[0]}"
    assert ran["v_first"] == 118 and ran["fused"] == 28 and ran["refused"] == 143, ran


# ---- one tall shape per sample kind, through every follower ---------------------------------------------------------------

IW, IH, OW, OH = 5, 640, 12, 77
FRAMES = 3
SENT = MC.SENTINEL
GUARD = 64
WINDOW = (3, 5, 7, 61)
CROP = (7, 61)
ORIGINS = np.array([(5, 16), (12, -3), (1, 3)], dtype=np.int32)   # the far corner, one the kernels clamp on both axes, an odd one
KINDS = {"u8x1": (1, np.uint8, False), "u8x3": (3, np.uint8, False), "rgba": (4, np.uint8, True), "u16x1": (1, np.uint16, False),
         "f32x3": (3, np.float32, False)}


@functools.lru_cache(maxsize=None)
def _frames(kind, iw=IW, ih=IH):
    c, dtype, alpha = KINDS[kind]
    rng = np.random.default_rng(900 + list(KINDS).index(kind))
    if dtype == np.float32:
        x = rng.standard_normal((FRAMES, ih, iw, c)).astype(np.float32)
    else:
        x = rng.integers(0, np.iinfo(dtype).max + 1, (FRAMES, ih, iw, c)).astype(dtype)
    if alpha:
        a = x[..., 3]
        a[rng.random(a.shape) < 0.25] = 0
        a[rng.random(a.shape) < 0.25] = 255
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _full(kind, iw=IW, ih=IH, ow=OW, oh=OH, box=None, gap=None):
    y = np.ascontiguousarray(FM.resize(_frames(kind, iw, ih), FM.LANCZOS, ow, oh, box, gap, alpha=KINDS[kind][2]))
    y.setflags(write=False)
    return y


def _desc(kind, iw=IW, ih=IH, ow=OW, oh=OH):
    c, dtype, alpha = KINDS[kind]
    return L.resize_desc(iw, ih, ow, oh, c, 3, alpha=alpha, bits=16 if dtype == np.uint16 else 8, f32=dtype == np.float32)


class _Out:
    """a device buffer of sentinels and the expected array beside it: GUARD elements, FRAMES frames `fs` elements apart (7
    more than a frame's extent), GUARD elements"""

    def __init__(self, torch, item, n):
        self.item, self.n, self.fs = item, n, n + 7
        self.total = GUARD + (FRAMES - 1) * self.fs + n + GUARD
        self.dev = torch.full((self.total * item,), SENT, dtype=torch.uint8, device="cuda")
        word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[item]
        self.want = np.full(self.total * item, SENT, dtype=np.uint8).view(word)

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD * self.item

    def check(self, torch, what, f32=False):
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy().view(self.want.dtype)
        diff = MC.first_difference(got, self.want, f32)
        assert diff is None, f"{what}: first difference at element {diff[0]}: {diff[1]:#x} != {diff[2]:#x}"


def _reports(ctx, what, tensor=None, source=None):
    assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS, (what, ctx.last_kernel())
    if tensor is not None:
        assert ctx.last_tensor_route() == tensor, (what, ctx.last_tensor_route())
    if source is not None:
        assert ctx.last_source_route() == source, (what, ctx.last_source_route())


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_follower_of_a_tall_request(ctx, kind):
    """5 x 640 -> 12 x 77, three frames, through the device entries on a side stream into sentinels, against the models composed
    on the CPU: the strided batch from an odd base, a sub-window, float32 and bfloat16 tensors in CHW and HWC, a view with a
    channel map and both flips, crop origins per frame, pitched and planar sources with noise in the bytes they do not name,
    and reducing_gap on both sides of the rule.  Every call reports RESIZE_TWO_PASS, CONVERTED and PACKED."""
    import torch
    c, dtype, alpha = KINDS[kind]
    item = np.dtype(dtype).itemsize
    f32 = dtype == np.float32
    u8 = dtype == np.uint8
    x = _frames(kind)
    full = _full(kind)
    assert M.pillow_vertical_first(IW, IH, OH) and not FM.same(full, FM.resize(x, FM.LANCZOS, OW, OH, alpha=alpha, order="h_first"))
    d = _desc(kind)
    side = torch.cuda.Stream()
    frame = IW * IH * c * item
    # the batch: frames an odd number of samples apart, the first an odd number of samples into its buffer
    in_fs = frame + 5 * item
    raw = np.random.default_rng(7).integers(1, 256, 3 * item + FRAMES * in_fs, dtype=np.uint8)
    for k in range(FRAMES):
        raw[3 * item + k * in_fs:3 * item + k * in_fs + frame] = x[k].reshape(-1).view(np.uint8)
    strided = torch.from_numpy(raw).cuda()
    tight = torch.from_numpy(x.reshape(-1).view(np.uint8).copy()).cuda()
    flips = torch.tensor([0, 1, 2], dtype=torch.uint8).cuda()
    origins = torch.from_numpy(ORIGINS).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        for force in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
            ctx.resize_force(force)
            o = _Out(torch, item, OW * OH * c)
            MC.compose(full, base=GUARD, frame_stride=o.fs, out=o.want)
            ctx.resize_device(d, strided.data_ptr() + 3 * item, o.ptr, FRAMES, in_frame_stride=in_fs, out_frame_stride=o.fs * item,
                              stream=s)
            o.check(torch, f"strided batch {FORCE_NAMES[force]}", f32)
            _reports(ctx, "strided batch")
        ctx.resize_force(L.RESIZE_FUSED)
        o = _Out(torch, item, OW * OH * c)
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(d, tight.data_ptr(), o.ptr, FRAMES, out_frame_stride=o.fs * item, stream=s)
        assert e.value.code == L.ERR_UNSUPPORTED
        o.check(torch, "the refused call wrote nothing", f32)
        ctx.resize_force(L.RESIZE_AUTO)
        # a sub-window
        o = _Out(torch, item, WINDOW[2] * WINDOW[3] * c)
        MC.compose(full, window=WINDOW, base=GUARD, frame_stride=o.fs, out=o.want)
        ctx.resize_device(d, tight.data_ptr(), o.ptr, FRAMES, out_frame_stride=o.fs * item, stream=s, window=WINDOW)
        o.check(torch, "window", f32)
        _reports(ctx, "window")
        # pitched rows (every kind) and planes (8-bit, more than one channel): noise in every byte the layout does not name
        sources = [("pitched", SM.build(x, "interleaved", (IW * c + 7) * item, base=(3 * item) % 4,
                                         frame_stride=IH * (IW * c + 7) * item + item, seed=3))]
        if u8 and c > 1:
            sources.append(("planar", SM.build(x, "planar", IW + 4, IH * (IW + 4) + 1, base=1, frame_stride=c * (IH * (IW + 4) + 1) + 1,
                                               seed=4)))
        for name, src in sources:
            buf = torch.from_numpy(src.buf).cuda()
            rs = L.resize_source(d, "planar" if name == "planar" else "interleaved", src.row_stride,
                                 src.chan_stride if name == "planar" else None)
            for window in (None, WINDOW):
                w, h = (OW, OH) if window is None else WINDOW[2:]
                o = _Out(torch, item, w * h * c)
                MC.compose(full, window=window, base=GUARD, frame_stride=o.fs, out=o.want)
                ctx.resize_device(d, buf.data_ptr() + src.at, o.ptr, FRAMES, in_frame_stride=src.frame_stride,
                                  out_frame_stride=o.fs * item, stream=s, window=window, source=rs)
                o.check(torch, f"{name} source, window {window}", f32)
                _reports(ctx, name, source=L.SOURCE_PACKED)
        if u8:
            ident = tuple(range(c))
            cmap = MC.channel_map(c)
            # (what, element bytes, layout, window, crop, channel map, uniform flip, per-frame flips)
            tensors = [("f32 chw", 4, "chw", None, None, ident, 0, None), ("f32 hwc", 4, "hwc", None, None, ident, 0, None),
                       ("bf16 chw", 2, "chw", None, None, ident, 0, None), ("bf16 hwc", 2, "hwc", WINDOW, None, ident, 0, None),
                       ("f32 view", 4, "chw", None, None, cmap, 3, (0, 1, 2)), ("bf16 view", 2, "hwc", WINDOW, None, cmap, 3, (0, 1, 2)),
                       ("f32 crops", 4, "hwc", None, CROP, cmap, 2, (0, 1, 2)), ("bf16 crops", 2, "chw", None, CROP, ident, 0, (0, 1, 2))]
            for what, elem, layout, window, crop, cm, flip, per_frame in tensors:
                w, h = crop if crop else (OW, OH) if window is None else window[2:]
                st = V.strides(layout, w, h, len(cm))
                lut = T32.identity_lut(len(cm)) if elem == 4 else T16.identity_lut16(len(cm))
                dl = torch.from_numpy(V.words(lut).view(np.uint8).reshape(-1).copy()).cuda()
                o = _Out(torch, elem, V.extent(w, h, len(cm), st))
                fl = [flip ^ p for p in per_frame] if per_frame else [flip] * FRAMES
                MC.compose(full, window, crop, ORIGINS if crop else None, lut, cm, fl, st, GUARD, o.fs, o.want)
                kw = dict(out_frame_stride=o.fs * elem, stream=s, dtype="float32" if elem == 4 else "bfloat16")
                if cm != ident or flip or per_frame:
                    kw.update(channels_out=cm, flip=flip, d_flip=flips.data_ptr() if per_frame else None)
                if crop:
                    kw.update(crop=crop, d_origin=origins.data_ptr())
                else:
                    kw.update(window=window)
                ctx.resize_tensor_device(d, tight.data_ptr(), o.ptr, FRAMES, dl.data_ptr(), st, **kw)
                o.check(torch, what)
                _reports(ctx, what, tensor=L.TENSOR_CONVERTED)
        if u8 and not alpha:
            # reducing_gap: 30 x 640 -> 3 x 333 is not tall, reduced by (10, 1) to 3 x 640 it is; 5 x 640 -> 12 x 77 is tall,
            # reduced by (1, 4) to 5 x 160 it is not and runs the fused kernel
            for (iw, ih, ow, oh, gap), factors, kernel in (((30, 640, 3, 333, 1.0), (10, 1), L.KERNEL_RESIZE_TWO_PASS),
                                                           ((IW, IH, OW, OH, 2.0), (1, 4), L.KERNEL_RESIZE_FUSED)):
                assert FM.gap_plan(FM.LANCZOS, iw, ih, ow, oh, None, gap)[:2] == factors
                xg = _frames(kind, iw, ih)
                o = _Out(torch, 1, ow * oh * c)
                MC.compose(_full(kind, iw, ih, ow, oh, None, gap), base=GUARD, frame_stride=o.fs, out=o.want)
                dev = torch.from_numpy(xg.reshape(-1).copy()).cuda()
                ctx.resize_device(_desc(kind, iw, ih, ow, oh), dev.data_ptr(), o.ptr, FRAMES, out_frame_stride=o.fs, stream=s,
                                  reducing_gap=gap)
                o.check(torch, f"gap {gap} on {iw}x{ih}")
                assert ctx.last_kernel() == kernel, (iw, ih, gap, ctx.last_kernel())
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["u8x3", "rgba", "f32x3"])
def test_first_use_inside_a_captured_graph(kind):
    """a context that has not seen the shape captures the request (tables built and scratch grown under capture), the graph is
    replayed twice with other contents, and the same context then runs it eagerly, with a larger batch, while the graph lives"""
    import torch
    c, dtype, alpha = KINDS[kind]
    item = np.dtype(dtype).itemsize
    f32 = dtype == np.float32
    x, full = _frames(kind), _full(kind)
    x2 = np.ascontiguousarray(x[::-1])
    ctx = L.Context(0)
    try:
        d = _desc(kind)
        dev = torch.from_numpy(x.reshape(-1).view(np.uint8).copy()).cuda()
        o = _Out(torch, item, OW * OH * c)
        MC.compose(full, base=GUARD, frame_stride=o.fs, out=o.want)
        g = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="relaxed"):
            ctx.resize_device(d, dev.data_ptr(), o.ptr, FRAMES, out_frame_stride=o.fs * item,
                              stream=torch.cuda.current_stream().cuda_stream)
        _reports(ctx, "capture")
        torch.cuda.synchronize()
        assert bool((o.dev == SENT).all())                      # captured, not run
        g.replay()
        o.check(torch, "first replay", f32)
        dev.copy_(torch.from_numpy(x2.reshape(-1).view(np.uint8).copy()))
        o.dev.fill_(SENT)
        MC.compose(np.ascontiguousarray(full[::-1]), base=GUARD, frame_stride=o.fs, out=o.want)
        g.replay()
        o.check(torch, "replay after the frames changed", f32)
        # eager on the same context: twice the frames, so the scratch of the capture is replaced while the graph may name it
        both = torch.from_numpy(np.concatenate([x, x2]).reshape(-1).view(np.uint8).copy()).cuda()
        out = torch.full((2 * FRAMES * OW * OH * c * item,), SENT, dtype=torch.uint8, device="cuda")
        ctx.resize_device(d, both.data_ptr(), out.data_ptr(), 2 * FRAMES)
        torch.cuda.synchronize()
        want = np.concatenate([full, full[::-1]])
        assert FM.same(out.cpu().numpy().view(dtype).reshape(want.shape), want)
        _reports(ctx, "eager")
        o.dev.fill_(SENT)
        g.replay()
        o.check(torch, "replay after the eager call", f32)
    finally:
        ctx.close()


# ---- the widest frame the rule reaches ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_w", [655, 656])
def test_the_size_edge_of_the_contract(ctx, in_w):
    """655 x 65535 -> 300 x 1000, one 8-bit channel, is the widest tall frame (65535 > 100 * 655): 395 vertical taps first, over
    all 655 columns.  656 x 65535 is its twin on the other side and runs horizontal first.  Both are compared with the model
    over every column of 72 output rows -- the first and last eight, the rest spread evenly -- through resize_window_model,
    which applies the whole-frame models' passes in the order of resize_model.pass_order (the whole 1000 rows take the model
    several seconds); and the two halves of the output, computed as windows, must be the halves of the whole."""
    in_h, ow, oh = 65535, 300, 1000
    assert M.pillow_vertical_first(in_w, in_h, oh) == (in_w == 655)
    img = np.random.default_rng(in_w).integers(0, 256, (in_h, in_w, 1), dtype=np.uint8)
    d = L.resize_desc(in_w, in_h, ow, oh, 1)
    assert L.resize_plan_host(d, 1).fused == 0
    f, cnt, k = L.resize_taps_host(d, 1)
    assert k.shape[1] == 395 and cnt.max() >= 393
    got = ctx.resize(img, ow, oh)
    assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS
    rows = np.unique(np.concatenate([np.arange(8), np.arange(oh - 8, oh), np.linspace(8, oh - 9, 56).astype(np.int64)]))
    assert len(rows) == 72
    want = W.resize(lambda y0, y1, x0, x1: img[y0:y1, x0:x1], in_w, in_h, ow, oh, 1, np.uint8, rows, np.arange(ow))
    bad = got[rows] != want
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} samples differ, the first at {tuple(np.argwhere(bad)[0])}"
    top = ctx.resize(img, ow, oh, window=(0, 0, ow, 499))
    bottom = ctx.resize(img, ow, oh, window=(0, 499, ow, 501))
    assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS
    assert np.array_equal(np.concatenate([top, bottom]), got)
