"""Host-side checks of a destination layout (lanczos_resize_dest, lanczos_resize_dest_init / _validate; include/lanczos_hip.h):
the struct, the tight layouts with and without a window, every refusal of the validator, and the numpy model of the layouts.  No
GPU.  (The frame stride is an argument of the entries, not of the validator: its refusal needs a context and is in
tests/test_resize_dest_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_dest_model as DM
import resize_source_model as SM

IW, IH, W, H = 30, 19, 21, 13     # the output is W x H
WIN = (3, 2, 11, 7)               # a window of it


def _code(desc, dst, win=None):
    return L._lib().lanczos_resize_dest_validate(ctypes.byref(desc), ctypes.byref(L.resize_window(desc, win)) if win else None,
                                                 ctypes.byref(dst) if dst is not None else None)


def _dst(rs, cs, ps, reserved=(0, 0, 0)):
    t = L.ResizeDest()
    t.row_stride, t.chan_stride, t.pix_stride = rs, cs, ps
    for i, r in enumerate(reserved):
        t.reserved[i] = r
    return t


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.ResizeDest) == 8 + 8 + 4 + 3 * 4
    S = L.ResizeDest
    assert (S.row_stride.offset, S.chan_stride.offset, S.pix_stride.offset, S.reserved.offset) == (0, 8, 16, 20)
    assert (L.DEST_INTERLEAVED, L.DEST_PLANAR, L.DEST_DIRECT, L.DEST_UNPACKED) == (0, 1, 1, 2)
    names = ("lanczos_resize_dest_init", "lanczos_resize_dest_validate", "lanczos_resize_dest_device", "lanczos_resize_dest_host",
             "lanczos_last_dest_route")
    for name in names:
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name), name
        assert "tensor" not in name
    assert L._lib().lanczos_last_dest_route(None) == 0


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("win", [None, WIN])
def test_init_is_the_tight_layout(c, win):
    w, h = (W, H) if win is None else win[2:]
    for kw, b in (({}, 1), ({"bits": 16}, 2), ({"f32": True}, 4)):
        d = L.resize_desc(IW, IH, W, H, c, **kw)
        t = L.resize_dest(d, "interleaved", window=win)
        assert (t.row_stride, t.chan_stride, t.pix_stride) == (w * c * b, b, c * b) and not any(t.reserved)
        assert _code(d, t, win) == L.OK
        assert DM.strides((1, h, w, c), b, "interleaved")[:3] == (t.row_stride, t.chan_stride, t.pix_stride)
        p = L.ResizeDest()
        wref = ctypes.byref(L.resize_window(d, win)) if win else None
        rc = L._lib().lanczos_resize_dest_init(ctypes.byref(p), ctypes.byref(d), wref, L.DEST_PLANAR)
        if b == 1:
            assert rc == L.OK and (p.row_stride, p.chan_stride, p.pix_stride) == (w, w * h, 1) and _code(d, p, win) == L.OK
            assert DM.strides((1, h, w, c), 1, "planar")[:3] == (w, w * h, 1)
        else:   # planar wide samples: frames * C one-channel frames for the plain entries
            assert rc == L.ERR_UNSUPPORTED
    d = L.resize_desc(IW, IH, W, H, 3)
    t = L.ResizeDest()
    assert L._lib().lanczos_resize_dest_init(ctypes.byref(t), ctypes.byref(d), None, 2) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_dest_init(None, ctypes.byref(d), None, 0) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert L._lib().lanczos_resize_dest_init(ctypes.byref(t), ctypes.byref(bad), None, 0) == L.ERR_BAD_ARG
    assert _code(bad, None) == L.ERR_BAD_ARG
    bw = L.ResizeWindow()
    bw.x0, bw.y0, bw.w, bw.h = 0, 0, W + 1, H
    assert L._lib().lanczos_resize_dest_init(ctypes.byref(t), ctypes.byref(d), ctypes.byref(bw), 0) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_dest_validate(ctypes.byref(d), ctypes.byref(bw), None) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.resize_dest(d, "chw")


def test_null_and_tight_validate_like_the_call_without_a_destination():
    for c, kw in ((1, {}), (3, {}), (4, {"alpha": True}), (3, {"bits": 16}), (4, {"f32": True})):
        d = L.resize_desc(IW, IH, W, H, c, **kw)
        assert _code(d, None) == L._lib().lanczos_resize_validate(ctypes.byref(d)) == L.OK
        assert _code(d, L.resize_dest(d, "interleaved")) == L.OK
        assert _code(d, None, WIN) == L.OK and _code(d, L.resize_dest(d, "interleaved", window=WIN), WIN) == L.OK


@pytest.mark.parametrize("win", [None, WIN])
def test_refusals_interleaved(win):
    w, h = (W, H) if win is None else win[2:]
    for c, kw, b in ((3, {}, 1), (4, {"alpha": True}, 1), (1, {}, 1), (3, {"bits": 16}, 2), (3, {"f32": True}, 4)):
        d = L.resize_desc(IW, IH, W, H, c, **kw)
        tight = w * c * b
        assert _code(d, _dst(tight, b, c * b), win) == L.OK
        assert _code(d, _dst(tight + 5 * b, b, c * b), win) == L.OK                      # pitched
        assert _code(d, _dst(tight - b, b, c * b), win) == L.ERR_BAD_ARG                  # a row short by one sample
        assert _code(d, _dst(tight - 1, b, c * b), win) == L.ERR_BAD_ARG
        if b > 1:
            assert _code(d, _dst(tight + 1, b, c * b), win) == L.ERR_BAD_ARG              # off the sample size
            assert _code(d, _dst(tight + b + 1, b, c * b), win) == L.ERR_BAD_ARG
        if b == 4:
            assert _code(d, _dst(tight + 2, b, c * b), win) == L.ERR_BAD_ARG              # float strides off 4
        for i in range(3):
            r = [0, 0, 0]
            r[i] = 1
            assert _code(d, _dst(tight, b, c * b, r), win) == L.ERR_BAD_ARG, i
        for rs, cs, ps in ((0, b, c * b), (-tight, b, c * b), (tight, 0, c * b), (tight, b, 0), (tight, b, -c * b),
                           (tight, -b, c * b)):
            assert _code(d, _dst(rs, cs, ps), win) == L.ERR_BAD_ARG, (rs, cs, ps)
        if c > 1:   # mixed shapes: an interleaved pixel stride with planes, a planar one with interleaved channels
            assert _code(d, _dst(tight, w * h * b, c * b), win) == L.ERR_BAD_ARG
            assert _code(d, _dst(w * b, b, b), win) == L.ERR_BAD_ARG
            assert _code(d, _dst(tight, b, (c + 1) * b), win) == L.ERR_BAD_ARG
            assert _code(d, _dst(tight, 2 * b, c * b), win) == L.ERR_BAD_ARG
    if win is not None:   # the window's extent counts, not the output's: the output's tight row is a pitched row of the window
        d = L.resize_desc(IW, IH, W, H, 3)
        assert _code(d, _dst(W * 3, 1, 3), win) == L.OK and _code(d, _dst(w * 3, 1, 3), None) == L.ERR_BAD_ARG


@pytest.mark.parametrize("win", [None, WIN])
def test_refusals_planar(win):
    w, h = (W, H) if win is None else win[2:]
    for c, kw in ((3, {}), (4, {}), (4, {"alpha": True})):
        d = L.resize_desc(IW, IH, W, H, c, **kw)
        assert _code(d, _dst(w, w * h, 1), win) == L.OK
        assert _code(d, _dst(w + 3, (h - 1) * (w + 3) + w, 1), win) == L.OK              # the last row of a plane needs no padding
        assert _code(d, _dst(w + 3, (h - 1) * (w + 3) + w - 1, 1), win) == L.ERR_BAD_ARG  # planes overlapping by one byte
        assert _code(d, _dst(w, w * h - 1, 1), win) == L.ERR_BAD_ARG
        assert _code(d, _dst(w - 1, w * h, 1), win) == L.ERR_BAD_ARG                      # a row short by one
        assert _code(d, _dst(w + 1, (w + 1) * h + 7, 1), win) == L.OK                     # no alignment asked of either stride
        for i in range(3):
            r = [0, 0, 0]
            r[i] = -1
            assert _code(d, _dst(w, w * h, 1, r), win) == L.ERR_BAD_ARG, i
        assert _code(d, _dst(w, w * h, 2), win) == L.ERR_BAD_ARG
        assert _code(d, _dst(w, -w * h, 1), win) == L.ERR_BAD_ARG                         # no negative strides
    # planar wide samples
    for kw, b in (({"bits": 16}, 2), ({"f32": True}, 4)):
        d = L.resize_desc(IW, IH, W, H, 3, **kw)
        assert _code(d, _dst(w * b, w * h * b, b), win) == L.ERR_UNSUPPORTED
        assert _code(d, _dst(w * b, w * h * b - b, b), win) == L.ERR_BAD_ARG              # ... a well-formed one only
        d1 = L.resize_desc(IW, IH, W, H, 1, **kw)                                          # one plane is the interleaved shape
        assert _code(d1, _dst(w * b, w * h * b, b), win) == L.OK
    d1 = L.resize_desc(IW, IH, W, H, 1)
    assert _code(d1, _dst(w + 2, 12345, 1), win) == L.OK and _code(d1, _dst(w + 2, 1, 1), win) == L.OK
    assert _code(d1, _dst(w - 1, 1, 1), win) == L.ERR_BAD_ARG


def test_python_helpers():
    d = L.resize_desc(IW, IH, W, H, 3)
    t = L.resize_dest(d, "planar", row_stride=W + 5)
    assert (t.row_stride, t.chan_stride, t.pix_stride) == (W + 5, (W + 5) * H, 1)
    t = L.resize_dest(d, "planar", row_stride=WIN[2] + 5, window=WIN)
    assert (t.row_stride, t.chan_stride, t.pix_stride) == (WIN[2] + 5, (WIN[2] + 5) * WIN[3], 1)
    L.resize_dest_validate(d, t, window=WIN)
    t = L.resize_dest(d, "planar", row_stride=W + 5, chan_stride=1000)
    assert (t.row_stride, t.chan_stride) == (W + 5, 1000)
    t = L.resize_dest(d, "interleaved", row_stride=256)
    assert (t.row_stride, t.chan_stride, t.pix_stride) == (256, 1, 3)
    assert L.resize_dest(d, t) is t
    L.resize_dest_validate(d, t)
    L.resize_dest_validate(d, None)
    t.row_stride = 3 * W - 1
    with pytest.raises(L.LanczosError) as e:
        L.resize_dest_validate(d, t)
    assert e.value.code == L.ERR_BAD_ARG


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_model_noise_mask_and_round_trip(layout):
    """build() fills the whole buffer with non-zero noise and ends it behind the last named byte; pack() / unpack() are inverse
    and touch named bytes only; and a destination read back as a source (tests/resize_source_model.py) gives the frames"""
    rng = np.random.default_rng(5)
    for dtype in (np.uint8,) if layout == "planar" else (np.uint8, np.uint16, np.float32):
        b = np.dtype(dtype).itemsize
        x = rng.integers(0, 256, (3, 7, 11, 3 * b), dtype=np.uint8).view(dtype)
        assert x.shape == (3, 7, 11, 3)
        for base in range(0, 4, b):
            rs = 11 * b + 3 * b if layout == "planar" else 11 * 3 * b + 5 * b
            cs = 7 * rs + 2 * b if layout == "planar" else None
            _, _, _, ext, named = DM.strides(x.shape, b, layout, rs, cs)
            assert named < ext                                                    # the last row's padding is not named
            for fs in (ext + 3 * b, named):                                       # frames apart, and as close as they may lie
                t = DM.build(x.shape, layout, rs, cs, base=base, frame_stride=fs, seed=2, itemsize=b)
                assert t.at % 4 == base and t.extent == ext and (t.buf != 0).all()
                assert t.buf.size == t.at + 2 * fs + named + DM.MARGIN
                m = DM.named_mask(t, x.shape, b)
                assert m.sum() == x.size * b and not m[:t.at].any() and not m[t.at + 2 * fs + named:].any() and m[t.at]
                assert m[t.at + 2 * fs + named - 1]
                after = DM.pack(t, x)
                assert np.array_equal(after[~m], t.buf[~m])
                assert np.array_equal(DM.unpack(t, x.shape, dtype, after).view(np.uint8), x.view(np.uint8))
                s = DM.as_source(t)._replace(buf=after)
                assert np.array_equal(SM.unpack(s, x.shape, dtype).view(np.uint8), x.view(np.uint8))
                assert np.array_equal(SM.named_mask(s, x.shape, b), m)
            # ... and the other way round: what the source model lays out, the destination model reads
            s = SM.build(x, layout, rs, cs, base=base, frame_stride=ext + 3 * b, seed=3)
            t = DM.Dest(s.buf, s.at, layout, s.row_stride, s.chan_stride, s.pix_stride, s.frame_stride, s.extent, named)
            assert np.array_equal(DM.unpack(t, x.shape, dtype).view(np.uint8), x.view(np.uint8))
