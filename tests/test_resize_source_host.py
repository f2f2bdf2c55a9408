"""Host-side checks of a source layout (lanczos_resize_source, lanczos_resize_source_init / _validate; include/lanczos_hip.h):
the struct, the tight layouts, every refusal of the validator, and the numpy model of the layouts.  No GPU.  (The frame stride
is an argument of the entries, not of the validator: its refusal needs a context and is in tests/test_resize_source_gpu.py.)"""
import ctypes

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_source_model as SM

W, H = 21, 13


def _code(desc, src):
    return L._lib().lanczos_resize_source_validate(ctypes.byref(desc), ctypes.byref(src) if src is not None else None)


def _src(rs, cs, ps, reserved=(0, 0, 0)):
    s = L.ResizeSource()
    s.row_stride, s.chan_stride, s.pix_stride = rs, cs, ps
    for i, r in enumerate(reserved):
        s.reserved[i] = r
    return s


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.ResizeSource) == 8 + 8 + 4 + 3 * 4
    S = L.ResizeSource
    assert (S.row_stride.offset, S.chan_stride.offset, S.pix_stride.offset, S.reserved.offset) == (0, 8, 16, 20)
    assert (L.SOURCE_INTERLEAVED, L.SOURCE_PLANAR, L.SOURCE_DIRECT, L.SOURCE_PACKED) == (0, 1, 1, 2)
    for name in ("lanczos_resize_source_init", "lanczos_resize_source_validate", "lanczos_resize_source_device",
                 "lanczos_resize_tensor_source_device", "lanczos_resize_source_host", "lanczos_resize_tensor_source_host",
                 "lanczos_last_source_route"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name), name
    assert L._lib().lanczos_last_source_route(None) == 0


@pytest.mark.parametrize("c", [1, 3, 4])
def test_init_is_the_tight_layout(c):
    for kw, b in (({}, 1), ({"bits": 16}, 2), ({"f32": True}, 4)):
        d = L.resize_desc(W, H, 9, 7, c, **kw)
        s = L.resize_source(d, "interleaved")
        assert (s.row_stride, s.chan_stride, s.pix_stride) == (W * c * b, b, c * b) and not any(s.reserved)
        assert _code(d, s) == L.OK
        assert SM.strides((1, H, W, c), b, "interleaved")[:3] == (s.row_stride, s.chan_stride, s.pix_stride)
        p = L.ResizeSource()
        rc = L._lib().lanczos_resize_source_init(ctypes.byref(p), ctypes.byref(d), L.SOURCE_PLANAR)
        if b == 1:
            assert rc == L.OK and (p.row_stride, p.chan_stride, p.pix_stride) == (W, W * H, 1) and _code(d, p) == L.OK
            assert SM.strides((1, H, W, c), 1, "planar")[:3] == (W, W * H, 1)
        else:   # planar wide samples: frames * C one-channel frames for the plain entries
            assert rc == L.ERR_UNSUPPORTED
    d = L.resize_desc(W, H, 9, 7, 3)
    s = L.ResizeSource()
    assert L._lib().lanczos_resize_source_init(ctypes.byref(s), ctypes.byref(d), 2) == L.ERR_BAD_ARG
    assert L._lib().lanczos_resize_source_init(None, ctypes.byref(d), 0) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert L._lib().lanczos_resize_source_init(ctypes.byref(s), ctypes.byref(bad), 0) == L.ERR_BAD_ARG
    assert _code(bad, None) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.resize_source(d, "chw")


def test_null_and_tight_validate_like_the_call_without_a_source():
    for c, kw in ((1, {}), (3, {}), (4, {"alpha": True}), (3, {"bits": 16}), (4, {"f32": True})):
        d = L.resize_desc(W, H, 9, 7, c, **kw)
        assert _code(d, None) == L._lib().lanczos_resize_validate(ctypes.byref(d)) == L.OK
        assert _code(d, L.resize_source(d, "interleaved")) == L.OK
        # (the plan queries take no source: a layout changes where bytes are fetched from and nothing of the launch shape, so there
        # is no second plan to compare on the host.  That a tight source runs the plan's kernel with the same bytes is checked on the
        # device, tests/test_resize_source_gpu.py::test_device_argument_checks)


def test_refusals_interleaved():
    for c, kw, b in ((3, {}, 1), (4, {"alpha": True}, 1), (1, {}, 1), (3, {"bits": 16}, 2), (3, {"f32": True}, 4)):
        d = L.resize_desc(W, H, 9, 7, c, **kw)
        tight = W * c * b
        assert _code(d, _src(tight, b, c * b)) == L.OK
        assert _code(d, _src(tight + 5 * b, b, c * b)) == L.OK                      # pitched
        assert _code(d, _src(tight - b, b, c * b)) == L.ERR_BAD_ARG                  # a row short by one sample
        assert _code(d, _src(tight - 1, b, c * b)) == L.ERR_BAD_ARG
        if b > 1:
            assert _code(d, _src(tight + 1, b, c * b)) == L.ERR_BAD_ARG              # off the sample size
            assert _code(d, _src(tight + b + 1, b, c * b)) == L.ERR_BAD_ARG
        if b == 4:
            assert _code(d, _src(tight + 2, b, c * b)) == L.ERR_BAD_ARG              # float strides off 4
        for i in range(3):
            r = [0, 0, 0]
            r[i] = 1
            assert _code(d, _src(tight, b, c * b, r)) == L.ERR_BAD_ARG, i
        for rs, cs, ps in ((0, b, c * b), (-tight, b, c * b), (tight, 0, c * b), (tight, b, 0), (tight, b, -c * b),
                           (tight, -b, c * b)):
            assert _code(d, _src(rs, cs, ps)) == L.ERR_BAD_ARG, (rs, cs, ps)
        if c > 1:   # mixed shapes: an interleaved pixel stride with planes, a planar one with interleaved channels
            assert _code(d, _src(tight, W * H * b, c * b)) == L.ERR_BAD_ARG
            assert _code(d, _src(W * b, b, b)) == L.ERR_BAD_ARG
            assert _code(d, _src(tight, b, (c + 1) * b)) == L.ERR_BAD_ARG
            assert _code(d, _src(tight, 2 * b, c * b)) == L.ERR_BAD_ARG


def test_refusals_planar():
    for c, kw in ((3, {}), (4, {}), (4, {"alpha": True})):
        d = L.resize_desc(W, H, 9, 7, c, **kw)
        assert _code(d, _src(W, W * H, 1)) == L.OK
        assert _code(d, _src(W + 3, (H - 1) * (W + 3) + W, 1)) == L.OK             # the last row of a plane needs no padding
        assert _code(d, _src(W + 3, (H - 1) * (W + 3) + W - 1, 1)) == L.ERR_BAD_ARG  # planes overlapping by one byte
        assert _code(d, _src(W, W * H - 1, 1)) == L.ERR_BAD_ARG
        assert _code(d, _src(W - 1, W * H, 1)) == L.ERR_BAD_ARG                      # a row short by one
        assert _code(d, _src(W + 1, (W + 1) * H + 7, 1)) == L.OK                     # no alignment asked of either stride
        for i in range(3):
            r = [0, 0, 0]
            r[i] = -1
            assert _code(d, _src(W, W * H, 1, r)) == L.ERR_BAD_ARG, i
        assert _code(d, _src(W, W * H, 2)) == L.ERR_BAD_ARG
        assert _code(d, _src(W, -W * H, 1)) == L.ERR_BAD_ARG                         # no negative strides
    # planar wide samples
    for kw, b in (({"bits": 16}, 2), ({"f32": True}, 4)):
        d = L.resize_desc(W, H, 9, 7, 3, **kw)
        assert _code(d, _src(W * b, W * H * b, b)) == L.ERR_UNSUPPORTED
        assert _code(d, _src(W * b, W * H * b - b, b)) == L.ERR_BAD_ARG              # ... a well-formed one only
        d1 = L.resize_desc(W, H, 9, 7, 1, **kw)                                       # one plane is the interleaved shape
        assert _code(d1, _src(W * b, W * H * b, b)) == L.OK
    d1 = L.resize_desc(W, H, 9, 7, 1)
    assert _code(d1, _src(W + 2, 12345, 1)) == L.OK and _code(d1, _src(W + 2, 1, 1)) == L.OK
    assert _code(d1, _src(W - 1, 1, 1)) == L.ERR_BAD_ARG


def test_python_helpers():
    d = L.resize_desc(W, H, 9, 7, 3)
    s = L.resize_source(d, "planar", row_stride=W + 5)
    assert (s.row_stride, s.chan_stride, s.pix_stride) == (W + 5, (W + 5) * H, 1)
    s = L.resize_source(d, "planar", row_stride=W + 5, chan_stride=1000)
    assert (s.row_stride, s.chan_stride) == (W + 5, 1000)
    s = L.resize_source(d, "interleaved", row_stride=256)
    assert (s.row_stride, s.chan_stride, s.pix_stride) == (256, 1, 3)
    assert L.resize_source(d, s) is s
    L.resize_source_validate(d, s)
    L.resize_source_validate(d, None)
    s.row_stride = 3 * W - 1
    with pytest.raises(L.LanczosError) as e:
        L.resize_source_validate(d, s)
    assert e.value.code == L.ERR_BAD_ARG


@pytest.mark.parametrize("layout", ["planar", "interleaved"])
def test_model_round_trip_and_noise(layout):
    """build() names every sample once, fills everything else with non-zero noise that depends on fill_seed alone, and unpack()
    is its inverse -- for every residue of base and odd strides"""
    rng = np.random.default_rng(5)
    for dtype in (np.uint8,) if layout == "planar" else (np.uint8, np.uint16, np.float32):
        b = np.dtype(dtype).itemsize
        x = rng.integers(0, 256, (3, 7, 11, 3 * b), dtype=np.uint8).view(dtype)
        assert x.shape == (3, 7, 11, 3)
        for base in range(0, 4, b):
            rs = 11 * b + 3 * b if layout == "planar" else 11 * 3 * b + 5 * b
            cs = 7 * rs + 2 * b if layout == "planar" else None
            ext = SM.strides(x.shape, b, layout, rs, cs)[3]
            s = SM.build(x, layout, rs, cs, base=base, frame_stride=ext + 3 * b, seed=2)
            assert s.at % 4 == base and s.extent == ext
            assert np.array_equal(SM.unpack(s, x.shape, dtype).view(np.uint8), x.view(np.uint8))
            m = SM.named_mask(s, x.shape, b)
            assert m.sum() == x.size * b and not m[:s.at].any() and not m[s.at + 2 * s.frame_stride + ext:].any()
            assert (s.buf[~m] != 0).all()
            t = SM.build(x, layout, rs, cs, base=base, frame_stride=ext + 3 * b, seed=2, fill_seed=99)
            assert np.array_equal(t.buf[m], s.buf[m]) and (t.buf[~m] != s.buf[~m]).mean() > 0.9
