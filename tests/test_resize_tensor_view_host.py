"""Host-side checks of the tensor view (lanczos_tensor_view, lanczos_resize_tensor_view_*, include/lanczos_hip.h): the numpy
model of its contract against torch's own indexing and flips on the CPU, every refusal of lanczos_resize_tensor_view_validate,
and the identity view against the validators of the entries without a map.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_tensor_view_model as V

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
W, H = 7, 5


def _wref(window):
    """a window built by hand, so that one the validators refuse gets to them"""
    if window is None:
        return None
    w = L.ResizeWindow()
    w.x0, w.y0, w.w, w.h = window
    return ctypes.byref(w)


def _code(desc, v, window=None):
    return L._lib().lanczos_resize_tensor_view_validate(ctypes.byref(desc), _wref(window),
                                                        ctypes.byref(v) if v is not None else None)


def _v(strides, src, elem=4, lut=1, flip=0, d_flip=None):
    return L.tensor_view(lut, strides, elem, src, flip, d_flip)


def _torch_want(bytes_fhwc, src, flips, mean, std, dtype):
    """torch's own pipeline on the CPU: index the channels, flip per frame, normalise, cast -- as bit patterns [F][OC][h][w]"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(bytes_fhwc)).permute(0, 3, 1, 2)[:, list(src)]
    x = torch.stack([fr.flip([d for d, bit in ((-1, 1), (-2, 2)) if m & bit]) if m & 3 else fr for fr, m in zip(x, flips)])
    x = x.float().div(255).sub(torch.tensor(mean, dtype=torch.float32)[:, None, None])
    x = x.div(torch.tensor(std, dtype=torch.float32)[:, None, None]).contiguous()
    if dtype == "float32":
        return x.view(torch.int32).numpy().view(np.uint32)
    return x.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_the_model_is_torchs_indexing(dtype):
    """channel selection, per-frame .flip(-1) / .flip(-2) and the normalise arithmetic, with mean / std in OUTPUT order"""
    cases = [(3, (2, 1, 0)), (3, (2, 0)), (3, (0, 1, 2)), (4, (0, 1, 2)), (4, (3, 0, 1, 2)), (4, (2, 1, 0)), (1, (0,))]
    for c, src in cases:
        b = np.stack([P.noise(H, W, c, seed=11 * k + c) for k in range(5)])
        flips = [0, 1, 2, 3, 1]
        oc = len(src)
        mean, std = MEAN[:oc], STD[:oc]
        lut = L.normalize_lut(3 if oc == 2 else oc, mean + (0,) * (oc == 2), std + (1,) * (oc == 2), dtype=dtype)[:oc]
        got = V.view(b, lut, src, flips)
        want = _torch_want(b, src, flips, mean, std, dtype)
        assert got.dtype == want.dtype and np.array_equal(got, want), (c, src, dtype)
        # HWC is the permutation of CHW, and an int flips every frame
        assert np.array_equal(V.view(b, lut, src, flips, "hwc"), want.transpose(0, 2, 3, 1))
        assert np.array_equal(V.view(b, lut, src, 1), _torch_want(b, src, [1] * 5, mean, std, dtype))
        # bits 2..7 of a flip byte are ignored
        assert np.array_equal(V.view(b, lut, src, [0xFC, 0x05, 0x82, 0x7F, 0x41]), want)


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.TensorView) == 8 + 3 * 8 + 4 + 4 + 4 * 4 + 4 + 4 + 8 + 4 * 4    # 4 bytes of padding before d_flip
    assert L.TensorView.d_flip.offset == 64 and L.TensorView.reserved.offset == 72
    assert (L.FLIP_H, L.FLIP_V) == (1, 2)
    for name in ("lanczos_tensor_view_init", "lanczos_resize_tensor_view_validate", "lanczos_resize_tensor_view_device",
                 "lanczos_resize_tensor_view_host"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name)


def test_view_init():
    d = L.resize_desc(20, 20, W, H, 3)
    for elem in (2, 4):
        v = L.tensor_view_init(d, elem)
        assert (v.chan_stride, v.row_stride, v.pix_stride) == (H * W, W, 1)
        assert (v.elem_bytes, v.out_channels, list(v.src_channel), v.flip, v.d_flip, v.d_lut) == (elem, 3, [0, 1, 2, 0], 0, None, None)
        assert list(v.reserved) == [0] * 4
        assert _code(d, v) == L.ERR_BAD_ARG              # no table yet
        v.d_lut = 1
        assert _code(d, v) == L.OK
    lib = L._lib()
    v = L.TensorView()
    for elem in (0, 1, 3, 8):
        assert lib.lanczos_tensor_view_init(ctypes.byref(v), ctypes.byref(d), elem) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_view_init(None, ctypes.byref(d), 4) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert lib.lanczos_tensor_view_init(ctypes.byref(v), ctypes.byref(bad), 4) == L.ERR_BAD_ARG
    assert L.tensor_view_init(L.resize_desc(20, 20, W, H, 4, alpha=True)).out_channels == 4


def test_validate_refusals():
    d = L.resize_desc(20, 20, W, H, 3)
    chw = L.tensor_strides("chw", W, H, 3)
    ident = (0, 1, 2)
    assert _code(d, _v(chw, ident)) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG                                         # a null struct
    assert _code(d, _v(chw, ident, lut=None)) == L.ERR_BAD_ARG                     # a null table
    for elem in (0, 1, 3, 8, -4):
        assert _code(d, _v(chw, ident, elem=elem)) == L.ERR_BAD_ARG, elem
    assert _code(d, _v(chw, ident, elem=2)) == L.OK
    for i in range(3):                                                             # everything the entries without a map refuse
        for bad in (0, -1, -chw[i], (1 << 40) + 1):
            st = list(chw)
            st[i] = bad
            assert _code(d, _v(st, ident)) == L.ERR_BAD_ARG, st
    assert _code(d, _v((1, 1, 1), ident)) == L.ERR_BAD_ARG
    assert _code(d, _v((H * W - 1, W, 1), ident)) == L.ERR_BAD_ARG
    for i in range(4):
        v = _v(chw, ident)
        v.reserved[i] = 1
        assert _code(d, v) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert _code(bad, _v(chw, (0, 1))) == L.ERR_BAD_ARG                            # what lanczos_resize_validate refuses
    assert _code(d, _v(chw, ident), window=(0, 0, W + 1, H)) == L.ERR_BAD_ARG      # a window outside the output
    # out_channels
    v = _v(chw, ident)
    for n in (0, -1, 4, 5):
        v.out_channels = n
        assert _code(d, v) == L.ERR_BAD_ARG, n
    d4 = L.resize_desc(20, 20, W, H, 4)
    assert _code(d4, _v(L.tensor_strides("chw", W, H, 4), (3, 0, 1, 2))) == L.OK
    assert _code(L.resize_desc(20, 20, W, H, 1), _v((1, W, 1), (0,))) == L.OK
    assert _code(L.resize_desc(20, 20, W, H, 1), _v((H * W, W, 1), (0, 0))) == L.ERR_BAD_ARG
    # src_channel: out of range, a duplicate, a non-zero one beyond out_channels
    for src in ((0, 1, 3), (0, 1, -1), (3, 1, 0), (0, 0, 1), (2, 1, 2), (1, 1), (2, 2)):
        assert _code(d, _v(chw, src)) == L.ERR_BAD_ARG, src
    assert _code(d4, _v(chw, (0, 1, 2))) == L.OK
    v = _v(chw, (0, 1, 2))
    v.src_channel[3] = 3
    assert _code(d4, v) == L.ERR_BAD_ARG                                           # a non-zero src_channel[3] with out_channels 3
    v = _v(chw, (2, 0))
    v.src_channel[2] = 1
    assert _code(d, v) == L.ERR_BAD_ARG
    # flip
    for flip in (0, 1, 2, 3):
        assert _code(d, _v(chw, ident, flip=flip)) == L.OK
    for flip in (4, 7, -1, 256):
        assert _code(d, _v(chw, ident, flip=flip)) == L.ERR_BAD_ARG, flip
    assert _code(d, _v(chw, (2, 1, 0), flip="hv", d_flip=1)) == L.OK               # a device pointer is not looked at
    # sample widths without a table
    assert _code(L.resize_desc(20, 20, W, H, 3, bits=16), _v(chw, ident)) == L.ERR_UNSUPPORTED
    assert _code(L.resize_desc(20, 20, W, H, 3, f32=True), _v(chw, ident)) == L.ERR_UNSUPPORTED
    assert _code(L.resize_desc(20, 20, W, H, 4, alpha=True), _v(chw, (0, 1, 2))) == L.OK
    with pytest.raises(L.LanczosError) as e:
        L.resize_tensor_view_validate(d, _v(chw, ident, flip=4))
    assert e.value.code == L.ERR_BAD_ARG
    L.resize_tensor_view_validate(d, _v(chw, (2, 1, 0), flip="h"))
    with pytest.raises(L.LanczosError):
        L.tensor_view(1, chw, 4, (0, 1, 2, 3, 0))


def test_the_overlap_rule_counts_the_output_channels():
    d = L.resize_desc(20, 20, W, H, 4)
    # CHW strides sized for `channels` are accepted with fewer out_channels, and so are those sized for out_channels
    for oc, src in ((4, (3, 2, 1, 0)), (3, (0, 1, 2)), (2, (3, 0)), (1, (2,))):
        assert _code(d, _v(L.tensor_strides("chw", W, H, 4), src)) == L.OK
        assert _code(d, _v(L.tensor_strides("chw", W, H, oc), src)) == L.OK
        # HWC with pix_stride = out_channels is accepted, out_channels - 1 is refused (one channel: its stride is free)
        assert _code(d, _v((1, W * oc, oc), src)) == L.OK, oc
        if oc > 1:
            assert _code(d, _v((1, W * oc, oc - 1), src)) == L.ERR_BAD_ARG, oc
            assert _code(d, _v((1, W * oc - 1, oc), src)) == L.ERR_BAD_ARG, oc
        # the model names every address once under the accepted strides, whatever the flips
        for st in (V.strides("chw", W, H, oc), V.strides("hwc", W, H, oc)):
            out = np.zeros(V.extent(W, H, oc, st), dtype=np.uint32)
            assert V.scatter(out, 0, np.zeros((4, H, W, 4), dtype=np.uint8), np.ones((oc, 256), dtype=np.float32), src,
                             [0, 1, 2, 3], st, 0) == 4 * out.size
            assert out.all()
    # HWC strides of the three kept channels under an RGBA source: four channels would overlap there
    hwc3 = (1, W * 3, 3)
    assert _code(d, _v(hwc3, (0, 1, 2))) == L.OK and _code(d, _v(hwc3, (0, 1, 2, 3))) == L.ERR_BAD_ARG


def test_an_identity_view_validates_where_the_window_entries_do():
    """over a small grid of strides and windows, both element widths"""
    lib = L._lib()
    c = 3
    d = L.resize_desc(20, 20, W, H, c)
    windows = [None, (0, 0, W, H), (1, 1, 4, 3), (2, 0, 5, 5), (0, 0, 1, 1), (3, 2, 5, 1), (0, 0, W + 1, H), (0, 0, 0, 1)]
    values = (0, 1, 3, 4, 5, 12, 15, 20, 35, 36)
    seen = set()
    for win in windows:
        wref = _wref(win)
        for st in itertools.product(values, repeat=3):
            t, t16 = L.tensor_out(1, st), L.tensor16_out(1, st)
            want = lib.lanczos_resize_tensor_window_validate(ctypes.byref(d), wref, ctypes.byref(t))
            assert lib.lanczos_resize_tensor16_window_validate(ctypes.byref(d), wref, ctypes.byref(t16)) == want
            for elem in (4, 2):
                v = L.tensor_view(1, st, elem, (0, 1, 2))
                assert lib.lanczos_resize_tensor_view_validate(ctypes.byref(d), wref, ctypes.byref(v)) == want, (win, st, elem)
            seen.add(want)
    assert seen == {L.OK, L.ERR_BAD_ARG}


def test_python_argument_checks():
    """what Context.resize_tensor refuses before any device call is made of it (a context is not needed for these)"""
    v = L.tensor_view(1, (35, 7, 1), 2, (2, 1, 0), "hv")
    assert (v.elem_bytes, v.out_channels, list(v.src_channel), v.flip) == (2, 3, [2, 1, 0, 0], 3)
    assert L.tensor_view(1, (35, 7, 1), flip="h").flip == 1 and L.tensor_view(1, (35, 7, 1), flip=None).flip == 0
    assert L.tensor_view(1, (35, 7, 1), flip=L.FLIP_V).flip == 2
