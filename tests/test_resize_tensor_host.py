"""Host-side checks of the tensor entry (lanczos_resize_tensor_*, include/lanczos_hip.h): the table of ToTensor() + Normalize()
against torch's own arithmetic as bit patterns, every refusal of lanczos_resize_tensor_validate, and the plan query.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor_model as T

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _torch_lut(channels, mean, std):
    """torchvision's ToTensor() + Normalize() over all 256 values on the CPU (IEEE division), as 32-bit patterns"""
    import torch
    v = torch.arange(256, dtype=torch.int32).to(torch.uint8)[None, :].expand(channels, 256)
    x = v.to(torch.float32).div(255)
    if mean is not None:
        x = x.sub(torch.tensor(mean, dtype=torch.float32)[:, None])
    if std is not None:
        x = x.div(torch.tensor(std, dtype=torch.float32)[:, None])
    return T.bits(x.contiguous().numpy())


def test_normalize_lut_is_torch_bit_for_bit():
    rng = np.random.default_rng(5)
    cases = [(3, IMAGENET_MEAN, IMAGENET_STD), (3, None, None), (1, None, None), (4, None, None),
             (3, IMAGENET_MEAN, None), (3, None, IMAGENET_STD)]
    for c in (1, 3, 4):
        for _ in range(4):
            cases.append((c, tuple(rng.uniform(-1, 1, c).astype(np.float32).tolist()),
                          tuple(rng.uniform(0.01, 4, c).astype(np.float32).tolist())))
    for c, mean, std in cases:
        lut = L.normalize_lut(c, mean, std)
        assert lut.shape == (c, 256) and lut.dtype == np.float32
        want = _torch_lut(c, mean, std)
        assert np.array_equal(T.bits(lut), want), (c, mean, std, int((T.bits(lut) != want).sum()))
    assert np.array_equal(T.bits(L.normalize_lut(1)), T.bits(np.arange(256, dtype=np.float32) / np.float32(255))[None])


def test_the_folded_form_is_another_table():
    """v * scale + bias with scale = 1 / (255 std), bias = -mean / std is NOT the recipe: the fixture constants show it, so
    an implementation that folds cannot pass the test above."""
    mean, std = np.float32(IMAGENET_MEAN)[:, None], np.float32(IMAGENET_STD)[:, None]
    v = np.arange(256, dtype=np.float32)[None, :]
    folded = v * (np.float32(1) / (np.float32(255) * std)) + (-mean / std)
    assert folded.dtype == np.float32
    differ = int((T.bits(folded) != T.bits(L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD))).sum())
    print("folded form differs in", differ, "of 768 entries")
    assert differ > 100


def test_normalize_lut_arguments():
    with pytest.raises(L.LanczosError):
        L.normalize_lut(2)
    with pytest.raises(L.LanczosError):
        L.normalize_lut(3, mean=(1.0, 2.0))
    assert np.array_equal(L.normalize_lut(3, 0.5, 0.25)[0], L.normalize_lut(3, (0.5,) * 3, (0.25,) * 3)[2])


def _t(strides, lut=1):
    return L.tensor_out(lut, strides)


def _code(desc, t):
    return L._lib().lanczos_resize_tensor_validate(ctypes.byref(desc), ctypes.byref(t) if t is not None else None)


W, H, C = 7, 5, 3
EXTENT = {"c": C, "y": H, "x": W}


def _packed(order):
    """strides (chan, row, pix) of a frame packed with `order[0]` innermost"""
    st, run = {}, 1
    for ax in order:
        st[ax] = run
        run *= EXTENT[ax]
    return [st["c"], st["y"], st["x"]]


@pytest.mark.parametrize("order", list(itertools.permutations("cyx")), ids="".join)
def test_validate_every_stride_order(order):
    d = L.resize_desc(20, 20, W, H, C)
    st = _packed(order)
    assert _code(d, _t(st)) == L.OK
    assert _code(d, _t([2 * s for s in st])) == L.OK                                    # every other float
    assert _code(d, _t([s + (5 if ax == order[2] else 0) for s, ax in zip(st, "cyx")])) == L.OK   # padded outermost axis
    for i, ax in enumerate("cyx"):
        if st[i] == 1:
            continue
        low = list(st)
        low[i] -= 1                          # one step below the legal stride: the last element of the axis inside it
        assert _code(d, _t(low)) == L.ERR_BAD_ARG, (order, ax, low)   # overlaps the next one
    # the model agrees: the legal strides name every address once
    words = np.zeros(T.extent(W, H, C, st), dtype=np.uint32)
    T.scatter(words, 0, np.zeros((1, H, W, C), dtype=np.uint8), T.identity_lut(C), st, words.size)


def test_validate_refusals():
    d = L.resize_desc(20, 20, W, H, C)
    chw = L.tensor_strides("chw", W, H, C)
    assert chw == (H * W, W, 1) and L.tensor_strides("hwc", W, H, C) == (1, W * C, C)
    assert _code(d, _t(chw)) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG
    assert _code(d, _t(chw, lut=None)) == L.ERR_BAD_ARG                       # a null table
    for i in range(3):
        for bad in (0, -1, -chw[i]):
            st = list(chw)
            st[i] = bad
            assert _code(d, _t(st)) == L.ERR_BAD_ARG, st
    for i in range(4):
        t = _t(chw)
        t.reserved[i] = 1
        assert _code(d, t) == L.ERR_BAD_ARG
    assert _code(d, _t((H * W, W, 1))) == L.OK and _code(d, _t((H * W - 1, W, 1))) == L.ERR_BAD_ARG
    assert _code(d, _t((1, 1, 1))) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert _code(bad, _t(chw)) == L.ERR_BAD_ARG                               # what lanczos_resize_validate refuses
    assert _code(L.resize_desc(20, 20, W, H, C, bits=16), _t(chw)) == L.ERR_UNSUPPORTED
    assert _code(L.resize_desc(20, 20, W, H, C, f32=True), _t(chw)) == L.ERR_UNSUPPORTED
    assert _code(L.resize_desc(20, 20, W, H, 4, alpha=True), _t(L.tensor_strides("chw", W, H, 4))) == L.OK
    # an axis of extent 1 never moves: its stride is free
    assert _code(L.resize_desc(20, 20, W, H, 1), _t((1, W, 1))) == L.OK
    assert _code(L.resize_desc(20, 20, 1, H, C), _t((1, C, 1))) == L.OK
    with pytest.raises(L.LanczosError) as e:
        L.resize_tensor_validate(d, _t((1, 1, 1)))
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.tensor_strides("cwh", W, H, C)


def test_one_plan_for_bytes_and_tensor():
    """A tensor request has no plan of its own and no plan query: it runs on the plan lanczos_resize_plan_host(_ex) reports for
    the byte request (the table adds no LDS), and the GPU tests assert the route of every call against that query.  Here: the
    requests the tensor entry accepts plan as the issue's shapes are expected to, fused or not."""
    for iw, ih, ow, oh, c, alpha, box, fused in (
            (200, 37, 261, 75, 3, False, None, 1), (3840, 2160, 1920, 1080, 3, False, None, 1),
            (400, 2160, 200, 90, 3, False, None, 0),                       # 145 vertical taps: the ring does not fit
            (77, 33, 77, 20, 3, False, None, 0),                           # one pass
            (500, 375, 224, 224, 3, False, (62.5, 0, 437.5, 375), 1), (70, 37, 150, 75, 4, True, None, 1)):
        d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
        L.resize_tensor_validate(d, _t(L.tensor_strides("chw", ow, oh, c)))
        p = L.resize_plan_host(d, 1, box=box)
        p = p.inner if box else p
        assert p.fused == fused, (iw, ih, ow, oh)
        assert p.lds_bytes <= 80 * 1024
    assert not [s for s in L.ABI_SYMBOLS if "tensor" in s and "plan" in s]


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.TensorOut) == 8 + 3 * 8 + 4 * 4
    assert (L.TENSOR_FUSED, L.TENSOR_CONVERTED) == (1, 2)
