"""Host-side checks of the 16-bit tensor entry (lanczos_resize_tensor16_*, include/lanczos_hip.h): the rounding of a float32
table to bfloat16 / float16 against torch's CPU cast as bit patterns, the table of ToTensor() + Normalize() in both formats,
and every refusal of lanczos_resize_tensor16_validate.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor16_model as T

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("bfloat16", "float16")


def _torch_cast(f32, dtype):
    """torch's CPU cast of a float32 array, as 16-bit patterns"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(f32)).to(getattr(torch, dtype))
    return t.view(torch.int16).numpy().view(np.uint16)


def _is_nan16(w, dtype):
    exp, man = (0x7F80, 0x007F) if dtype == "bfloat16" else (0x7C00, 0x03FF)
    return ((w & exp) == exp) & ((w & man) != 0)


# every upper half-word of a float32, times twelve lower half-words: at and next to the ties of bfloat16 (0x8000) and of a
# normal float16 (0x1000 below an even and 0x3000 below an odd unit), and the ends.  float16's subnormal ties lie in the upper
# half-word and at lower half-word 0, so they are among these too
LOWER = (0x0000, 0x0001, 0x0FFF, 0x1000, 0x1001, 0x2FFF, 0x3000, 0x3001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


@pytest.fixture(scope="module")
def patterns():
    hi, lo = np.meshgrid(np.arange(1 << 16, dtype=np.uint32), np.array(LOWER, dtype=np.uint32), indexing="ij")
    bits = (hi << 16 | lo).reshape(-1)
    f = bits.view(np.float32)
    nan = np.isnan(f)
    assert int((~nan).sum()) == 783362
    return f, nan


@pytest.mark.parametrize("dtype", DTYPES)
def test_lut_convert16_is_torchs_cast(patterns, dtype):
    f, nan = patterns
    got = L.lut_convert16(f, dtype)
    assert got.shape == f.shape and got.dtype == (np.float16 if dtype == "float16" else np.uint16)
    got = T.words(got)
    want = _torch_cast(f, dtype)
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (dtype, bad.size, hex(int(f.view(np.uint32)[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    assert _is_nan16(got[nan], dtype).all()           # a NaN stays a NaN; sign and payload are not part of the contract
    if dtype == "float16":                            # numpy rounds the same way
        with np.errstate(over="ignore"):
            assert np.array_equal(got[~nan], f[~nan].astype(np.float16).view(np.uint16))
    else:                                             # the formula of the header
        b = f.view(np.uint32)[~nan].astype(np.uint64)
        assert np.array_equal(got[~nan], ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16))


def test_lut_convert16_arguments():
    a = np.zeros(4, dtype=np.float32)
    out = np.zeros(4, dtype=np.uint16)
    lib = L._lib()
    for fmt in (0, 3, -1):
        assert lib.lanczos_tensor_lut_convert16(a.ctypes.data, 4, fmt, out.ctypes.data) == L.ERR_BAD_ARG
        assert lib.lanczos_tensor16_lut_normalize(3, None, None, fmt, np.zeros(768, dtype=np.uint16).ctypes.data) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_lut_convert16(None, 4, L.TENSOR_BF16, out.ctypes.data) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_lut_convert16(a.ctypes.data, 4, L.TENSOR_BF16, None) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_lut_convert16(a.ctypes.data, -1, L.TENSOR_BF16, out.ctypes.data) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_lut_convert16(a.ctypes.data, 0, L.TENSOR_F16, out.ctypes.data) == L.OK
    assert lib.lanczos_tensor16_lut_normalize(2, None, None, L.TENSOR_BF16, out.ctypes.data) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor16_lut_normalize(3, None, None, L.TENSOR_BF16, None) == L.ERR_BAD_ARG
    for bad in ("float64", "half", None):
        with pytest.raises(L.LanczosError):
            L.lut_convert16(a, bad)
        with pytest.raises(L.LanczosError):
            L.normalize_lut(3, dtype=bad)
    assert L.lut_convert16(np.float32([[1.0, -2.0]]), "float16").tolist() == [[1.0, -2.0]]
    assert L.lut_convert16(np.float32([1.0, -2.0]), "bfloat16").tolist() == [0x3F80, 0xC000]


def _torch_lut(channels, mean, std, dtype):
    """torchvision's ToTensor() + Normalize() over all 256 values on the CPU in float32, cast by torch, as 16-bit patterns"""
    import torch
    v = torch.arange(256, dtype=torch.int32).to(torch.uint8)[None, :].expand(channels, 256)
    x = v.to(torch.float32).div(255)
    if mean is not None:
        x = x.sub(torch.tensor(mean, dtype=torch.float32)[:, None])
    if std is not None:
        x = x.div(torch.tensor(std, dtype=torch.float32)[:, None])
    return x.contiguous().to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_lut16_is_torch_bit_for_bit(dtype):
    rng = np.random.default_rng(5)
    cases = [(3, IMAGENET_MEAN, IMAGENET_STD), (3, None, None), (1, None, None), (4, None, None),
             (3, IMAGENET_MEAN, None), (3, None, IMAGENET_STD),
             (3, IMAGENET_MEAN, (1e-6,) * 3),      # float16 overflows to inf
             (3, IMAGENET_MEAN, (1e6,) * 3)]       # float16 subnormals
    for c in (1, 3, 4):
        for _ in range(3):
            cases.append((c, tuple(rng.uniform(-1, 1, c).astype(np.float32).tolist()),
                          tuple(rng.uniform(0.01, 4, c).astype(np.float32).tolist())))
    for c, mean, std in cases:
        lut = L.normalize_lut(c, mean, std, dtype=dtype)
        assert lut.shape == (c, 256) and lut.dtype == (np.float16 if dtype == "float16" else np.uint16)
        want = _torch_lut(c, mean, std, dtype)
        assert np.array_equal(T.words(lut), want), (dtype, c, mean, std, int((T.words(lut) != want).sum()))
        # and it is the float32 table, converted
        assert np.array_equal(T.words(lut), T.words(L.lut_convert16(L.normalize_lut(c, mean, std), dtype)))
    if dtype == "float16":
        big = T.words(L.normalize_lut(3, IMAGENET_MEAN, (1e-6,) * 3, dtype=dtype))
        # inf wherever |v / 255 - mean| / 1e-6 reaches 65520: all but the 2 * 0.0655 * 255 = 34 bytes around each mean
        assert ((big & 0x7FFF) == 0x7C00).sum() >= 768 - 3 * 35
        small = T.words(L.normalize_lut(3, IMAGENET_MEAN, (1e6,) * 3, dtype=dtype))
        # |v / 255 - mean| / 1e6 is below 2^-14 everywhere: subnormals, but for the 16 or so bytes around each mean that fall
        # below 2^-25 and round to 0
        assert (((small & 0x7C00) == 0) & ((small & 0x03FF) != 0)).sum() >= 768 - 3 * 17


def test_the_fixture_tells_rounding_from_truncation():
    """Dropping the lower half-word of the float32 entries is NOT the bfloat16 table: ImageNet's constants show it in more than
    300 of the 768 entries, so an implementation that truncates cannot pass the test above."""
    f32 = L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD)
    truncated = (f32.view(np.uint32) >> 16).astype(np.uint16)
    differ = int((truncated != L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD, dtype="bfloat16")).sum())
    print("truncation differs from round-to-nearest-even in", differ, "of 768 entries")
    assert differ >= 300


def test_the_defaults_are_the_float_entry():
    assert np.array_equal(L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD).view(np.uint32),
                          L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD, dtype="float32").view(np.uint32))
    assert L.normalize_lut(3).dtype == np.float32


def _t(strides, lut=1):
    return L.tensor16_out(lut, strides)


def _code(desc, t):
    return L._lib().lanczos_resize_tensor16_validate(ctypes.byref(desc), ctypes.byref(t) if t is not None else None)


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
    assert _code(d, _t([2 * s for s in st])) == L.OK                                    # every other element
    assert _code(d, _t([s + (5 if ax == order[2] else 0) for s, ax in zip(st, "cyx")])) == L.OK   # padded outermost axis
    for i, ax in enumerate("cyx"):
        if st[i] == 1:
            continue
        low = list(st)
        low[i] -= 1                          # one step below the legal stride: the last element of the axis inside it
        assert _code(d, _t(low)) == L.ERR_BAD_ARG, (order, ax, low)   # overlaps the next one
    # the model agrees: the legal strides name every address once
    out = np.zeros(T.extent(W, H, C, st), dtype=np.uint16)
    T.scatter(out, 0, np.zeros((1, H, W, C), dtype=np.uint8), T.identity_lut16(C), st, out.size)


def test_validate_refusals():
    d = L.resize_desc(20, 20, W, H, C)
    chw = L.tensor_strides("chw", W, H, C)
    assert _code(d, _t(chw)) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG                                    # a null struct
    assert _code(d, _t(chw, lut=None)) == L.ERR_BAD_ARG                       # a null table
    for i in range(3):
        for bad in (0, -1, -chw[i], (1 << 40) + 1):
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
        L.resize_tensor16_validate(d, _t((1, 1, 1)))
    assert e.value.code == L.ERR_BAD_ARG
    L.resize_tensor16_validate(d, _t(chw))


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.TensorOut16) == 8 + 3 * 8 + 4 * 4
    assert (L.TENSOR_BF16, L.TENSOR_F16) == (1, 2)
    for name in ("lanczos_resize_tensor16_validate", "lanczos_tensor_lut_convert16", "lanczos_tensor16_lut_normalize",
                 "lanczos_resize_tensor16_device", "lanczos_resize_tensor16_host"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name)
