"""Host-side checks of the normalised-tensor entry for 16-bit and float samples (lanczos_tensor_norm,
lanczos_resize_tensor_norm_*, include/lanczos_hip.h): the struct and its init, every refusal of the validator, the numpy model of
the contract (tests/resize_tensor_norm_model.py) against torch's own pipeline on the CPU over every 16-bit value and over the
special floats, a pin that the folded form is another function, and rs_route's answer for norm requests, asked on the host by
tests/native/resize_norm_route_check.hip.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor_norm_model as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 7, 5
DTYPES = ["float32", "bfloat16", "float16"]
# (div, mean, std): ImageNet-like over the 16-bit range; a 12-bit range whose small values are float16 subnormals; values that
# overflow float16
PARAMS = [(65535.0, 0.485, 0.229), (4095.0, 0.0, 256.0), (1.0, -3.5, 0.5)]


def _wref(window):
    if window is None:
        return None
    w = L.ResizeWindow()
    w.x0, w.y0, w.w, w.h = window
    return ctypes.byref(w)


def _code(desc, n, window=None):
    return L._lib().lanczos_resize_tensor_norm_validate(ctypes.byref(desc), _wref(window), ctypes.byref(n) if n is not None else None)


def _n(strides, src, dtype="float32", flip=0, d_flip=None):
    return L.tensor_norm(strides, 65535.0, 0.5, 0.25, dtype, src, flip, d_flip)


def _torch_want(samples, div, mean, std, dtype):
    """torch's own pipeline on the CPU over [..., C] samples, parameters passed as tensors: bit patterns of the same shape"""
    import torch
    a = np.ascontiguousarray(samples)
    x = torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint16 else a).float()
    c = a.shape[-1]
    d, m, s = (torch.from_numpy(np.array(np.broadcast_to(np.asarray(v, dtype=np.float32), (c,)))) for v in (div, mean, std))
    x = x.div(d).sub(m).div(s).contiguous()
    if dtype == "float32":
        return x.view(torch.int32).numpy().view(np.uint32)
    return x.to(getattr(torch, dtype)).view(torch.int16).numpy().view(np.uint16)


def test_abi_struct_matches_the_header():
    assert ctypes.sizeof(L.TensorNorm) == 3 * 16 + 3 * 8 + 4 + 4 + 4 * 4 + 4 + 4 + 8 + 4 * 4    # 4 bytes of padding before d_flip
    assert (L.TensorNorm.div.offset, L.TensorNorm.mean.offset, L.TensorNorm.std.offset, L.TensorNorm.chan_stride.offset) == (0, 16, 32, 48)
    assert (L.TensorNorm.format.offset, L.TensorNorm.src_channel.offset, L.TensorNorm.d_flip.offset, L.TensorNorm.reserved.offset) == (72, 80, 104, 112)
    assert (L.TENSOR_BF16, L.TENSOR_F16, L.TENSOR_F32) == (1, 2, 3)               # the existing values keep their numbers
    for name in ("lanczos_tensor_norm_init", "lanczos_resize_tensor_norm_validate", "lanczos_resize_tensor_norm_device",
                 "lanczos_resize_tensor_norm_host"):
        assert name in L.ABI_SYMBOLS and hasattr(L._lib(), name), name
    with open(os.path.join(ROOT, "include", "lanczos_hip.h")) as f:
        header = f.read()
    for macro, value in (("LANCZOS_TENSOR_F32", 3), ("LANCZOS_TENSOR_BF16", 1), ("LANCZOS_TENSOR_F16", 2), ("LANCZOS_TENSOR_CHW", 0),
                         ("LANCZOS_TENSOR_HWC", 1)):
        assert "#define %s %d" % (macro, value) in header, macro


def test_norm_init():
    lib = L._lib()
    for kw, c in (({"bits": 16}, 3), ({"f32": True}, 1), ({"bits": 16}, 4)):
        d = L.resize_desc(20, 20, W, H, c, **kw)
        for dtype in DTYPES:
            n = L.tensor_norm_init(d, dtype, "chw")
            assert (n.chan_stride, n.row_stride, n.pix_stride) == (H * W, W, 1)
            assert (n.format, n.out_channels, list(n.src_channel), n.flip, n.d_flip) == (L._TENSOR_NORM_FORMATS[dtype], c, list(range(c)) + [0] * (4 - c), 0, None)
            assert (list(n.div), list(n.mean), list(n.std), list(n.reserved)) == ([1.0] * 4, [0.0] * 4, [1.0] * 4, [0] * 4)
            assert _code(d, n) == L.OK
            n = L.tensor_norm_init(d, dtype, "hwc")
            assert (n.chan_stride, n.row_stride, n.pix_stride) == (1, W * c, c) and _code(d, n) == L.OK
    d = L.resize_desc(20, 20, W, H, 3, bits=16)
    n = L.TensorNorm()
    for fmt in (0, 4, -1, 16):
        assert lib.lanczos_tensor_norm_init(ctypes.byref(n), ctypes.byref(d), fmt, L.TENSOR_CHW) == L.ERR_BAD_ARG
    for layout in (2, -1):
        assert lib.lanczos_tensor_norm_init(ctypes.byref(n), ctypes.byref(d), L.TENSOR_F32, layout) == L.ERR_BAD_ARG
    assert lib.lanczos_tensor_norm_init(None, ctypes.byref(d), L.TENSOR_F32, L.TENSOR_CHW) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert lib.lanczos_tensor_norm_init(ctypes.byref(n), ctypes.byref(bad), L.TENSOR_F32, L.TENSOR_CHW) == L.ERR_BAD_ARG
    for i in range(4):   # init clears what was there
        n.reserved[i] = 7
    assert lib.lanczos_tensor_norm_init(ctypes.byref(n), ctypes.byref(d), L.TENSOR_F16, L.TENSOR_CHW) == L.OK and not any(n.reserved)
    with pytest.raises(L.LanczosError):
        L.tensor_norm_init(d, "float64")


def test_validate_refusals():
    d = L.resize_desc(20, 20, W, H, 3, bits=16)
    chw = L.tensor_strides("chw", W, H, 3)
    ident = (0, 1, 2)
    for dd in (d, L.resize_desc(20, 20, W, H, 3, f32=True)):
        for dtype in DTYPES:
            assert _code(dd, _n(chw, ident, dtype)) == L.OK
    assert _code(d, None) == L.ERR_BAD_ARG                                         # a null struct
    # an 8-bit descriptor: the table entries serve those
    assert _code(L.resize_desc(20, 20, W, H, 3), _n(chw, ident)) == L.ERR_UNSUPPORTED
    assert _code(L.resize_desc(20, 20, W, H, 4, alpha=True), _n(chw, ident)) == L.ERR_UNSUPPORTED
    for fmt in (0, 4, -1, 8):                                                      # an unknown format
        n = _n(chw, ident)
        n.format = fmt
        assert _code(d, n) == L.ERR_BAD_ARG, fmt
    for i in range(3):                                                             # everything the view validator refuses
        for bad in (0, -1, -chw[i], (1 << 40) + 1):
            st = list(chw)
            st[i] = bad
            assert _code(d, _n(st, ident)) == L.ERR_BAD_ARG, st
    assert _code(d, _n((1, 1, 1), ident)) == L.ERR_BAD_ARG
    assert _code(d, _n((H * W - 1, W, 1), ident)) == L.ERR_BAD_ARG
    for i in range(4):
        n = _n(chw, ident)
        n.reserved[i] = 1
        assert _code(d, n) == L.ERR_BAD_ARG
    bad = L.ResizeDesc.from_buffer_copy(d)
    bad.channels = 2
    assert _code(bad, _n(chw, (0, 1))) == L.ERR_BAD_ARG                            # what lanczos_resize_validate refuses
    nn = L.ResizeDesc.from_buffer_copy(d)
    nn.reserved[0] |= L.filter_code("nearest") << 8
    assert _code(nn, _n(chw, ident)) == L.ERR_UNSUPPORTED                          # NEAREST with 16-bit samples stays unsupported
    assert _code(L.resize_desc(20, 20, W, H, 3, f32=True, filter="nearest"), _n(chw, ident)) == L.OK
    assert _code(d, _n(chw, ident), window=(0, 0, W + 1, H)) == L.ERR_BAD_ARG      # a window outside the output
    assert _code(d, _n(L.tensor_strides("chw", 4, 3, 3), ident), window=(1, 1, 4, 3)) == L.OK
    n = _n(chw, ident)
    for oc in (0, -1, 4, 5):
        n.out_channels = oc
        assert _code(d, n) == L.ERR_BAD_ARG, oc
    d4 = L.resize_desc(20, 20, W, H, 4, bits=16)
    assert _code(d4, _n(L.tensor_strides("chw", W, H, 4), (3, 0, 1, 2))) == L.OK
    assert _code(d4, _n(chw, (2, 1, 0))) == L.OK                                   # a channel dropped
    for src in ((0, 1, 3), (0, 1, -1), (3, 1, 0), (0, 0, 1), (2, 1, 2), (1, 1), (2, 2)):
        assert _code(d, _n(chw, src)) == L.ERR_BAD_ARG, src
    n = _n(chw, (0, 1, 2))
    n.src_channel[3] = 3
    assert _code(d4, n) == L.ERR_BAD_ARG                                           # a non-zero src_channel[3] with out_channels 3
    for flip in (0, 1, 2, 3):
        assert _code(d, _n(chw, ident, flip=flip)) == L.OK
    for flip in (4, 7, -1, 256):
        assert _code(d, _n(chw, ident, flip=flip)) == L.ERR_BAD_ARG, flip
    assert _code(d, _n(chw, (2, 1, 0), flip="hv", d_flip=1)) == L.OK               # a device pointer is not looked at
    # div / mean / std are not inspected: the arithmetic is defined for every float
    n = _n(chw, ident)
    n.div[0], n.mean[1], n.std[2] = 0.0, float("nan"), float("-inf")
    assert _code(d, n) == L.OK
    with pytest.raises(L.LanczosError) as e:
        L.resize_tensor_norm_validate(L.resize_desc(20, 20, W, H, 3), _n(chw, ident))
    assert e.value.code == L.ERR_UNSUPPORTED
    L.resize_tensor_norm_validate(d, _n(chw, (2, 1, 0), flip="h"))
    with pytest.raises(L.LanczosError):
        L.tensor_norm(chw, channels_out=(0, 1, 2, 3, 0))
    with pytest.raises(L.LanczosError):
        L.tensor_norm(chw, div=(1.0, 2.0))                                         # one value, or one per output channel


def test_the_old_entries_still_refuse_wide_samples():
    chw = L.tensor_strides("chw", W, H, 3)
    lib = L._lib()
    for kw in ({"bits": 16}, {"f32": True}):
        d = L.resize_desc(20, 20, W, H, 3, **kw)
        v = L.tensor_view(1, chw, 4, (0, 1, 2))
        assert lib.lanczos_resize_tensor_view_validate(ctypes.byref(d), None, ctypes.byref(v)) == L.ERR_UNSUPPORTED
        t = L.tensor_out(1, chw)
        assert lib.lanczos_resize_tensor_validate(ctypes.byref(d), ctypes.byref(t)) == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_model_is_torchs_arithmetic_on_every_16_bit_value(dtype):
    v = np.arange(65536, dtype=np.uint16).reshape(-1, 1)
    for div, mean, std in PARAMS:
        got = N.elements(v, div, mean, std, dtype)
        want = _torch_want(v, div, mean, std, dtype)
        assert got.dtype == want.dtype and np.array_equal(got, want), (div, mean, std)
    # per-channel parameters go with their channel
    rgb = np.stack([np.arange(65536), np.arange(65536)[::-1], (np.arange(65536) * 7919) % 65536], axis=-1).astype(np.uint16)
    div, mean, std = zip(*PARAMS)
    assert np.array_equal(N.elements(rgb, div, mean, std, dtype), _torch_want(rgb, div, mean, std, dtype))
    if dtype == "float16":   # the parameter sets reach what they were chosen for
        sub = N.elements(v, *PARAMS[1], dtype)
        assert ((sub & 0x7C00) == 0).sum() > 4 and (sub & 0x03FF)[(sub & 0x7C00) == 0].any()      # float16 subnormals
        assert (N.elements(v, *PARAMS[2], dtype) == 0x7C00).any()                                  # overflow to inf


def _special_floats():
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x3F800000, 0xBF800000, 0x33800000, 0x38800000,
                     0x387FFFFF, 0x477FE000, 0x477FF000, 0x00400000, 0x80000100], dtype=np.uint32)
    rng = np.random.default_rng(5)
    noise = (rng.standard_normal(4000) * np.exp(rng.uniform(-100, 88, 4000))).astype(np.float32)
    return np.concatenate([bits.view(np.float32), noise]).reshape(-1, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_model_is_torchs_arithmetic_on_special_floats(dtype):
    v = _special_floats()
    assert np.isnan(v).sum() == 3 and np.isinf(v).sum() >= 2 and ((v != 0) & (np.abs(v) < 1.2e-38)).sum() >= 6
    for div, mean, std in [(1.0, 0.0, 1.0), (3.0, 0.25, 0.5), (1e-30, 1e-10, 1e20), (65535.0, 0.485, 0.229)]:
        got = N.elements(v, div, mean, std, dtype)
        want = _torch_want(v, div, mean, std, dtype)
        assert N.same_bits(got, want, dtype), (div, mean, std)
    # the identity parameters return the sample's own bits (NaNs aside)
    ident = N.elements(v, 1.0, 0.0, 1.0, "float32")
    assert N.same_bits(ident, v.view(np.uint32), "float32")


def test_the_folded_form_is_another_function():
    """v * (1 / (div * std)) + (-mean / std) is not the contract: it differs on thousands of 16-bit values, so a test over all of
    them tells the two apart"""
    v = np.arange(65536, dtype=np.uint16).reshape(-1, 1)
    for div, mean, std in PARAMS[:2]:
        differ = int((N.elements(v, div, mean, std) != N.folded(v, div, mean, std)).sum())
        assert differ > 1000, (div, mean, std, differ)


def test_scatter_names_every_address_once():
    p = (np.arange(2 * H * W * 4).reshape(2, H, W, 4) * 37 % 65536).astype(np.uint16)
    for src in ((0, 1, 2, 3), (2, 1, 0), (3,)):
        oc = len(src)
        for st in (N.strides("chw", W, H, oc), N.strides("hwc", W, H, oc), (H * (W + 3) + 5, W + 3, 1)):
            n = N.extent(W, H, oc, st)
            out = np.full(2 * (n + 4), 0xDEADBEEF, dtype=np.uint32)
            assert N.scatter(out, 1, p, 65535.0, 0.5, 0.25, "float32", src, [1, 2], st, n + 4) == 2 * oc * H * W
            assert (out != 0xDEADBEEF).sum() == 2 * oc * H * W
    # torch-style indexing of the tight result: channel map, then per-frame flips
    full = N.norm(p, 65535.0, 0.5, 0.25, "float32")
    got = N.norm(p, 65535.0, 0.5, 0.25, "float32", src=(2, 0), flips=[1, 2])
    assert np.array_equal(got[0], full[0][[2, 0]][:, :, ::-1]) and np.array_equal(got[1], full[1][[2, 0]][:, ::-1, :])
    assert np.array_equal(N.norm(p, 65535.0, 0.5, 0.25, "bfloat16", layout="hwc"), N.norm(p, 65535.0, 0.5, 0.25, "bfloat16").transpose(0, 2, 3, 1))


def test_python_argument_checks():
    n = L.tensor_norm((35, 7, 1), (1.0, 2.0, 4.0), 0.5, (0.25, 0.5, 1.0), "bfloat16", (2, 1, 0), "hv")
    assert (n.format, n.out_channels, list(n.src_channel), n.flip) == (L.TENSOR_BF16, 3, [2, 1, 0, 0], 3)
    assert (list(n.div)[:3], list(n.mean)[:3], list(n.std)[:3]) == ([1.0, 2.0, 4.0], [0.5] * 3, [0.25, 0.5, 1.0])
    with pytest.raises(L.LanczosError):
        L.tensor_norm((35, 7, 1), dtype="int8")


def test_the_route_of_norm_requests(tmp_path):
    """rs_route answers FUSED exactly where the sample request's plan is fused and the element frame spans less than 2^31 bytes,
    a frame of exactly 2^31 bytes included, and CONVERTED behind the sample request's own main step everywhere else"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "lanczos-hls_amd", "csrc")
    exe = str(tmp_path / "resize_norm_route_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-I" + csrc,
                    os.path.join(ROOT, "tests", "native", "resize_norm_route_check.hip"), os.path.join(csrc, "lanczos_resize_route.cpp"),
                    "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BAD" not in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.split("\n") if ln.startswith("NORM ")]
    assert r.stdout.strip().endswith("ok %d" % len(lines)) and len(lines) == 20
    routes = {ln[5:31].strip(): int(ln.split(" route ")[1].split()[0]) for ln in lines}
    assert routes["2^31 bytes"] == L.TENSOR_CONVERTED and routes["2^31 - 4 bytes"] == L.TENSOR_FUSED
    assert set(routes.values()) == {0, L.TENSOR_FUSED, L.TENSOR_CONVERTED}
