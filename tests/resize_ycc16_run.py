"""What the GPU tests of lanczos_resize_ycc16 share (tests/test_resize_ycc16_gpu.py, tests/test_resize_ycc16_edges_gpu.py): the
device calls on the model's buffers (tests/resize_ycc16_model.py).  Buffers are uint16 arrays with strides in words; every call
gets a whole buffer with noise or sentinels in everything it must not write, and the whole buffer comes back."""
import numpy as np

import lanczos_hls_amd as L
import resize_tensor_norm_model as TN
import resize_ycc16_model as M

GUARD = 16   # words of sentinel around an RGB or element buffer


def eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dev(words):
    """a uint16 (or uint32) numpy array on the device, through a signed view torch has everywhere"""
    import torch
    a = np.ascontiguousarray(words)
    return torch.from_numpy(a.view({2: np.int16, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])).cuda()


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


def desc(in_w, in_h, out_w, out_h, filt="lanczos"):
    return L.resize_desc(in_w, in_h, out_w, out_h, 3, bits=16, filter=filt)


def src_struct(d, layout, s):
    code, sx, sy = M.LAYOUTS[layout]
    return L.ycc16_source(d, code, sx, sy, **M.byte_strides(s))


def dst_struct(d, layout, s, window=None):
    code, sx, sy = M.LAYOUTS[layout]
    return L.ycc16_dest(d, code, window, sx, sy, **M.byte_strides(s))


def forced(ctx, path, fn):
    ctx.resize_force(path)
    try:
        return fn()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


def to_ycc(ctx, d, src_layout, s, dst_layout, before, window=None, box=None, path=L.RESIZE_AUTO, frames=None):
    """frames of Frames `s` into the buffer of Frames `before`: the whole buffer afterwards (uint16), and the call's info"""
    import torch
    frames = M.FRAMES if frames is None else frames
    x, o = dev(s.buf), dev(before.buf)
    forced(ctx, path, lambda: ctx.resize_ycc16_to_ycc_device(
        d, src_struct(d, src_layout, s), dst_struct(d, dst_layout, before, window), x.data_ptr() + 2 * s.at, o.data_ptr() + 2 * before.at,
        frames, in_frame_stride=2 * s.frame_stride, out_frame_stride=2 * before.frame_stride, stream=stream(), box=box, window=window))
    torch.cuda.synchronize()
    return back(o, np.uint16), ctx.last_ycc16_info()


def rgb_buffers(want, at_dword=True, seed=11):
    """(before, expected, at, frame stride) in words for packed RGB frames `want` [F][h][w][3]: frames a dword multiple apart
    with a noise word between them where a frame's words are odd, noise around"""
    f = want.shape[0]
    n = want[0].size
    fs = (n + 1) & ~1
    rng = np.random.default_rng(seed)
    before = rng.integers(0, 65536, GUARD + f * fs + GUARD, dtype=np.uint16)
    expected = before.copy()
    for k in range(f):
        expected[GUARD + k * fs:GUARD + k * fs + n] = want[k].reshape(-1)
        before[GUARD + k * fs:GUARD + k * fs + n] = want[k].reshape(-1) ^ 0xFFFF
    return before, expected, GUARD, fs


def to_rgb(ctx, d, src_layout, s, matrix, want, window=None, box=None, path=L.RESIZE_AUTO, frames=None):
    """-> (the whole output buffer, the expected one, info)"""
    import torch
    frames = want.shape[0] if frames is None else frames
    before, expected, at, fs = rgb_buffers(want)
    x, o = dev(s.buf), dev(before)
    forced(ctx, path, lambda: ctx.resize_ycc16_rgb_device(
        d, src_struct(d, src_layout, s), M.matrix_struct(L, matrix), x.data_ptr() + 2 * s.at, o.data_ptr() + 2 * at, frames,
        in_frame_stride=2 * s.frame_stride, out_frame_stride=2 * fs, stream=stream(), box=box, window=window))
    torch.cuda.synchronize()
    return back(o, np.uint16), expected, ctx.last_ycc16_info()


SENTINEL = {"float32": 0x7FC0DEAD, "bfloat16": 0x7FCD, "float16": 0x7EAD}


def tensor_buffers(rgb, div, mean, std, dtype, src, flips, strides, frame_gap=3):
    """(before, expected, at, frame stride) in elements: the contract's elements scattered over sentinels"""
    f, h, w, _ = rgb.shape
    ext = TN.extent(w, h, len(src), strides)
    fs = ext + frame_gap
    word = np.uint32 if dtype == "float32" else np.uint16
    before = np.full(GUARD + f * fs + GUARD, SENTINEL[dtype], dtype=word)
    expected = before.copy()
    TN.scatter(expected, GUARD, rgb, div, mean, std, dtype, src, flips, strides, fs)
    return before, expected, GUARD, fs


def to_tensor(ctx, d, src_layout, s, matrix, rgb, div=65535.0, mean=0.0, std=1.0, dtype="float32", src=(0, 1, 2), flip=0, flips=None,
              strides=None, window=None, box=None, path=L.RESIZE_AUTO):
    """rgb: the expected RGB words [F][h][w][3].  flips: one byte per frame for d_flip (XORed with `flip`).  -> (got, expected, info)"""
    import torch
    f, h, w, _ = rgb.shape
    strides = TN.strides("chw", w, h, len(src)) if strides is None else strides
    per_frame = [(flip ^ (int(flips[k]) if flips is not None else 0)) & 3 for k in range(f)]
    before, expected, at, fs = tensor_buffers(rgb, div, mean, std, dtype, src, per_frame, strides)
    eb = before.dtype.itemsize
    x, o = dev(s.buf), dev(before)
    d_flip = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).cuda() if flips is not None else None
    n = L.tensor_norm(strides, div, mean, std, dtype, src, flip, d_flip.data_ptr() if d_flip is not None else None)
    forced(ctx, path, lambda: ctx.resize_ycc16_tensor_device(
        d, src_struct(d, src_layout, s), M.matrix_struct(L, matrix), n, x.data_ptr() + 2 * s.at, o.data_ptr() + eb * at, f,
        in_frame_stride=2 * s.frame_stride, out_frame_stride=eb * fs, stream=stream(), box=box, window=window))
    torch.cuda.synchronize()
    return back(o, before.dtype), expected, ctx.last_ycc16_info()


def planned_kernel(in_w, in_h, out_w, out_h, filt, box, frames, window=None):
    """the kernel lanczos_resize_window_plan_host predicts for a one-channel plane of words under AUTO (KERNEL_NONE: no pass runs)"""
    d = L.resize_desc(in_w, in_h, out_w, out_h, 1, bits=16, filter=filt)
    p = L.resize_window_plan_host(d, window, frames, box=box if box is not None else (0, 0, in_w, in_h))
    if not (p.pass_h or p.pass_v):
        return L.KERNEL_NONE
    return L.KERNEL_RESIZE_FUSED if p.inner.fused else L.KERNEL_RESIZE_TWO_PASS
