"""What the GPU checks of lanczos_resize_ycc_* share (tests/test_resize_ycc_gpu.py, tests/test_resize_ycc_edges_gpu.py): the
device entries run on the model's buffers (tests/resize_ycc_model.py) with every output between sentinels, and every sentinel
checked."""
import numpy as np

import lanczos_hls_amd as L
import resize_tensor_view_model as V
import resize_ycc_model as Y

GUARD = 64
LAYOUT_CODE = {Y.PLANAR: L.YCC_PLANAR, Y.NV12: L.YCC_NV12, Y.NV21: L.YCC_NV21}


def _desc(case):
    return L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3, filter=case.filt)


def _source(d, case, s):
    return L.ycc_source(d, LAYOUT_CODE[s.layout], case.sx, case.sy, y_row_stride=s.y_row_stride, c_row_stride=s.c_row_stride,
                        cb_offset=s.cb_offset, cr_offset=s.cr_offset)


def _eq(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


def _bytes(ctx, case, s, frames, d_table, window=None, path=L.RESIZE_AUTO, pad=0):
    """lanczos_resize_ycc_device on the model's buffer: RGB frames between sentinels, the first of which sits directly behind
    a frame's w * h * 3 bytes.  Returns [F][h][w][3]"""
    import torch
    d = _desc(case)
    w, h = (case.out_w, case.out_h) if window is None else window[2:]
    n = w * h * 3
    fs = (n + 3) // 4 * 4 + 4 * pad
    total = GUARD + frames * fs + GUARD
    yb = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    x = torch.from_numpy(s.buf).cuda()
    assert x.data_ptr() % 4 == 0 and yb.data_ptr() % 4 == 0
    ctx.resize_force(path)
    try:
        ctx.resize_ycc_device(d, _source(d, case, s), d_table.data_ptr(), x.data_ptr() + s.at, yb.data_ptr() + GUARD, frames,
                              in_frame_stride=s.frame_stride, out_frame_stride=fs if pad else 0,
                              stream=torch.cuda.current_stream().cuda_stream, box=case.box, reducing_gap=case.gap, window=window)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    raw = yb.cpu().numpy()
    keep = np.zeros(total, dtype=bool)
    out = []
    for f in range(frames):
        a = GUARD + f * fs
        keep[a:a + n] = True
        out.append(raw[a:a + n].reshape(h, w, 3))
    assert (raw[~keep] == 0xA5).all(), "a byte outside the RGB frames was written"
    return np.stack(out)


def _tensor(ctx, case, s, frames, d_table, ref, lut, src, flips, st, dtype, window=None, host_flip=None, path=L.RESIZE_AUTO):
    """lanczos_resize_ycc_tensor_device into sentinels: every word the view names equals the model's scatter over `ref` (the RGB
    bytes [F][h][w][3]) and every other word still holds the sentinel"""
    import torch
    d = _desc(case)
    elem = 4 if dtype == "float32" else 2
    word, signed, SENT = (np.uint32, np.int32, 0xA5A5A5A5) if elem == 4 else (np.uint16, np.int16, 0xA5A5)
    _, h, w, _ = ref.shape
    oc = len(src)
    n = V.extent(w, h, oc, st)
    fs = n + 5
    total = GUARD + (frames - 1) * fs + n + GUARD
    want = np.full(total, SENT, dtype=word)
    assert V.scatter(want, GUARD, ref, lut, src, flips, st, fs) == frames * oc * h * w
    yb = torch.from_numpy(np.full(total, SENT, dtype=word).view(signed)).cuda()
    x = torch.from_numpy(s.buf).cuda()
    dl = torch.from_numpy(V.words(lut).view(signed)).cuda()
    kw = {}
    if host_flip is not None:                  # one flip for every frame in the struct, nothing on the device
        kw["flip"] = host_flip
    else:
        df = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).cuda()
        kw["d_flip"] = df.data_ptr()
    ctx.resize_force(path)
    try:
        ctx.resize_ycc_tensor_device(d, _source(d, case, s), d_table.data_ptr(), x.data_ptr() + s.at, yb.data_ptr() + elem * GUARD,
                                     frames, dl.data_ptr(), st, in_frame_stride=s.frame_stride, out_frame_stride=elem * fs,
                                     stream=torch.cuda.current_stream().cuda_stream, box=case.box, reducing_gap=case.gap,
                                     dtype=dtype, window=window, channels_out=src, **kw)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    got = yb.cpu().numpy().view(word)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} words differ, first at {int(bad[0][0]) - GUARD}: {int(got[bad[0][0]]):#x} != "
                             f"{int(want[bad[0][0]]):#x}")
