"""GPU checks that isolate the three kernels of lanczos_resize_ycc16 at sizes taken from their own cover arithmetic
(tests/resize_ycc16_model.py: PAIRS_PER_WORKGROUP, MERGE_GROUP, MERGE_BLOCK).  The routes here run no resize kernel (asserted
LANCZOS_KERNEL_NONE: an axis that keeps its size over its whole span is not filtered), so the words of k_rs_ycc_split16,
k_rs_ycc_join16 and k_rs_ycc16_merge show one to one: pairs -> planes and planes -> pairs at the same even size, and 4:4:4
planes at the same size through a matrix.  Whole buffers are compared, noise in every unnamed word."""
import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_ycc16_model as M
import resize_ycc16_run as R
from resize_ycc16_run import eq

pytestmark = pytest.mark.gpu

WG = M.PAIRS_PER_WORKGROUP
ROW_PAIRS = (1, 2, 3, 4, 5) + tuple(k * WG + e for k in (1, 2, 3) for e in (-1, 0, 1))
NONE2 = (L.KERNEL_NONE, L.KERNEL_NONE)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _noise_planes(w, h, sx, sy, frames, seed):
    rng = np.random.default_rng([9800, w, h, seed])
    cw, ch = M.chroma_size(w, h, sx, sy)
    return tuple(rng.integers(0, 65536, s, dtype=np.uint16) for s in ((frames, h, w), (frames, ch, cw), (frames, ch, cw)))


def test_cover_arithmetic_of_the_rows():
    """the shapes below reach what they are there for: a word in front (odd rows of odd widths), a word behind, dwords in the
    first, second and third workgroup and not in the next"""
    seen = set()
    for cw in ROW_PAIRS:
        for row in (0, 1):
            head, nd, rest = M.pairs_cover(row, cw)
            seen.add((head, rest, (nd + M.PAIRS_THREADS - 1) // M.PAIRS_THREADS))
    # (a word in front leaves an even number of pairs behind it: never a word at both ends)
    assert {(1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 1, 3), (1, 0, 3), (0, 1, 0), (1, 0, 0)} <= seen, seen


@pytest.mark.parametrize("cw", ROW_PAIRS)
def test_split16_and_join16_alone(ctx, cw):
    """pairs -> planes and planes -> pairs at the same even size, both pair orders, the interleaved rows at every residue of the
    widest access (8 bytes: bases of 0 .. 3 words) and on a pitch of odd words, so that rows alternate between residues"""
    w, h = 2 * cw, 4
    planes = _noise_planes(w, h, 1, 1, 2, cw)
    d = R.desc(w, h, w, h)
    residues = set()
    for base in range(4):
        for pairs in ("p010", "nv21"):
            crs = 2 * cw + 1 + 2 * (base & 1)                                  # odd words: 2 mod 4 bytes
            s = M.build(*planes, M.layout_code(pairs), c_row_stride=crs, base=base, gap=base & 1, frame_gap=1, seed=base)
            before, want = M.expected_dest(planes, "i420", seed=7 + base, y_row_stride=w + 1, c_row_stride=cw + 1, base=1)
            got, info = R.to_ycc(ctx, d, pairs, s, "i420", before)
            eq(got, want.buf, f"split16 alone: {cw} pairs, {pairs}, base {base}")
            assert (info.luma_kernel, info.chroma_kernel) == NONE2 and info.split and not info.join, info
            s = M.build(*planes, M.PLANAR, base=1, seed=base)
            before, want = M.expected_dest(planes, pairs, seed=9 + base, c_row_stride=crs, base=base, gap=base & 1, frame_gap=1)
            got, info = R.to_ycc(ctx, d, "i420", s, pairs, before)
            eq(got, want.buf, f"join16 alone: {cw} pairs, {pairs}, base {base}")
            assert (info.luma_kernel, info.chroma_kernel) == NONE2 and info.join and not info.split, info
            residues |= {(2 * (want.at + f * want.frame_stride + want.cb_offset + r * crs)) % 8 for f in range(2) for r in range(2)}
    assert residues == {0, 2, 4, 6}


def _merge_only(ctx, planes, m, what, window=None, kinds=("rgb", "float32", "bfloat16")):
    """4:4:4 planes at their own size through matrix m: RGB words, float32 CHW and bfloat16 HWC elements"""
    f, h, w = planes[0].shape
    d = R.desc(w, h, w, h)
    s = M.build(*planes, M.PLANAR, base=1, seed=2)
    cut = planes if window is None else tuple(p[:, window[1]:window[1] + window[3], window[0]:window[0] + window[2]] for p in planes)
    rgb = M.convert(m, *cut)
    for kind in kinds:
        if kind == "rgb":
            got, want, info = R.to_rgb(ctx, d, "i444", s, m, rgb, window=window)
        else:
            hh, ww = rgb.shape[1:3]
            st = (hh * ww, ww, 1) if kind == "float32" else (1, 3 * ww, 3)
            got, want, info = R.to_tensor(ctx, d, "i444", s, m, rgb, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.25), dtype=kind, strides=st,
                                          flips=[(k + 1) & 3 for k in range(f)], window=window)
        eq(got, want, f"{what} -> {kind}")
        assert (info.luma_kernel, info.chroma_kernel) == NONE2 and info.merge and not info.split and not info.join, info
    return rgb


def _every_luma_word():
    """256 x 256: every luma word once, chroma hashed from it"""
    i = np.arange(65536, dtype=np.uint32)
    y = i.astype(np.uint16).reshape(1, 256, 256)
    cb = ((i * 40503 + 12345) & 0xFFFF).astype(np.uint16).reshape(1, 256, 256)
    cr = ((i * 25173 + 13849) & 0xFFFF).astype(np.uint16).reshape(1, 256, 256)
    return y, cb, cr


@pytest.mark.parametrize("standard", [M.BT709, M.BT2020])
def test_merge16_every_luma_word(ctx, standard):
    m = M.matrix(standard, 10, True, False)
    assert np.array_equal(M.matrix_of_struct(L.ycc16_matrix(standard, 10, True, False)).k, m.k)
    rgb = _merge_only(ctx, _every_luma_word(), m, f"every luma word, standard {standard}")
    assert rgb.min() == 0 and rgb.max() == 65535                       # both clamps are met


def test_merge16_pass_through_shows_the_words(ctx):
    """R = cb, G = y, B = cr with shift 0: the RGB words are the planes' words"""
    planes = _every_luma_word()
    rgb = _merge_only(ctx, planes, M.passthrough_matrix(), "pass-through", kinds=("rgb",))
    assert np.array_equal(rgb[..., 0], planes[1]) and np.array_equal(rgb[..., 1], planes[0]) and np.array_equal(rgb[..., 2], planes[2])


@pytest.mark.parametrize("shift,top", [(0, 0), (0, 1023), (0, 65535), (30, 0), (30, 1023), (30, 65535)])
def test_merge16_extreme_matrices(ctx, shift, top):
    """k = +-(2^24 - 1) with the shift at either end and the maximum at 0, 1023 and 65535: int64 sums of both signs, both clamps"""
    big = (1 << 24) - 1
    m = M.Matrix(np.array([[big, -big, big], [-big, big, -big], [big, big, big]], dtype=np.int64), [0, 32768, 65535], shift, top)
    planes = _noise_planes(61, 40, 0, 0, 2, shift + top)
    s = M.sums(m, *planes)
    assert s.min() < -(1 << 40) and s.max() > (1 << 40)                # far outside int32 on both sides
    rgb = _merge_only(ctx, planes, m, f"extreme matrix shift {shift} max {top}")
    assert rgb.min() == 0 and rgb.max() <= top
    if shift == 0 or top <= 1023:                                      # (shifted by 30 the sums end near 1536)
        assert rgb.max() == top
    if shift == 30 and top == 65535:                                   # between the clamps too
        assert ((rgb > 0) & (rgb < top)).any()


@pytest.mark.parametrize("w,h", [(61, 40), (1, 1500), (2500, 1), (1100, 3)])
def test_merge16_frame_shapes(ctx, w, h):
    """w == 1, one long row, rows that start inside a workgroup's pixels (a row origin that is no multiple of the block)"""
    _merge_only(ctx, _noise_planes(w, h, 0, 0, 2, 1), M.matrix(M.BT2020, 10, True, False), f"{w} x {h}")


def test_merge16_tails_behind_the_first_workgroup(ctx):
    """windows of MERGE_BLOCK + 1 .. MERGE_BLOCK + MERGE_GROUP - 1 pixels: the last thread's group holds fewer pixels than its
    words would, and the word behind the frame is noise that has to stay"""
    planes = _noise_planes(61, 40, 0, 0, 2, 5)
    for tail in range(1, M.MERGE_GROUP):
        n = M.MERGE_BLOCK + tail
        wins = [(x0, y0, ww, n // ww) for ww in range(1, 62) if n % ww == 0 and n // ww <= 40 for x0, y0 in ((0, 0), (61 - ww, 40 - n // ww))]
        assert wins, n
        for win in wins:
            _merge_only(ctx, planes, M.matrix(M.BT709, 12, False, True), f"window {win}: a tail of {tail}", window=win)


def test_past_65535_frames(ctx):
    """65537 frames of tiny planes: every kernel that puts frames on a grid dimension goes out in two groups"""
    import torch
    n = 65537
    planes = _noise_planes(2, 1, 0, 0, n, 3)                           # 4:4:4, 2 x 1: merge only
    d = R.desc(2, 1, 2, 1)
    src = M.tight(*planes, "i444")
    m = M.passthrough_matrix()
    rgb = M.convert(m, *planes)
    x = R.dev(src)
    o = torch.zeros(n * 6 + 8, dtype=torch.int16, device="cuda")
    ctx.resize_ycc16_rgb_device(d, L.ycc16_source(d, "i444"), M.matrix_struct(L, m), x.data_ptr(), o.data_ptr(), n, stream=R.stream())
    torch.cuda.synchronize()
    info = ctx.last_ycc16_info()
    got = R.back(o, np.uint16)
    eq(got[:n * 6], rgb.reshape(-1), "65537 frames through the merge")
    assert not got[n * 6:].any()
    assert (info.luma_kernel, info.chroma_kernel) == NONE2 and info.merge and info.launches == 3 + 2, info   # three plane copies, the merge twice
    planes = _noise_planes(4, 2, 1, 1, n, 4)                           # P010-shaped 4 x 2 -> NV21-shaped: split and join, no resize
    d = R.desc(4, 2, 4, 2)
    x = R.dev(M.tight(*planes, "p010"))
    want = M.tight(*planes, "nv21")
    o = torch.zeros(want.size + 8, dtype=torch.int16, device="cuda")
    ctx.resize_ycc16_to_ycc_device(d, L.ycc16_source(d, "p010"), L.ycc16_dest(d, "nv21"), x.data_ptr(), o.data_ptr(), n, stream=R.stream())
    torch.cuda.synchronize()
    info = ctx.last_ycc16_info()
    got = R.back(o, np.uint16)
    eq(got[:want.size], want.reshape(-1), "65537 frames through the split and the join")
    assert not got[want.size:].any()
    assert (info.luma_kernel, info.chroma_kernel) == NONE2 and info.split and info.join, info
    assert info.launches == 1 + 2 + 1 + 2, info                        # luma copy, split twice, one chroma copy of 2 n planes, join twice
