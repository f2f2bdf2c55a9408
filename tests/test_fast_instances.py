"""The tables behind tests/test_fast_instances_gpu.py, checked against csrc/lanczos_fast.hpp and the oracle without a GPU: every
k_fast instance of LZ_FAST_CONFIGS_G0..G3 is listed and has exactly one frame in each shape table, every frame and every cut
list still has -- at the header's current MR, NGRP, UPR and WL_CAP -- the properties it was chosen for, and the two contents
that steer the worklist still steer it: the list of a sparse_flips tile cannot outgrow half of WL_CAP, that of a dense_flips
tile in the middle tile row must overflow it, and in both the oracle really stores v0 - 1 at integer phases, so a FIXUP step
that skipped them would be seen.  An instance added to the header, or a tile size changed, fails here until the tables follow."""
import numpy as np
import pytest

import fast_cfg as F
import lanczos_hls_amd as L
import oracle_lib as O

INSTANCES = sorted(F.FAST_INSTANCES)


def test_every_fast_instance_of_the_header_is_listed_once():
    insts = F.header_instances()
    assert len(insts) == len(set(insts)) == 35, insts
    assert set(insts) == F.FAST_INSTANCES, set(insts) ^ F.FAST_INSTANCES
    assert set(F.FAST_SHAPES) == F.FAST_INSTANCES and len(F.FAST_SHAPES) == len(insts), set(F.FAST_SHAPES) ^ F.FAST_INSTANCES
    assert set(F.FAST_SHAPES16) == F.FAST_INSTANCES and len(F.FAST_SHAPES16) == len(insts), set(F.FAST_SHAPES16) ^ F.FAST_INSTANCES


def _check_shapes(shapes, shapes16, shape):
    """Every FAST_SHAPES / FAST_SHAPES16 row and its strip cuts: the properties of fast_cfg's docstring, and the smallest frame
    that has them."""
    for inst, (w, h) in shapes.items():
        k = F.fast_cfg(inst, shape)
        assert not F.static_assert_errors(k), (inst, F.static_assert_errors(k))
        f = F.shape_facts(inst, w, h, shape)
        what = (inst, w, h, f)
        assert not f["in_rows_16"] and f["out_rows_dwords"], what                      # a plain call reaches the tile kernel
        assert f["tiles_x"] >= 2 and f["partial_tile"] and f["whole_unit_in_last_tile"], what
        assert f["partial_unit"] == F.partial_unit_possible(inst, shape), what
        assert f["tiles_y"] >= 3 and f["ragged_bottom"] and f["middle_halo_in_image"], what
        assert f["out_samples"] < (F.MAX_OUT_SAMPLES_BIG if inst in F.BIG_FRAMES else F.MAX_OUT_SAMPLES), what   # tests stay quick
        assert (w, h) == F.smallest_frame(inst, shape), (what, F.smallest_frame(inst, shape))
        w16 = shapes16[inst]
        f16 = F.shape_facts(inst, w16, h, shape)
        assert f16["in_rows_16"] and f16["out_rows_dwords"] and f16["tiles_x"] >= 2 and f16["partial_tile"], (inst, w16, f16)
        assert w16 == F.smallest_width16(inst, shape) and f16["out_samples"] < F.MAX_OUT_SAMPLES_BIG, (inst, w16, f16)
        cuts = F.strip_cuts(inst, f["out_h"], shape)
        assert not F.cut_errors(inst, cuts, f["out_h"], shape), (inst, cuts, F.cut_errors(inst, cuts, f["out_h"], shape))


def test_shape_tables_keep_their_properties_at_the_headers_tile_sizes():
    _check_shapes(F.FAST_SHAPES, F.FAST_SHAPES16, F.header_shape())
    # what the issue's examples say: u8 RGB 2x a = 3 is 134 x 63, 8-bit one-channel frames 260-270 wide, 16-bit ones 65-70
    assert F.FAST_SHAPES[1, 3, 2, 3] == (134, 63)
    assert all(260 <= w <= 270 for (sb, c, s, a), (w, h) in F.FAST_SHAPES.items() if (sb, c) == (1, 1))
    assert all(65 <= w <= 70 for (sb, c, s, a), (w, h) in F.FAST_SHAPES.items() if sb == 2)
    # a frame ends on a unit boundary only where dword output rows force it: 8-bit and 16-bit RGB at 3x
    assert {i for i in INSTANCES if not F.partial_unit_possible(i)} == {i for i in INSTANCES if i[1] == 3 and i[2] == 3}
    # the instances that fill the 16-bit worklist entry exactly (TWS_OUT == 1 << WL_SMP_BITS): 8-bit RGBA at 2x and at 4x
    full = {i for i in INSTANCES if F.fast_cfg(i).TWS_OUT == 1 << F.fast_cfg(i).WL_SMP_BITS}
    assert full == {i for i in INSTANCES if i[:2] == (1, 4) and i[2] in (2, 4)}, full
    assert {F.fast_cfg(i).WL_ROW_BITS for i in INSTANCES if i[2] == 2} == {6} and {F.fast_cfg(i).WL_ROW_BITS for i in INSTANCES if i[2] > 2} == {5}
    assert F.fast_cfg((1, 3, 2, 3)).WL_CAP == 4096 == F.header_shape()["wl_cap"]


def test_shape_check_notices_a_table_or_tile_size_that_no_longer_fits():
    """The check above can fail: a frame one unit narrower (the last tile holds no whole unit any more), a height that is a
    whole number of tile rows, a header with another MR or with one more instance."""
    shape = F.header_shape()
    inst = (1, 3, 2, 3)
    w, h = F.FAST_SHAPES[inst]
    k = F.fast_cfg(inst)
    for bad in ((w - k.P, h), (w, 2 * k.MR), (w, 3 * k.MR), (w + 1, h), (w + 2, h)):   # 130: two px past the tile; 60 / 90 rows: whole tile
        with pytest.raises(AssertionError):                                           # rows; 135: ragged dword rows; 136: unit boundary
            _check_shapes({inst: bad}, F.FAST_SHAPES16, shape)
    with pytest.raises(AssertionError):
        _check_shapes({inst: (w, h)}, {inst: F.FAST_SHAPES16[inst] - 16}, shape)      # 128 px: one tile
    for s, mr in ((2, 32), (3, 21), (4, 16)):
        with pytest.raises(AssertionError):
            _check_shapes(F.FAST_SHAPES, F.FAST_SHAPES16, dict(shape, mr={**shape["mr"], s: mr}))
    text = F.header_text()
    assert "MR = S == 2 ? 30 :" in text
    assert F.header_shape(text.replace("MR = S == 2 ? 30 :", "MR = S == 2 ? 32 :"))["mr"][2] == 32       # a changed MR is read, not assumed
    more = text.replace("X(uint16_t, 3, 3, 3)", "X(uint16_t, 3, 3, 3) X(uint16_t, 1, 2, 3)")
    assert set(F.header_instances(more)) - F.FAST_INSTANCES == {(2, 1, 2, 3)}
    more = text.replace("X(uint8_t, 1, 2, 4)\n", "X(uint8_t, 1, 2, 4) \\\n    X(uint8_t, 3, 2, 5)\n")     # on a line of its own
    assert set(F.header_instances(more)) - F.FAST_INSTANCES == {(1, 3, 2, 5)}


# The figures of worklist_figures() on the committed frames, so that they can be read here and cannot drift unseen:
# instance -> (sparse_flips: largest upper bound of a tile's worklist (<= WL_CAP / 2 = 2048),
#              dense_flips: smallest count of samples equal to 1 in a full tile of the middle tile row (> WL_CAP = 4096),
#              motifs of sparse_flips, oracle flips at them (samples: motifs x C for a >= 3, none for a = 2),
#              oracle flips in the first full tile of the middle tile row of dense_flips)
WORKLIST_FIGURES = {
    (1, 1, 2, 2): (128, 7392, 10, 0, 0),
    (1, 1, 2, 3): (128, 7840, 10, 10, 1920),
    (1, 1, 2, 4): (128, 8288, 10, 10, 1920),
    (1, 1, 3, 2): (192, 5152, 10, 0, 0),
    (1, 1, 3, 3): (192, 5600, 10, 10, 1280),
    (1, 1, 3, 4): (192, 6048, 10, 10, 1280),
    (1, 1, 4, 2): (256, 4320, 10, 0, 0),
    (1, 1, 4, 3): (256, 4480, 10, 10, 960),
    (1, 1, 4, 4): (256, 4928, 10, 10, 960),
    (1, 3, 2, 2): (192, 11088, 10, 0, 0),
    (1, 3, 2, 3): (192, 11760, 10, 30, 2880),
    (1, 3, 2, 4): (240, 12432, 8, 24, 2880),
    (1, 3, 3, 2): (432, 7728, 10, 0, 0),
    (1, 3, 3, 3): (432, 8400, 10, 30, 1920),
    (1, 3, 3, 4): (432, 9072, 10, 30, 1920),
    (1, 3, 4, 2): (384, 6048, 10, 0, 0),
    (1, 3, 4, 3): (480, 6720, 8, 24, 1440),
    (1, 3, 4, 4): (480, 7392, 8, 24, 1440),
    (1, 4, 2, 2): (256, 14784, 10, 0, 0),
    (1, 4, 2, 3): (320, 15680, 8, 32, 3840),
    (1, 4, 2, 4): (320, 16576, 8, 32, 3840),
    (1, 4, 3, 2): (384, 10304, 10, 0, 0),
    (1, 4, 3, 3): (480, 11200, 8, 32, 2560),
    (1, 4, 3, 4): (480, 12096, 8, 32, 2560),
    (1, 4, 4, 2): (512, 8064, 10, 0, 0),
    (1, 4, 4, 3): (640, 8960, 8, 32, 1920),
    (1, 4, 4, 4): (640, 9856, 8, 32, 1920),
    (2, 3, 2, 3): (192, 5880, 8, 24, 1440),
    (2, 3, 2, 4): (216, 6216, 8, 24, 1440),
    (2, 3, 3, 3): (252, 4200, 8, 24, 960),
    (2, 3, 3, 4): (324, 4536, 8, 24, 960),
    (2, 4, 2, 3): (256, 7840, 8, 32, 1920),
    (2, 4, 2, 4): (288, 8288, 8, 32, 1920),
    (2, 4, 3, 3): (384, 5600, 8, 32, 1280),
    (2, 4, 3, 4): (432, 6048, 8, 32, 1280),
}

_ORACLE = {}


def _oracle(inst, name):
    """(frame, oracle output) of an instance's FAST_SHAPES frame with content sparse_flips / dense_flips, computed once."""
    if (inst, name) not in _ORACLE:
        sb, c, s, a = inst
        w, h = F.FAST_SHAPES[inst]
        img = (F.sparse_flips if name == "sparse" else F.dense_flips)(inst, h, w)
        cfg = O.cfg(w, h, w * s, h * s, c, a, s, 1)
        _ORACLE[inst, name] = (img, (O.expected_hwc_u16 if sb == 2 else O.expected_hwc_u8)(cfg, img, 4))
    return _ORACLE[inst, name]


def worklist_figures(inst):
    """The figures of one instance: the largest sparse upper bound over its tiles, the smallest dense lower bound over the full
    tiles of the middle tile row, and the oracle's integer-phase flips in both frames."""
    sb, c, s, a = inst
    k = F.fast_cfg(inst)
    w, h = F.FAST_SHAPES[inst]
    sp, want_sp = _oracle(inst, "sparse")
    de, want_de = _oracle(inst, "dense")
    bound = F.sparse_bound(inst, sp)
    count = F.dense_count(inst, de)
    full_mid = [(tx, 1) for tx in range(w // k.TWP_IN)]
    fl_sp, fl_de = F.integer_phase_flips(sp, want_sp, s), F.integer_phase_flips(de, want_de, s)
    mot = F.sparse_motifs(inst, h, w)
    return {
        "bound_min": min(bound.values()), "bound_max": max(bound.values()), "dense_min": min(count[t] for t in full_mid),
        "motifs": len(mot), "motifs_flipped": sum(int(fl_sp[y, x].all()) for (y, x) in mot), "sparse_flips": int(fl_sp.sum()),
        "dense_flips_mid_tile": int(fl_de[k.MR:2 * k.MR, 0:k.TWP_IN].sum()), "dense_flips": int(fl_de.sum()),
        "motifs_per_tile_max": max(F.motifs_per_tile(inst, h, w).values()),
    }


@pytest.mark.parametrize("inst", INSTANCES, ids=F.inst_id)
def test_worklist_conditions_hold_on_the_committed_frames(inst):
    """sparse_flips: in every tile the upper bound of the worklist is positive and at most WL_CAP / 2 (the list branch, with
    room); at most 16 motifs meet a tile; the motifs sit where fast_cfg.sparse_motifs says: first and last unit of a full
    tile, first and last LDS row of the middle tile row, the last in-image column, the partial last unit.  dense_flips: every
    full tile of the middle tile row holds more than WL_CAP samples equal to 1 (the redo-everything branch under any
    vlim >= 1)."""
    k = F.fast_cfg(inst)
    w, h = F.FAST_SHAPES[inst]
    fig = worklist_figures(inst)
    assert 0 < fig["bound_min"] and fig["bound_max"] <= k.WL_CAP // 2, (inst, fig)
    assert fig["motifs_per_tile_max"] <= 16, (inst, fig)
    assert fig["dense_min"] > k.WL_CAP, (inst, fig)
    mot = set(F.sparse_motifs(inst, h, w))
    r_lo, r_hi = k.MR - k.A + 1, k.MR - k.A + k.NR                      # LDS rows 0 and NR - 1 of tile row 1
    assert 0 < r_lo and r_hi == 2 * k.MR + k.A - 1 == h - 1, (inst, "both halo rows of the middle tile row are image rows")
    assert (r_lo, 2) in mot and 2 // k.P == (0 if k.P > 2 else 1), (inst, "first unit of the full tile (its max; the 1 too where P > 2), LDS row 0")
    assert (r_hi, k.TWP_IN - 1) in mot, (inst, "last pixel of the last unit of the full tile, LDS row NR - 1")
    assert (r_lo, w - 1) in mot and (w % k.P != 0) == F.partial_unit_possible(inst), (inst, "last in-image column, in the partial last unit")
    sp, _ = _oracle(inst, "sparse")
    assert int(np.count_nonzero(sp.any(axis=2))) == 2 * len(mot)      # isolated motifs: two pixels each, none shared


def test_the_oracle_flips_what_the_fixup_step_must_flip():
    """Taken from the oracle alone.  For every instance with a >= 3 the oracle's output at the integer phase of the `1` of every
    sparse_flips motif (want[S y, S x]) is not 1, in every channel, and in the first full tile of the middle tile row of
    dense_flips there are such flips too: the reference's double chain really lands below v0 there, so a tile kernel whose
    worklist, FIXUP step or redo-everything branch lost them would differ from the oracle.  For a = 2 the oracle flips no
    integer-phase sample in either frame -- L(1) is positive and L(2) is the product of two zeros of sin, about 1e-33: no
    integer-phase fix-up is ever needed there, those nine instances cannot be steered and simply run the same frames.
    (16-bit: parity unpinned by the reference; the oracle is the restatement templated on the sample type.)"""
    lines = []
    for inst in INSTANCES:
        fig = worklist_figures(inst)
        lines.append(f"{inst}: sparse bound <= {fig['bound_max']}, dense count >= {fig['dense_min']}, oracle flips: "
                     f"{fig['motifs_flipped']} of {fig['motifs']} motifs ({fig['sparse_flips']} samples), "
                     f"{fig['dense_flips_mid_tile']} in the dense middle tile ({fig['dense_flips']} in the frame)")
    print("\n".join(lines))
    for inst, line in zip(INSTANCES, lines):
        fig = worklist_figures(inst)
        assert WORKLIST_FIGURES[inst] == (fig["bound_max"], fig["dense_min"], fig["motifs"], fig["sparse_flips"], fig["dense_flips_mid_tile"]), line
        if inst[3] >= 3:
            assert fig["motifs_flipped"] == fig["motifs"] > 0 and fig["sparse_flips"] == fig["motifs"] * inst[1], line
            assert fig["dense_flips_mid_tile"] > 0, line
        else:
            assert fig["sparse_flips"] == 0 and fig["dense_flips"] == 0, line


def test_prefix_rows_as_the_library_computes_them():
    for inst, (w, h) in F.FAST_SHAPES.items():
        sb, c, s, a = inst
        for width in (w, F.FAST_SHAPES16[inst]):
            assert L.inplace_rows(L.make_desc(width, h, c, s, 1, a, sb)) == F.prefix_K(s, a), inst


def test_generic_frames():
    """The k_generic frames of test_generic_in_strips_and_batches: two tiles each way of the header's tile size, ragged, more than
    a tile's rows at and below K, dword rows exactly where asked -- and no ragged-row width exactly where none can exist."""
    tw, th = F.generic_tile()
    assert (tw, th) == (256, 32)
    for sb in (1, 2):
        for (sn, sd) in ((2, 1), (7, 5), (9, 8)):
            for c in (1, 3, 4):
                for a in (2, 3, 4):
                    for ragged in (False, True):
                        fr = F.generic_frame(c, sb, sn, sd, a, ragged, (tw, th))
                        if fr is None:
                            assert ragged and (c == 4 or (sb == 2 and sn % 2 == 0)), (sb, c, sn, sd, a)
                            continue
                        w, h = fr
                        n, oh = w * sn // sd * c, h * sn // sd
                        d = L.make_desc(w, h, c, sn, sd, a, sb)
                        K = L.inplace_rows(d)
                        assert (d.out_w * c, d.out_h) == (n, oh) and K == F.prefix_rows(sn, sd, a)
                        assert tw < n < 2 * tw and th < oh and oh % th != 0 and oh - K > th and ((n * sb) % 4 != 0) == ragged
                        cuts = F.generic_cuts(sn, sd, a, oh)
                        assert cuts == sorted(set(cuts)) and cuts[1] > K and cuts[-1] == oh, (cuts, K)
