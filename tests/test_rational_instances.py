"""The tables behind tests/test_rational_instances_gpu.py, checked against csrc/lanczos_rational.hpp without a GPU: every
k_ratp instance of LZ_RATP_CONFIGS is listed and has exactly one frame, and every frame still has -- at the header's current
LZ_RATP_ROWS, LZ_RATP_NVG and NT -- the properties it was chosen for.  An instance added to the header, or a tile size changed,
fails here until the tables follow."""
import lanczos_hls_amd as L
import ratp_cfg as R


def _header_kw(text=None):
    return dict(rows=R.header_constant("LZ_RATP_ROWS", text), nvg=R.header_constant("LZ_RATP_NVG", text), nt=R.header_constant("NT", text))


def test_every_ratp_instance_of_the_header_is_listed_once():
    insts = R.header_instances()
    assert len(insts) == len(set(insts)), insts
    assert set(insts) == R.RATP_INSTANCES, set(insts) ^ R.RATP_INSTANCES
    assert set(R.RATP_SHAPES) == R.RATP_INSTANCES and len(R.RATP_SHAPES) == len(insts), set(R.RATP_SHAPES) ^ R.RATP_INSTANCES
    from test_parity_gpu import RATP_INSTANCES       # one list: the parity module uses this one
    assert RATP_INSTANCES is R.RATP_INSTANCES


def _check_shapes(shapes, kw):
    """Every RATP_SHAPES row: two tiles each way (three tile rows at the tall height), a last tile that ends inside a unit, a
    last period cut by the frame, dword output rows (rat_supports), input rows off a dword where C * SB allows, an axis
    ratp_prepare accepts -- and the strip cuts of the tall frame fall where the strip test says they do."""
    for inst, (w, h, tall) in shapes.items():
        k = R.ratp_cfg(inst, **kw)
        assert k.TP % k.NVG == 0 and k.NVT * k.NVG <= k.NT and k.UNIT_IN_B % 4 == 0, (inst, k)         # the header's static_asserts
        assert k.WIN_DW0 * 4 + (k.NUW - 1) * k.UNIT_IN_B + k.NW * 4 <= k.IN_PITCH, (inst, k)          # a unit's window stays in its LDS row
        for height, tiles_y in ((h, 2), (tall, 3)):
            f = R.shape_facts(inst, w, height, **kw)
            what = (inst, w, height, f)
            assert f["tiles_x"] >= 2 and f["tiles_y"] >= tiles_y, what
            assert f["partial_unit"] and f["partial_period"] and f["out_rows_dwords"] and f["periodic_axis"], what
            assert f["in_rows_dwords"] == ((k.C * k.SB) % 4 == 0), what
            assert f["out_w"] * f["out_h"] < 100000, what                                             # tests stay quick
        out_h = tall * k.N // k.D
        cuts = R.strip_cuts(inst, out_h, **kw)
        K = f["K"]
        assert cuts == sorted(set(cuts)) and cuts[0] == 0 and cuts[-1] == out_h and cuts[1] >= K, (inst, cuts, K)
        assert all(c % k.TH != 0 and c % k.N != 0 for c in cuts[1:-1]), (inst, cuts)
        assert any(0 < b - a_ < k.N for a_, b in zip(cuts, cuts[1:])), (inst, cuts)                      # narrower than a period
        assert len({c // k.TH for c in cuts[:-1]}) >= 2 and cuts[-2] // k.TH < (out_h - 1) // k.TH, (inst, cuts)   # strips in and across tile rows


def test_shape_table_keeps_its_properties_at_the_headers_tile_sizes():
    _check_shapes(R.RATP_SHAPES, _header_kw())
    for inst, (w, h, tall) in R.RATP_SHAPES.items():     # K as the library computes it
        sb, c, n, d, a = inst
        assert L.inplace_rows(L.make_desc(w, tall, c, n, d, a, sb)) == R.prefix_rows(n, d, a), inst


def test_shape_check_notices_a_table_or_tile_size_that_no_longer_fits():
    """The check above can fail: a frame one unit narrower (one tile across), a height that is a whole number of periods,
    a header with taller tiles or with one more instance."""
    import pytest
    kw = _header_kw()
    inst = (1, 3, 4, 3, 3)
    w, h, tall = R.RATP_SHAPES[inst]
    for bad in ((w - 18, h, tall), (w, h + 1, tall), (w + 1, h, tall)):     # 141 -> 188 px: one tile; 45 -> 60 rows: whole periods; 160 px: ragged dword rows
        with pytest.raises(AssertionError):
            _check_shapes({inst: bad}, kw)
    with pytest.raises(AssertionError):
        _check_shapes(R.RATP_SHAPES, dict(kw, rows=96))
    text = R.header_text().replace("    X(uint16_t, 4, 3, 2, 3)", "    X(uint16_t, 4, 3, 2, 3) \\\n    X(uint16_t, 3, 3, 2, 3)")
    assert set(R.header_instances(text)) - R.RATP_INSTANCES == {(2, 3, 3, 2, 3)}


def test_handover_and_rat_frames():
    """The frames either side of ratp_prepare's size condition (4/3, a = 3, RGB: 15 x 15 fails on both axes, 18 x 15 qualifies by
    width, 15 x 16 by height) and the k_rat frames: two tiles each way of the header's tile size, ragged, dword output rows."""
    assert R.handover_frames((1, 3, 4, 3, 3)) == [(15, 15, False), (18, 15, True), (15, 16, True)]
    assert R.handover_frames((1, 4, 3, 2, 3)) == [(10, 10, False), (11, 10, True), (10, 11, True)]
    row_b, tile_h = R.header_constant("kRatCols") * 4, R.header_constant("kRatTileH")
    for sb in (1, 2):
        for (sn, sd) in ((5, 3), (7, 4)):
            for c in (1, 3, 4):
                w, h = R.rat_frame(c, sb, sn, sd, row_b, tile_h)
                assert (w, h) == R.rat_frame(c, sb, sn, sd)       # (the defaults are the header's)
                row, oh = w * sn // sd * c * sb, h * sn // sd
                assert row > row_b and row % row_b != 0 and row % 4 == 0 and oh > tile_h and oh % tile_h != 0 and row // sb * oh < 100000
