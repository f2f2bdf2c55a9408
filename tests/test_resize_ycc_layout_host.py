"""The YCbCr layout validators against the answers of the four separate ones they replaced (no GPU): every case of
tests/golden/resize_ycc_layout_parity.npz -- drawn by tests/resize_ycc_layout_cfg.py, recorded by
tests/golden/make_resize_ycc_layout_golden.py from the commit before lanczos_resize_ycc_layout.cpp -- replayed on this build.
Every return code and every byte an init entry fills must be equal.  tests/native/ycc_layout_check.cpp runs the resolver itself,
linked without the library, over a handful of the cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_ycc_layout_cfg as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_ycc_layout_parity.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_is_the_draw_and_has_not_degenerated(golden):
    validate, init = C.draw()
    assert np.array_equal(golden["validate"], validate) and np.array_equal(golden["init"], init)
    codes = golden["validate_codes"]
    assert len(codes) == C.N_VALIDATE >= 3000
    ok = int((codes == L.OK).sum())
    assert 3 * ok >= len(codes) and 3 * (len(codes) - ok) >= len(codes), ok
    v = golden["validate"]
    for B in (1, 2):                                                     # both widths, sources and destinations, the three layouts
        for dest in (0, 1):
            for layout in C.LAYOUTS:
                sel = (v[:, 0] == B) & (v[:, 1] == dest) & (v[:, 15] == layout)
                assert (codes[sel] == L.OK).sum() > 50 and (codes[sel] != L.OK).sum() > 50, (B, dest, layout)
    assert {1, 9} <= set(v[:, 2:6].ravel().tolist())                      # 1-pixel planes and the largest size
    assert ((v[:, 6] == 1) & (v[:, 7] & 1 == 1)).sum() > 100 and ((v[:, 6] == 1) & (v[:, 8] & 1 == 1)).sum() > 100   # odd origins
    assert (v[:, 18] >= 0).sum() > 50 and ((v[:, 16] | v[:, 17]) & ~1 != 0).sum() > 50
    words = v[:, 0] == 2
    assert ((v[words, 11:15] & 1).any(axis=1)).sum() > 100                # odd strides and offsets of 16-bit layouts
    assert (golden["init_codes"] == L.OK).sum() > 100 and (golden["init_codes"] != L.OK).sum() > 100


def test_validators_answer_as_the_recorded_ones(golden):
    got = C.replay_validate(L._lib(), golden["validate"])
    bad = np.flatnonzero(got != golden["validate_codes"])
    assert bad.size == 0, (bad[:5], golden["validate"][bad[:5]], got[bad[:5]], golden["validate_codes"][bad[:5]])


def test_init_entries_fill_what_the_recorded_ones_filled(golden):
    codes, filled = C.replay_init(L._lib(), golden["init"])
    bad = np.flatnonzero((codes != golden["init_codes"]) | (filled != golden["init_filled"]).any(axis=1))
    assert bad.size == 0, (bad[:5], golden["init"][bad[:5]], codes[bad[:5]], golden["init_codes"][bad[:5]])


def test_resolver_links_without_the_library_and_agrees(golden, tmp_path):
    """tests/native/ycc_layout_check.cpp with lanczos_resize_ycc_layout.cpp alone: no library load, no kernel, no GPU.  Every drawn
    window lies inside its output and every descriptor is legal, so the resolver's code is the entry's"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "lanczos-hls_amd", "csrc")
    exe = str(tmp_path / "ycc_layout_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I" + csrc,
                    os.path.join(ROOT, "tests", "native", "ycc_layout_check.cpp"), os.path.join(csrc, "lanczos_resize_ycc_layout.cpp"),
                    "-o", exe], check=True, timeout=600)
    v, codes = golden["validate"], golden["validate_codes"]
    pick = np.concatenate([np.flatnonzero(codes == L.OK)[:40], np.flatnonzero(codes != L.OK)[:40]])
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for row in v[pick]:
            f.write(" ".join(str(int(x)) for x in row) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.split()
    assert out[-2:] == ["done", str(len(pick))] and [int(x) for x in out[:-2]] == codes[pick].tolist()
