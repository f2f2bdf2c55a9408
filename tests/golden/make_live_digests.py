#!/usr/bin/env python3
"""Generate tests/golden/live_reference_digests.json from the REFERENCE's own compiled software path (oracle/_ref).

Run where the reference tree exists, after `make -C oracle ref`:
    python tests/golden/make_live_digests.py
Writes FNV-1a-64 digests of the reference's planar output for every input of test_oracle.live_cases(), so that
test_oracle.py::test_against_live_reference_build checks the restatement without the reference build present.
Data only (digests of outputs); no reference source is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
from test_oracle import LIVE_DIGESTS, live_cases  # noqa: E402


def main():
    digests = {}
    for key, cfg, _, img in live_cases():
        ref = O.ref_expected_planar_u8(cfg, img)
        if ref is None:
            raise SystemExit(f"reference build missing for {key}: run `make -C oracle ref`")
        digests[key] = f"{O.fnv1a64(ref):016x}"
    out = {"generator": "tests/golden/make_live_digests.py",
           "input": "test_oracle.live_cases(): numpy default_rng(7) noise 0..255 and 0..39, all-255, 4-pixel checkerboard",
           "digests": digests}
    with open(LIVE_DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {LIVE_DIGESTS}")


if __name__ == "__main__":
    main()
