#!/usr/bin/env python3
"""Generate tests/golden/resize_ycc_layout_parity.npz: the return codes of lanczos_ycc{,16}_{source,dest}_validate and the codes
and filled structs of lanczos_ycc{,16}_{source,dest}_init for the drawn cases of tests/resize_ycc_layout_cfg.py, recorded from
the library of ONE commit -- the parent of a change to the YCbCr layout validation that must not move an answer.

    git worktree add --detach /tmp/parent <commit> && make -C /tmp/parent/lanczos-hls_amd
    LANCZOS_LIB=/tmp/parent/lanczos-hls_amd/liblanczos_hip.so python tests/golden/make_resize_ycc_layout_golden.py

The cases and the replay are this tree's, the library is the one LANCZOS_LIB names.  No GPU is needed: every entry called is
host only.  Never regenerate the fixture from the library a change is being checked on.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lanczos_hls_amd as L  # noqa: E402
import resize_ycc_layout_cfg as C  # noqa: E402


def main():
    if not os.environ.get("LANCZOS_LIB"):
        sys.exit("set LANCZOS_LIB to the library of the commit to record")
    lib = L._lib()
    validate, init = C.draw()
    codes = C.replay_validate(lib, validate)
    init_codes, init_filled = C.replay_init(lib, init)
    ok = int((codes == L.OK).sum())
    print("validate: %d cases, %d accepted, %d refused; codes %s" % (len(codes), ok, len(codes) - ok, sorted(set(codes.tolist()))))
    print("init: %d cases, %d accepted" % (len(init_codes), int((init_codes == L.OK).sum())))
    for B in (1, 2):
        for dest in (0, 1):
            sel = (validate[:, 0] == B) & (validate[:, 1] == dest)
            print("  B %d dest %d: %d cases, %d accepted" % (B, dest, int(sel.sum()), int((codes[sel] == L.OK).sum())))
    assert 3 * ok >= len(codes) and 3 * (len(codes) - ok) >= len(codes), "the draw degenerated: a third accepted, a third refused"
    np.savez_compressed(os.path.join(HERE, "resize_ycc_layout_parity.npz"), validate=validate, validate_codes=codes, init=init,
                        init_codes=init_codes, init_filled=init_filled)


if __name__ == "__main__":
    main()
