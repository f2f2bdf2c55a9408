#!/usr/bin/env python3
"""Generate tests/golden/binding_calls.json: what every call of tests/binding_calls_cfg.py hands to the C ABI, recorded from the
Python binding of ONE commit -- the parent of a change to lanczos-hls_amd/__init__.py that must not move the mapping.

    git worktree add --detach /tmp/parent <commit>
    LANCZOS_LIB=$PWD/lanczos-hls_amd/liblanczos_hip.so python tests/golden/make_binding_calls_golden.py --root /tmp/parent

--root: the tree whose module is recorded (its HEAD is written into the fixture); the cases and the recorder are this tree's,
the library is this tree's build.  No GPU is needed: no launching entry is called.  Never regenerate the fixture from the module
a change is being checked on.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import binding_calls_cfg as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=B.ROOT, help="the tree whose lanczos-hls_amd/__init__.py is recorded")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    status = subprocess.run(["git", "-C", root, "status", "--porcelain", "--", "lanczos-hls_amd/__init__.py"],
                            check=True, capture_output=True, text=True).stdout.strip()
    if status:
        raise SystemExit(f"{root}: lanczos-hls_amd/__init__.py differs from its commit ({status}); record a clean checkout")
    commit = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    L = B.load_module(root)
    cases = B.run_all(L)
    reached = sorted({c["entry"] for r in cases.values() for c in r["calls"]})
    if reached != B.launching(L):
        raise SystemExit(f"the cases do not reach {sorted(set(B.launching(L)) - set(reached))}")
    out = {"generator": "tests/golden/make_binding_calls_golden.py", "commit": commit, "launching": reached, "cases": cases}
    with open(B.GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases, {sum(len(r['calls']) for r in cases.values())} calls of {len(reached)} entries at {commit[:7]} -> {B.GOLDEN}")


if __name__ == "__main__":
    main()
